"""gprhip_sample_paths on the device: posterior draws as functions against the 80-bit reference of tests/sample_paths_ref.py
(pinned to the oracle's posterior by tests/test_sample_paths_host.py) on every path and kernel width, the structure of the
draws from the device's own outputs (mean, covariance, variance), the same draw at other points, chunks, the per-draw
selection with its gradients, the contract of the entry point and the front ends.  The cases are those of
tests/test_gpu_predict_grad.py.

Bounds: a draw and the mean are the same contraction K (coefficients) with coefficients of the same conditioning, so the
project's own constants hold with NO conditioning allowance: the largest absolute deviation over the largest absolute entry of
the column is at most TOL_POST (3e-10) for sample values and TOL_GRAD (1e-8) for the winners' gradients.  Every achieved ratio
is recorded (GPR_MARGINS_LOG -> profiles/sample_paths_margins.txt)."""
import ctypes
import functools

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from oracle import fitc_oracle as O
from tests import margins as M
from tests.sample_paths_ref import path_state, sample_paths_from_state
from tests.test_gpu_input_grad import _case
from tests.test_gpu_parity import TOL_GRAD, TOL_POST
from tests.test_gpu_predict_grad import COND_MAX, DIMS, NTS, PAIRS_WIDE, PROJ_DIMS, SIGMA2, _problem, _test_points

gpu = pytest.mark.gpu
SHAPES = [(1, 1), (15, 3), (64, 10), (65, 64), (200, 65), (200, 129), (300, 257)]
DRAWS = [1, 15, 16, 17, 33, 64]   # every NB = ceil(ns / 16), a full tile and ragged ones
NT = 65


@functools.lru_cache(maxsize=None)
def _state(key):
    Xs, y, Zs, args, ok, cond = _case(*key)
    assert cond <= COND_MAX, (key, cond)
    return path_state(ok, Zs, Xs, y, SIGMA2)


def _draws(key, nt, ns, seed=0):
    """(z m x ns, eps nt x ns): standard normal, fixed seed"""
    m = _case(*key)[2].shape[1]
    rng = np.random.default_rng(9000 + 131 * ns + nt + seed)
    return np.asfortranarray(rng.standard_normal((m, ns))), np.asfortranarray(rng.standard_normal((nt, ns)))


def _ref(key, Xt, z, **kw):
    Xs, y, Zs, args, ok, cond = _case(*key)
    return sample_paths_from_state(ok, Zs, _state(key), Xt, z, SIGMA2, **kw)


def _hold_columns(what, got, ref, tol=TOL_POST):
    """every column against the reference column, relative to that column's largest entry: the worst is printed and recorded"""
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    worst = max(M.relinf(got[:, j], ref[:, j]) for j in range(ref.shape[1]))
    jw = int(np.argmax([M.relinf(got[:, j], ref[:, j]) for j in range(ref.shape[1])]))
    print("%s: worst column %.3e of its largest entry (bound %.0e)" % (what, worst, tol))
    M.check_vec(what, got[:, jw], ref[:, jw], tol)


def _note(key, **extra):
    Xs, y, Zs, args, ok, cond = _case(*key)
    M.note(cond=cond, kind=key[0], n=key[1], m=key[2], d=key[3], D=Xs.shape[0], **extra)


def _check_values(p, key, what, nt, ns_list=(17,)):
    """with eps (predictive on and off) and without, per ns"""
    Xt = _test_points(key, nt)
    for ns in ns_list:
        z, eps = _draws(key, nt, ns)
        _note(key, nt=nt, ns=ns)
        path = p.sample_paths(Xt, z)["samples"]
        _hold_columns("%s.ns%d.path" % (what, ns), path, _ref(key, Xt, z)["samples"])
        for predictive in (False, True):
            got = p.sample_paths(Xt, z, eps=eps, predictive=predictive)["samples"]
            _hold_columns("%s.ns%d.%s" % (what, ns, "predictive" if predictive else "latent"), got,
                          _ref(key, Xt, z, eps=eps, predictive=predictive)["samples"])


# ---- 1. values against the reference ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", SHAPES)
def test_iso_d3_against_the_reference(n, m):
    key = ("iso", n, m, 3)
    p = _problem(key)
    try:
        p.set_timing(2)
        _check_values(p, key, "paths.iso", NT)
        stages = p.last_timings()
        assert {"sp_coeff", "sp_path", "sp_resid"} <= set(stages) and "pg_m" not in stages, stages
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("nt", NTS)
def test_row_tile_edges_and_every_draw_count(nt, n, m):
    key = ("iso", n, m, 3)
    p = _problem(key)
    try:
        _check_values(p, key, "paths.iso_nt%d" % nt, nt, DRAWS)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", [(64, 10)])
def test_small_shape_on_the_engine_path(n, m, monkeypatch):
    monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")
    key = ("iso", n, m, 3)
    p = _problem(key)
    try:
        _check_values(p, key, "paths.iso_engine", NT)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("d", DIMS)
def test_every_kernel_width(d, n, m):
    key = ("iso", n, m, d)
    p = _problem(key)
    try:
        _check_values(p, key, "paths.iso_d%d" % d, NT, (16, 64))
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_fat_without_projection(n, m):
    key = ("fat", n, m, 3, 3)
    p = _problem(key)
    try:
        _check_values(p, key, "paths.fat", NT)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("D,d", PROJ_DIMS)
def test_fat_with_projection(D, d, n, m):
    key = ("proj", n, m, d, D)
    p = _problem(key)
    try:
        _check_values(p, key, "paths.proj_%d_%d" % (D, d), NT, (33,))
    finally:
        p.close()


# ---- 2. structure, from the device alone -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", [(64, 10), (200, 65), (200, 129)])
def test_mean_covariance_and_variance_from_the_device(n, m):
    """z = 0 gives predict's means in every column; with identity columns of z (ceil(m / 64) calls) L = F - mu 1^T has
    (L L^T)_rs = covariances(kind="FIC")_rs off the diagonal, and sum_j L_rj^2 + (samples(z = 0, eps = 1) - mu)_r^2 is predict's
    latent variance."""
    key = ("iso", n, m, 3)
    nt = 40
    Xt = _test_points(key, nt)
    _note(key, nt=nt)
    p = _problem(key)
    try:
        mu, var = p.predict(Xt, predictive=False)
        zero = p.sample_paths(Xt, np.zeros((m, 3)))["samples"]
        for j in range(3):
            M.check_vec("paths.structure.mean", zero[:, j], mu, TOL_POST)
        L = np.zeros((nt, m))
        for c0 in range(0, m, 64):
            w = min(64, m - c0)
            z = np.zeros((m, w))
            z[c0 + np.arange(w), np.arange(w)] = 1.0
            L[:, c0:c0 + w] = p.sample_paths(Xt, z)["samples"] - zero[:, :1]
        cov = p.covariances(Xt, kind="FIC", predictive=False)
        off = ~np.eye(nt, dtype=bool)
        LLt = L @ L.T
        print("paths.structure.covariance: %.3e of the largest off-diagonal entry (bound %.0e)" % (M.relinf(LLt[off], cov[off]), TOL_POST))
        M.check_vec("paths.structure.covariance", LLt[off], cov[off], TOL_POST)
        sd = p.sample_paths(Xt, np.zeros((m, 1)), eps=np.ones((nt, 1)))["samples"][:, 0] - zero[:, 0]
        assert np.all(sd >= 0)
        M.check_vec("paths.structure.variance", (L * L).sum(1) + sd * sd, var, TOL_POST)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_a_test_point_on_an_inducing_point(n, m):
    """there sf2 - |K_r U^-1|^2 is jitter-sized and may round below zero: the residual part stays finite and non-negative"""
    key = ("iso", n, m, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    Xt = np.asfortranarray(Zs[:, :min(m, 8)])
    nt = Xt.shape[1]
    p = _problem(key)
    try:
        zero = p.sample_paths(Xt, np.zeros((m, 1)))["samples"][:, 0]
        sd = p.sample_paths(Xt, np.zeros((m, 1)), eps=np.ones((nt, 1)))["samples"][:, 0] - zero
        assert np.all(np.isfinite(sd)) and np.all(sd >= 0) and np.all(sd < 0.1 * np.exp(0.5 * ok.log_sf2))
    finally:
        p.close()


# ---- 3. the same function --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_one_draw_is_one_function(n, m):
    """one z, two candidate sets sharing points at other row positions (one chunk each; other chunks: the next test): the
    values at the shared points agree to the bound; two identical calls agree bitwise; host and device outputs agree bitwise"""
    import torch
    key = ("iso", n, m, 3)
    ns = 5
    A = _test_points(key, 200)
    shared = np.arange(0, 200, 7)
    rng = np.random.default_rng(3)
    B = np.asfortranarray(np.concatenate([_test_points(key, 64, seed=1), A[:, shared[::-1]], _test_points(key, 15, seed=2)], axis=1))
    pos = 64 + np.arange(len(shared))[::-1]
    z, _ = _draws(key, 200, ns)
    eps = np.asfortranarray(rng.standard_normal((200, ns)))
    _note(key, nt=200, ns=ns)
    p = _problem(key)
    try:
        fa = p.sample_paths(A, z)["samples"]
        fb = p.sample_paths(B, z)["samples"]
        _hold_columns("paths.same_function", fb[pos], fa[shared])
        assert np.array_equal(fa, p.sample_paths(A, z)["samples"])
        sa = p.sample_paths(A, z, eps=eps, predictive=True)["samples"]
        assert np.array_equal(sa, p.sample_paths(A, z, eps=eps, predictive=True)["samples"])
        dev = torch.device("cuda:0")
        xt = torch.tensor(np.ascontiguousarray(A.T), device=dev)
        et = torch.tensor(np.ascontiguousarray(eps.T), device=dev)
        out = torch.full((ns, 200), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        assert p.sample_paths(xt.data_ptr(), z, out_device_ptrs={"samples": out.data_ptr()}, nt=200) == {}
        assert np.array_equal(out.cpu().numpy().T, fa)
        p.sample_paths(xt.data_ptr(), z, eps=et.data_ptr(), predictive=True, out_device_ptrs={"samples": out.data_ptr()}, nt=200)
        assert np.array_equal(out.cpu().numpy().T, sa)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_one_draw_is_one_function_across_chunks_on_device_pointers(n, m):
    """one z; a set of 200 points, and a set of 131072 + 65 (two chunks) that holds copies of 29 of them in its first chunk
    and again in its second, evaluated on DEVICE pointers (inputs, eps and samples offset by the chunk): the values at the
    shared points agree with the first set's to the bound and with each other bitwise, the device outputs equal the host
    call's bitwise, and the gradient of the path part at a winner planted in the second chunk equals the reference's"""
    import torch
    key = ("iso", n, m, 3)
    ns, nt, edge = 3, 131072 + 65, 131072
    A = _test_points(key, 200)
    shared = np.arange(0, 200, 7)
    rng = np.random.default_rng(17)
    D = A.shape[0]
    B = np.asfortranarray(np.tile(_test_points(key, 4099), (1, nt // 4099 + 1))[:, :nt] + 1e-3 * rng.normal(size=(D, nt)))
    pos1, pos2 = 1000 + np.arange(len(shared)), edge + 5 + np.arange(len(shared))
    B[:, pos1] = A[:, shared]
    B[:, pos2] = A[:, shared]
    z, _ = _draws(key, 200, ns)
    eps = np.asfortranarray(rng.standard_normal((nt, ns)))
    win = edge + 50
    eps[win, :] = 40.0           # (predictive: the residual deviation is at least sigma, so this row wins every draw)
    _note(key, nt=nt, ns=ns)
    p = _problem(key)
    try:
        fa = p.sample_paths(A, z)["samples"]
        dev = torch.device("cuda:0")
        xt = torch.tensor(np.ascontiguousarray(B.T), device=dev)
        et = torch.tensor(np.ascontiguousarray(eps.T), device=dev)
        out = torch.full((ns, nt), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        assert p.sample_paths(xt.data_ptr(), z, out_device_ptrs={"samples": out.data_ptr()}, nt=nt) == {}
        fb = out.cpu().numpy().T
        assert np.all(np.isfinite(fb))
        _hold_columns("paths.same_function.first_chunk", fb[pos1], fa[shared])
        _hold_columns("paths.same_function.second_chunk", fb[pos2], fa[shared])
        assert np.array_equal(fb[pos1], fb[pos2])
        assert np.array_equal(fb, p.sample_paths(B, z)["samples"])
        got = p.sample_paths(xt.data_ptr(), z, eps=et.data_ptr(), predictive=True, top_k=4,
                             out_device_ptrs={"samples": out.data_ptr()}, nt=nt)
        sb = out.cpu().numpy().T
        host = p.sample_paths(B, z, eps=eps, predictive=True, top_k=4)
        assert np.array_equal(sb, host["samples"])
        for name in ("top_index", "top_values", "top_dvalues"):
            assert np.array_equal(got[name], host[name]), name
        _assert_selection(sb, got, 4, True)
        assert np.all(got["top_index"][0] == win)
        rows = np.unique(np.concatenate([np.arange(edge - 40, nt), rng.integers(0, nt, size=100)]))
        _hold_columns("paths.same_function.device_eps", sb[rows],
                      _ref(key, np.asfortranarray(B[:, rows]), z, eps=eps[rows], predictive=True)["samples"])
        ref = _ref(key, np.asfortranarray(B[:, [win]]), z, grad_at=[(0, j) for j in range(ns)])["grads"]
        M.check_vec("paths.same_function.second_chunk.dvalues", got["top_dvalues"][:, 0, :], ref, TOL_GRAD)
    finally:
        p.close()


# ---- 4. chunks -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_chunk_rows_128_and_300_points(n, m):
    key = ("iso", n, m, 3)
    nt, ns = 300, 17
    Xt = _test_points(key, nt)
    z, eps = _draws(key, nt, ns)
    _note(key, nt=nt, ns=ns)
    p = _problem(key, chunk_rows=128)
    try:
        got = p.sample_paths(Xt, z, eps=eps, predictive=True, top_k=16)
        _hold_columns("paths.chunk_rows_128", got["samples"], _ref(key, Xt, z, eps=eps, predictive=True)["samples"])
        _assert_selection(got["samples"], got, 16, True)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_several_chunks(n, m):
    """131072 + 65 test points: two chunks of the prediction's own chunk rule -- the offsets of eps and samples and the merge of
    the chunks' winners.  The reference is computed for the rows around the chunk edge, the ends and 200 random rows."""
    key = ("iso", n, m, 3)
    nt, ns = 131072 + 65, 3
    rng = np.random.default_rng(11)
    D = _case(*key)[0].shape[0]
    Xt = np.asfortranarray(np.tile(_test_points(key, 4099), (1, nt // 4099 + 1))[:, :nt] + 1e-3 * rng.normal(size=(D, nt)))
    rows = np.unique(np.concatenate([np.arange(0, 70), np.arange(131072 - 70, 131072 + 65), rng.integers(0, nt, size=200)]))
    z, _ = _draws(key, 7, ns)
    eps = np.asfortranarray(rng.standard_normal((nt, ns)))
    eps[[100, 131080], :] = 40.0   # (one winner planted in each chunk; predictive: the residual deviation is at least sigma)
    _note(key, nt=nt, ns=ns)
    p = _problem(key)
    try:
        got = p.sample_paths(Xt, z, eps=eps, predictive=True, top_k=64)
        assert np.all(np.isfinite(got["samples"]))
        ref = _ref(key, np.asfortranarray(Xt[:, rows]), z, eps=eps[rows], predictive=True)
        _hold_columns("paths.chunks", got["samples"][rows], ref["samples"])
        _assert_selection(got["samples"], got, 64, True)
        for j in range(ns):
            assert {100, 131080} <= set(got["top_index"][:2, j])
        blind = p.sample_paths(Xt, z, eps=eps, predictive=True, top_k=64, want_samples=False)
        assert np.array_equal(blind["top_index"], got["top_index"]) and np.array_equal(blind["top_values"], got["top_values"])
    finally:
        p.close()


# ---- 5. top-k --------------------------------------------------------------------------------------------------------------------
def _expected_order(col, k, maximise):
    """stable arg-sort of the column (its negation for the smallest): value descending, the lower index first, NaN never"""
    s = np.where(np.isnan(col), -np.inf, col if maximise else -col) + 0.0
    order = np.argsort(-s, kind="stable")
    order = order[~np.isnan(col[order])]
    out = np.full(k, -1, dtype=np.int64)
    out[:min(k, len(order))] = order[:k]
    return out


def _assert_selection(samples, got, k, maximise):
    ns = samples.shape[1]
    assert got["top_index"].shape == (k, ns) and got["top_values"].shape == (k, ns)
    for j in range(ns):
        want = _expected_order(samples[:, j], k, maximise)
        assert np.array_equal(got["top_index"][:, j], want), (j, got["top_index"][:, j], want)
        live = want >= 0
        assert np.array_equal(got["top_values"][live, j], samples[want[live], j])       # bitwise the samples' entries
        assert np.all(np.isnan(got["top_values"][~live, j])) and np.all(np.isnan(got["top_dvalues"][:, ~live, j]))


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
@pytest.mark.parametrize("k", [1, 16, 64])
def test_top_k_per_draw(k, n, m):
    """top_index per draw against a stable numpy arg-sort of the device's own column, both directions (k = 64 > nt = 40: -1
    fill); top_values bitwise the samples' entries; top_dvalues against the reference gradient; samples = NULL: the same winners"""
    key = ("iso", n, m, 3)
    nt, ns = (40 if k == 64 else 200), 17
    Xt = _test_points(key, nt)
    z, eps = _draws(key, nt, ns)
    _note(key, nt=nt, ns=ns, k=k)
    p = _problem(key)
    try:
        for maximise in (True, False):
            for e in (None, eps):
                got = p.sample_paths(Xt, z, eps=e, maximise=maximise, top_k=k)
                _assert_selection(got["samples"], got, k, maximise)
                blind = p.sample_paths(Xt, z, eps=e, maximise=maximise, top_k=k, want_samples=False)
                assert set(blind) == {"top_index", "top_values", "top_dvalues"}
                for name in blind:
                    assert np.array_equal(blind[name], got[name], equal_nan=True), name
                pairs = [(int(got["top_index"][i, j]), j) for j in range(ns) for i in range(k) if got["top_index"][i, j] >= 0]
                ref = _ref(key, Xt, z, grad_at=pairs)["grads"]
                have = np.stack([got["top_dvalues"][:, i, j] for j in range(ns) for i in range(k) if got["top_index"][i, j] >= 0], axis=1)
                assert np.all(np.isfinite(have))
                M.check_vec("paths.top%d.%s.dvalues" % (k, "max" if maximise else "min"), have, ref, TOL_GRAD)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("D,d", [(5, 2), (70, 4)])
def test_top_k_gradients_with_a_projection(D, d):
    key = ("proj", 200, 129, d, D)
    nt, ns, k = 65, 5, 4
    Xt = _test_points(key, nt)
    z, _ = _draws(key, nt, ns)
    _note(key, nt=nt, ns=ns, k=k)
    p = _problem(key)
    try:
        got = p.sample_paths(Xt, z, top_k=k)
        _assert_selection(got["samples"], got, k, True)
        pairs = [(int(got["top_index"][i, j]), j) for j in range(ns) for i in range(k)]
        have = np.stack([got["top_dvalues"][:, i, j] for j in range(ns) for i in range(k)], axis=1)
        assert have.shape[0] == D
        M.check_vec("paths.proj_%d_%d.dvalues" % (D, d), have, _ref(key, Xt, z, grad_at=pairs)["grads"], TOL_GRAD)
    finally:
        p.close()


@gpu
def test_ties_and_nan_in_a_column():
    """two copies of every test point give equal path values (the lower index first), and a NaN in eps a NaN sample that is
    never selected"""
    key = ("iso", 200, 129, 3)
    half = _test_points(key, 30)
    Xt = np.asfortranarray(np.concatenate([half, half], axis=1))
    nt, ns = 60, 3
    z, _ = _draws(key, nt, ns)
    p = _problem(key)
    try:
        got = p.sample_paths(Xt, z, top_k=64)
        assert np.array_equal(got["samples"][:30], got["samples"][30:])
        _assert_selection(got["samples"], got, 64, True)
        eps = np.zeros((nt, ns), order="F")
        eps[got["top_index"][0, 0], 0] = np.nan
        eps[7, 2] = np.nan
        bad = p.sample_paths(Xt, z, eps=eps, top_k=64, maximise=False)
        assert np.isnan(bad["samples"][7, 2]) and np.sum(np.isnan(bad["samples"])) == 2
        _assert_selection(bad["samples"], bad, 64, False)
        assert 7 not in bad["top_index"][:, 2] and bad["top_index"][58, 2] >= 0 and bad["top_index"][59, 2] == -1
    finally:
        p.close()


# ---- 6. states and refusals ------------------------------------------------------------------------------------------------------
def _raw(p, z, Xt, samples, ns=None, ldz=None, ld=None, nt=None, eps=None, lde=None, lds=None, top_k=0, top_index=None, on_device=0):
    vp = ctypes.c_void_p
    D, m = Xt.shape[0], z.shape[0]
    nt_ = Xt.shape[1] if nt is None else nt
    return p._lib.gprhip_sample_paths(
        p._handle(), z.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), m if ldz is None else ldz, z.shape[1] if ns is None else ns,
        vp(Xt.ctypes.data), D if ld is None else ld, nt_, vp(eps.ctypes.data) if eps is not None else vp(None),
        Xt.shape[1] if lde is None else lde, 1, vp(samples.ctypes.data) if samples is not None else vp(None),
        Xt.shape[1] if lds is None else lds, 1, top_k, top_index, None, None, on_device)


@gpu
def test_refusals_leave_the_next_correct_call_working():
    key = ("fat", 64, 10, 3, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    D, n = Xs.shape
    m = Zs.shape[1]
    nt, ns = NT, 4
    Xt = _test_points(key, nt)
    z, eps = _draws(key, nt, ns)
    ref = _ref(key, Xt, z, eps=eps, predictive=True)["samples"]
    out = np.full((nt, ns), np.nan, order="F")
    idx = np.zeros(64 * ns, dtype=np.int64)
    ip = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    p = _problem(key)
    f32 = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, m, precision=gpr_amd.F32_BULK)
    empty = gpr_amd.Problem(gpr_amd.COV_SE_FAT, n, D, D, m)
    wide = gpr_amd.Problem(gpr_amd.COV_SE_ISO, 40, 65, 65, 5)
    try:
        p.set_timing(2)
        bad = [dict(ns=0), dict(ns=65), dict(ldz=m - 1), dict(ld=D - 1), dict(ld=D + 1, on_device=1), dict(nt=0),
               dict(eps=eps, lde=nt - 1), dict(lds=nt - 1), dict(top_k=-1, top_index=ip), dict(top_k=65, top_index=ip),
               dict(top_k=3)]
        for kw in bad:
            assert _raw(p, z, Xt, out, **kw) == _lib.EBADARG, kw
            assert np.all(np.isnan(out)) and p.last_timings() == {}, kw      # nothing was enqueued
        assert _raw(p, z, Xt, None) == _lib.EBADARG                           # nothing requested
        assert _raw(p, z, Xt, out, eps=eps) == _lib.OK                        # ... each followed by a clean call
        M.note(cond=cond, kind="fat", n=n, m=m, d=3, nt=nt, ns=ns)
        _hold_columns("paths.after_bad_arguments", out, ref)
        out[:] = np.nan
        # a multiscale model state
        lms = np.asfortranarray(np.random.default_rng(3).uniform(-1.0, 0.5, size=(D, m)))
        p.eval(want_grad=False, sigma2=SIGMA2, inducing=Zs, log_multiscales_m05=lms, **args)
        assert _raw(p, z, Xt, out) == _lib.EBADARG and np.all(np.isnan(out))
        # after eval_targets
        p.set_targets_many(np.asfortranarray(np.stack([y, 2.0 * y], axis=1)))
        p.eval_targets(want_grad=False, sigma2=SIGMA2, inducing=Zs, **args)
        assert _raw(p, z, Xt, out) == _lib.ESTATE and np.all(np.isnan(out))
        # fp32-bulk problem, no model, 65 point dimensions
        assert _raw(f32, z, Xt, out) == _lib.EBADARG
        assert _raw(empty, z, Xt, out) == _lib.ESTATE
        rng = np.random.default_rng(5)
        Xw, Zw = np.asfortranarray(rng.normal(size=(65, 40))), np.asfortranarray(rng.normal(size=(65, 5)))
        wide.set_inputs(Xw)
        wide.set_targets(rng.normal(size=40))
        wide.eval(want_grad=False, log_ell=float(np.log(8.0)), log_sf2=0.0, sigma2=SIGMA2, inducing=Zw)
        ow = np.full((4, 2), np.nan, order="F")
        assert _raw(wide, np.zeros((5, 2), order="F"), np.asfortranarray(Xw[:, :4]), ow) == _lib.EBADARG and np.all(np.isnan(ow))
        assert np.all(np.isnan(out))
        # the next correct call works
        p.eval(want_grad=False, sigma2=SIGMA2, inducing=Zs, **args)
        assert _raw(p, z, Xt, out, eps=eps) == _lib.OK
        _hold_columns("paths.after_refusals", out, ref)
    finally:
        for q in (p, f32, empty, wide):
            q.close()


@gpu
@pytest.mark.parametrize("n,m", PAIRS_WIDE)
def test_loaded_predictor_and_a_later_evaluation(n, m):
    """load_predictor with the oracle's coefficients and factors gives the reference's draws; without factors the call is
    refused (GPRHIP_ESTATE); after a later eval the same z gives the draws of the new state"""
    key = ("iso", n, m, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    out = O.evaluate(ok, Zs, Xs, y, SIGMA2, want_grad=False, keep=True)
    model = out["model"]
    Xt = _test_points(key, NT)
    z, eps = _draws(key, NT, 9)
    _note(key, nt=NT, ns=9)
    ref = _ref(key, Xt, z, eps=eps)["samples"]
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO, n, 3, 3, m)
    try:
        p.load_predictor(sigma2=SIGMA2, inducing=Zs, coeffs=out["coeffs"],
                         co_variance_coeffs=(np.triu(model["inducing"]["chol_km"]), np.triu(model["r_mat"])), **args)
        _hold_columns("paths.loaded", p.sample_paths(Xt, z, eps=eps)["samples"], ref)
        p.load_predictor(sigma2=SIGMA2, inducing=Zs, coeffs=out["coeffs"], **args)
        with pytest.raises(gpr_amd.GprHipError) as e:
            p.sample_paths(Xt, z)
        assert e.value.status == _lib.ESTATE
    finally:
        p.close()
    q = _problem(key)
    try:
        first = q.sample_paths(Xt, z, eps=eps)["samples"]
        _hold_columns("paths.before_the_later_eval", first, ref)
        q.eval(want_grad=False, sigma2=0.25, inducing=Zs, **args)
        other = q.sample_paths(Xt, z, eps=eps)["samples"]
        state = path_state(ok, Zs, Xs, y, 0.25)
        _hold_columns("paths.after_the_later_eval", other, sample_paths_from_state(ok, Zs, state, Xt, z, 0.25, eps=eps)["samples"])
        assert not np.array_equal(first, other)
    finally:
        q.close()


# ---- 7. the neighbours keep their bits, the front end ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", [("iso", 64, 10, 3), ("iso", 200, 129, 3)], ids=str)
def test_acquire_predict_and_predict_input_grad_keep_their_bits(key):
    """calls made before and after sample_paths calls in one process give the same bits, `pg_m` stays valid, and a call
    changes nothing in the predictor state"""
    Xt = _test_points(key, 200)
    z, eps = _draws(key, 200, 17)
    p = _problem(key)
    try:
        acq = dict(maximise=False, best=0.1, xi=0.01, want=("values", "dvalues", "means", "variances"), top_k=16)
        before = (p.predict(Xt), p.predict_input_grad(Xt), p.acquire(Xt, "log_ei", **acq))
        p.set_timing(2)
        p.sample_paths(Xt, z, eps=eps, predictive=True, top_k=16)
        p.sample_paths(Xt, z, maximise=False, top_k=64, want_samples=False)
        after_grad = p.predict_input_grad(Xt)
        assert "pg_m" not in p.last_timings()      # M of the first call is still valid
        after = (p.predict(Xt), after_grad, p.acquire(Xt, "log_ei", **acq))
        assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
        for a, b in ((before[1], after[1]), (before[2], after[2])):
            assert set(a) == set(b)
            for name in a:
                assert np.array_equal(a[name], b[name]), name
    finally:
        p.close()


@gpu
def test_functor_path_sampler():
    """Eval.Path_sampler keeps its draws: samples without the residual part are Problem.sample_paths' bits, `best` its
    winners, and the same sampler gives the same function at other inputs"""
    from gpr_amd import cov_se_iso, fitc_gp
    key = ("iso", 200, 65, 3)
    Xs, y, Zs, args, ok, cond = _case(*key)
    Xt = _test_points(key, NT)
    GP = fitc_gp.Make_deriv(cov_se_iso)
    F = GP.FITC
    q = _problem(key)
    try:
        kernel = cov_se_iso.Kernel.create(cov_se_iso.Params(log_ell=args["log_ell"], log_sf2=args["log_sf2"]))
        inputs = F.Deriv.Inputs.calc(F.Deriv.Inducing.calc(kernel, Zs), Xs)
        trained = F.Deriv.Trained.calc(F.Deriv.Model.calc(inputs, SIGMA2), y)
        sampler = F.Eval.Path_sampler.calc(trained, 5, rng=np.random.default_rng(1))
        z = F.Eval.Path_sampler.get_draws(sampler)
        assert z.shape == (65, 5)
        tin = F.Eval.Inputs.calc(Xt, inputs.inducing)
        want = q.sample_paths(Xt, z, top_k=3)
        got = F.Eval.Path_sampler.samples(sampler, tin, residual=False)
        assert np.array_equal(got, want["samples"])
        best = F.Eval.Path_sampler.best(sampler, tin, 3, True)
        assert np.array_equal(best["top_index"], want["top_index"]) and np.array_equal(best["top_values"], want["top_values"])
        noisy = F.Eval.Path_sampler.samples(sampler, tin, rng=np.random.default_rng(2))
        assert noisy.shape == (NT, 5) and not np.array_equal(noisy, got)
    finally:
        q.close()
        GP.close()
