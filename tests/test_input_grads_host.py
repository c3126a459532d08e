"""The CPU half of tests/test_gpu_input_grads.py: the 80-bit references of tests/input_grads_ref.py and their bounds are pinned
here, before any device is involved, on the oracle's own operands (t, U = chol_km, R~^-1 = U r_mat^-1 inverted in 80 bits, M
formed from them in float64, X = x_mat of the oracle's gradient):
  1. the references reproduce tests/predict_grad_ref.py and tests/input_grad_ref.py;
  2. float64 restatements of every kernel form -- the expansion with the shift under fmax, raw direct differences,
     p~ rowsum - E z~, the nested one-kernel G, K M; left to right and in 16-column tiles -- stay inside every bound on every
     device case; the worst ratio is recorded;
  3. planted defects miss the bound of the entry they touch by at least 100 x;
  4. what the max-norm check misses: a dropped column and a late G block on a far row pass margins.check_vec at TOL_GRAD and fail
     the entry bound;
  5. the cases have far rows: entries above 1e-2 and below 1e-8 of the largest, fewer than 10 % of the K entries underflow.
"""
import functools

import numpy as np
import pytest

from oracle import fitc_oracle as O
from tests import input_grads_ref as G
from tests import margins as M
from tests import posterior_ref as R
from tests.input_grad_ref import input_grad_from_parts
from tests.predict_grad_ref import model_state, predict_grad_from_state
from tests.test_gpu_input_grads import (NAMES, PREDICT_CASES, SIGMA2, XGRAD, Case, case_id, data, expected_path, geometry, hypers_of,
                                        points, reference, xgrad_reads_k)
from tests.test_posterior_host import _matmul, _sum_lr, _sum_pw
from tests.util import _ld_triu_inverse

TOL_GRAD, TOL_POST = 1e-8, 3e-10       # as tests/test_gpu_parity.py
POWER = 100.0
LD = R.LD


def _kernel(c, args):
    if c.kind == "iso":
        return O.SeIsoKernel(args["log_ell"], args["log_sf2"])
    return O.SeFatKernel(c.d, args["log_sf2"], args.get("tproj"), args.get("log_hetero_skedasticity"), None)


@functools.lru_cache(maxsize=8)
def _oracle(c, variational=False):
    """the oracle's operands of a case: t, uinv, rinv, pg_m (float64, as a device would hold them), and the parts"""
    X, y, Z, args = data(c)
    parts = O.evaluate(_kernel(c, args), Z, X, y, SIGMA2, variational=variational, hypers=[], keep=True)
    model = parts["model"]
    U = np.triu(model["inducing"]["chol_km"]).astype(LD)
    uinv = _ld_triu_inverse(U)
    rinv = np.triu(U @ _ld_triu_inverse(np.triu(model["r_mat"]).astype(LD)))
    uinv, rinv = uinv.astype(np.float64), rinv.astype(np.float64)
    pg_m = uinv @ (np.eye(c.m) - rinv @ rinv.T) @ uinv.T
    return dict(t=parts["coeffs"], uinv=uinv, rinv=rinv, pg_m=pg_m, parts=parts)


def _ops(c):
    o = _oracle(c)
    return {k: o[k] for k in ("t", "uinv", "rinv", "pg_m")}


# ---- 1. agreement with the existing references ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [Case("iso", 100, 17, 3), Case("iso", 100, 65, 3, forced=True), Case("proj", 100, 65, 2, 5, True, forced=True),
                               Case("iso", 100, 40, 17)], ids=case_id)
def test_the_references_reproduce_predict_grad_ref(c):
    X, y, Z, args = data(c)
    ok = _kernel(c, args)
    old = predict_grad_from_state(ok, Z, model_state(ok, Z, X, y, SIGMA2), points(c, 65)[0], SIGMA2, True)
    new = reference(c, 65, _ops(c), expected_path(c), SIGMA2)
    for name in NAMES:
        M.check_vec("host.igrads.%s" % name, new[name][0].astype(np.float64), old[name], TOL_GRAD if name[0] == "d" else TOL_POST)


@pytest.mark.parametrize("c", [Case("iso", 65, 65, 3), Case("iso", 65, 17, 65, forced=True), Case("proj", 65, 65, 3, 40)], ids=case_id)
def test_the_reference_reproduces_input_grad_ref(c):
    X, y, Z, args = data(c)
    parts = _oracle(c)["parts"]
    old = input_grad_from_parts(_kernel(c, args), Z, X, parts, False)
    g = G.geometry(X, Z, **hypers_of(c, args))
    new, _ = G.train_input_grad(g, parts["hyper_t"]["x_mat"], False)
    M.check_vec("host.igrads.xgrad", new.T.astype(np.float64), old, TOL_GRAD)


# ---- 2. float64 restatements inside the bounds ----------------------------------------------------------------------------------
def _sum_tiles(terms):
    """16-column tiles, four partial sums as the lanes hold them (columns 4 lq .. 4 lq + 3 of every tile), then the lanes"""
    n = terms.shape[-1]
    lanes = []
    for lq in range(4):
        idx = [cb + 4 * lq + r for cb in range(0, n, 16) for r in range(4) if cb + 4 * lq + r < n]
        lanes.append(_sum_lr(terms[..., idx]) if idx else np.zeros(terms.shape[:-1]))
    return _sum_lr(np.stack(lanes, axis=-1))


def _k64(c, Xt, Z, args, expansion):
    """(K, p~, z~, p, inv_ell2) in float64: the expansion with the shift under fmax, or raw direct differences"""
    tp = args.get("tproj")
    P = (Xt if tp is None else tp.T @ Xt).T.copy()
    Zm = Z.T.copy()
    s = G.shift_of(Z)
    Pt, Zt = P - s[None, :], Zm - s[None, :]
    a = -0.5 * np.exp(-2.0 * args["log_ell"]) if c.kind == "iso" else -0.5
    if expansion:
        pn, zn = _sum_lr(Pt * Pt), _sum_lr(Zt * Zt)
        S = _sum_lr(Pt[:, None, :] * Zt[None, :, :])
        dist = np.maximum(pn[:, None] + zn[None, :] - 2.0 * S, 0.0)
    else:
        dist = np.zeros((P.shape[0], Zm.shape[0]))
        for k in range(c.d):
            diff = P[:, k][:, None] - Zm[:, k][None, :]
            dist = dist + diff * diff
    return np.exp(args["log_sf2"] + a * dist), Pt, Zt, -2.0 * a


def _restate_grad(E, Pt, Zt, ie2, order, tp, sign):
    rs = order(E)
    acc = np.stack([order(E * Zt[:, k][None, :]) for k in range(Zt.shape[1])], axis=-1)
    g = sign * ie2 * (Pt * rs[:, None] - acc)
    if tp is not None:
        g = np.stack([_sum_lr(tp[b][None, :] * g) for b in range(tp.shape[0])], axis=-1)
    return rs, g


def restate_predict(c, nt, ops, path, order):
    X, y, Z, args = data(c)
    Xt = points(c, nt)[0]
    tp = args.get("tproj")
    engine = path == "engine"
    Ke, Pt, Zt, ie2 = _k64(c, Xt, Z, args, engine)
    Ks = _k64(c, Xt, Z, args, False)[0]
    mu, dmu = _restate_grad(Ke * ops["t"][None, :], Pt, Zt, ie2, order, tp, -1.0)
    if engine:
        Gm = _matmul(Ks, ops["pg_m"], order)
    else:
        V = _matmul(Ks, ops["uinv"], order)
        Q = _matmul(V, ops["rinv"], order)
        Gm = _matmul(V - _matmul(Q, ops["rinv"].T, order), ops["uinv"].T, order)
    rsv, dv = _restate_grad(Ke * Gm, Pt, Zt, ie2, order, tp, 2.0)
    return dict(means=mu, variances=(np.exp(args["log_sf2"]) - rsv) + SIGMA2, dmeans=dmu.T, dvariances=dv.T)


@pytest.mark.parametrize("c,nts", PREDICT_CASES, ids=case_id)
def test_float64_restatements_of_the_prediction_gradient_stay_inside_the_bounds(c, nts):
    path, ops = expected_path(c), _ops(c)
    nt = nts[-1]
    ref = reference(c, nt, ops, path, SIGMA2)
    for order in (_sum_lr, _sum_tiles):
        got = restate_predict(c, nt, ops, path, order)
        for name in NAMES:
            r, at = G.ratio(got[name], *ref[name])
            M.record("host.igrads.restated.%s.%s" % (path, name), r, 1.0, case=case_id(c))
            assert r <= 1.0, (case_id(c), name, order.__name__, r, at)


@pytest.mark.parametrize("c", sorted(set(c._replace(forced=False) for c in list(zip(*PREDICT_CASES))[0] if c.m > 1), key=case_id), ids=case_id)
def test_a_float64_m_stays_inside_its_bound(c):
    o = _oracle(c)
    Mr, Mb = G.m_matrix(o["uinv"], o["rinv"])
    for order in (_sum_lr, _sum_pw):
        B = _matmul(o["rinv"], o["rinv"].T, order)
        Md = _matmul(o["uinv"], _matmul(np.eye(c.m) - B, o["uinv"].T, order), order)
        r, at = G.ratio(Md, Mr, Mb)
        M.record("host.igrads.restated.pg_m", r, 1.0, case=case_id(c))
        assert r <= 1.0, (case_id(c), r, at)


@pytest.mark.parametrize("c,variational,model_only", XGRAD, ids=case_id)
def test_float64_restatements_of_the_training_input_gradient_stay_inside_the_bound(c, variational, model_only):
    X, y, Z, args = data(c)
    parts = _oracle(c, variational)["parts"]
    Xm = O.model_prepare_hyper(parts["cm"])["x_mat"] if model_only else parts["hyper_t"]["x_mat"]
    path = "engine" if (c.forced or c.m > 256) else "other"
    read_k = xgrad_reads_k(c, path)
    g = G.geometry(X, Z, **hypers_of(c, args))
    ref, bound = G.train_input_grad(g, Xm, read_k)
    K, Pt, Zt, ie2 = _k64(c, X, Z, args, not read_k)
    for order in (_sum_lr, _sum_tiles):
        got = _restate_grad(Xm * K, Pt, Zt, ie2, order, args.get("tproj"), 1.0)[1]
        r, at = G.ratio(got, ref, bound)
        M.record("host.igrads.restated.xgrad.%s" % ("readK" if read_k else "recompute"), r, 1.0, case=case_id(c))
        assert r <= 1.0, (case_id(c), order.__name__, r, at)


# ---- 3. / 4. planted defects ----------------------------------------------------------------------------------------------------
DEFECT_CASE = Case("iso", 100, 65, 17)        # engine path, DT = 2, m = 65: mc = 80, a ragged last tile of one live column
NT = 65


def _planted(defect, row):
    """{name: values} of the engine path with one defect, formed in 80 bits as the reference is, and the entries it touches"""
    c = DEFECT_CASE
    X, y, Z, args = data(c)
    ops = _ops(c)
    g = dict(geometry(c, NT))
    K, t, Mm = g["K"], ops["t"], ops["pg_m"]
    keep = np.ones((NT, c.m), LD)
    Gm, eG = G.g_engine(g, Mm)
    touched = (slice(None), row)
    scale_dv = 1.0
    if defect == "one column dropped":
        keep[row, int(np.argmax(np.abs(K[row] * t)))] = 0
    elif defect == "the last 16-column tile dropped":
        keep[row, 64:] = 0
    elif defect == "G read one 16-column block late":
        Gm = Gm.copy()
        Gm[row] = np.concatenate([np.zeros(16, LD), Gm[row, :-16]])
    elif defect == "the factor 2 of dvar missing":
        scale_dv = 0.5
    elif defect == "M of a previous model":
        o2 = _oracle(c._replace(log_sf2=0.3))
        Gm = g["K"] @ R._ld(o2["pg_m"])
    elif defect == "I - B~^-1 taken as I":
        Gm = g["K"] @ R._ld(ops["uinv"] @ ops["uinv"].T)
    elif defect == "the strictly lower part of M zero":
        Gm = g["K"] @ R._ld(np.triu(Mm))
    elif defect == "the last row of a ragged 16-row block zero":
        touched = (slice(None), NT - 1)       # (a far row: its entries are tiny, and still each misses its own bound)
    elif defect == "one dimension tile dropped":
        g["Zm"] = g["Zm"].copy()
        g["Pm"] = g["Pm"].copy()
        g["Zm"][:, 16:] = 0        # the products E z~ and p~ rowsum of k >= 16 are not added
        g["Pm"][:, 16:] = 0
        touched = (slice(16, None), row)
    elif defect == "the shift not put back":
        pass
    else:
        raise AssertionError(defect)
    g["K"] = K * keep
    out = {k: v for k, (v, b) in G.predict(g, t, SIGMA2, True, Gm, eG).items()}
    if defect == "the shift not put back":      # p for p~ in the first term: inv_ell2 s_k rowsum(E) is added
        s = R._ld(G.shift_of(Z))[None, :]
        out["dmeans"] = out["dmeans"] - g["ie2"] * s * out["means"][:, None]
        out["dvariances"] = out["dvariances"] + 2 * g["ie2"] * s * (g["K"] * Gm).sum(1)[:, None]
    out["dvariances"] = out["dvariances"] * scale_dv
    if defect == "the last row of a ragged 16-row block zero":
        out = {k: v.copy() for k, v in out.items()}
        for v in out.values():
            v[NT - 1] = 0
    return {k: (v.T if v.ndim == 2 else v) for k, v in out.items()}, touched


DEFECTS = [("one column dropped", ("means", "dmeans", "variances", "dvariances")),
           ("the last 16-column tile dropped", ("means", "dmeans", "variances", "dvariances")),
           ("G read one 16-column block late", ("variances", "dvariances")),
           ("the shift not put back", ("dmeans", "dvariances")),
           ("one dimension tile dropped", ("dmeans", "dvariances")),
           ("the factor 2 of dvar missing", ("dvariances",)),
           ("M of a previous model", ("variances", "dvariances")),
           ("I - B~^-1 taken as I", ("variances", "dvariances")),
           ("the strictly lower part of M zero", ("variances", "dvariances")),
           ("the last row of a ragged 16-row block zero", ("means", "dmeans", "variances", "dvariances"))]


def _miss(got, ref, bound, touched):
    sel = touched if ref.ndim == 2 else touched[1]
    return G.ratio(np.asarray(got[sel], LD), ref[sel], bound[sel])[0]


@pytest.mark.parametrize("defect,names", DEFECTS, ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else "")
def test_planted_defects_miss_the_bound_of_the_entry_they_touch(defect, names):
    c = DEFECT_CASE
    ref = reference(c, NT, _ops(c), "engine", SIGMA2)
    row = 0                                   # a training input: inside the data
    got, touched = _planted(defect, row)
    for name in names:
        r = _miss(got[name], *ref[name], touched)
        M.record("host.igrads.defect.%s" % name, r, POWER, case=defect)
        assert r >= POWER, (defect, name, r)


def test_the_strictly_lower_part_and_the_transposed_projection_show_on_m_and_the_back_projection():
    """defects on M itself, and tproj transposed in the back-projection at D = d"""
    c = DEFECT_CASE
    o = _oracle(c)
    Mr, Mb = G.m_matrix(o["uinv"], o["rinv"])
    assert G.ratio(np.triu(o["pg_m"]), Mr, Mb)[0] >= POWER
    assert G.ratio(_oracle(c._replace(log_sf2=0.3))["pg_m"], Mr, Mb)[0] >= POWER
    g = dict(geometry(c, NT))
    rng = np.random.default_rng(3)
    g["tp"] = R._ld(np.eye(c.d) + 0.1 * rng.uniform(-1, 1, size=(c.d, c.d)))
    val = -g["ie2"] * G._moment(g, g["K"] * R._ld(o["t"])[None, :])
    ref, bound = G.back_project(g, val, 1e-14 * np.abs(val))
    r = G.ratio(val @ g["tp"], ref, bound)[0]
    M.record("host.igrads.defect.tproj_transposed", r, POWER)
    assert r >= POWER


@pytest.mark.parametrize("defect", ["one column dropped", "G read one 16-column block late"])
def test_what_the_max_norm_check_misses(defect):
    """planted on a FAR row (5 .. 8 length scales from the nearest inducing point): the whole row is below 1e-8 of the
    matrix's largest entry, margins.check_vec at TOL_GRAD passes, the entry bound fails"""
    c = DEFECT_CASE
    ref = reference(c, NT, _ops(c), "engine", SIGMA2)
    name = "dmeans" if defect == "one column dropped" else "dvariances"
    val, bound = ref[name]
    rows = [i for i in range(NT) if i % 3 == 1 and i != 13 and np.max(np.abs(val[:, i])) < 1e-8 * np.max(np.abs(val))]
    assert rows, "no far row below 1e-8 of the largest entry"
    got, touched = _planted(defect, rows[0])
    M.check_vec("host.igrads.old_check.%s" % name, got[name].astype(np.float64), val.astype(np.float64), TOL_GRAD)   # passes
    r = _miss(got[name], val, bound, touched)
    M.record("host.igrads.old_check_misses.%s" % name, r, POWER, case=defect)
    assert r >= POWER, (defect, r)


# ---- 5. the cases have far rows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,nts", [cn for cn in PREDICT_CASES if max(cn[1]) >= 15], ids=case_id)
def test_the_cases_have_far_rows_and_few_underflows(c, nts):
    """(for 15 test points and more: fewer hold no far row)"""
    nt = max(nts)
    g = geometry(c, nt)
    val = np.abs(reference(c, nt, _ops(c), expected_path(c), SIGMA2, var=False)["dmeans"][0]).astype(np.float64)
    live = val[:, ~points(c, nt)[1]]
    assert np.any(live > 1e-2 * val.max()) and np.any((live < 1e-8 * val.max()) & (live > 0)), case_id(c)
    if c.d > 1:
        assert np.mean(np.asarray(g["K"] < R.ETA)) < 0.10, case_id(c)
    else:
        # on a line cond(K_m) <= 1e5 leaves the inducing points many length scales apart: most K entries of EVERY row
        # underflow, far or not.  What the allowance could carry is an output entry: fewer than 10 % of those lie below eta.
        assert np.mean(val < R.ETA) < 0.10, case_id(c)
