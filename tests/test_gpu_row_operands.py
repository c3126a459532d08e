"""The operands a gradient evaluation contracts the covariance derivatives with -- the per-row vectors r, 1/s, v, w, the mean
coefficients t, the m x m matrix W and the n x m matrix X of Trained.prepare_hyper (lib/fitc_gp.ml:1158-1207) -- read back
through gprhip_debug_fetch after one evaluation and compared with the oracle ROW BY ROW, on every path that produces them.
Everything else in the suite sees the row vectors only through sums over n (l, dl/dsigma2, the gradient), where one wrong row
hides at 1/n of its error (test_one_wrong_row_hides_from_the_sums_but_not_from_the_row_check).

Which kernels a group of cases reaches (asserted per case from last_timings(), as tests/test_gpu_factors.py::_taken does):
  small    m <= 64           small_pass1 / small_pass2 (small.hip, 64-row blocks, 512 / 256 workgroups: at n = 32 833 a pass-1
                             workgroup handles more than one block and a pass-2 workgroup more than two), W by small_finish;
  mid1     65 <= m <= 128    mid_pass1 / mid_pass2 in their one-tile form (mid.hip, 64-row blocks, 256 workgroups: n = 16 449
                             gives one workgroup a second block), W by mid_finish;
  mid2     129 <= m <= 256   mid_pass1 / mid_pass2 in their two-tile form (32-row blocks, 256 workgroups: n = 8225), with the
                             Gram launch pair of mid.hip up to MID_GRAM_ROWS = 4096 rows and the engine's launch above (n =
                             4096, 4097), W by mid_finish;
  engine   m > 256, or both  pass1_rows_kernel / pass2_rows_kernel (rowops.hip, 256-row kernels over 128-row padded chunks, fed by
           one-kernel paths  the epilogue partial sums of the engine's V and Q' products: 3, 4, 6 and 9 column blocks at m = 257,
           switched off      385, 641, 1100), W by build_w.  Cov_se_fat with multiscales runs on small and engine only.
Row chunks (chunk_rows = 256 at n = 700, 128 at n = 300: a ragged last chunk) run on every path but mid2; shards of a
ShardedDeviceProblem on mid1, mid2 and engine.  The padded rows are not visible through gprhip_debug_fetch.

Cases are tests/util.py::factor_case: the recipe of tests/test_gpu_factors.py with n a parameter, the length scale chosen so
that cond(K_m + jitter I) <= 1e5 by numpy.linalg.eigvalsh on the oracle's K_m (test_conditioning_of_every_case).  No bound here
carries a conditioning allowance and Problem.condition() is not used.

Bounds.  The reference of every device check is the oracle (oracle/fitc_oracle.py: _fast_model, deriv_trained_calc,
trained_prepare_hyper, model_prepare_hyper -- the statements evaluate_fast runs).  How good the oracle itself is was measured
on the CPU against tests/util.py::longdouble_operands, an 80-bit restatement on the same K_m and K_nm, over every case of the
list (test_oracle_against_the_80_bit_restatement; figures in profiles/row_operand_margins.txt):
  1. r, 1/s at TOL_ROW = 1e-10, v, w at TOL_ROWVW = 2e-10, t at TOL_POST = 3e-10, of the largest entry: the constants of
     tests/test_gpu_parity.py, unchanged.  The oracle is within 1/10 of each (asserted; 1/30 at worst, v at n = 32 833).
  2. 1/s, v, w once more, every row relative to max(|ref_i|, 1e-3 max|ref|), at TOL_ROWREL: 100 x the oracle's worst such
     figure, the margin TOL_ROW has over the oracle.  A wrong small entry cannot hide behind the largest one.
  3. model_only: w == 0 exactly, v against cm_calc_v1_vec at TOL_ROWVW / TOL_ROWREL.
  4. W symmetric to 1e-12 of its largest entry; triu(W) against the oracle's w_mat at TOL_W, X (single-chunk cases) against
     x_mat at TOL_X, of the largest entry; both 10 x the oracle's worst deviation from the restatement, rounded up to one
     digit, and checked on every case, n = 1 excepted (_matrices_compared).  The oracle is within 1/10 of each (asserted).
"""
import collections
import functools

import numpy as np
import pytest

import gpr_amd
from oracle import fitc_oracle as O
from tests import margins as M
from tests.util import factor_case, longdouble_operands, oracle_km_full
from tests.util import taken as _taken

gpu = pytest.mark.gpu

TOL_DS2 = 4e-10     # as tests/test_gpu_parity.py
TOL_ROW = 1e-10
TOL_ROWVW = 2e-10
TOL_POST = 3e-10
# Derived from the oracle's own error against the 80-bit restatement, never from the device (profiles/row_operand_margins.txt,
# "oracle_*" lines: worst over all cases of test_oracle_against_the_80_bit_restatement):
TOL_ROWREL = 5e-8   # check 2: 100 x 4.3e-10, w of n = 32 833, m = 16 (1/s: 1.1e-12, v: 1.9e-10 at worst): a row of w down at
                    # 1e-3 of the largest carries the largest row's rounding error, for the oracle's QR too
TOL_W = 1e-10       # 10 x 9.76e-12 (n = 4097, m = 129; Cov_se_fat with a projection at n = 800, m = 257: 8.7e-12)
TOL_X = 6e-11       # 10 x 5.26e-12 (n = 4097, m = 129).  Both figures are the same with 2 .. 16 BLAS threads (5.1e-12, 3.2e-12
                    # with one)
ROWREL_FLOOR = 1e-3

SIGMA2 = 0.1
SIGMA2_NEXT = 0.37

Case = collections.namedtuple("Case", "path kind n m d chunk variational model_only engine_env", defaults=(0, False, False, False))


def _d(kind):
    return 2 if kind == "iso" else 3


def _cases():
    out = []

    def add(path, kind, n, m, d=None, **kw):
        c = Case(path, kind, n, m, _d(kind) if d is None else d, **kw)
        if c not in out:
            out.append(c)

    # small.hip: 64-row blocks
    for n in (1, 63, 64, 65, 200):
        add("small", "iso", n, 17)
    for m in (1, 16, 64):
        add("small", "iso", 200, m)
    add("small", "iso", 64 * 512 + 65, 16, 2)
    add("small", "iso", 700, 17, chunk=256)
    for kind in ("fat_het", "fat_proj_het", "fat_ms"):
        add("small", kind, 200, 17)
    add("small", "iso", 200, 17, variational=True)
    add("small", "iso", 200, 17, model_only=True)
    # mid.hip, one tile: 64-row blocks
    for m in (65, 128):
        for n in (63, 64, 65, 129, 800):
            add("mid", "iso", n, m)
    add("mid", "iso", 64 * 256 + 65, 65)
    add("mid", "iso", 700, 65, chunk=256)
    for kind in ("fat_het", "fat_proj_het"):
        add("mid", kind, 800, 65)
    add("mid", "iso", 800, 65, variational=True)
    add("mid", "iso", 800, 65, model_only=True)
    # mid.hip, two tiles: 32-row blocks
    for m in (129, 256):
        for n in (31, 32, 33, 800):
            add("mid", "iso", n, m)
    for n in (4096, 4097, 32 * 256 + 33):
        add("mid", "iso", n, 129)
    for kind in ("fat_het", "fat_proj_het"):
        add("mid", kind, 800, 129)
    add("mid", "iso", 800, 129, variational=True)
    add("mid", "iso", 800, 129, model_only=True)
    # the engine and rowops.hip
    for n in (127, 128, 129, 255, 256, 257, 800):
        add("engine", "iso", n, 257)
    for m in (385, 641, 1100):
        add("engine", "iso", 800, m)
    add("engine", "iso", 700, 257, chunk=256)
    add("engine", "iso", 300, 257, chunk=128)
    for m in (50, 129):
        add("engine", "iso", 300, m, engine_env=True)
    for kind in ("fat_het", "fat_proj_het", "fat_ms"):
        add("engine", kind, 800, 257)
    add("engine", "iso", 800, 257, variational=True)
    add("engine", "iso", 800, 257, model_only=True)
    return out


def _case_id(c):
    s = "%s-%s-n%d-m%d" % (c.path, c.kind, c.n, c.m)
    if c.chunk:
        s += "-c%d" % c.chunk
    return s + ("-var" if c.variational else "") + ("-model" if c.model_only else "") + ("-forced" if c.engine_env else "")


CASES = _cases()


def _matrices_compared(c):
    """W and X are compared with the oracle on every case but n = 1, where the oracle itself misses the bound (asserted in
    test_oracle_against_the_80_bit_restatement): with one training point T, t t^T and Um^T diag(v) Um cancel to 1e-12 of
    their own size, and what is left of W and X is rounding noise in any evaluation order."""
    return c.n > 1


# ---- the CPU half: data, the oracle's operands, their 80-bit restatement ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(kind, n, m, d):
    return factor_case(kind, n, m, d)


@functools.lru_cache(maxsize=6)
def _model(kind, n, m, d, variational, sigma2):
    X, y, Z, args, ok, cond = _data(kind, n, m, d)
    return O._fast_model(ok, Z, X, sigma2, variational)


@functools.lru_cache(maxsize=6)
def _reference(kind, n, m, d, variational=False, model_only=False, sigma2=SIGMA2):
    """The oracle's operands of one evaluation: dict(r, is_, v, w, t, W (upper triangle valid), X)."""
    X, y, Z, args, ok, cond = _data(kind, n, m, d)
    mp = _model(kind, n, m, d, variational, sigma2)
    model = mp["model"]
    tr = O.deriv_trained_calc(mp["cm"], y)
    if model_only:
        ht = O.model_prepare_hyper(mp["cm"])
        return dict(r=model["r_vec"], is_=model["is_vec"], v=O.cm_calc_v1_vec(mp["cm"]), w=np.zeros(n), t=None,
                    W=ht["w_mat"], X=ht["x_mat"])
    ht = O.trained_prepare_hyper(tr, us=mp["us"], u1tu1=mp["u1tu1"])
    return dict(r=model["r_vec"], is_=model["is_vec"], v=tr["v_vec"], w=tr["w_vec"], t=tr["coeffs"], W=ht["w_mat"], X=ht["x_mat"],
                dl_dsigma2=O.common_calc_log_evidence_sigma2(mp["cm"], tr["v_vec"]))


def _ref_of(c, sigma2=SIGMA2):
    return _reference(c.kind, c.n, c.m, c.d, c.variational, c.model_only, sigma2)


@functools.lru_cache(maxsize=2)
def _restatement(kind, n, m, d, variational):
    X, y, Z, args, ok, cond = _data(kind, n, m, d)
    mp = _model(kind, n, m, d, variational, SIGMA2)
    return longdouble_operands(oracle_km_full(ok, Z), mp["knm"], ok.sf2, y, SIGMA2, variational, O.CHOLESKY_JITTER)


def rowrel(got, ref):
    """max_i |got_i - ref_i| / max(|ref_i|, ROWREL_FLOOR max|ref|)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.maximum(np.abs(ref), ROWREL_FLOOR * np.max(np.abs(ref)))
    return float(np.max(np.abs(got - ref) / np.maximum(scale, 1e-300)))


class _Checks:
    """Runs every check of a case, records each figure (tests/margins.py) and asserts once at the end, so that the log of a
    failing case still holds all of its figures."""

    def __init__(self, label):
        self.label, self.bad = label, []

    def vec(self, what, got, ref, tol):
        try:
            M.check_vec(what, got, ref, tol)
        except AssertionError as e:
            self.bad.append(str(e))

    def rel(self, what, got, ref, tol):
        err = rowrel(got, ref)
        M._record(what, err, tol)
        if not err <= tol:
            i = int(np.argmax(np.abs(got - ref) / np.maximum(np.abs(ref), ROWREL_FLOOR * np.max(np.abs(ref)))))
            self.bad.append("%s: %.3e > %.1e at row %d of %d (got %r, ref %r)" % (what, err, tol, i, len(ref), got[i], ref[i]))

    def true(self, what, ok):
        if not ok:
            self.bad.append(what)

    def done(self):
        assert not self.bad, "%s: %s" % (self.label, "; ".join(self.bad))


def _check_rows(ck, got, ref, names=("r", "is", "v", "w", "t"), prefix=""):
    """Checks 1 and 2 on fetched vectors `got` = {name: array}"""
    for name in names:
        key = "is_" if name == "is" else name
        if ref[key] is None:
            continue
        tol = {"r": TOL_ROW, "is": TOL_ROW, "v": TOL_ROWVW, "w": TOL_ROWVW, "t": TOL_POST}[name]
        ck.true("%s has %d entries, expected %d" % (name, got[name].shape[0], ref[key].shape[0]), got[name].shape == ref[key].shape)
        ck.true("%s is not finite" % name, bool(np.all(np.isfinite(got[name]))))
        if np.max(np.abs(ref[key])) > 0:
            ck.vec(prefix + "row_" + name, got[name], ref[key], tol)
            if name in ("is", "v", "w"):
                ck.rel(prefix + "rowrel_" + name, got[name], ref[key], TOL_ROWREL)


def _measure_oracle(c):
    """The oracle's operands against their 80-bit restatement: {quantity: error}, recorded."""
    ref, ld = _ref_of(c), _restatement(c.kind, c.n, c.m, c.d, c.variational)
    vk, Wk, Xk = ("v1", "W1", "X1") if c.model_only else ("v", "W", "X")
    out = dict(row_r=M.relinf(ref["r"], ld["r"]), row_is=M.relinf(ref["is_"], ld["is_"]), row_v=M.relinf(ref["v"], ld[vk]),
               rowrel_is=rowrel(ref["is_"], ld["is_"]), rowrel_v=rowrel(ref["v"], ld[vk]),
               w_mat=M.relinf(np.triu(ref["W"]), np.triu(ld[Wk])), x_mat=M.relinf(ref["X"], ld[Xk]))
    if not c.model_only:
        out.update(row_w=M.relinf(ref["w"], ld["w"]), rowrel_w=rowrel(ref["w"], ld["w"]), row_t=M.relinf(ref["t"], ld["t"]))
    return out


ORACLE_BOUNDS = dict(row_r=TOL_ROW / 10, row_is=TOL_ROW / 10, row_v=TOL_ROWVW / 10, row_w=TOL_ROWVW / 10, row_t=TOL_POST / 10,
                     rowrel_is=TOL_ROWREL / 100, rowrel_v=TOL_ROWREL / 100, rowrel_w=TOL_ROWREL / 100, w_mat=TOL_W / 10,
                     x_mat=TOL_X / 10)


@pytest.mark.parametrize("key", sorted({(c.kind, c.n, c.m, c.d) for c in CASES}), ids=str)
def test_conditioning_of_every_case(key):
    """cond(K_m + jitter I) <= 1e5 from numpy.linalg.eigvalsh of the oracle's K_m, on the inducing points of the case itself"""
    kind, n, m, d = key
    X, y, Z, args, ok, cond = _data(kind, n, m, d)
    w = np.linalg.eigvalsh(oracle_km_full(ok, Z) + O.CHOLESKY_JITTER * np.eye(m))
    assert w[0] > 0 and w[-1] / w[0] <= 1e5 and cond <= 1e5, (key, w[0], w[-1], cond)


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_oracle_against_the_80_bit_restatement(c):
    """The reference of the device checks is itself within 1/10 of every bound of checks 1 and 4 and 1/100 of TOL_ROWREL.
    TOL_W, TOL_X and TOL_ROWREL are 10 x / 100 x the worst figure measured here, rounded up to one digit, so the worst cases
    pass with little to spare (9.76e-12 against 1e-11 for W at n = 4097, m = 129).  The oracle's figures depend on LAPACK's
    summation order: with 2 .. 16 BLAS threads they were the same to three digits, with one thread W of that case was
    5.1e-12.  If another BLAS build moves a figure past its tenth, the constant is re-derived from the new worst figure as
    above; it is not a device finding."""
    errs = _measure_oracle(c)
    if not _matrices_compared(c):
        assert errs["w_mat"] > TOL_W / 10 and errs["x_mat"] > TOL_X / 10, "the oracle holds the bound: compare W and X here too"
        del errs["w_mat"], errs["x_mat"]
    for what, e in errs.items():
        M._record("oracle_" + what, e, ORACLE_BOUNDS[what])
    bad = {k: e for k, e in errs.items() if not e <= ORACLE_BOUNDS[k]}
    assert not bad, (_case_id(c), bad, errs)


def test_one_wrong_row_hides_from_the_sums_but_not_from_the_row_check():
    """Power: one row of v off by 1e-6 of its own value.  dl/dsigma2 = -1/2 sum v moves by 1e-6 / n of itself and still
    passes TOL_DS2; the per-row check 2 sees 1e-6."""
    c = next(c for c in CASES if c.n == 64 * 512 + 65)
    ref = _ref_of(c)
    v = ref["v"].copy()
    i = int(np.argmin(np.abs(v - np.median(v))))      # a typical row
    v[i] *= 1.0 + 1e-6
    ds2 = -0.5 * float(np.sum(v))
    assert abs(ds2 - ref["dl_dsigma2"]) <= TOL_DS2 * abs(ref["dl_dsigma2"])
    assert rowrel(v, ref["v"]) > TOL_ROWREL
    assert rowrel(ref["v"], ref["v"]) == 0.0


# ---- the GPU half ---------------------------------------------------------------------------------------------------------
def _cov(kind):
    return gpr_amd.COV_SE_ISO if kind == "iso" else gpr_amd.COV_SE_FAT


def _problem(c, X, y):
    p = gpr_amd.Problem(_cov(c.kind), c.n, X.shape[0], c.d, c.m, chunk_rows=c.chunk)
    p.set_inputs(X)
    p.set_targets(y)
    p.set_timing(2)
    return p


def _fetch(p, names=("r", "is", "v", "w", "t")):
    return {k: p.debug_fetch(k) for k in names}


def _check_matrices(ck, p, c, ref):
    """Check 4"""
    W = p.debug_fetch_matrix("w_mat")
    ck.true("W is not finite", bool(np.all(np.isfinite(W))))
    asym = float(np.max(np.abs(W - W.T)) / max(np.max(np.abs(W)), 1e-300))
    M._record("w_mat_asym", asym, 1e-12)
    ck.true("W is asymmetric by %.3e of its largest entry" % asym, asym <= 1e-12)
    if not _matrices_compared(c):
        return
    ck.vec("w_mat", np.triu(W), np.triu(ref["W"]), TOL_W)
    if c.chunk == 0:
        ck.vec("x_mat", p.debug_fetch_matrix("x_rows", c.n), ref["X"], TOL_X)


@gpu
@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_row_operands_of_one_evaluation(c, monkeypatch):
    if c.engine_env:
        monkeypatch.setenv("GPRHIP_SMALL_PATH", "0")   # read when the problem is created
        monkeypatch.setenv("GPRHIP_MID_PATH", "0")
    X, y, Z, args, ok, cond = _data(c.kind, c.n, c.m, c.d)
    ref = _ref_of(c)
    p = _problem(c, X, y)
    try:
        p.eval(sigma2=SIGMA2, inducing=Z, variational=c.variational, model_only=c.model_only, **args)
        stages = set(p.last_timings())
        assert _taken(stages) == c.path, (_case_id(c), stages)
        ck = _Checks(_case_id(c))
        got = _fetch(p, ("r", "is", "v", "w") if c.model_only else ("r", "is", "v", "w", "t"))
        if c.model_only:
            ck.true("w of a model-only evaluation is not exactly zero", bool(np.all(got["w"] == 0.0)))
        _check_rows(ck, got, ref)
        _check_matrices(ck, p, c, ref)
        ck.done()
    finally:
        p.close()


BASE = {"small": Case("small", "iso", 200, 17, 2), "mid_one_tile": Case("mid", "iso", 800, 65, 2),
        "mid_two_tiles": Case("mid", "iso", 800, 129, 2), "engine": Case("engine", "iso", 800, 257, 2)}


@gpu
@pytest.mark.parametrize("name", sorted(BASE))
def test_row_operands_after_a_change_of_sigma2_alone(name):
    """eval(reuse_v=True, sigma2=s'): K_nm, V and r are kept -- r bit for bit -- and 1/s, v, w, t are those of s'."""
    c = BASE[name]
    X, y, Z, args, ok, cond = _data(c.kind, c.n, c.m, c.d)
    p = _problem(c, X, y)
    try:
        p.eval(sigma2=SIGMA2, inducing=Z, **args)
        assert _taken(set(p.last_timings())) == c.path
        r0 = p.debug_fetch("r")
        p.eval(sigma2=SIGMA2_NEXT, inducing=Z, reuse_v=True, **args)
        got = _fetch(p)
        ck = _Checks(name)
        ck.true("r changed under reuse_v", bool(np.array_equal(got["r"], r0)))
        _check_rows(ck, got, _ref_of(c, SIGMA2_NEXT), prefix="reuse_")
        ck.done()
    finally:
        p.close()


def _three_targets(X, y):
    s = X.sum(0)
    return np.asfortranarray(np.stack([y, np.cos(0.7 * s) + 0.05 * y, 0.3 * s - y], axis=1))


@gpu
@pytest.mark.parametrize("chunk", [0, 256], ids=["engine", "chunks"])
def test_row_operands_of_a_three_target_evaluation(chunk):
    """gprhip_eval_targets (the engine path by contract): v = v1 - mean_k w_k^2 with the oracle's per-column w_k; r and 1/s
    are those of a plain evaluation."""
    c = Case("engine", "iso", 700 if chunk else 800, 257, 2, chunk)
    X, y, Z, args, ok, cond = _data(c.kind, c.n, c.m, c.d)
    Y = _three_targets(X, y)
    mp = _model(c.kind, c.n, c.m, c.d, False, SIGMA2)
    w2 = np.mean([O.deriv_trained_calc(mp["cm"], np.ascontiguousarray(Y[:, k]))["w_vec"] ** 2 for k in range(3)], axis=0)
    ref = dict(r=mp["model"]["r_vec"], is_=mp["model"]["is_vec"], v=O.cm_calc_v1_vec(mp["cm"]) - w2)
    p = _problem(c, X, y)
    try:
        p.eval(sigma2=SIGMA2, inducing=Z, **args)
        plain = _fetch(p, ("r", "is"))
        p.set_targets_many(Y)
        p.eval_targets(sigma2=SIGMA2, inducing=Z, **args)
        stages = set(p.last_timings())
        assert _taken(stages) == "engine" and "p1_targets" in stages, stages
        got = _fetch(p, ("r", "is", "v"))
        ck = _Checks("targets-c%d" % chunk)
        ck.true("r differs from a plain evaluation's", bool(np.array_equal(got["r"], plain["r"])))
        ck.true("1/s differs from a plain evaluation's", bool(np.array_equal(got["is"], plain["is"])))
        _check_rows(ck, got, ref, names=("r", "is", "v"), prefix="targets_")
        ck.done()
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("m", [65, 129, 257])
def test_row_operands_of_every_shard(m, shards):
    """Shards of one device (gprhip_sharded_*): shard i holds the rows [row_lo, row_hi) of the oracle's vectors, and the shards
    cover every row exactly once."""
    c = Case("mid" if m <= 256 else "engine", "iso", 700, m, 2)
    X, y, Z, args, ok, cond = _data(c.kind, c.n, c.m, c.d)
    ref = _ref_of(c)
    ctx = gpr_amd.Context([0] * shards)
    sp = gpr_amd.ShardedDeviceProblem(ctx, _cov(c.kind), c.n, X.shape[0], c.d, c.m)
    try:
        sp.set_inputs(X)
        sp.set_targets(y)
        for i in range(shards):
            sp.problem(i).set_timing(2)
        sp.eval(sigma2=SIGMA2, inducing=Z, **args)
        ck = _Checks("shards-m%d-%d" % (m, shards))
        covered = np.zeros(c.n, dtype=int)
        for i in range(shards):
            _, lo, hi = sp.shard(i)
            covered[lo:hi] += 1
            q = sp.problem(i)
            assert _taken(set(q.last_timings())) == c.path, q.last_timings()
            part = dict(r=ref["r"][lo:hi], is_=ref["is_"][lo:hi], v=ref["v"][lo:hi], w=ref["w"][lo:hi], t=ref["t"])
            _check_rows(ck, _fetch(q), part, prefix="shard_")
        ck.true("the shards do not cover every row exactly once", bool(np.all(covered == 1)))
        ck.done()
    finally:
        sp.close()
        ctx.close()
