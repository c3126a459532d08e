"""CPU half of tests/test_gpu_exchange.py: the packed layout of the exchange buffers (the library's device-free
gprhip_exchange_len / gprhip_exchange_offset) and two conditions on the reference tests/exchange_ref.py alone, over the case
list of the GPU module, with operands formed in float64 numpy on the oracle's covariances:
  (a) plain float64 numpy in three summation orders (forward, reversed rows, 64-row blocks summed pairwise) lies within the
      bound at every entry;
  (b) the bound sees one row: the contribution of the row with the median |is_r| sum_c V_rc^2 is larger than the bound, so
      dropping or doubling it leaves the reference by more than the bound -- at every entry of B~, G~, c~ and the sum E row
      in which the row has a share (it adds at least the n-th part of the entry's value: the covariance is local, and a row
      far from an inducing point adds 1e-45 of an entry to that column) and every tail scalar that sums over rows, at the
      largest-n case of each path.
tests/staged_double.py's buffers (Cov_se_iso) lie within the same bound.  Figures: profiles/exchange_margins.txt.
"""
import numpy as np
import pytest
import scipy.linalg as sl

from oracle import fitc_oracle as O
from tests import exchange_ref as R
from tests import margins as M
from tests.staged_double import StagedDouble
from tests.test_gpu_exchange import CASES, PER_PATH, SIGMA2, case_id, hypers, layout_for
from tests.util import oracle_km_full


@pytest.mark.parametrize("m", [1, 127, 128, 129, 256, 257, 384, 385])
def test_layout(m):
    from gpr_amd import _lib
    lib = _lib.load()
    mp = -(-m // 128) * 128
    nt = mp // 128
    packed = nt * (nt + 1) // 2 * 128 * 128
    seen = np.zeros(packed, dtype=int)
    for r in range(mp):
        for c in range(mp):
            o = lib.gprhip_exchange_offset(m, r, c)
            if r // 128 <= c // 128:
                assert 0 <= o < packed, (r, c, o)
                seen[o] += 1
            else:
                assert o == -1, (r, c, o)
    assert np.all(seen == 1)
    for r, c in ((-1, 0), (0, -1), (mp, 0), (0, mp), (mp, mp), (-1, -1), (mp - 1, mp), (2 ** 30, 0)):
        assert lib.gprhip_exchange_offset(m, r, c) == -1, (r, c)
    assert lib.gprhip_exchange_offset(0, 0, 0) == -1
    for D, d in ((2, 2), (5, 3)):
        assert lib.gprhip_exchange_len(0, D, d, m, 1) == packed + mp + R.A1_TAIL
        assert lib.gprhip_exchange_len(1, D, d, m, 1) == packed + mp + R.A1_TAIL
        assert lib.gprhip_exchange_len(0, D, d, m, 2) == packed + (d + 1) * mp + R.A2_TAIL
        assert lib.gprhip_exchange_len(1, D, d, m, 2) == packed + (d + 1 + D + d) * mp + D * d + R.A2_TAIL
    for bad in ((2, 2, 2, m, 1), (0, 0, 2, m, 1), (0, 2, 0, m, 2), (0, 2, 2, 0, 1), (0, 2, 2, m, 0), (0, 2, 2, m, 3), (-1, 2, 2, m, 1)):
        assert lib.gprhip_exchange_len(*bad) == 0, bad


def host_operands(c):
    """The operands of one shard in float64 numpy (the algebra of tests/staged_double.py, any covariance of the oracle)"""
    X, y, Z, hyp, refkw = hypers(c)
    if c.kind == "iso":
        ok = O.SeIsoKernel(hyp["log_ell"], c.log_sf2)
    else:
        ok = O.SeFatKernel(c.d, c.log_sf2, hyp.get("tproj"), hyp.get("log_hetero_skedasticity"), hyp.get("log_multiscales_m05"))
    m, n = c.m, c.n
    K, _ = O.spec_calc_shared_cross(ok, X, Z)
    Ui = sl.solve_triangular(np.linalg.cholesky(oracle_km_full(ok, Z) + O.CHOLESKY_JITTER * np.eye(m)).T, np.eye(m))
    V = K @ Ui
    r = ok.sf2 - np.sum(V * V, axis=1)
    is_ = 1.0 / (r + SIGMA2)
    yy = np.zeros(n) if c.model_only else y
    Ri = sl.solve_triangular(np.linalg.cholesky(np.eye(m) + (V * is_[:, None]).T @ V).T, np.eye(m))
    b = Ri.T @ (V.T @ (is_ * yy))
    tt = Ri @ b
    Q = V @ Ri
    res = yy - Q @ b
    w = is_ * res
    q = is_ * np.sum(Q * Q, axis=1)
    v1 = is_ * (2.0 - is_ * r - q) if c.variational else is_ * (1.0 - q)
    v = v1 - w * w
    Xm = (is_[:, None] * (Q @ Ri.T) - v[:, None] * V - np.outer(w, tt)) @ Ui.T
    ops = dict(inputs=X, Z=Z, y=None if c.model_only else y, uinv=np.triu(Ui), r=r, is_=is_, v=v, w=w, X=Xm)
    return ops, dict(K=K, V=V, yy=yy), refkw


def _blocks(n, order):
    idx = np.arange(n) if order != "reversed" else np.arange(n)[::-1]
    return [idx[i:i + 64] for i in range(0, n, 64)]


def _sum(parts, order):
    """forward / reversed: the blocks one after the other; pairwise: a tree over the blocks"""
    parts = list(parts)
    if order != "pairwise":
        acc = parts[0]
        for p in parts[1:]:
            acc = acc + p
        return acc
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def float64_buffers(lay, ops, aux, c, refkw, order):
    """Both buffers in plain float64, the rows added block by block in the given order (within a block: numpy's own)"""
    m, mp, d = lay["m"], lay["mp"], lay["d"]
    K, V, yy = aux["K"], aux["V"], aux["yy"]
    X, Z = ops["inputs"], ops["Z"]
    tp = refkw["tproj"]
    P = X if tp is None else tp.T @ X
    is_, r, v, w, Xm = ops["is_"], ops["r"], ops["v"], ops["w"], ops["X"]
    E = Xm * K
    blocks = _blocks(K.shape[0], order)
    S = lambda f: _sum([f(b) for b in blocks], order)      # noqa: E731
    b1, b2 = np.zeros(lay["len1"]), np.zeros(lay["len2"])
    rr, cc = np.nonzero(lay["off"] >= 0)
    keep = (rr < m) & (cc < m) & (rr <= cc)
    rr, cc = rr[keep], cc[keep]
    pos = lay["off"][rr, cc]
    b1[pos] = S(lambda b: (V[b] * is_[b, None]).T @ V[b])[rr, cc]
    b2[pos] = S(lambda b: (V[b] * v[b, None]).T @ V[b])[rr, cc]
    b1[lay["c1"]:lay["c1"] + m] = S(lambda b: V[b].T @ (is_[b] * yy[b]))
    t1, t2 = lay["tail1"], lay["tail2"]
    b1[t1 + R.A1_SUMLOGS] = S(lambda b: np.sum(np.log(r[b] + SIGMA2)))
    b1[t1 + R.A1_ISY2] = S(lambda b: np.sum(is_[b] * yy[b] * yy[b]))
    b1[t1 + R.A1_ISR] = S(lambda b: np.sum(is_[b] * r[b]))
    b2[t2 + R.A2_SUMV] = S(lambda b: np.sum(v[b]))
    b2[t2 + R.A2_SUMIS] = S(lambda b: np.sum(is_[b]))
    b2[t2 + R.A2_WRES] = S(lambda b: np.sum(w[b] * (w[b] / is_[b])))
    b2[t2 + R.A2_SUMV1] = S(lambda b: np.sum(v[b] + w[b] * w[b]))
    rows = [S(lambda b: E[b].sum(0))[None, :], S(lambda b: P[:, b] @ E[b])]
    if tp is not None:
        rows.append(S(lambda b: X[:, b] @ E[b]))
    ms = None if refkw["log_ms"] is None else np.exp(refkw["log_ms"]) + 0.5
    if ms is not None:
        rows.append(S(lambda b: (P[:, b] * P[:, b]) @ E[b]))
    col = np.vstack(rows)
    b2[lay["col"]:lay["proj"]].reshape(lay["col_rows"], mp)[:col.shape[0], :m] = col
    b2[t2 + R.A2_SUME] = S(lambda b: np.sum(E[b]))
    if c.kind == "iso":
        dist = sum((P[k][:, None] - Z[k][None, :]) ** 2 for k in range(d))
        b2[t2 + R.A2_SUMED] = S(lambda b: np.sum(E[b] * dist[b]))
    if tp is not None:
        if ms is None:
            es = E.sum(1)
            b2[lay["proj"]:t2] = S(lambda b: (X[:, b] * es[b][None, :]) @ P[:, b].T).reshape(-1)
        else:
            es2 = E @ (1.0 / ms).T
            b2[lay["proj"]:t2] = S(lambda b: X[:, b] @ (P[:, b].T * es2[b])).reshape(-1)
    return b1, b2


def _record(prefix, c, got1, got2, ref, bad):
    for which, got in ((1, got1), (2, got2)):
        for name, (worst, pos) in R.ratios(got, ref["ref%d" % which], ref["bound%d" % which], ref["has%d" % which],
                                          ref["cls%d" % which]).items():
            M._record("%sex%d_%s" % (prefix, which, name), worst, 1.0, pos=pos)
            if not worst <= 1.0:
                bad.append("%s exchange %d %s: %.3g x its bound at %d" % (prefix, which, name, worst, pos))


LARGEST = {}
for _c in CASES:
    if _c.kind == "iso" and (_c.path not in LARGEST or _c.n > LARGEST[_c.path].n):
        LARGEST[_c.path] = _c


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_reference_conditions(c):
    """Condition (a) on every case, condition (b) on the largest-n case of each path"""
    ops, aux, refkw = host_operands(c)
    X = ops["inputs"]
    lay = layout_for(c, X)
    M.note(path=c.path, case=case_id(c))
    ref = R.reference(lay, ops, **refkw)
    bad = []
    for order in ("forward", "reversed", "pairwise"):
        b1, b2 = float64_buffers(lay, ops, aux, c, refkw, order)
        _record("host_%s_" % order, c, b1, b2, ref, bad)
        # the padding of the reference itself
        assert np.all(ref["ref1"][ref["cls1"] == R._CLS["pad"]] == 0) and np.all(ref["ref2"][ref["cls2"] == R._CLS["pad"]] == 0)
    if c == LARGEST.get(c.path):
        bad += _one_row(c, lay, ops, ref)
    assert not bad, (case_id(c), bad)


def _one_row(c, lay, ops, ref):
    """Condition (b): the median row's own contribution to every entry, over the entry's bound (the smallest ratio per class
    is recorded; it must exceed 1)"""
    LD = R.LD
    V, n, m = ref["V"], ref["n"], c.m
    is_, r, v, w = (np.asarray(ops[k], LD) for k in ("is_", "r", "v", "w"))
    y = np.zeros(n, LD) if ops["y"] is None else np.asarray(ops["y"], LD)
    score = np.asarray(np.abs(is_) * (V * V).sum(1), np.float64)
    i = int(np.argsort(score)[n // 2])
    rr, cc = np.nonzero(lay["off"] >= 0)
    keep = (rr < m) & (cc < m) & (rr <= cc)
    rr, cc = rr[keep], cc[keep]
    pos = lay["off"][rr, cc]
    outer = np.abs(V[i][rr] * V[i][cc])
    t1, t2, c1 = lay["tail1"], lay["tail2"], lay["c1"]
    s = 1 / is_[i]
    E_i = ref["E"][i]
    out = []
    contrib = [("B", ref["bound1"][pos], np.abs(is_[i]) * outer), ("G", ref["bound2"][pos], np.abs(v[i]) * outer),
               ("c", ref["bound1"][c1:c1 + m], np.abs(V[i] * is_[i] * y[i])),
               ("sumlogs", ref["bound1"][t1 + R.A1_SUMLOGS], np.abs(np.log(r[i] + LD(SIGMA2)))),
               ("isy2", ref["bound1"][t1 + R.A1_ISY2], np.abs(is_[i] * y[i] * y[i])),
               ("isr", ref["bound1"][t1 + R.A1_ISR], np.abs(is_[i] * r[i])),
               ("sumv", ref["bound2"][t2 + R.A2_SUMV], np.abs(v[i])), ("sumis", ref["bound2"][t2 + R.A2_SUMIS], np.abs(is_[i])),
               ("wres", ref["bound2"][t2 + R.A2_WRES], w[i] * w[i] * s), ("sumv1", ref["bound2"][t2 + R.A2_SUMV1], np.abs(v[i] + w[i] * w[i])),
               ("colE", ref["bound2"][lay["col"]:lay["col"] + m], np.abs(E_i)),
               ("sumE", ref["bound2"][t2 + R.A2_SUME], np.abs(E_i.sum()))]
    vals = dict(B=ref["ref1"][pos], G=ref["ref2"][pos], c=ref["ref1"][c1:c1 + m], colE=ref["ref2"][lay["col"]:lay["col"] + m])
    for name, bound, delta in contrib:
        delta, bound = np.atleast_1d(np.asarray(delta, np.float64)), np.atleast_1d(np.asarray(bound, np.float64))
        # the entries this row has a share in: with a local covariance a row far from an inducing point adds 1e-45 of an
        # entry to its column, which no bound can see; an entry counts where the row adds at least the n-th part of its value
        share = delta >= np.abs(np.asarray(vals[name], np.float64)) / n if name in vals else np.ones(delta.shape, bool)
        share &= delta > 0
        if not share.any():
            out.append("row %d has a share in no entry of %s" % (i, name))
            continue
        if name in vals:   # how many entries the filter leaves: recorded beside the ratio (profiles/exchange_margins.txt)
            M._record("one_row_share_" + name, 1.0 - float(share.mean()), 1.0, row=i, entries=int(share.sum()), of=int(share.size))
        ratio = float(np.min(delta[share] / np.maximum(bound[share], 1e-300)))
        M._record("one_row_" + name, 1.0 / max(ratio, 1e-300), 1.0, row=i)
        if not ratio > 1.0:
            out.append("one row (%d) moves %s by only %.3g x the bound" % (i, name, ratio))
    return out


@pytest.mark.parametrize("name", sorted(PER_PATH))
def test_the_staged_double_fills_the_devices_layout(name):
    """tests/staged_double.py's two buffers against the reference formed from ITS operands, within the same bound"""
    c = PER_PATH[name]
    X, y, Z, hyp, refkw = hypers(c)
    lay = layout_for(c, X)
    sd = StagedDouble(lambda le, lsf, tp: O.SeIsoKernel(le, lsf), c.n, c.d, c.d, c.m)
    sd.set_inputs(X)
    sd.set_targets(y)
    a1, a2 = np.full(sd.ar1_len(), 1e300), np.full(sd.ar2_len(), 1e300)
    assert (sd.ar1_len(), sd.ar2_len()) == (lay["len1"], lay["len2"])
    kw = {k: hyp[k] for k in ("log_ell", "log_sf2", "sigma2", "inducing")}
    sd.eval_pass1(a1.ctypes.data, c.n, **kw)
    sd.eval_pass2(a1.ctypes.data, a2.ctypes.data)
    ops = dict(inputs=X, Z=Z, y=y, uinv=np.triu(sd.Ui), r=sd.r, is_=sd.is_, v=sd.v, w=sd.w, X=sd.Xm)
    ref = R.reference(lay, ops, **refkw)
    M.note(path=c.path, case=case_id(c) + "-double")
    bad = []
    _record("double_", c, a1, a2, ref, bad)
    for which, got in ((1, a1), (2, a2)):
        zero = np.isin(ref["cls%d" % which], [R._CLS["pad"], R._CLS["unused"], R._CLS["below"]])
        assert np.all(got[zero] == 0.0)
    assert not bad, bad
