"""The CPU half of tests/test_gpu_hyper_grad.py: the 80-bit reference of tests/hyper_grad_ref.py and its bound (L + C) u A are
pinned here, before any device is involved, on the operands W, X, v of the oracle:
  1. the reference reproduces the oracle's gradient, family by family (figures: profiles/hyper_grad_margins.txt, oracle_*);
  2. on every case of the GPU list, the oracle's float64 gradient (moments against the raw coordinates, direct differences) and a
     plain float64 numpy restatement of the form the device kernels use (centroid-shifted moments, expanded distances, the
     shift_k sum E correction, the host's assembly) are inside the bound -- A and C hold without a device;
  3. planted defects in that restatement miss the bound by at least 100 x on some entry, so the bound is not vacuous;
  4. headroom: A[theta] <= 1e6 max |g| of the family for every inducing entry, so the bound is ~1e-10 of the family's scale.
"""
import functools

import numpy as np
import pytest

from oracle import fitc_oracle as O
from tests import hyper_grad_ref as H
from tests import margins as M
from tests.test_gpu_hyper_grad import CASES, CHUNKED, SIGMA2, Case, _factor_case, case_id, data, host_key, reference_of

ORACLE_TOL = 1e-11      # of the family's largest entry: TOL_ROW / 10, what tests/test_gpu_row_operands.py asks of the oracle
HEADROOM = 1e6
POWER = 100.0


_key = host_key


@functools.lru_cache(maxsize=4)
def _oracle(key):
    """The oracle's operands and float64 gradient of a case: dict(W full, X, v, grad or None)"""
    c = key
    X, y, Z, args = data(c)
    ok = _factor_case(c.kind, c.n, c.m, c.d, c.D)[4]
    mp = O._fast_model(ok, Z, X, SIGMA2, c.variational)
    if c.model_only:
        ht = O.model_prepare_hyper(mp["cm"])
        grad = None
    else:
        tr = O.deriv_trained_calc(mp["cm"], y)
        ht = O.trained_prepare_hyper(tr, us=mp["us"], u1tu1=mp["u1tu1"])
        grad = O._fast_target(mp, y)["grad"]
    w = np.zeros(c.n) if c.model_only else tr["w_vec"]
    rows = dict(r=mp["model"]["r_vec"], is_=mp["model"]["is_vec"], w=w, y=None if c.model_only else y, variational=c.variational)
    return dict(W=O._upper_to_full(ht["w_mat"]), X=np.asarray(ht["x_mat"]), v=np.asarray(ht["v_vec"]), grad=grad,
                rows=rows if "tproj" in args else None)


def restate64(W, Xr, v, Xin, Z, *, iso, log_sf2, log_ell=0.0, tproj=None, log_hetero=None, form="shifted", defect=None,
              slab=64, k_entry=None):
    """The last stage of a gradient evaluation in plain float64 numpy, in the form the device adds it (no multiscales).
    "shifted": points and inducing points less the centroid of the inducing points, |p~|^2 + |z~|^2 - 2 S distances, the
    moments sum_r p~_kr E_rc + shift_k sum_r E_rc (grad_mfma.hip:128-138, :277); "raw": direct differences and moments
    against the coordinates as given (rowops.hip:281-293).  The K_m traces use direct differences (finalize.hip:174-185), the
    assembly is the host's (gprhip.hip:1606-1659).  defect: one of the planted errors of the power test."""
    d, m = Z.shape
    n = Xin.shape[1]
    P = Xin if tproj is None else tproj.T @ Xin
    ie2 = np.exp(-2.0 * log_ell) if iso else 1.0
    sf2 = np.exp(log_sf2)
    sh = Z.mean(axis=1) if form == "shifted" else np.zeros(d)
    Pt, Zt = P - sh[:, None], Z - sh[:, None]
    if form == "shifted":
        dist = np.maximum((Pt * Pt).sum(0)[:, None] + (Zt * Zt).sum(0)[None, :] - 2.0 * (Pt.T @ Zt), 0.0)
    else:
        dist = np.zeros((n, m))
        for k in range(d):
            dist += (P[k][:, None] - Z[k][None, :]) ** 2
    K = np.exp(log_sf2 - 0.5 * ie2 * dist)
    E = Xr * K
    if defect == "row":
        E[n // 3] = 0.0
    elif defect == "tile":       # the last 16-row tile of the first slab
        E[min(slab, n) - 16:min(slab, n)] = 0.0
    elif defect == "column":     # the last live column of the last 128-column block
        E[:, m - 1] = 0.0
    cs = E.sum(0)
    G = Pt @ E
    if defect != "no_shift":
        G = G + sh[:, None] * cs
    if tproj is not None:       # (grad_mfma.hip:336-344: the moments follow from those against the original inputs)
        Gb = Xin @ E
        G = tproj.T @ Gb
    sE, sED = E.sum(), (E * dist).sum()
    Dm = np.zeros((m, m))
    for k in range(d):
        Dm += (Z[k][:, None] - Z[k][None, :]) ** 2
    Km = np.exp(log_sf2 - 0.5 * ie2 * Dm)
    np.fill_diagonal(Km, sf2)
    Q = W * Km
    if defect == "k_entry":      # one entry of K_m
        Q[k_entry] *= 1.0 + 1e-9
    tr_wk, tr_wkd = Q.sum(), (Q * Dm).sum()
    if defect == "diag_twice":
        tr_wk += np.trace(Q)
    out = []
    if iso:
        out.append([0.5 * ie2 * tr_wkd - ie2 * sED])
    out.append([-0.5 * (sf2 * v.sum() - tr_wk) - sE])
    gi = np.empty((m, d))
    for k in range(d):
        gi[:, k] = ie2 * (Q * (Z[k][:, None] - Z[k][None, :])).sum(0) - ie2 * (G[k] - Z[k] * cs)
    out.append(gi.ravel())
    if tproj is not None:
        term1 = Gb @ Z.T                                   # [big][small] = sum_c z_small,c sum_r x_big,r E_rc
        term2 = Xin @ (P.T * E.sum(1)[:, None])
        out.append((-(term1 - term2)).ravel())
    if log_hetero is not None:
        out.append(0.5 * np.exp(log_hetero) * np.diag(W))
    return np.concatenate(out)


def _most_visible_km_entry(c, op, Z, args, ref):
    """(r, c) of the entry of K_m whose term sum_r W_rc K_rc (z_kr - z_kc) / ell^2 is the largest share of its gradient entry's
    bound: the place where a wrong K entry shows best"""
    d, m = Z.shape
    ie2 = np.exp(-2.0 * args.get("log_ell", 0.0)) if c.kind == "iso" else 1.0
    Dm = sum((Z[k][:, None] - Z[k][None, :]) ** 2 for k in range(d))
    Q = op["W"] * np.exp(args["log_sf2"] - 0.5 * ie2 * Dm)
    bound = ref["bound"][dict(ref["fams"])["inducing"]].reshape(m, d)
    share = np.max([np.abs(Q * (Z[k][:, None] - Z[k][None, :])) * ie2 / bound[:, k][None, :] for k in range(d)], axis=0)
    return np.unravel_index(int(np.argmax(share)), share.shape)


def _restate(c, op, X, Z, args, form, defect=None, k_entry=None):
    return restate64(k_entry=k_entry, W=op["W"], Xr=op["X"], v=op["v"], Xin=X, Z=Z, **_restate_kw(c, args, form, defect))


def _restate_kw(c, args, form, defect):
    return dict(iso=c.kind == "iso", log_sf2=args["log_sf2"],
                     log_ell=args.get("log_ell", 0.0), tproj=args.get("tproj"), log_hetero=args.get("log_hetero_skedasticity"),
                     form=form, defect=defect)


def _worst(got, ref):
    return max(r for r, _ in H.ratios(got, ref).values())


def _record_all(prefix, label, got, ref):
    for (name, sl) in ref["fams"]:
        r, at = H.ratios(got, ref)[name]
        M.record("%s.%s" % (prefix, name), r, 1.0, case=label, L=float(ref["L"][sl][0]), C=H.C)


ORACLE_CASES = [Case("", "iso", 200, 17, 2), Case("", "iso", 800, 65, 2), Case("", "iso", 300, 257, 3),
                Case("", "fat_het", 200, 17, 3), Case("", "fat_proj_het", 200, 17, 3, 5), Case("", "fat_proj_het", 300, 129, 5, 17),
                Case("", "fat_ms", 200, 17, 3), Case("", "fat_ms", 300, 129, 3), Case("", "fat_proj_ms", 200, 17, 3, 8), Case("", "iso", 200, 17, 2, variational=True),
                Case("", "iso", 300, 129, 3, variational=True)]


@pytest.mark.parametrize("c", ORACLE_CASES, ids=case_id)
def test_the_reference_reproduces_the_oracle(c):
    """Every family of the oracle's float64 gradient within ORACLE_TOL of the family's largest entry, and every entry inside
    the bound of the raw form, which is the oracle's own."""
    X, y, Z, args = data(c)
    op = _oracle(_key(c))
    ref = reference_of(c, op["W"], op["X"], op["v"], X, Z, args, op["rows"])
    g = ref["g"].astype(np.float64)
    bad = {}
    for name, sl in ref["fams"]:
        e = M.relinf(op["grad"][sl], g[sl])
        M.record("oracle_" + name, e, ORACLE_TOL, case=case_id(c))
        if not e <= ORACLE_TOL:
            bad[name] = e
    assert not bad, (case_id(c), bad)
    assert _worst(op["grad"], ref) <= 1.0, H.ratios(op["grad"], ref)


HOST_CASES = sorted({_key(c): c for c in CASES + CHUNKED}.items(), key=lambda kc: case_id(kc[1]))
FORMS = {}      # the forms the device cases of a key use: the headroom is asked of those
for _c in CASES + CHUNKED:
    FORMS.setdefault(_key(_c), set()).add(_c.form)


@pytest.mark.parametrize("key", [k for k, _ in HOST_CASES], ids=[case_id(c) for _, c in HOST_CASES])
def test_float64_restatements_obey_the_bound_and_the_bound_has_headroom(key):
    c = key
    X, y, Z, args = data(c)
    op = _oracle(key)
    raw = reference_of(c, op["W"], op["X"], op["v"], X, Z, args, op["rows"])
    label = case_id(c)
    bad = {}
    if op["grad"] is not None:
        _record_all("host_oracle", label, op["grad"], raw)
        if not _worst(op["grad"], raw) <= 1.0:
            bad["oracle"] = H.ratios(op["grad"], raw)
    if c.kind not in ("fat_ms", "fat_proj_ms"):
        for form in ("raw", "shifted", "shifted_once"):
            ref = raw if form == "raw" else reference_of(c._replace(form=form), op["W"], op["X"], op["v"], X, Z, args, op["rows"])
            got = _restate(c, op, X, Z, args, "raw" if form == "raw" else "shifted")
            _record_all("host_" + form, label, got, ref)
            if not _worst(got, ref) <= 1.0:
                bad[form] = H.ratios(got, ref)
            sl = dict(ref["fams"])["inducing"]
            head = float(np.max(ref["A"][sl]) / np.max(np.abs(ref["g"][sl])))
            M.record("headroom_%s.inducing" % form, head, HEADROOM, case=label)
            if form in FORMS[key] and not head <= HEADROOM:
                bad["headroom_" + form] = head
    assert not bad, (label, bad)


POWER_SHAPES = [Case("small", "iso", 200, 17, 3, offset=1e3), Case("mid", "iso", 800, 65, 3, offset=1e3),
                Case("engine", "iso", 200, 257, 3, offset=1e3)]
DEFECTS = ["row", "tile", "column", "no_shift", "diag_twice", "k_entry"]


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("c", POWER_SHAPES, ids=case_id)
def test_planted_defects_miss_the_bound_by_two_orders(c, defect):
    """One training row dropped; the last 16-row tile of a slab dropped; the last live column dropped; the shift_k sum E
    correction omitted (inputs offset by 1e3, there alone); the diagonal of W .* K'_m counted twice; one entry of K_m off by a relative 1e-9, where that shows best --
    each in the float64 restatement of the device's form, which without the defect is inside the bound."""
    if defect != "no_shift":
        c = c._replace(offset=0.0)
    X, y, Z, args = data(c)
    op = _oracle(_key(c))
    ref = reference_of(c._replace(form="shifted"), op["W"], op["X"], op["v"], X, Z, args, op["rows"])
    assert _worst(_restate(c, op, X, Z, args, "shifted"), ref) <= 1.0
    where = _most_visible_km_entry(c, op, Z, args, ref) if defect == "k_entry" else None
    miss = _worst(_restate(c, op, X, Z, args, "shifted", defect, where), ref)
    M.record("power_" + defect, miss, POWER, case=case_id(c))
    assert miss >= POWER, (case_id(c), defect, miss)


@pytest.mark.parametrize("defect", ["row", "tile", "column"])
def test_planted_defects_show_in_the_proj_family_too(defect):
    """The Proj entries carry the allowance for the row identity behind their second term (tests/hyper_grad_ref.py); it leaves
    the bound sharp enough: a dropped row, row tile or column misses it by at least 100 x in that family alone."""
    c = Case("engine", "fat_proj_het", 200, 257, 3, 16)
    X, y, Z, args = data(c)
    op = _oracle(_key(c))
    ref = reference_of(c, op["W"], op["X"], op["v"], X, Z, args, op["rows"])
    assert H.ratios(_restate(c, op, X, Z, args, "raw"), ref)["proj"][0] <= 1.0
    miss = H.ratios(_restate(c, op, X, Z, args, "raw", defect), ref)["proj"][0]
    M.record("power_proj_" + defect, miss, POWER, case=case_id(c))
    assert miss >= POWER, (defect, miss)
