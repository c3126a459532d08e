"""Every entry of the two exchange buffers of ONE shard of a staged evaluation (eval_pass1 / eval_pass2), contracted in 80 bits
from given operands, with a running-error bound for every entry.  Imports nothing from the library or the oracle: the same
code serves the CPU and the GPU tests; the positions come from the library's device-free gprhip_exchange_len /
gprhip_exchange_offset, which the caller hands in as two callables (`layout`).  fp64 problems only: an fp32-bulk problem
stores V in float and needs another bound.

The layout (gprhip.hip: enums A1_* / A2_*, ex1_of / ex2_of; include/gprhip.h next to gprhip_exchange_offset), mp = m rounded
up to 128:
    exchange 1   [packed upper 128 x 128 tiles of B~_part = V^T diag(1/s) V | c~ (mp) | tail (A1_TAIL = 4)]
                 c~_c = sum_r V_rc is_r y_r;  tail = [sum log s, sum is y^2, sum is r, 0]
    exchange 2   [packed upper tiles of G~_part = V^T diag(v) V | column block (col_rows x mp) | Proj second term (dbig x d)
                 | tail (A2_TAIL = 8)],  col_rows = d + 1 (Cov_se_iso), d + 1 + D + d (Cov_se_fat; dbig = D there, 0 for iso)
                 column block rows, E = X .* K:  sum_r E_rc;  sum_r p_kr E_rc (d rows);  with a projection sum_r x_br E_rc
                 (D rows);  with multiscales sum_r p_kr^2 E_rc (d rows, DIRECTLY behind the rows before them: at row
                 d + 1 + D with a projection, d + 1 without, gprhip.hip:1675);  every further row zero
                 Proj second term (b, k) = sum_r x_br p_kr es_r [multiscales: sum_r x_br p_kr sum_c E_rc / ms_kc]; zero
                 without a projection
                 tail = [sum v, sum is, sum w res, sum v1, sum E, sum E dist, 0, 0], dist_rc = |p_r - z_c|^2 (not divided
                 by ell^2) [multiscales: sum_k (p_kr - z_kc)^2 / ms_kc + log ms_kc], res = w s, v1 = v + w^2
Entries of a tile with row or column >= m, of c~ and of the column block with column >= m, and the unused tail slots are +0.0.
Entries below the diagonal (r > c) of a DIAGONAL tile are not specified: no reader looks at them (class "below", no
reference).

The operands are the device's own of the same evaluation: U^-1 ("uinv"), the row vectors r, is, v, w (debug_fetch), X
("x_rows": single-chunk problems; without it the column block, the Proj term and the two E scalars get no reference), the
targets, the inputs (and tproj) and the hyper-parameters.
K is NOT fetched: "knm_rows" returns what the chunk builder rebuilds, for the first row chunk only, while small.hip and mid.hip
build their own K inside the row kernels.  K is formed here in 80 bits from direct differences (tests/posterior_ref.py::geometry)
and every K entry carries the weight 1 + kappa_rc of tests/hyper_grad_ref.py / tests/posterior_ref.py -- the LARGER of the
two forms, entry by entry: posterior_ref's with the coordinates as given (direct differences: small_pass1_body.inc,
mid.hip:629-635, cov_kernels.hip:44) and hyper_grad_ref's with the coordinates less the centroid of the inducing points (the
expansion of grad_mfma.hip:128-133, which pass 2 of the engine forms E with).
V = K U^-1 is not fetchable either: it is formed here from that K and the fetched U^-1, and its error is carried explicitly,
    eV_rc = (c + LK + C) u sum_{k <= c} |K_rk| (1 + kappa_rk) |Ui_kc|      (posterior_ref.chain; LK = d + 2 D, C = 8)
which holds the device's rounding of V (gamma_m sum |K| |Ui|) and of K.  It enters every entry that holds V to first order.

The bounds, u = 2^-53; gamma_L holds for any summation order (64-row blocks and sum_parts of small.hip:162-175, the two-tile
Gram launch pair mid.hip:1240-1251, the engine's k-slices with launch_sum_slices / launch_reduce_rows gprhip.hip:953-958, and
the caller's sum over shards need no model).  FIRST = 1.01 for the second-order terms:
    tiles     FIRST (sum_r |a_r| (eV_rc |V_rc'| + |V_rc| eV_rc') + (n + 3) u sum_r |a_r| |V_rc| |V_rc'|),   a = is or v
    c~        FIRST (sum_r |is_r y_r| eV_rc + (n + 4) u sum_r |is_r y_r| |V_rc|)                 (is y is rounded once)
    sum log s (n + 3) u sum |log s_r| + 2 n u      s = r + sigma2 is rounded before the logarithm: u absolute per term
    sum is y^2, sum is r, sum v, sum is:  (n + 3) u sum |term|
    sum w res (n + 4) u sum w^2 s              res is not kept: w = fl(is res), so res = w s (1 + u)
    sum v1    (n + 4) u sum (|v| + w^2)        v = fl(v1 - fl(w^2))
    column block, L = n + d + 3 D + C + 3:   L u sum_r coef_r |X_rc| |K_rc| (1 + kappa_rc),  coef = 1 (sum E);
              P~_kr + 2 |shift_k| (p_k rows: the raw sum of small_pass2_body.inc:190 and the shifted one with its correction
              shift_k sum E of mid.hip:737 and grad_mfma.hip:277 are both within it; P~ = sum_b |tproj_bk| |x_br| stands for
              |p_kr| with a projection, where the engine derives these rows from the x_b rows, launch_proj_inducing_grad);
              |x_br| (x_b rows);  (P~_kr + 2 |shift_k|)^2 (p_k^2 rows)
    sum E     the same with L + m;  sum E dist: (L + m) u sum |X| |K| (dist' (1 + kappa) + kappa / inv_ell2), dist' the
              distance with |log ms| in the place of log ms (tests/hyper_grad_ref.py, Log_ell)
              Cov_se_fat: the finish stage reads sum E dist for Log_ell alone (gprhip.hip:1627-1633), so the slot is not
              specified there and gets no reference
    Proj      without multiscales es_r is not added up from E but taken from the identity es = qd - v (sf2 - r) - w sb
              (small_pass2_body.inc:125, mid.hip:575, rowops.hip:124), qd = 1 - (v + w^2) s [variational: 2 - r / s -
              (v + w^2) s], sb = y - w s: the reference evaluates the same identity from the fetched rows, and the bound is
              (n + D + 4) u sum_r |x_br| P~_kr |es_r| + (m + 8) u sum_r |x_br| P~_kr (1 + |qd_r| + |v_r| (sf2 - r_r) + |w_r sb_r|)
              -- the identity's own roundings as tests/hyper_grad_ref.py counts them (two sums over m, six roundings) and two
              more for qd recovered from v.  With multiscales: L u sum_rc |x_br| P~_kr |X_rc| |K_rc| (1 + kappa_rc) / ms_kc.
"""
import numpy as np

from tests.posterior_ref import C, ETA, LD, U, _ld, geometry

FIRST = 1.01
# slots of the two scalar tails: the enums A1_* / A2_* of gprhip.hip
A1_SUMLOGS, A1_ISY2, A1_ISR, A1_UNUSED, A1_TAIL = 0, 1, 2, (3,), 4
A2_SUMV, A2_SUMIS, A2_WRES, A2_SUMV1, A2_SUME, A2_SUMED, A2_UNUSED, A2_TAIL = 0, 1, 2, 3, 4, 5, (6, 7), 8
TILE = 128

CLASSES = ("tile", "below", "c", "tail", "col", "proj", "pad", "unused")
_CLS = {k: i for i, k in enumerate(CLASSES)}


def layout(exchange_len, exchange_offset, fat, D, d, m):
    """Positions of both buffers.  exchange_len(cov_kind, D, d, m, which), exchange_offset(m, r, c): the library's."""
    mp = -(-m // TILE) * TILE
    kind = 1 if fat else 0
    len1, len2 = int(exchange_len(kind, D, d, m, 1)), int(exchange_len(kind, D, d, m, 2))
    packed = len1 - mp - A1_TAIL
    dbig = D if fat else 0
    col_rows = d + 1 + dbig + (d if fat else 0)
    assert len2 == packed + col_rows * mp + dbig * d + A2_TAIL, (len2, packed, col_rows, dbig)
    off = np.full((mp, mp), -1, dtype=np.int64)
    for r in range(mp):
        for c in range(r // TILE * TILE, mp):
            off[r, c] = exchange_offset(m, r, c)
    return dict(m=m, mp=mp, d=d, D=D, fat=fat, len1=len1, len2=len2, packed=packed, dbig=dbig, col_rows=col_rows, off=off,
                c1=packed, tail1=packed + mp, col=packed, proj=packed + col_rows * mp, tail2=packed + col_rows * mp + dbig * d)


def _tile_classes(lay, cls):
    m, mp, off = lay["m"], lay["mp"], lay["off"]
    rr, cc = np.nonzero(off >= 0)
    pos = off[rr, cc]
    kind = np.where((rr >= m) | (cc >= m), _CLS["pad"], np.where(rr > cc, _CLS["below"], _CLS["tile"]))
    cls[pos] = kind
    return rr, cc, pos


def classes(lay, has_proj, has_ms):
    """(cls1, cls2): the class of every entry of the two buffers as indices into CLASSES"""
    m, mp, d = lay["m"], lay["mp"], lay["d"]
    cls1 = np.full(lay["len1"], -1, dtype=np.int64)
    cls2 = np.full(lay["len2"], -1, dtype=np.int64)
    _tile_classes(lay, cls1)
    _tile_classes(lay, cls2)
    cls1[lay["c1"]:lay["c1"] + mp] = np.where(np.arange(mp) < m, _CLS["c"], _CLS["pad"])
    cls1[lay["tail1"]:] = _CLS["tail"]
    cls1[lay["tail1"] + np.array(A1_UNUSED)] = _CLS["unused"]
    live_rows = 1 + d + (lay["D"] if has_proj else 0) + (d if has_ms else 0)
    col = cls2[lay["col"]:lay["proj"]].reshape(lay["col_rows"], mp)
    col[:] = _CLS["pad"]
    col[:live_rows, :m] = _CLS["col"]
    cls2[lay["proj"]:lay["tail2"]] = _CLS["proj"] if has_proj else _CLS["pad"]
    cls2[lay["tail2"]:] = _CLS["tail"]
    cls2[lay["tail2"] + np.array(A2_UNUSED)] = _CLS["unused"]
    assert cls1.min() >= 0 and cls2.min() >= 0
    return cls1, cls2


def reference(lay, ops, *, iso, log_sf2, sigma2, log_ell=0.0, tproj=None, log_ms=None, variational=False):
    """ops: dict(inputs D x n (d x n without a projection), Z d x m, y (n) or None (model only), uinv m x m upper, r, is_, v, w
    (n each; v, w None: exchange 1 only), X n x m or None).
    Returns dict(ref1, ref2 longdouble; bound1, bound2 float64; has1, has2 bool: entries with a reference; cls1, cls2)."""
    assert np.finfo(LD).eps < 1e-18, "numpy longdouble is not an extended type here"
    m, mp, d = lay["m"], lay["mp"], lay["d"]
    Xin, Z = _ld(ops["inputs"]), _ld(ops["Z"])
    n = Xin.shape[1]
    tp = _ld(tproj)
    has_proj, has_ms = tp is not None, log_ms is not None
    D = tp.shape[0] if has_proj else 0
    # (geometry also forms the covariance between its points: 256 rows at a time)
    gs = [geometry(Xin[:, i:i + 256], Z, iso=iso, log_sf2=log_sf2, log_ell=log_ell, tproj=tproj, log_ms=log_ms)
          for i in range(0, n, 256)]
    g = dict(K=np.vstack([q["K"] for q in gs]), wK=np.vstack([q["wK"] for q in gs]), P=np.hstack([q["P"] for q in gs]))
    K, P, sf2, LK = g["K"], g["P"], gs[0]["sf2"], gs[0]["LK"]
    ie2 = np.exp(LD(-2) * LD(log_ell)) if iso else LD(1)
    ms = np.exp(_ld(log_ms)) + LD(0.5) if has_ms else None
    shift = Z.mean(axis=1)
    Pt, Zt = P - shift[:, None], Z - shift[:, None]
    if ms is None:   # kappa less the centroid (tests/hyper_grad_ref.py), and the larger of the two forms
        kap_s = abs(LD(log_sf2)) + ((Pt * Pt).sum(0)[:, None] + (Zt * Zt).sum(0)[None, :]) * ie2
    else:
        kap_s = abs(LD(log_sf2)) + (2 * (Pt * Pt).T @ (1 / ms) + (2 * Zt * Zt / ms + np.abs(np.log(ms))).sum(0)[None, :])
    aK = np.abs(K).astype(np.float64)
    kap = np.maximum(np.asarray(g["wK"], np.float64) / np.maximum(aK, 1e-300) - 1.0, np.asarray(kap_s, np.float64))
    kap = np.where(aK > 0, kap, np.asarray(kap_s, np.float64))
    wK = aK * (1.0 + kap)
    Ui = np.triu(_ld(ops["uinv"]))
    aUi = np.abs(Ui).astype(np.float64)
    V = K @ Ui
    j1 = np.arange(1, m + 1, dtype=np.float64)[None, :]
    eV = (j1 + LK + C) * U * (wK @ aUi) + ETA * aUi.sum(0)[None, :]
    aV = np.abs(V).astype(np.float64)
    r_, is_ = _ld(ops["r"]), _ld(ops["is_"])
    y = np.zeros(n, LD) if ops.get("y") is None else _ld(ops["y"])
    cls1, cls2 = classes(lay, has_proj, has_ms)
    rr, cc = np.nonzero(lay["off"] >= 0)
    keep = (rr < m) & (cc < m) & (rr <= cc)
    rr, cc, pos = rr[keep], cc[keep], lay["off"][rr[keep], cc[keep]]

    def gram(a):
        al = _ld(a)
        aa = np.abs(al).astype(np.float64)
        val = V.T @ (V * al[:, None])
        cross = eV.T @ (aV * aa[:, None])
        bnd = FIRST * (cross + cross.T + (n + 3) * U * (aV.T @ (aV * aa[:, None])))
        return val[rr, cc], bnd[rr, cc]

    def vec(terms, extra=3):
        return terms.sum(), float((n + extra) * U * np.abs(terms).sum())

    ref1, bound1 = np.zeros(lay["len1"], LD), np.zeros(lay["len1"])
    ref1[pos], bound1[pos] = gram(is_)
    isy = is_ * y
    aisy = np.abs(isy).astype(np.float64)
    ref1[lay["c1"]:lay["c1"] + m] = V.T @ isy
    bound1[lay["c1"]:lay["c1"] + m] = FIRST * (eV.T @ aisy + (n + 4) * U * (aV.T @ aisy))
    t1 = lay["tail1"]
    logs = np.log(r_ + LD(sigma2))
    ref1[t1 + A1_SUMLOGS], bound1[t1 + A1_SUMLOGS] = vec(logs)
    bound1[t1 + A1_SUMLOGS] += 2 * n * U
    ref1[t1 + A1_ISY2], bound1[t1 + A1_ISY2] = vec(isy * y)
    ref1[t1 + A1_ISR], bound1[t1 + A1_ISR] = vec(is_ * r_)
    has1 = np.isin(cls1, [_CLS["tile"], _CLS["c"], _CLS["tail"]])
    out = dict(ref1=ref1, bound1=bound1, has1=has1, cls1=cls1, cls2=cls2, V=V, eV=eV, n=n)
    if ops.get("v") is None:
        return out

    v, w = _ld(ops["v"]), _ld(ops["w"])
    s = 1 / is_
    ref2, bound2 = np.zeros(lay["len2"], LD), np.zeros(lay["len2"])
    ref2[pos], bound2[pos] = gram(v)
    t2 = lay["tail2"]
    ref2[t2 + A2_SUMV], bound2[t2 + A2_SUMV] = vec(v)
    ref2[t2 + A2_SUMIS], bound2[t2 + A2_SUMIS] = vec(is_)
    ref2[t2 + A2_WRES], bound2[t2 + A2_WRES] = vec(w * w * s, 4)
    ref2[t2 + A2_SUMV1] = (v + w * w).sum()
    bound2[t2 + A2_SUMV1] = float((n + 4) * U * (np.abs(v) + w * w).sum())
    has2 = np.isin(cls2, [_CLS["tile"], _CLS["tail"]])
    if ops.get("X") is not None:
        X = _ld(ops["X"])
        E = X * K
        aEw = np.abs(X).astype(np.float64) * wK
        aEk = np.abs(X).astype(np.float64) * aK
        Pa = (np.abs(Xin) if tp is None else np.abs(tp).T @ np.abs(Xin)).astype(np.float64)     # d x n
        Pw = Pa + 2 * np.abs(shift).astype(np.float64)[:, None]
        L = n + d + 3 * D + C + 3
        rows_v = [E.sum(0)[None, :], P @ E]
        rows_b = [aEw.sum(0)[None, :], Pw @ aEw]
        if has_proj:
            rows_v.append(Xin @ E)
            rows_b.append(np.abs(Xin).astype(np.float64) @ aEw)
        if has_ms:
            rows_v.append((P * P) @ E)
            rows_b.append((Pw * Pw) @ aEw)
        cv, cb = np.vstack(rows_v), L * U * np.vstack(rows_b)
        live = cv.shape[0]
        colv = ref2[lay["col"]:lay["proj"]].reshape(lay["col_rows"], mp)
        colb = bound2[lay["col"]:lay["proj"]].reshape(lay["col_rows"], mp)
        colv[:live, :m], colb[:live, :m] = cv, cb
        dist, dabs = np.zeros((n, m), LD), np.zeros((n, m), LD)
        for k in range(d):
            df = P[k][:, None] - Z[k][None, :]
            if ms is None:
                dist += df * df
                dabs += df * df
            else:
                dist += df * (df / ms[k][None, :]) + np.log(ms[k][None, :])
                dabs += df * (df / ms[k][None, :]) + np.abs(np.log(ms[k][None, :]))
        ref2[t2 + A2_SUME], bound2[t2 + A2_SUME] = E.sum(), float((L + m) * U * aEw.sum())
        ref2[t2 + A2_SUMED] = (E * dist).sum()
        bound2[t2 + A2_SUMED] = float((L + m) * U * (aEk * (np.asarray(dabs, np.float64) * (1 + kap) + kap / float(ie2))).sum())
        out["E"] = E
        has2 |= cls2 == _CLS["col"]
        has2[t2 + A2_SUMED] = bool(iso)
        if has_proj:
            aX = np.abs(Xin).astype(np.float64)
            if ms is None:
                v1 = v + w * w
                qd = (2 - is_ * r_ - v1 * s) if variational else (1 - v1 * s)
                sb = y - w * s if ops.get("y") is not None else np.zeros(n, LD)
                es = qd - v * (sf2 - r_) - w * sb
                mag = (1 + np.abs(qd) + np.abs(v) * np.abs(sf2 - r_) + np.abs(w * sb)).astype(np.float64)
                pv = (Xin * es[None, :]) @ P.T
                pb = (n + D + 4) * U * ((aX * np.abs(es).astype(np.float64)[None, :]) @ Pa.T) \
                    + (m + 8) * U * ((aX * mag[None, :]) @ Pa.T)
            else:
                ims = (1 / ms).astype(np.float64)                       # d x m
                pv = Xin @ (P.T * (E @ (1 / ms).T))
                pb = L * U * (aX @ (Pa.T * (aEw @ ims.T)))
            ref2[lay["proj"]:lay["tail2"]] = np.asarray(pv).reshape(-1)           # (big-major: entry b * d + k)
            bound2[lay["proj"]:lay["tail2"]] = np.asarray(pb, np.float64).reshape(-1)
            has2 |= cls2 == _CLS["proj"]
    else:
        has2[t2 + A2_SUME] = has2[t2 + A2_SUMED] = False
    out.update(ref2=ref2, bound2=bound2, has2=has2)
    return out


def ratios(got, ref, bound, has, cls):
    """{class: (worst |got - ref| / bound over the class's entries with a reference, position)}"""
    err = np.abs(_ld(got) - ref).astype(np.float64)
    rat = np.where(has, err / np.maximum(bound, 1e-300), 0.0)
    rat = np.where(has & (err == 0), 0.0, rat)
    out = {}
    for name, i in _CLS.items():
        sel = has & (cls == i)
        if sel.any():
            j = int(np.argmax(np.where(sel, rat, -1.0)))
            out[name] = (float(rat[j]), j)
    return out
