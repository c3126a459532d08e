"""The gradient of the log evidence contracted in 80 bits from given operands W (m x m, full symmetric), X (n x m) and
v (n) -- the last stage of a gradient evaluation, and nothing before it -- with a running-error bound for every entry.
Imports nothing from the library or the oracle: the same code serves the CPU and the GPU tests.

    g[theta] = -1/2 v . diag K'_n(theta) + 1/2 tr(W K'_m(theta)) - tr(X^T K'_nm(theta))

in numpy.longdouble, with analytic K' formed from direct differences p_r - z_c (p = tproj^T x with a projection), in the
reference's Hyper.get_all order (tests/margins.py::families).  The covariances restated (oracle/fitc_oracle.py):
    Cov_se_iso   K_rc = sf2 exp(-|p_r - z_c|^2 / (2 ell^2)), K_m likewise, diagonal sf2
    Cov_se_fat   the same with ell = 1; heteroskedastic noise exp(log_het_c) on diag K_m
    multiscales  ms = exp(log_ms) + 1/2;  K_rc = sf2 exp(-1/2 sum_k [(p_kr - z_kc)^2 / ms_kc + log ms_kc]);
                 K_m off the diagonal with ms_kr + ms_kc - 1 in the place of ms_kc, diagonal sf2 exp(-1/2 sum_k log(2 ms_kc - 1))
With E = X .* K_nm, Q = W .* K_m (heteroskedastic noise not in Q), D the squared distances:
    Log_sf2          -1/2 sf2 sum v + 1/2 sum Q - sum E
    Log_ell          (1/2 sum_{r != c} Q_rc Dm_rc - sum E_rc Dn_rc) / ell^2
    inducing (c, k)  (sum_r Q_rc (z_kr - z_kc) [/ (ms_kr + ms_kc - 1)] - sum_r E_rc (p_kr - z_kc) [/ ms_kc]) / ell^2
    Proj (b, k)      sum_rc x_br E_rc (p_kr - z_kc) [/ ms_kc]
    Log_hetero i     1/2 exp(log_het_i) W_ii
    Log_ms (c, k)    f (sum_{r != c} Q_rc (i_rc - (z_kr - z_kc)^2 i_rc^2) - sum_r E_rc (1/ms_kc - ((p_kr - z_kc)/ms_kc)^2))
                     + 1/2 W_cc K_cc (1/2 - ms_kc) / (2 ms_kc - 1),   f = 1/2 (1/2 - ms_kc), i_rc = 1 / (ms_kr + ms_kc - 1)

The bound.  |g_dev[theta] - g[theta]| <= (L + C) u A[theta], u = 2^-53.
A[theta] is the sum of the absolute values of the products IN THE FORM THE KERNELS ADD THEM; each product that holds a
covariance entry carries the weight 1 + kappa_rc, kappa_rc = |log sf2| + (|p~_r|^2 + |z~_c|^2) / ell^2 (the argument is
log_sf2 + inv_ell2_05 dist, grad_mfma.hip:133, rowops.hip:286: its sum is rounded relative to |log sf2| too; ~: less the centroid
of the inducing points; multiscales: sum_k 2 (p~_kr^2 + z~_kc^2) / ms + |log ms|), because the argument of the exponential is
known to u kappa only: the expansion |p~|^2 + |z~|^2 - 2 S (grad_mfma.hip:128-133) has the absolute error (d + 2) u (|p~|^2 +
|z~|^2), times 1/(2 ell^2); direct differences (rowops.hip:281-286, small_pass2_body.inc:177-187, mid.hip:629-635, and the
builders of the K_m and K_nm that are read back) (d + 2) u |p - z|^2 / (2 ell^2), which is no more.  Per family and `form`:
    Log_sf2   1/2 sf2 sum |v| + 1/2 sum |Q| w + sum |E| w                    (gprhip.hip:1614)
    Log_ell   (1/2 sum |Q| (Dm w + kappa) + sum |E| (Dn w + kappa)) / ell^2    (grad_mfma.hip:138: E dist, dist itself to u kappa ell^2)
    inducing  m x m part sum_r |Q_rc| |z_kr - z_kc| w / ell^2 on every path (finalize.hip:179-181, mid.hip:914-921); n x m part
      "shifted" (grad_mfma.hip:148-150, :277; mid.hip:483-489, :737):  sum_r p~_kr E_rc, + shift_k sum_r E_rc, and on the host
                - z_kc sum_r E_rc (gprhip.hip:1633):  sum_r (|p~_kr| + |z~_kc|) |E_rc| w
                + (ceil(n / 64) + 3) (|shift_k| + |z_kc|) sum_r |E_rc| / (L + C) -- shift_k sum E is added slab by slab (grad_mfma.hip:277
                is inside a slab's write; 64 rows is the smallest slab, gprhip.hip:699-703), so the slabs' products and the
                additions of reduce_rows round numbers of the size |shift_k| sum_slab |sum E|, once per slab and not L times;
                3 for the host's product, its subtraction and the centroid; otherwise the two cancel to z~_kc sum E exactly.
                "shifted_once" (mid.hip:737: the correction is added once, after the workgroups' sums): 1 + 3 in the place of
                ceil(n / 64) + 3
      "raw"     (rowops.hip:288, small_pass2_body.inc:190; gprhip.hip:1633):  sum_r (|p_kr| + |z_kc|) |E_rc| w
      with a projection (grad_mfma.hip:285, :342; rowops.hip:290):  sum_b |tproj_bk| sum_r |x_br| |E_rc| w + |z_kc| sum_r |E_rc| w,
                which also bounds the moments against the projected points themselves; "shifted" adds 2 |shift_k| sum_r |E_rc| w
    Proj      sum_rc |x_br| |E_rc| (|p_kr| + |z_kc|) w [/ ms_kc]                (rowops.hip:552-557, gprhip.hip:1644-1652: unshifted)
              + (m + 6) / (L + C) sum_r |x_br| |p_kr| (|qd_r| + |v_r| (sf2 - r_r) + |w_r sb_r|)   (without multiscales)
              -- the row sums es_r = sum_c E_rc of the second term are not added up from E: pass 2 takes them from the identity
              es_r = qd_r - v_r (sf2 - r_r) - w_r sb_r (rowops.hip:124, small_pass2_body.inc:125, mid.hip:575), qd_r = is_r |Q'_r|^2,
              sb_r = Q'_r . b.  Its three terms cancel, so its rounding error has their size and not that of E: the two sums
              over m, gamma_m each, and 6 roundings (is s2, sf2 - r, its product with v, w sb, two subtractions).  The term
              needs the row vectors r, 1/s, w and the targets (`rows`), from which qd = 1 - (v + w^2) s [variational:
              2 - r / s - (v + w^2) s] and sb = y - w s follow.  It counts the identity's own roundings only; the identity
              itself holds for exact factors.  Where the covariances are tiny the allowance is many orders above the
              contraction's term, and the Proj entries of such a case see no defect of the accumulation.  With
              multiscales the row sums sum_c E_rc / ms_kc are added up from E (rowops.hip:386-393, :425-434,
              small_pass2_body.inc:207-224) and there is no allowance.
    Log_het   1/2 het_i |W_ii|                                                  (gprhip.hip:1659)
    Log_ms    |f| (sum_{r != c} |Q_rc| (i_rc + (z_kr - z_kc)^2 i_rc^2) w + sum_r |E_rc| (1/ms + (|p_kr| + |z_kc|)^2 / ms^2) w)
              + |1/2 W_cc K_cc (1/2 - ms) / (2 ms - 1)|                          (finalize.hip:279-282, rowops.hip:381-382, gprhip.hip:1672-1674)
L is the number of summands of the entry plus d, the length of the sums inside every distance (grad_mfma.hip:128, the
d-step product S; rowops.hip:282-285) (Higham's gamma_L, any order:
slabs, chunks, reduce_rows and the MFMA accumulation order need no model):  Log_sf2 nm + mm + n + d;  Log_ell nm + mm + d;
inducing n (D + 1) + m + d with a projection (tproj's D products per row), n + m + d without;  Proj 2 nm + d;  Log_het 1;
Log_ms 3 n + 2 m + 1 + d.
C = 12 roundings per term: exp_fast within 1 ulp = 2 u (exp_fast.h:7-8); 1/ell^2 = exp(-2 log ell) 2 u; the product and the sum
of the argument 2; X K 1; the difference or the shifted coordinate 1; its product with E 1; the host's scale 1, its 1/2 or
z sum E product 1, and the final subtraction 1.  W, X, v are exact inputs: both sides read the same doubles.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
C = 12


def _ld(a):
    return None if a is None else np.asarray(a, dtype=LD)


def families(iso, d, m, D=0, het=False, ms=False):
    """[(family, slice)] in Hyper.get_all order, as tests/margins.py::families"""
    out, pos = [], 0
    for name, cnt in ((("log_ell", 1),) if iso else ()) + (("log_sf2", 1), ("inducing", d * m)) + \
            ((("proj", D * d),) if D else ()) + ((("hetero", m),) if het else ()) + ((("multiscale", d * m),) if ms else ()):
        out.append((name, slice(pos, pos + cnt)))
        pos += cnt
    return out


def reference(W, X, v, inputs, Z, *, iso, log_sf2, log_ell=0.0, tproj=None, log_hetero=None, log_ms=None, form="raw", rows=None):
    """rows: dict(r, is_, w, y or None, variational) of the same evaluation, for the Proj family (see above).  inputs: D x n (d x n without a projection), Z: d x m, tproj: D x d.  Returns dict(g, A, L, bound, fams): longdouble g
    and float64 A, L, bound = (L + C) u A per entry."""
    assert np.finfo(LD).eps < 1e-18, "numpy longdouble is not an extended type here"
    assert form in ("raw", "shifted", "shifted_once")
    slabs = 1 if form == "shifted_once" else -(-np.shape(inputs)[1] // 64)
    if form == "shifted_once":
        form = "shifted"
    W, X, v, Xin, Z = _ld(W), _ld(X), _ld(v), _ld(inputs), _ld(Z)
    d, m = Z.shape
    n = Xin.shape[1]
    assert W.shape == (m, m) and X.shape == (n, m) and v.shape == (n,)
    tp = _ld(tproj)
    D = 0 if tp is None else tp.shape[0]
    P = Xin if tp is None else tp.T @ Xin                      # d x n
    ie2 = np.exp(LD(-2) * LD(log_ell)) if iso else LD(1)
    lsf = LD(log_sf2)
    sf2 = np.exp(lsf)
    ms = None if log_ms is None else np.exp(_ld(log_ms)) + LD(0.5)     # d x m
    shift = Z.mean(axis=1)
    Pt, Zt = P - shift[:, None], Z - shift[:, None]

    # ---- covariances from direct differences, and the weights 1 + kappa
    accn, accm = np.zeros((n, m), LD), np.zeros((m, m), LD)
    Dn, Dm = np.zeros((n, m), LD), np.zeros((m, m), LD)
    for k in range(d):
        dn = P[k][:, None] - Z[k][None, :]
        dm = Z[k][:, None] - Z[k][None, :]
        Dn += dn * dn
        Dm += dm * dm
        if ms is None:
            accn += dn * dn
            accm += dm * dm
        else:
            sc = ms[k][:, None] + ms[k][None, :] - LD(1)
            accn += dn * (dn / ms[k][None, :]) + np.log(ms[k][None, :])
            accm += dm * (dm / sc) + np.log(sc)
    K = np.exp(lsf - LD(0.5) * ie2 * accn)
    Km = np.exp(lsf - LD(0.5) * ie2 * accm)
    kdiag = np.full(m, sf2) if ms is None else np.exp(lsf - LD(0.5) * np.log(2 * ms - 1).sum(0))
    Km[np.diag_indices(m)] = kdiag
    if ms is None:
        kn = abs(lsf) + ((Pt * Pt).sum(0)[:, None] + (Zt * Zt).sum(0)[None, :]) * ie2
        km_ = abs(lsf) + ((Zt * Zt).sum(0)[:, None] + (Zt * Zt).sum(0)[None, :]) * ie2
    else:
        kn = abs(lsf) + (2 * (Pt * Pt).T @ (1 / ms) + (2 * Zt * Zt / ms + np.abs(np.log(ms))).sum(0)[None, :])
        isym = 1 / np.minimum(ms[:, :, None] + ms[:, None, :] - 1, LD(1e300))          # d x m x m
        km_ = abs(lsf) + sum(2 * (Zt[k] ** 2)[:, None] * isym[k] + 2 * (Zt[k] ** 2)[None, :] * isym[k]
                             + np.abs(np.log(ms[k][:, None] + ms[k][None, :] - 1)) for k in range(d))
    wn, wm = 1 + kn, 1 + km_
    E, Q = X * K, W * Km
    aE, aQ = np.abs(E), np.abs(Q)
    aEw, aQw = aE * wn, aQ * wm
    off = ~np.eye(m, dtype=bool)

    g, A, L = [], [], []

    def put(gv, av, lv):
        gv = np.atleast_1d(gv).ravel()
        g.append(gv)
        A.append(np.atleast_1d(av).ravel())
        L.append(np.full(gv.shape, float(lv)))

    if iso:
        put((LD(0.5) * (Q * Dm)[off].sum() - (E * Dn).sum()) * ie2,
            (LD(0.5) * (aQ * (Dm * ie2 * wm + km_))[off].sum() + (aE * (Dn * ie2 * wn + kn)).sum()), n * m + m * m + d)
    put(LD(-0.5) * sf2 * v.sum() + LD(0.5) * Q.sum() - E.sum(),
        LD(0.5) * sf2 * np.abs(v).sum() + LD(0.5) * aQw.sum() + aEw.sum(), n * m + m * m + n + d)

    # inducing (ind-major: entry c * d + k)
    Lind = n * (D + 1) + m + d if D else n + m + d
    gi, ai = np.zeros((m, d), LD), np.zeros((m, d), LD)
    F = np.zeros((n, d), LD)        # F_rk = sum_c E_rc (p_kr - z_kc) [/ ms_kc]   (Proj)
    FA = np.zeros((n, d), LD)
    colEa, colEw = aE.sum(0), aEw.sum(0)
    if D:
        bigw = np.abs(Xin) @ aEw     # D x m: sum_r |x_br| |E_rc| w
    for k in range(d):
        dn = P[k][:, None] - Z[k][None, :]
        dm = Z[k][:, None] - Z[k][None, :]
        imsn = LD(1) if ms is None else 1 / ms[k][None, :]
        imsm = LD(1) if ms is None else 1 / (ms[k][:, None] + ms[k][None, :] - 1)
        t_n = E * dn * imsn
        gi[:, k] = ((Q * dm * imsm)[:, :].sum(0) - t_n.sum(0)) * ie2
        F[:, k] = t_n.sum(1)
        FA[:, k] = (aEw * (np.abs(P[k])[:, None] + np.abs(Z[k])[None, :]) * imsn).sum(1)
        a_m = (aQw * np.abs(dm) * imsm).sum(0)
        if D:
            a_n = (np.abs(tp[:, k])[:, None] * bigw).sum(0) + np.abs(Z[k]) * colEw
            if form == "shifted":
                a_n = a_n + 2 * abs(shift[k]) * colEw
        elif form == "shifted":
            a_n = (aEw * (np.abs(Pt[k])[:, None] + np.abs(Zt[k])[None, :])).sum(0) \
                + (slabs + 3) * (abs(shift[k]) + np.abs(Z[k])) * colEa / (Lind + C)
        else:
            a_n = (aEw * (np.abs(P[k])[:, None] + np.abs(Z[k])[None, :])).sum(0)
        ai[:, k] = (a_m + a_n * (imsn.ravel() if ms is not None else 1)) * ie2
    put(gi, ai, Lind)
    if D:
        Lp = 2 * n * m + d
        ap = np.abs(Xin) @ FA
        if rows is not None and ms is None:
            r_, is_, w_ = _ld(rows["r"]), _ld(rows["is_"]), _ld(rows["w"])
            v1 = v + w_ * w_
            qd = (2 - is_ * r_ - v1 / is_) if rows.get("variational") else (1 - v1 / is_)
            sb = 0 if rows.get("y") is None else _ld(rows["y"]) - w_ / is_
            mag = np.abs(qd) + np.abs(v) * np.abs(sf2 - r_) + np.abs(w_ * sb)
            ap = ap + (m + 6) / LD(Lp + C) * (np.abs(Xin) @ (np.abs(P).T * mag[:, None]))
        put(Xin @ F, ap, Lp)       # (big-major: entry b * d + k)
    if log_hetero is not None:
        het = np.exp(_ld(log_hetero))
        put(LD(0.5) * het * np.diag(W), LD(0.5) * het * np.abs(np.diag(W)), 1)
    if ms is not None:
        gm, am = np.zeros((m, d), LD), np.zeros((m, d), LD)
        for k in range(d):
            f = LD(0.5) * (LD(0.5) - ms[k])                                    # per column c
            dn = P[k][:, None] - Z[k][None, :]
            dm = Z[k][:, None] - Z[k][None, :]
            isc = 1 / (ms[k][:, None] + ms[k][None, :] - 1)
            tm = np.where(off, Q * (isc - dm * dm * isc * isc), 0).sum(0)
            tn = (E * (1 / ms[k][None, :] - (dn / ms[k][None, :]) ** 2)).sum(0)
            dg = LD(0.5) * np.diag(W) * kdiag * (LD(0.5) - ms[k]) / (2 * ms[k] - 1)
            gm[:, k] = f * (tm - tn) + dg
            am[:, k] = np.abs(f) * (np.where(off, aQw * (isc + dm * dm * isc * isc), 0).sum(0)
                                    + (aEw * (1 / ms[k][None, :] + ((np.abs(P[k])[:, None] + np.abs(Z[k])[None, :])
                                                                   / ms[k][None, :]) ** 2)).sum(0)) + np.abs(dg)
        put(gm, am, 3 * n + 2 * m + 1 + d)
    g, A, L = np.concatenate(g), np.concatenate(A).astype(np.float64), np.concatenate(L)
    fams = families(iso, d, m, D, log_hetero is not None, ms is not None)
    assert fams[-1][1].stop == g.shape[0]
    return dict(g=g, A=A, L=L, bound=(L + C) * U * A, fams=fams)


def ratios(got, ref):
    """{family: (max_theta |got - g| / bound, the entry's position in the family)}"""
    err = np.abs(_ld(got) - ref["g"]).astype(np.float64)
    r = err / np.maximum(ref["bound"], 1e-300)
    return {name: (float(np.max(r[sl])), int(np.argmax(r[sl]))) for name, sl in ref["fams"] if sl.stop > sl.start}
