"""gprhip_sample_paths (sample_paths.hip) and gprhip_sample_paths_refine (path_refine.hip) contracted in 80 bits from GIVEN
operands -- t, U^-1, R~^-1 (debug_fetch "t", "uinv", "rinv"), the caller's draws z, eps, and the weights A ("sp_a") -- with a
running-error bound for every entry.  Imports nothing from the library or the oracle.  K, kappa and the shifted coordinates come
from tests/input_grads_ref.geometry (posterior_ref.geometry inside it), the back-projection from input_grads_ref.back_project,
the stored-K chain of the residual from posterior_ref.chain.  Nothing is inverted: no condition number enters.

    weights      w1 = R~^-1 z,  A = t 1^T + U^-1 w1                                      (sp_weights_kernel / sp_tri_row)
    paths        F_rj = sum_c K_rc A_cj                                                   (sample_paths_kernel)
    gradient     dF_rj/dp_rk = -inv_ell2 sum_c K_rc A_cj (p_rk - z_ck), times tproj       (path_grad_at_kernel; path_eval)
    residual     resid_r = (sf2 - |K_r U^-1|^2) + add                                     (two routes, below)
    samples      F_rj + sqrt(max(0, resid_r)) eps_rj                                      (sp_combine_kernel)

Every bound is (L + C) u A, u = 2^-53: L the number of summands (gamma_L holds for any order), C the roundings per term, A the sum
of absolute values in the form the kernel adds them; ETA (TINY for a sum) is added for entries below the smallest normal number.

weights (sample_paths.hip:42-62).  Row i is a sum of n = m - i products by fused multiply-adds (:56), the k range split over
64 / cw lanes and the parts added by shuffles (:58).  A term passes its own fma and then only additions that join two
non-empty parts -- at most n - 1 of them; an addition of a part without terms adds an exact zero -- so n roundings, and
(n + 1) u covers gamma_n.  The second product adds t_i once more (:59): C_W = 2 for both.
    e1_ij = (n + C_W) u sum_k |Ri_ik| |z_kj| + n TINY
    eA_ij = sum_k |Ui_ik| e1_kj + (n + C_W) u (|t_i| + sum_k |Ui_ik| (|w1_kj| + e1_kj)) + n TINY
The k-split, the shuffle order and the one- or two-launch route only reorder the additions.

paths (sample_paths.hip:97-153).  The distance is fmax(pn + zn - 2 S, 0) of the SHIFTED coordinates (:101, :116, :145), the
argument log_sf2 + inv_ell2_05 dist (:146): line by line the K of predict_grad_kernel, so the bound is input_grads_ref.predict's
"means" with t := a_j and expansion=True: (m + LK + C_E) u sum_c K_rc (1 + kappa~_rc) |A_cj| + ETA sum_c |A_cj|.  The product
K A is fused into the MFMA (:152); C_E = 9 counts it as one rounding more, which only loosens.  The weights are the FETCHED ones:
the error of A is held by weights(), not here.  The shift is the centroid as the host sums it (gprhip.hip:621-624, left to
right, then one division: device_shift below); the reference does not depend on it and the bound only through |p~|, |z~|.
The device's own copy of the shift has no fetch and is NOT verified: tests/test_sample_paths_pin_host.py only holds the
restated host sum against input_grads_ref.shift_of.

gradient, direct=False (path_eval, path_refine.hip:63-141): E_rc = K_rc A[c][draw_of[r]] (:114), value = sign rowsum(E) (:126),
gradient = sign inv_ell2 (p~ rowsum(E) - sum_c E_rc z~_c) (:138): predict_grad_kernel's dmeans with t gathered per ROW --
C_E = 9 for the value, C_D = 16 for a gradient entry, as input_grads_ref.py counts them; with a projection
launch_input_grad_project follows (gprhip.hip: do_sample_paths_refine), input_grads_ref.back_project.

gradient, direct=True (path_grad_at_kernel, sample_paths.hip:197-245), roundings per term C_DIRECT = 17:
    the weight K_rc A_cj: p~ = p - s (:209) 1; z~ = z - s and the difference p~ - z~ (:219) 2; the argument's product and sum (:222)
    2; inv_ell2_05 from the host's exp 2; exp_fast 2; the product with A_cj (:222) 1                                          = 10
    the factor (p~_k - z~_ck) (:229): p~ and z~ as factors 2, their difference 1, the product with the weight 1              =  4
    the scale 2 inv_ell2_05 (:232) 1 and inv_ell2 itself 2                                                                    =  3
The sums of the distance (:220, d terms) and of the columns (:229, in blocks of 64) are in L = m + LK.  The differences are
formed from shifted coordinates: kappa~ and A_rk = inv_ell2 sum_c K_rc |A_cj| (1 + kappa~_rc) (|p~_rk| + |z~_ck|), which bounds
the |p~ - z~| the kernel adds.  The kernel's own back-projection (:240-243) is a d-term sum per output: back_project's bound.

residual.  small=True (launch_sp_row_sumsq, m <= 64 and d <= 16): V = K U^-1 with the K of the EXPANSION through the same MFMA
chain (C_E, kappa~), all m columns of a row of U^-1 (the zeros below the diagonal add exactly), then the sum of the squares of
the accumulators (sample_paths.hip:156-163).  small=False: the stored K of launch_cov_cross from RAW coordinates (no shift is
passed, gprhip.hip: do_sample_paths), the engine's TRI_KHI_BN product and launch_row_sumsq_dot: posterior_ref.chain's V, eV
(C = 8, kappa with the coordinates as given) -- the same three launches as gprhip_predict's variance.  Either way
    ek_r = sum_j (2 |V_rj| eV_rj + eV_rj^2) + (m + 2) u sum_j (|V_rj| + eV_rj)^2          (no first-order step)
    e_r  = ek_r + 2 u (sf2 + k_r + |add|) + 2 u sf2        the two additions of sp_combine_kernel (:191); sf2 from the host's libm

samples (sp_combine_kernel, sample_paths.hip:191-192).  The square root is bounded as an INTERVAL, not to first order: the
device's argument lies within e of resid, sqrt and fmax are monotone, sqrt is rounded once, so the device's standard
deviation lies in [sqrt(max(0, resid - e)) (1 - u), sqrt(max(0, resid + e)) (1 + u)].  Times eps (ends ordered by its sign),
plus F -+ eF, widened by the product's and the sum's roundings: 1.01 u (2 |sd eps| + |F| + eF) + TINY.  Returned as the
interval's centre and half width, so that ratio() holds it like any other bound.
"""
import numpy as np

from tests import input_grads_ref as G
from tests import posterior_ref as R
from tests.input_grads_ref import C_D, C_E, TINY, back_project, geometry, shift_of  # noqa: F401  (the tests use them from here)
from tests.posterior_ref import ETA, FIRST_ORDER, LD, U, _ld

C_W = 2
C_DIRECT = 17


def device_shift(Z):
    """the centroid as upload_hypers sums it in float64 (gprhip.hip:621-624): left to right over the points, one division"""
    Z = np.asarray(Z, np.float64)
    acc = np.zeros(Z.shape[0])
    for c in range(Z.shape[1]):
        acc = acc + Z[:, c]
    return acc / Z.shape[1]


def shift_bound(Z):
    """|device_shift - the exact centroid| <= (m + 1) u sum_c |z_c| / m, per dimension"""
    Z = np.asarray(Z, np.float64)
    return (Z.shape[1] + 1) * U * np.abs(Z).sum(1) / Z.shape[1]


def _cols(z):
    z = _ld(z)
    return z.reshape(-1, 1) if z.ndim == 1 else z


def first_product(rinv, z):
    """(w1, e1), m x ns: w1 = R~^-1 z with its bound"""
    Ri, zl = np.triu(_ld(rinv)), _cols(z)
    m = Ri.shape[0]
    n = (m - np.arange(m, dtype=np.float64))[:, None]          # summands of row i
    return Ri @ zl, (n + C_W) * U * (np.abs(Ri) @ np.abs(zl)) + n * TINY


def weights(t, uinv, rinv, z):
    """(A, eA), m x ns"""
    tl, Ui = _ld(t), np.triu(_ld(uinv))
    m = Ui.shape[0]
    n = (m - np.arange(m, dtype=np.float64))[:, None]
    aUi = np.abs(Ui)
    w1, e1 = first_product(rinv, z)
    A = tl[:, None] + Ui @ w1
    eA = aUi @ e1 + (n + C_W) * U * (np.abs(tl)[:, None] + aUi @ (np.abs(w1) + e1)) + n * TINY
    return A, eA


def paths(g, A):
    """(F, eF), nt x ns: input_grads_ref.predict's means with t := a_j, expansion=True, for every draw at once"""
    Al = _cols(A)
    aA = np.abs(Al)
    return g["K"] @ Al, (g["m"] + g["LK"] + C_E) * U * (g["wKs"] @ aA) + ETA * aA.sum(0)[None, :]


def _rowwise(g, Wr, c_grad):
    """value (nt) and d/dx (nt x D) of sum_c K_rc Wr_rc with their bounds: one weight vector per ROW"""
    m, LK, ie2 = g["m"], g["LK"], g["ie2"]
    aW = np.abs(Wr)
    E = g["K"] * Wr
    val = E.sum(1)
    eval_ = (m + LK + C_E) * U * (g["wKs"] * aW).sum(1) + ETA * aW.sum(1)
    bound = ie2 * ((m + LK + c_grad) * U * G._amoment(g, g["wKs"] * aW) + ETA * G._amoment(g, aW))
    grad, egrad = back_project(g, -ie2 * G._moment(g, E), bound)
    return val, eval_, grad, egrad


def path_grads(g, A, direct):
    """(dF, edF), ns x nt x D: the gradient of every draw's path part at every test point with respect to that test input.
    direct: path_grad_at_kernel (C_DIRECT); else path_eval's form (C_D)."""
    Al = _cols(A)
    out = [_rowwise(g, np.broadcast_to(Al[:, j][None, :], (g["nt"], g["m"])), C_DIRECT if direct else C_D)[2:] for j in range(Al.shape[1])]
    return np.stack([o[0] for o in out]), np.stack([np.asarray(o[1], np.float64) for o in out])


def evaluator(g, A, draw_of, sign):
    """path_eval at the points of g, point r on draw draw_of[r]: {"values": (sign f, bound), "dvalues": (D x nt, bound)}"""
    Wr = _cols(A)[:, np.asarray(draw_of, dtype=np.int64)].T
    val, eval_, grad, egrad = _rowwise(g, Wr, C_D)
    return dict(values=(LD(sign) * val, np.asarray(eval_, np.float64)), dvalues=((LD(sign) * grad).T, np.asarray(egrad, np.float64).T))


def resid(g, uinv, add, small):
    """(resid, e), nt: (sf2 - |K_r U^-1|^2) + add and what the device's argument of the square root may differ from it by"""
    m = g["m"]
    if small:
        Ui = np.triu(_ld(uinv))
        aUi = np.abs(Ui)
        V = g["K"] @ Ui
        eV = (m + g["LK"] + C_E) * U * (g["wKs"] @ aUi) + ETA * aUi.sum(0)[None, :]
    else:
        ch = R.chain(g, uinv, np.eye(m))        # (Q = V: the second product is not part of this call)
        V, eV = ch["V"], ch["eV"]
    aV = np.abs(V)
    k = (V * V).sum(1)
    ek = (2 * aV * eV + eV * eV).sum(1) + (m + 2) * U * ((aV + eV) ** 2).sum(1)
    sf2, add = g["sf2"], LD(add)
    return (sf2 - k) + add, ek + 2 * U * (sf2 + k + abs(add)) + 2 * U * sf2


def samples(F, eF, resid_, e, eps):
    """(centre, half width), nt x ns, of the interval the device's sample must lie in"""
    ep = _cols(eps)
    lo_sd = np.sqrt(np.maximum(resid_ - e, 0)) * (1 - LD(U))
    hi_sd = np.sqrt(np.maximum(resid_ + e, 0)) * (1 + LD(U))
    a, b = lo_sd[:, None] * ep, hi_sd[:, None] * ep
    tlo, thi = np.minimum(a, b), np.maximum(a, b)
    tmax = np.maximum(np.abs(tlo), np.abs(thi))
    w = FIRST_ORDER * U * (2 * tmax + np.abs(F) + eF) + TINY
    lo, hi = F - eF + tlo - w, F + eF + thi + w
    return (lo + hi) / 2, (hi - lo) / 2


ratio = R.ratio
