"""The two calls that differentiate with respect to inputs -- gprhip_eval_input_grad (input_grad.hip) and
gprhip_predict_input_grad (predict_grad_body.inc, small_predict_grad_body.inc, ensure_predict_m / pg_chunk of gprhip.hip) --
contracted in 80 bits from GIVEN operands: X (debug_fetch "x_rows"), t, U^-1, R~^-1 ("t", "uinv", "rinv") and M ("pg_m"), with a
running-error bound for every entry.  Imports nothing from the library or the oracle; K, kappa with the coordinates as given, the
nested errors eV, eQ and the constants come from tests/posterior_ref.py.  Nothing is inverted: no condition number enters.

    training inputs   g_rk  = inv_ell2 sum_c X_rc K_rc (p_rk - z_ck)
    M                 M     = Ui (I - Ri Ri^T) Ui^T
    engine path       G = K M,  mu_r = sum_c K_rc t_c,  var_r = (sf2 - sum_c K_rc G_rc) + add
                      dmu_rk  = -inv_ell2 sum_c K_rc t_c  (p_rk - z_ck)
                      dvar_rk = 2 inv_ell2 sum_c K_rc G_rc (p_rk - z_ck)
    one-kernel path   the same with G = ((V - (V Ri) Ri^T) Ui^T), V = K Ui, nested; there is no M
    with a projection every d/dp is carried back: out_rb = sum_k tproj_bk (d/dp)_rk

Every bound is (L + C) u A, u = 2^-53: L the number of summands (Higham's gamma_L holds for any order, so neither the 16-column
tiles nor the four partial sums of the lanes are modelled), C the roundings per term, A the sum of absolute values IN THE FORM THE
KERNEL ADDS THEM.  The kernels add  p~_rk rowsum(E)_r - sum_c E_rc z~_ck  (input_grad.hip:155, predict_grad_body.inc:141-142,
small_predict_grad_body.inc:124-125), ~ = less the shift s: the centroid of the inducing points for d <= 64, the first inducing
point beyond (gprhip.hip: input_grad_chunk), so
    A_rk = inv_ell2 sum_c |E_rc| (1 + kappa_rc) (|p~_rk| + |z~_ck|).
With a projection |p~_rk| is replaced by sum_b |tproj_bk| |x_br| + |s_k|, which also bounds the error gamma_D of the device's
projected point (posterior_ref.py does the same inside kappa).
kappa (posterior_ref.py, hyper_grad_ref.py) is what the argument of the exponential is known to:
  * the expansion fmax(pn + zn - 2 S, 0) (input_grad.hip:128, predict_grad_body.inc:73; KR = false and predict_grad_kernel) is
    formed from the SHIFTED coordinates: kappa~_rc = |log sf2| + (|p~_r|^2 + |z~_c|^2) / ell^2.  fmax only moves a negative
    rounded distance towards the true one.
  * a K that is read (input_grad.hip:86-88, KR = true: the resident store or the rebuilt chunk; the K of G = K M, gprhip.hip:
    pg_chunk -> launch_cov_cross; small_predict_grad_body.inc:40-43) comes from raw differences: kappa_rc with the coordinates as
    given (posterior_ref.geometry's wK).
L = m + LK, LK = d + 2 D the sums inside a distance, as posterior_ref.py counts them.
Roundings per term:
  C_E = 9   a summand K_rc w_c of a row sum (mean, sum K G): exp_fast 2 (exp_fast.h:7-8); 1/ell^2 = exp(-2 log ell) 2; the product
            and the sum of the argument 2 (predict_grad_body.inc:74); the two shifted coordinates 2 (:20, :48; raw: the one
            difference, small_predict_grad_body.inc:40); the product with t_c or G_rc 1 (:75-76).
  C_D = 16  a summand of a gradient entry: C_E (with X_rc in the place of t_c, input_grad.hip:130; K X for a read K, :88), and the
            roundings of p~ and z~ once more as FACTORS 2 (input_grad.hip:154, :100); the product p~ rowsum 1; the subtraction 1;
            the scale 1 and inv_ell2 itself 2 (:145, :155).  The products E z~ are fused into the MFMA's additions (in L).
  G (engine)  eG_rc = (m + LK + C) u sum_j K_rj (1 + kappa_rj) |M_jc| + eta sum_j |M_jc|, C = 8 of posterior_ref.py: the stored K
            of launch_cov_cross (raw coordinates) times the given M.
  G (one kernel)  eT_rc = sum_j eQ_rj |Ri_cj| + (m + C) u sum_j |Q_rj| |Ri_cj|,  eH = eV + eT + u (|V| + |T|)
            (small_predict_grad_body.inc:62-64),  eG_rc = sum_j eH_rj |Ui_cj| + (m + C) u sum_j |H_rj| |Ui_cj| (:66): posterior_ref's
            eV, eQ carried two products further.
  row sum of K .* G:  sum_c K_rc eG_rc + (m + LK + C_E) u sum_c K_rc (1 + kappa) |G_rc|
  variance  1.01 (that + 3 u (sf2 + sum K |G| + add) + 2 u sf2)   as posterior_ref.variance (predict_grad_body.inc:99)
  dvar      1.01 * 2 inv_ell2 (sum_c K_rc eG_rc (|p~| + |z~|)) + (m + LK + C_D) u A_rk, A with |E| = K |G|
  M         |M_dev - M|_ij <= (3 m + C_M) u (|Ui| (I + |Ri| |Ri|^T) |Ui|^T)_ij, C_M = 4: three products of length <= m in any
            order (triu_xxt, two gemm_splitk launches: the k-slices only reorder the additions), the subtraction from the
            identity 1 (predict_grad.hip:153), and one for each product's first-order form.  Products that fall below the
            smallest normal number are rounded to multiples of 2^-1074 (on a line the factors decay to subnormals): each of the
            3 m products of an entry adds 2^-1074, times the row sums 1 + sum_j |Ui_ij| of the factors it still passes through.
  back-projection (input_grad.hip:174)  sum_k |tproj_bk| bound_rk + (d + 1) u sum_k |tproj_bk| (|g_rk| + bound_rk)
A K entry below the smallest normal number is a subnormal or zero on the device (exp_fast clamps at -800): every K entry carries
eta = 2^-1022 besides, times the factors it is multiplied with.
"""
import numpy as np

from tests import posterior_ref as R
from tests.posterior_ref import ETA, FIRST_ORDER, LD, U, _ld

C_E = 9
C_D = 16
C_M = 4
TINY = 2.0 ** -1074


def shift_of(Z):
    """the shift of the gradient kernels: the centroid of the inducing points (d <= 64), the first inducing point beyond"""
    Z = np.asarray(Z, np.float64)
    return Z.mean(axis=1) if Z.shape[0] <= 64 else Z[:, 0].copy()


def geometry(Xt, Z, *, iso, log_sf2, log_ell=0.0, tproj=None):
    """posterior_ref.geometry (K, wK = K (1 + kappa) with the coordinates as given, P, LK ...) and, point-major, the shifted
    coordinates with their stand-ins and wKs = K (1 + kappa~) of the expansion"""
    g = dict(R.geometry(Xt, Z, iso=iso, log_sf2=log_sf2, log_ell=log_ell, tproj=tproj))
    Zl, Xl, tp = _ld(Z), _ld(Xt), _ld(tproj)
    s = _ld(shift_of(Z))[:, None]
    P = g["P"]
    Pt, Zt = P - s, Zl - s
    aPt = np.abs(Pt) if tp is None else np.abs(tp).T @ np.abs(Xl) + np.abs(s)
    aZt = np.abs(Zt)
    ie2 = np.exp(LD(-2) * LD(log_ell)) if iso else LD(1)
    kap = abs(LD(log_sf2)) + ((aPt * aPt).sum(0)[:, None] + (aZt * aZt).sum(0)[None, :]) * ie2
    g.update(Pm=P.T.copy(), Zm=Zl.T.copy(), aPt=aPt.T.copy(), aZt=aZt.T.copy(), wKs=np.abs(g["K"]) * (1 + kap), ie2=ie2, tp=tp)
    return g


def _moment(g, E):
    """sum_c E_rc (p_rk - z_ck), nt x d, from direct differences"""
    out = np.empty((g["nt"], g["d"]), LD)
    for k in range(g["d"]):
        out[:, k] = (E * (g["Pm"][:, k][:, None] - g["Zm"][:, k][None, :])).sum(1)
    return out


def _amoment(g, W):
    """sum_c W_rc (|p~_rk| + |z~_ck|) for non-negative W"""
    return g["aPt"] * W.sum(1)[:, None] + W @ g["aZt"]


def back_project(g, val, bound):
    """d/dp (nt x d) -> d/dx (nt x D) with a projection; unchanged without"""
    tp = g["tp"]
    if tp is None:
        return val, np.asarray(bound, np.float64)
    a = np.abs(tp)
    b = _ld(bound)
    return val @ tp.T, np.asarray(b @ a.T + (g["d"] + 1) * U * ((np.abs(val) + b) @ a.T), np.float64)


def train_input_grad(g, X, read_k):
    """(g, bound), n x D: the geometry is that of the training inputs; X n x m (the device's own); read_k: the kernel
    multiplies a K from memory (KR = true)"""
    Xl = _ld(X)
    aX = np.abs(Xl)
    w = g["wK"] if read_k else g["wKs"]
    val = g["ie2"] * _moment(g, Xl * g["K"])
    bound = g["ie2"] * ((g["m"] + g["LK"] + C_D) * U * _amoment(g, aX * w) + ETA * _amoment(g, aX))
    return back_project(g, val, bound)


def m_matrix(uinv, rinv):
    """(M, bound) from the fetched factors"""
    Ui, Ri = np.triu(_ld(uinv)), np.triu(_ld(rinv))
    m = Ui.shape[0]
    aUi, aRi = np.abs(Ui), np.abs(Ri)
    eye = np.eye(m, dtype=LD)
    Mr = Ui @ (eye - Ri @ Ri.T) @ Ui.T
    A = aUi @ (eye + aRi @ aRi.T) @ aUi.T
    rs = 1 + aUi.sum(1)
    tiny = 3 * m * TINY * rs[:, None] * rs[None, :]
    return Mr, np.asarray((3 * m + C_M) * U * A + tiny, np.float64)


def g_engine(g, M):
    """(G = K M, eG): the stored K of launch_cov_cross times the given M"""
    Ml = _ld(M)
    aM = np.abs(Ml)
    return g["K"] @ Ml, (g["m"] + g["LK"] + R.C) * U * (g["wK"] @ aM) + ETA * aM.sum(0)[None, :]


def g_small(g, uinv, rinv):
    """(G, eG) nested as small_predict_grad_kernel forms it"""
    m = g["m"]
    ch = R.chain(g, uinv, rinv)
    Ui, Ri = np.triu(_ld(uinv)), np.triu(_ld(rinv))
    aUi, aRi = np.abs(Ui), np.abs(Ri)
    T = ch["Q"] @ Ri.T
    eT = ch["eQ"] @ aRi.T + (m + R.C) * U * (np.abs(ch["Q"]) @ aRi.T)
    H = ch["V"] - T
    eH = ch["eV"] + eT + U * (np.abs(ch["V"]) + np.abs(T))
    return H @ Ui.T, eH @ aUi.T + (m + R.C) * U * (np.abs(H) @ aUi.T)


def predict(g, t, add, expansion, G=None, eG=None):
    """{name: (reference, bound)}: means, dmeans (nt x D) and, with G, variances and dvariances.  expansion: the K that is
    multiplied comes from the shifted expansion (predict_grad_kernel), not from raw differences (small_predict_grad_kernel)."""
    K, m, LK, ie2 = g["K"], g["m"], g["LK"], g["ie2"]
    w = g["wKs"] if expansion else g["wK"]
    tl = _ld(t)
    at = np.abs(tl)
    ones = np.ones((g["nt"], 1), LD)
    out = {}
    out["means"] = (K @ tl, np.asarray((m + LK + C_E) * U * (w @ at) + ETA * at.sum(), np.float64))
    bound = ie2 * ((m + LK + C_D) * U * _amoment(g, w * at[None, :]) + ETA * _amoment(g, ones * at[None, :]))
    out["dmeans"] = back_project(g, -ie2 * _moment(g, K * tl[None, :]), bound)
    if G is None:
        return out
    aG = np.abs(G)
    sf2, add = g["sf2"], LD(add)
    e_rs = (K * eG).sum(1) + (m + LK + C_E) * U * (w * aG).sum(1) + ETA * aG.sum(1)
    out["variances"] = ((sf2 - (K * G).sum(1)) + add,
                        np.asarray(FIRST_ORDER * (e_rs + 3 * U * (sf2 + (K * aG).sum(1) + add) + 2 * U * sf2), np.float64))
    bound = FIRST_ORDER * 2 * ie2 * (_amoment(g, K * eG) + (m + LK + C_D) * U * _amoment(g, w * aG) + ETA * _amoment(g, aG))
    out["dvariances"] = back_project(g, 2 * ie2 * _moment(g, K * G), bound)
    return out


ratio = R.ratio
