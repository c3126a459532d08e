"""The posterior outputs -- means, variances, FITC / FIC covariance matrices, training statistics, sampler factors -- contracted
in 80 bits from GIVEN operands t (m), U^-1 and R~^-1 (m x m, upper; debug_fetch "t", "uinv", "rinv"), with a running-error bound
for every entry.  Imports nothing from the library or the oracle: the same code serves the CPU and the GPU tests.  No factor is
inverted here, so no condition number enters: every output is a short contraction of operands both sides hold exactly.

    K_rc   = sf2 exp(-|p_r - z_c|^2 / (2 ell^2))   from direct differences, p = tproj^T x in 80 bits with a projection;
             multiscales: sf2 exp(-1/2 sum_k [(p_kr - z_kc)^2 / ms_kc + log ms_kc]), ms = exp(log_ms) + 1/2 (cov_cross_ms_kernel)
    mu_r   = sum_c K_rc t_c
    V_rj   = sum_{c<=j} K_rc Ui_cj,   Q_rj = sum_{c<=j} V_rc Ri_cj,   k_r = |V_r|^2,  b_r = |Q_r|^2
    var_r  = (sf2 - (k_r - b_r)) + add
    FITC   = K_tt(i,j) - V_i . V_j + Q_i . Q_j      K_tt the plain kernel between the projected points, no multiscales
    FIC    = Q_i . Q_j + delta_ij (sf2 - sum_c K_ic^2)                  (+ add on either diagonal)

The bounds.  u = 2^-53; gamma_n bounds of Higham hold for any summation order, so neither the engine's tile order nor the
scalar kernels' lane order is modelled.  Every product that holds a K entry carries the weight 1 + kappa_rc,
    kappa_rc = |log sf2| + (|p_r|^2 + |z_c|^2) / ell^2      [multiscales: |log sf2| + sum_k 2 (p_kr^2 + z_kc^2) / ms_kc + |log ms_kc|]
as tests/hyper_grad_ref.py defines it, but with the coordinates AS GIVEN, not less a centroid: cov_cross_kernel,
cov_cross_ms_kernel, cov_cross_wide_kernel and small_predict_kernel subtract the raw p_kr - z_kc (cov_kernels.hip:44,
small.hip:295).  The argument log_sf2 + inv_ell2_05 acc is known to u kappa only: |p - z|^2 <= 2 (|p|^2 + |z|^2).
With a projection p~ = sum_b |tproj_bk| |x_br| stands in the place of |p_kr| (the device's p carries gamma_D of that sum).
Roundings per term, C = 8: exp_fast within 1 ulp = 2 u (exp_fast.h:7-8); 1/ell^2 = exp(-2 log ell) 2 u; the product and the sum
of the argument 2; the difference p - z 1; the product with t_c (or Ui_cj) 1.  The sums INSIDE a distance are counted in the
length, as tests/hyper_grad_ref.py counts them in its L: a K entry adds d products (and 2 D roundings of the two projected
coordinates' D-term sums), so a sum of n terms has the length n + d + 2 D.  With LK = d + 2 D:
    mean      |dmu_r|  <= (m + LK + C) u sum_c |K_rc| |t_c| (1 + kappa_rc)
    V         eV_rj    =  (j + LK + C) u sum_{c<=j} |K_rc| |Ui_cj| (1 + kappa_rc)              (j counted from 1)
    Q         eQ_rj    =  sum_c eV_rc |Ri_cj| + (j + C) u sum_c |V_rc| |Ri_cj|
    k, b      ek_r     =  2 sum_j |V_rj| eV_rj + (m + 2) u k_r,   eb_r likewise from Q, eQ
    variance  1.01 (ek + eb + 3 u (sf2 + k + b + add) + 2 u sf2)     three roundings of the combination (rowops.hip:185,
              small.hip:334), and sf2 = exp(log_sf2) from the host's libm within 1 ulp; first order, times 1.01 as the fp32
              kernel tests take it
    FITC      1.01 (eKtt_ij + sum_c (eV_ic |V_jc| + |V_ic| eV_jc) + the same of Q + (m + 3) u (|Ktt_ij| + |V_i| . |V_j| + |Q_i| . |Q_j| + add))
              eKtt_ij = (LK + C - 1) u Ktt_ij (1 + kappa_ij), kappa_ij from |p_i|^2 + |p_j|^2
    FIC       1.01 (the Q part + delta_ij (2 sum_c |K_ic| eK_ic + (m + 4) u (sf2 + sum_c K_ic^2) + 2 u sf2 + u add))
Where K is below the smallest normal number the device's entry is a subnormal or zero (exp_fast clamps at -800): every K entry
carries the absolute allowance eta = 2^-1022 besides, as factor_ratio of tests/test_gpu_factors.py does.

fp32-bulk (`bulk32=True`; do_predict<float>, do_train_stats<float>): cov_cross_kernel<DT, float> rounds the fp64 value to float
on store (cov_kernels.hip:51) -- every K entry carries u32 = 2^-24 besides; the second operands are np.float32(uinv) and
np.float32(rinv), the round-to-nearest copies launch_to_float makes, taken as exact operands here; the engine's fp32 kernels
accumulate in fp32 and store V and Q as floats, so eV has (j + 1) u32 sum |K| |Ui| (accumulation and store) and eQ
(j + 1) u32 sum |V| |Ri| in the place of the fp64 terms.  row_sumsq_dot_kernel<float> widens every entry and multiplies and adds
in fp64 (rowops.hip:156-162): the products with t, k, b and the combination keep u.
The training means of an fp32-bulk problem with 16 <= d <= 64 and no multiscales (gprhip_train_stats: cov_chunk passes
p->zshift, gprhip.hip:772, and launch_cov_cross<float> then takes cov_cross_mfma_kernel, cov_kernels.hip:431) come from the
expansion |p - s|^2 + |z - s|^2 - 2 S around the centroid s of the inducing points (`shift=s`, no projection).  There a K
entry carries the entry bound tests/test_gpu_f32_kernels.py derives and pins for that kernel,
    eK_rc = 1.01 |K_rc| (u32 + 8 u (1 + |arg_rc|) + |a| (gamma_{DP+3} + 2 u) A_rc) + eta,   A_rc = sum_k (|p_rk - s_k| + |z_ck - s_k|)^2,
a = inv_ell2_05, DP = 16, 32, 64 the padded width: the rounded shifts move the distance by 2 u A_rc, the chains behind the
three sums are DP + 2 roundings on terms that sum to A_rc, 8 u (1 + |arg|) holds the argument's product and sum and exp_fast.
The mean is then  sum_c eK_rc |t_c| + (m + 1) u sum_c |K_rc| |t_c|  (the fp64 products and any order of m additions).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
U32 = 2.0 ** -24
C = 8
ETA = 2.0 ** -1022
FIRST_ORDER = 1.01


def _ld(a):
    return None if a is None else np.asarray(a, dtype=LD)


def _exp(arg):
    """exp in longdouble; arguments that the 80-bit exponent range cannot hold give 0 (they are far below eta)"""
    return np.where(arg > -11000, np.exp(np.maximum(arg, LD(-11000))), LD(0))


def geometry(Xt, Z, *, iso, log_sf2, log_ell=0.0, tproj=None, log_ms=None, bulk32=False, shift=None):
    """K (nt x m) at the test points Xt (D x nt), its absolute error eK, the plain K_tt and its error, all longdouble.
    shift: the centroid of the inducing points as the host sums it -- the entries come from cov_cross_mfma_kernel<., float>."""
    assert np.finfo(LD).eps < 1e-18, "numpy longdouble is not an extended type here"
    Xl, Zl, tp = _ld(Xt), _ld(Z), _ld(tproj)
    d, m = Zl.shape
    D = 0 if tp is None else tp.shape[0]
    P = Xl if tp is None else tp.T @ Xl
    Pa = np.abs(Xl) if tp is None else np.abs(tp).T @ np.abs(Xl)       # what |p| stands for in kappa
    lsf = LD(log_sf2)
    ie2 = np.exp(LD(-2) * LD(log_ell)) if iso else LD(1)
    ms = None if log_ms is None else np.exp(_ld(log_ms)) + LD(0.5)
    nt = P.shape[1]
    acc, att = np.zeros((nt, m), LD), np.zeros((nt, nt), LD)
    for k in range(d):
        dn = P[k][:, None] - Zl[k][None, :]
        acc += dn * dn if ms is None else dn * (dn / ms[k][None, :]) + np.log(ms[k][None, :])
        dt = P[k][:, None] - P[k][None, :]
        att += dt * dt
    K = _exp(lsf - LD(0.5) * ie2 * acc)
    Ktt = _exp(lsf - LD(0.5) * ie2 * att)
    p2 = (Pa * Pa).sum(0)
    if ms is None:
        kap = abs(lsf) + (p2[:, None] + (Zl * Zl).sum(0)[None, :]) * ie2
    else:
        kap = abs(lsf) + 2 * (Pa * Pa).T @ (1 / ms) + (2 * Zl * Zl / ms + np.abs(np.log(ms))).sum(0)[None, :]
    ktt = abs(lsf) + (p2[:, None] + p2[None, :]) * ie2
    LK = d + 2 * D
    wK = np.abs(K) * (1 + kap)
    eK_exp = None
    if shift is not None:
        assert bulk32 and tp is None and ms is None and 16 <= d <= 64, "the expansion kernel serves fp32, 16 <= d <= 64, no multiscales"
        sh = _ld(shift)[:, None]
        ap, az = np.abs(P - sh), np.abs(Zl - sh)
        A = sum((ap[k][:, None] + az[k][None, :]) ** 2 for k in range(d))
        DP = 16 if d <= 16 else (32 if d <= 32 else 64)
        a = LD(0.5) * ie2
        gam = (DP + 3) * U / (1 - (DP + 3) * U)
        eK_exp = FIRST_ORDER * np.abs(K) * (U32 + 8 * U * (1 + np.abs(lsf - a * acc)) + a * (gam + 2 * U) * A) + ETA
    return dict(eK_exp=eK_exp, K=K, wK=wK, Ktt=Ktt, eKtt=(LK + C - 1) * U * Ktt * (1 + ktt) + ETA, P=P, sf2=np.exp(lsf), m=m, d=d, D=D, LK=LK,
                nt=nt, k32=U32 * np.abs(K) if bulk32 else 0, bulk32=bulk32)


def _eK(g):
    """absolute error of one K entry by itself (no product behind it)"""
    return (g["LK"] + C - 1) * U * g["wK"] + ETA + g["k32"]


def mean(g, t):
    """(mu, bound) for one coefficient vector (m) or a matrix of them (m x k)"""
    tl = _ld(t)
    at = np.abs(tl)
    mu = g["K"] @ tl
    if g["eK_exp"] is not None:
        return mu, np.asarray(g["eK_exp"] @ at + (g["m"] + 1) * U * (np.abs(g["K"]) @ at), np.float64)
    bound = (g["m"] + g["LK"] + C) * U * (g["wK"] @ at) + (ETA + 0) * at.sum(0) + (g["k32"] @ at if g["bulk32"] else 0)
    return mu, np.asarray(bound, np.float64)


def chain(g, uinv, rinv):
    """V, Q, k, b and their entry-wise errors.  uinv, rinv: m x m upper (the fp32-bulk caller passes np.float32 copies)."""
    m = g["m"]
    Ui, Ri = np.triu(_ld(uinv)), np.triu(_ld(rinv))
    aUi, aRi = np.abs(Ui), np.abs(Ri)
    j1 = np.arange(1, m + 1, dtype=np.float64)[None, :]
    V = g["K"] @ Ui
    eV = (j1 + g["LK"] + C) * U * (g["wK"] @ aUi) + ETA * aUi.sum(0)[None, :]
    if g["bulk32"]:
        eV = eV + (g["k32"] @ aUi) + (j1 + 1) * U32 * (np.abs(g["K"]) @ aUi)
    Q = V @ Ri
    eQ = eV @ aRi + ((j1 + 1) * U32 if g["bulk32"] else (j1 + C) * U) * (np.abs(V) @ aRi)
    k, b = (V * V).sum(1), (Q * Q).sum(1)
    ek = 2 * (np.abs(V) * eV).sum(1) + (m + 2) * U * k
    eb = 2 * (np.abs(Q) * eQ).sum(1) + (m + 2) * U * b
    return dict(V=V, Q=Q, eV=eV, eQ=eQ, k=k, b=b, ek=ek, eb=eb)


def variance(g, ch, add):
    sf2, add = g["sf2"], LD(add)
    var = (sf2 - (ch["k"] - ch["b"])) + add
    bound = FIRST_ORDER * (ch["ek"] + ch["eb"] + 3 * U * (sf2 + ch["k"] + ch["b"] + add) + 2 * U * sf2)
    return var, np.asarray(bound, np.float64)


def _gram(A, eA):
    aA = np.abs(A)
    ea = eA @ aA.T
    return A @ A.T, ea + ea.T, aA @ aA.T


def covariances(g, ch, kind, add):
    """(nt x nt matrix, entry bounds), full symmetric"""
    m, sf2, add = g["m"], g["sf2"], LD(add)
    eye = np.eye(g["nt"], dtype=LD)
    QQ, eQQ, aQQ = _gram(ch["Q"], ch["eQ"])
    if kind == "FITC":
        VV, eVV, aVV = _gram(ch["V"], ch["eV"])
        cov = g["Ktt"] - VV + QQ + add * eye
        bound = g["eKtt"] + eVV + eQQ + (m + 3) * U * (np.abs(g["Ktt"]) + aVV + aQQ + add * eye)
    else:
        assert kind == "FIC"
        K = g["K"]
        kk = (K * K).sum(1)
        cov = QQ + np.diag(sf2 - kk + add)
        bound = eQQ + (m + 3) * U * aQQ + np.diag(2 * (np.abs(K) * _eK(g)).sum(1) + (m + 4) * U * (sf2 + kk) + 2 * U * sf2 + U * add)
    return cov, np.asarray(FIRST_ORDER * bound, np.float64)


def train_stats(y, means_dev):
    """From the training means the device returned: the four sums of residual_stats_kernel.  maxad is exact -- the kernel
    forms fl(y - mean) and takes maxima, which do not round --; the three sums of positive terms are held relatively:
    one rounding of the difference is in fl(y - mean) itself, its square or y^2 adds one, and any order of n additions
    gamma_{n-1}: within (n + 3) u of the 80-bit sums of the fp64 terms."""
    y, mu = np.asarray(y, np.float64), np.asarray(means_dev, np.float64)
    r = y - mu                                                      # fl(y - mean), the double the kernel forms
    rl, yl = _ld(r), _ld(y)
    sums = np.array([(rl * rl).sum(), np.abs(rl).sum(), 0, (yl * yl).sum()], dtype=LD)
    return dict(sums=sums, maxad=float(np.max(np.abs(r))), rel=(y.shape[0] + 3) * U)


def samples(L, means, z):
    """(means_i + sum_k L_ik z_kj, bound (nt + 2) u (|means_i| + sum |L_ik| |z_kj|)) with L a given operand"""
    Ll, zl, mu = _ld(L), _ld(z), _ld(means)
    s = mu[:, None] + Ll @ zl
    bound = (Ll.shape[0] + 2) * U * (np.abs(mu)[:, None] + np.abs(Ll) @ np.abs(zl))
    return s, np.asarray(bound, np.float64)


def ratio(got, ref, bound):
    """max |got - ref| / bound over the entries (0 / 0 counts as 0), and where"""
    err = np.abs(_ld(got) - ref).astype(np.float64)
    r = np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)
    at = int(np.argmax(r)) if r.size else 0
    return (float(r.ravel()[at]) if r.size else 0.0), at
