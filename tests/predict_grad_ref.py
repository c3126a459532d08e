"""Reference for the gradients of the predictive mean and variance with respect to the test inputs.

From the oracle's own K_m (heteroskedastic noise included) and K_nm -- taken as exact -- the model state is restated in numpy
longdouble with the helpers of tests/util.py (plain Cholesky and back-substitution loops):

    U = chol(K_m + jitter I), V = K_nm U^-1, s = sf2 - |V_i|^2 + sigma2, B~ = I + V^T S^-1 V = R~^T R~,
    t = U^-1 R~^-1 R~^-T V^T (y / s),   M = U^-1 (I - R~^-1 R~^-T) U^-T

and at the test points, with the oracle's K = K_tm, p_r the point the kernel sees (x*_r, or tproj^T x*_r) and G = K M:

    mu_r     = sum_c K_rc t_c                          dmu_r/dp_rk     = -inv_ell2 sum_c K_rc t_c  (p_rk - z_ck)
    sigma2_r = sf2 - sum_c K_rc G_rc (+ sigma2)        dsigma2_r/dp_rk = 2 inv_ell2 sum_c K_rc G_rc (p_rk - z_ck)
    d./dx*_r = tproj d./dp_r

(inv_ell2 = exp(-2 log_ell) for Cov_se_iso, 1 for Cov_se_fat), formed with direct differences.
tests/test_predict_grad_host.py pins this against central differences of the oracle's predict_means / predict_variances."""
import numpy as np

from oracle import fitc_oracle as O
from tests.util import _ld_chol_upper, _ld_matmul, _ld_triu_inverse, oracle_km_full

LD = np.longdouble


def model_state(k, Z, X, y, sigma2, jitter=O.CHOLESKY_JITTER):
    """(t, M) in longdouble: the mean coefficients and the m x m operand of the variance."""
    assert np.finfo(LD).eps < 1e-18, "numpy longdouble is not an extended type here"
    Z, X = np.asfortranarray(Z), np.asfortranarray(X)
    m = Z.shape[1]
    mm = _ld_matmul
    sf2 = np.exp(LD(k.log_sf2))
    A = np.asarray(oracle_km_full(k, Z), LD) + LD(jitter) * np.eye(m, dtype=LD)
    knm, _ = O.spec_calc_shared_cross(k, X, Z)
    K, yl = np.asarray(knm, LD), np.asarray(y, LD)
    Ui = _ld_triu_inverse(_ld_chol_upper(A))
    V = mm(K, Ui)
    is_ = 1 / (sf2 - (V * V).sum(1) + LD(sigma2))
    Ri = _ld_triu_inverse(_ld_chol_upper(np.eye(m, dtype=LD) + mm(V.T, V * is_[:, None])))   # R~^-1
    Bi = mm(Ri, Ri.T)
    t = Ui @ (Bi @ (V.T @ (yl * is_)))
    M = mm(mm(Ui, np.eye(m, dtype=LD) - Bi), Ui.T)
    return t, M


def predict_grad_from_state(k, Z, state, Xt, sigma2, predictive=True):
    """dict(means [nt], variances [nt], dmeans (D, nt), dvariances (D, nt)) in float64 at the test inputs Xt (D x nt)."""
    t, M = state
    Z, Xt = np.asfortranarray(Z), np.asfortranarray(Xt)
    fat = isinstance(k, O.SeFatKernel)
    assert not (fat and k.log_multiscales_m05 is not None), "multiscales are not covered"
    proj = fat and k.tproj is not None
    sf2 = np.exp(LD(k.log_sf2))
    inv_ell2 = LD(1) if fat else np.exp(LD(-2) * LD(k.log_ell))
    ktm, _ = O.spec_calc_shared_cross(k, Xt, Z)
    K = np.asarray(ktm, LD)
    P = np.asarray(k.tproj, LD).T @ np.asarray(Xt, LD) if proj else np.asarray(Xt, LD)
    Zl = np.asarray(Z, LD)
    Em = K * t[None, :]
    Ev = K * _ld_matmul(K, M)
    means = Em.sum(1)
    var = sf2 - Ev.sum(1) + (LD(sigma2) if predictive else LD(0))
    d, nt = P.shape
    dm, dv = np.zeros((d, nt), LD), np.zeros((d, nt), LD)
    for kk in range(d):
        diff = P[kk][:, None] - Zl[kk][None, :]
        dm[kk] = -inv_ell2 * (Em * diff).sum(1)
        dv[kk] = 2 * inv_ell2 * (Ev * diff).sum(1)
    if proj:
        dm, dv = np.asarray(k.tproj, LD) @ dm, np.asarray(k.tproj, LD) @ dv
    f = lambda a: np.asfortranarray(a.astype(np.float64))
    return dict(means=means.astype(np.float64), variances=var.astype(np.float64), dmeans=f(dm), dvariances=f(dv))


def predict_grad_ref(k, Z, X, y, sigma2, Xt, predictive=True):
    return predict_grad_from_state(k, Z, model_state(k, Z, X, y, sigma2), Xt, sigma2, predictive)
