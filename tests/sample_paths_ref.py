"""Reference for the posterior sample paths of gprhip_sample_paths.

From the oracle's own K_m (heteroskedastic noise included) and K_nm -- taken as exact -- the model state is restated in numpy
longdouble with the helpers tests/predict_grad_ref.py uses (plain Cholesky and back-substitution loops), as its model_state:

    U = chol(K_m + jitter I), V = K_nm U^-1, s = sf2 - |V_i|^2 + sigma2, B~ = I + V^T S^-1 V = R~^T R~,
    t = U^-1 R~^-1 R~^-T V^T (y / s)

and with the caller's normal draws Z (m x ns), eps (nt x ns), the oracle's K = K_tm and p_r the point the kernel sees:

    A = t 1^T + U^-1 (R~^-1 Z),   F = K A,   resid_r = sf2 - |K_r U^-1|^2 (+ sigma2),
    samples = F + sqrt(max(0, resid)) eps,
    dF_rj/dp_r = -inv_ell2 sum_c K_rc A_cj (p_r - z_c),   d./dx*_r = tproj d./dp_r      (direct differences)

tests/test_sample_paths_host.py pins this against the oracle's predict_means, predict_variances and fic_covariances."""
import numpy as np

from oracle import fitc_oracle as O
from tests.util import _ld_chol_upper, _ld_matmul, _ld_triu_inverse, oracle_km_full

LD = np.longdouble


def path_state(k, Z, X, y, sigma2, jitter=O.CHOLESKY_JITTER):
    """(t, U^-1, R~^-1) in longdouble"""
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
    t = Ui @ (mm(Ri, Ri.T) @ (V.T @ (yl * is_)))
    return t, Ui, Ri


def weights(state, z):
    """A = t 1^T + U^-1 (R~^-1 Z), longdouble m x ns"""
    t, Ui, Ri = state
    z = np.asarray(z, LD)
    z = z.reshape(-1, 1) if z.ndim == 1 else z
    return t[:, None] + _ld_matmul(Ui, _ld_matmul(Ri, z))


def sample_paths_from_state(k, Z, state, Xt, z, sigma2, eps=None, predictive=False, grad_at=None):
    """dict(paths (nt, ns), resid [nt], samples (nt, ns)) in float64; with grad_at = [(r, j), ...] also grads (D, len): the
    gradient of draw j's path part at test point r with respect to that test input."""
    t, Ui, Ri = state
    Z, Xt = np.asfortranarray(Z), np.asfortranarray(Xt)
    fat = isinstance(k, O.SeFatKernel)
    assert not (fat and k.log_multiscales_m05 is not None), "multiscales are not covered"
    proj = fat and k.tproj is not None
    sf2 = np.exp(LD(k.log_sf2))
    inv_ell2 = LD(1) if fat else np.exp(LD(-2) * LD(k.log_ell))
    ktm, _ = O.spec_calc_shared_cross(k, Xt, Z)
    K = np.asarray(ktm, LD)
    A = weights(state, z)
    F = _ld_matmul(K, A)
    V = _ld_matmul(K, Ui)
    resid = sf2 - (V * V).sum(1) + (LD(sigma2) if predictive else LD(0))
    out = dict(paths=np.asfortranarray(F.astype(np.float64)), resid=resid.astype(np.float64))
    if eps is not None:
        e = np.asarray(eps, LD)
        e = e.reshape(-1, 1) if e.ndim == 1 else e
        out["samples"] = np.asfortranarray((F + np.sqrt(np.maximum(resid, 0))[:, None] * e).astype(np.float64))
    else:
        out["samples"] = out["paths"]
    if grad_at is not None:
        P = np.asarray(k.tproj, LD).T @ np.asarray(Xt, LD) if proj else np.asarray(Xt, LD)
        Zl = np.asarray(Z, LD)
        g = np.zeros((P.shape[0], len(grad_at)), LD)
        for e_, (r, j) in enumerate(grad_at):
            w = K[r] * A[:, j]
            g[:, e_] = -inv_ell2 * ((P[:, r][:, None] - Zl) * w[None, :]).sum(1)
        if proj:
            g = np.asarray(k.tproj, LD) @ g
        out["grads"] = np.asfortranarray(g.astype(np.float64))
    return out


def sample_paths_ref(k, Z, X, y, sigma2, Xt, z, **kw):
    return sample_paths_from_state(k, Z, path_state(k, Z, X, y, sigma2), Xt, z, sigma2, **kw)
