"""Reference for the gradient of the log evidence with respect to the training inputs.

diag K_n = sf2 and K_m do not depend on the training inputs, so of the reference's gradient entry
-1/2 (v . diag K'_n - tr(W K'_m)) - tr(X^T K'_nm) (lib/fitc_gp.ml:956-991) only the last term is left.  With the oracle's own
X (`x_mat` of Trained.prepare_hyper, or of Model.prepare_hyper for a model-only evaluation), its K_nm and p_r the point the
kernel sees (x_r, or tproj^T x_r for Cov_se_fat with a projection)

    dl/dp_rk = inv_ell2 sum_c X_rc K_rc (p_rk - z_ck)      (inv_ell2 = exp(-2 log_ell) for Cov_se_iso, 1 for Cov_se_fat)
    dl/dx_r  = tproj dl/dp_r

formed with direct differences in numpy longdouble.  tests/test_input_grad_host.py pins this against central differences of
the oracle's evidence."""
import numpy as np

from oracle import fitc_oracle as O

LD = np.longdouble


def oracle_parts(k, Z, X, y, sigma2, variational=False):
    """One oracle evaluation with everything kept (shared by the trained and the model-only reference of a case)."""
    return O.evaluate(k, np.asfortranarray(Z), np.asfortranarray(X), y, sigma2, variational=variational, keep=True)


def input_grad_from_parts(k, Z, X, parts, model_only=False):
    """(D, n) float64: dl/dx for the trained evidence l, or dl1/dx of the model evidence (model_only)."""
    x_mat = O.model_prepare_hyper(parts["cm"])["x_mat"] if model_only else parts["hyper_t"]["x_mat"]
    knm = parts["shared"]["knm"]
    fat = isinstance(k, O.SeFatKernel)
    assert not (fat and k.log_multiscales_m05 is not None), "multiscales are not covered"
    P = O.se_fat_project(k, np.asfortranarray(X)) if fat else np.asfortranarray(X)
    inv_ell2 = LD(1) if fat else np.exp(LD(-2) * LD(k.log_ell))
    E = np.asarray(x_mat, LD) * np.asarray(knm, LD)           # (n, m)
    Pl, Zl = np.asarray(P, LD), np.asarray(Z, LD)
    d, n = Pl.shape
    G = np.zeros((d, n), LD)
    for kk in range(d):
        G[kk] = inv_ell2 * (E * (Pl[kk][:, None] - Zl[kk][None, :])).sum(1)
    if fat and k.tproj is not None:
        G = np.asarray(k.tproj, LD) @ G                      # (D, d) (d, n)
    return np.asfortranarray(G.astype(np.float64))


def input_grad_ref(k, Z, X, y, sigma2, variational=False, model_only=False):
    return input_grad_from_parts(k, Z, X, oracle_parts(k, Z, X, y, sigma2, variational), model_only)
