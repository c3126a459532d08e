import glob
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import fitc_oracle as O

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def golden_names():
    """Evidence + gradient fixtures."""
    return [n for n in _names() if not n.startswith("posterior_") and not n.startswith("illcond_")]


def illcond_golden_names():
    """Jitter-dominated K_m (ell = e): the regime SURVEY.md 7 singles out; own stated tolerances."""
    return [n for n in _names() if n.startswith("illcond_")]


def posterior_golden_names():
    """Prediction / covariance / sampler / stats fixtures (make_golden.save_posterior)."""
    return [n for n in _names() if n.startswith("posterior_")]


STAT_KEYS = ("n_samples", "target_variance", "sse", "mse", "rmse", "smse", "msll", "mad", "maxad")


def load_golden(name):
    g = dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False))
    g["kind"] = str(g["kind"])
    return g


def oracle_kernel(g):
    if g["kind"] == "iso":
        return O.SeIsoKernel(float(g["log_ell"]), float(g["log_sf2"]))
    return O.SeFatKernel(int(g["d"]), float(g["log_sf2"]), g.get("tproj"), g.get("log_hetero"), g.get("log_multiscales"))


def synth(seed, n, m, d):
    """BASELINE.md section 2 synthetic generator."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(d, n))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=n)
    Z = X[:, rng.permutation(n)[:m]] + 0.01 * rng.normal(size=(d, m))
    return np.asfortranarray(X), y, np.asfortranarray(Z)


def relinf(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


# ---- an 80-bit (x87 long double) evaluation of the FITC mean coefficients and evidence from the textbook formulas:
# dense Cholesky / substitution loops in numpy longdouble (eps 1.1e-19), independent of LAPACK and of the oracle's
# operation sequence.  Cov_se_iso only; a few thousand points, a few hundred inducing points.
def _ld_chol_upper(A):
    m = A.shape[0]
    U = np.zeros_like(A)
    for j in range(m):
        U[j, j] = np.sqrt(A[j, j] - np.dot(U[:j, j], U[:j, j]))
        U[j, j + 1:] = (A[j, j + 1:] - U[:j, j] @ U[:j, j + 1:]) / U[j, j]
    return U


def longdouble_fitc(X, y, Z, log_ell, log_sf2, sigma2, jitter=1e-6, Xt=None):
    """Returns (l, t) in float64 -- with test inputs Xt also the posterior means K_tm t and variances
    sf2 - |K_tm U^-1|^2 + |K_tm R^-1|^2, R = R~ U (lib/fitc_gp.ml:418-425, :498-518) -- from an evaluation in numpy longdouble: U = chol(K_m + jitter I), V = K_nm U^-1,
    s = sf2 - |V_i|^2 + sigma2, B~ = I + V^T S^-1 V = R~^T R~, t = U^-1 R~^-1 R~^-T V^T (y / s),
    l = -1/2 (log|B~| + sum log s + n log 2 pi) - 1/2 (y^T S^-1 y - |R~^-T V^T (y/s)|^2)."""
    LD = np.longdouble
    assert np.finfo(LD).eps < 1e-18, "numpy longdouble is not an extended type here"
    Xl, Zl, yl = np.asarray(X, LD), np.asarray(Z, LD), np.asarray(y, LD)
    n, m = Xl.shape[1], Zl.shape[1]
    ie, sf2 = np.exp(LD(-2) * LD(log_ell)), np.exp(LD(log_sf2))

    def cov(A, B):
        return sf2 * np.exp(LD(-0.5) * ie * ((A.T[:, None, :] - B.T[None, :, :]) ** 2).sum(-1))

    U = _ld_chol_upper(cov(Zl, Zl) + LD(jitter) * np.eye(m, dtype=LD))
    K = cov(Xl, Zl)
    V = np.zeros_like(K)
    for j in range(m):
        V[:, j] = (K[:, j] - V[:, :j] @ U[:j, j]) / U[j, j]
    s = sf2 - (V * V).sum(1) + LD(sigma2)
    R = _ld_chol_upper(np.eye(m, dtype=LD) + V.T @ (V / s[:, None]))
    c = V.T @ (yl / s)
    b = np.zeros_like(c)
    for i in range(m):
        b[i] = (c[i] - np.dot(R[:i, i], b[:i])) / R[i, i]
    tt = np.zeros_like(c)
    for i in range(m - 1, -1, -1):
        tt[i] = (b[i] - np.dot(R[i, i + 1:], tt[i + 1:])) / R[i, i]
    t = np.zeros_like(c)
    for i in range(m - 1, -1, -1):
        t[i] = (tt[i] - np.dot(U[i, i + 1:], t[i + 1:])) / U[i, i]
    l = (LD(-0.5) * (2 * np.sum(np.log(np.diag(R))) + np.sum(np.log(s)) + n * np.log(2 * LD(np.pi)))
         - LD(0.5) * (np.dot(yl, yl / s) - np.dot(b, b)))
    if Xt is None:
        return float(l), t.astype(np.float64)
    Kt = cov(np.asarray(Xt, LD), Zl)
    Vt = np.zeros_like(Kt)
    for j in range(m):
        Vt[:, j] = (Kt[:, j] - Vt[:, :j] @ U[:j, j]) / U[j, j]
    Qt = np.zeros_like(Kt)
    for j in range(m):   # Q_t = V_t R~^-1 = K_tm R^-1
        Qt[:, j] = (Vt[:, j] - Qt[:, :j] @ R[:j, j]) / R[j, j]
    var = sf2 - (Vt * Vt).sum(1) + (Qt * Qt).sum(1)
    return float(l), t.astype(np.float64), (Kt @ t).astype(np.float64), var.astype(np.float64)


def longdouble_fat_evidence(X, y, Z, log_sf2, sigma2, tproj=None, log_hetero=None, log_multiscales_m05=None, jitter=1e-6):
    """FITC log evidence of Cov_se_fat in numpy longdouble (all inputs may be longdouble arrays): values only --
    k(p, z_c) = sf2 exp(-1/2 sum_k [(p_k - z_kc)^2 / ms_kc + log ms_kc]) with p = tproj^T x, ms = exp(log_ms) + 1/2
    (1 without multiscales); K_m off-diagonal with scale ms_kr + ms_kc - 1, diagonal sf2 exp(-1/2 sum_k log(2 ms_kc - 1))
    + exp(log_hetero_c) + jitter  (lib/cov_se_fat.ml:62-75, :85-142, :224-252).  Used to difference numerically."""
    LD = np.longdouble
    Xl, Zl, yl = np.asarray(X, LD), np.asarray(Z, LD), np.asarray(y, LD)
    d, m = Zl.shape
    n = Xl.shape[1]
    lsf = LD(log_sf2)
    P = Xl if tproj is None else np.asarray(tproj, LD).T @ Xl
    ms = None if log_multiscales_m05 is None else np.exp(np.asarray(log_multiscales_m05, LD)) + LD(0.5)
    acc = np.zeros((n, m), LD)
    for k in range(d):
        diff = P[k, :][:, None] - Zl[k, :][None, :]
        acc += diff * diff if ms is None else diff * (diff / ms[k, :][None, :]) + np.log(ms[k, :][None, :])
    K = np.exp(lsf - LD(0.5) * acc)
    accm = np.zeros((m, m), LD)
    for k in range(d):
        diff = Zl[k, :][:, None] - Zl[k, :][None, :]
        if ms is None:
            accm += diff * diff
        else:
            sc = ms[k, :][:, None] + ms[k, :][None, :] - LD(1)
            accm += diff * (diff / sc) + np.log(sc)
    Km = np.exp(lsf - LD(0.5) * accm)
    dg = np.full(m, np.exp(lsf)) if ms is None else np.exp(lsf - LD(0.5) * np.log(2 * ms - 1).sum(0))
    if log_hetero is not None:
        dg = dg + np.exp(np.asarray(log_hetero, LD))
    Km[np.diag_indices(m)] = dg + LD(jitter)
    U = _ld_chol_upper(Km)
    V = np.zeros_like(K)
    for j in range(m):
        V[:, j] = (K[:, j] - V[:, :j] @ U[:j, j]) / U[j, j]
    s = np.exp(lsf) - (V * V).sum(1) + LD(sigma2)          # calc_diag = sf2 (lib/cov_se_fat.ml:222)
    R = _ld_chol_upper(np.eye(m, dtype=LD) + V.T @ (V / s[:, None]))
    c = V.T @ (yl / s)
    b = np.zeros_like(c)
    for i in range(m):
        b[i] = (c[i] - np.dot(R[:i, i], b[:i])) / R[i, i]
    return (LD(-0.5) * (2 * np.sum(np.log(np.diag(R))) + np.sum(np.log(s)) + n * np.log(2 * LD(np.pi)))
            - LD(0.5) * (np.dot(yl, yl / s) - np.dot(b, b)))


# ---- well-conditioned synthetic cases (tests/test_gpu_factors.py, tests/test_gpu_row_operands.py) ----------------------------
FACTOR_N_TRAIN = 800


def taken(stages):
    """The row path of an evaluation from the stage names of last_timings()"""
    return "small" if "p1_small" in stages else ("mid" if "p1_mid" in stages else ("engine" if "p1_trmm_V" in stages else "?"))


def oracle_km_full(ok, Z):
    """K_m as the oracle builds it (heteroskedastic noise on the diagonal, no jitter), full symmetric"""
    km, _ = O.spec_calc_shared_upper(ok, np.asfortranarray(Z))
    km = np.triu(np.nan_to_num(km, nan=0.0))
    return km + np.triu(km, 1).T


def cond_of(a):
    w = np.linalg.eigvalsh(a)
    return float(w[-1] / w[0]) if w[0] > 0 else np.inf


def factor_case(kind, n, m, d=None, D=None):
    """Inputs, targets, inducing points, Problem.eval arguments, the oracle's kernel, cond(K_m + jitter I) of a case whose
    length scale is CHOSEN as the largest of 0.8^k at which the oracle's K_m + jitter I has a condition number of at most 1e5
    (asserted here: the search may not run out).
    kind: "iso"; "fat_het" (Cov_se_fat, heteroskedastic noise); "fat_proj_het" (... and a projection from D input dimensions,
    d + 2 by default, D >= d); "fat_ms" (Cov_se_fat with multiscales); "fat_proj_ms" (multiscales and a projection, no noise); "fat_het_ms" (noise and multiscales); "fat_proj_het_ms" (all three options).  d defaults to 2 for "iso" and 3 otherwise.
    The points are synth(900 + m, max(n, 800, m), m, d) with the first n training points kept: up to 800 training points every
    n shares the inducing points (and so the length scale) of its m, and n < m is possible."""
    if d is None:
        d = 2 if kind == "iso" else 3
    X, y, Z = synth(900 + m, max(n, FACTOR_N_TRAIN, m), m, d)
    X, y = np.asfortranarray(X[:, :n]), y[:n].copy()
    het = None if kind in ("iso", "fat_ms", "fat_proj_ms") else np.random.default_rng(m).uniform(-7.0, -4.0, size=m)
    tproj = lms = None
    if kind in ("fat_proj_het", "fat_proj_ms", "fat_proj_het_ms"):
        # tproj = Q A with Q (D x d) orthonormal and A a perturbed identity; the inputs are Q x plus a part orthogonal to
        # Q that the projection removes, so the projected points are A^T x and the inducing points A^T z
        rng = np.random.default_rng(1000 + m)
        D = d + 2 if D is None else D
        assert D >= d, (D, d)
        Q, _ = np.linalg.qr(rng.normal(size=(D, d)))
        A = np.eye(d) + 0.1 * rng.uniform(-1.0, 1.0, size=(d, d))
        off = rng.normal(size=(D, n))
        X = np.asfortranarray(Q @ X + (off - Q @ (Q.T @ off)))
        tproj = np.asfortranarray(Q @ A)
        Z = np.asfortranarray(A.T @ Z)
    if kind in ("fat_ms", "fat_proj_ms", "fat_het_ms", "fat_proj_het_ms"):
        lms = np.asfortranarray(np.random.default_rng(2000 + m).uniform(-1.0, 0.5, size=(d, m)))
    ell = 1.0
    for _ in range(40):
        if kind == "iso":
            ok, Zs = O.SeIsoKernel(float(np.log(ell)), 0.0), Z
        else:  # Cov_se_fat has unit length scales: the points carry the scale
            ok, Zs = O.SeFatKernel(d, 0.0, tproj, het, lms), np.asfortranarray(Z / ell)
        cond = cond_of(oracle_km_full(ok, Zs) + O.CHOLESKY_JITTER * np.eye(m))
        if cond <= 1e5:
            break
        ell *= 0.8
    assert cond <= 1e5, (kind, m, ell, cond)
    if kind == "iso":
        args = dict(log_ell=float(np.log(ell)), log_sf2=0.0)
        Xs = X
    else:
        args = dict(log_sf2=0.0)
        if het is not None:
            args["log_hetero_skedasticity"] = het
        if tproj is not None:
            args["tproj"] = tproj
        if lms is not None:
            args["log_multiscales_m05"] = lms
        Xs = np.asfortranarray(X / ell)
    return Xs, y, Zs, args, ok, cond


# ---- the gradient operands of Deriv Trained.calc / prepare_hyper (lib/fitc_gp.ml:1037-1207) in numpy longdouble ---------------
def _ld_triu_inverse(U):
    """U^-1 of an upper-triangular longdouble matrix, column by column (back substitution)"""
    m = U.shape[0]
    Ui = np.zeros_like(U)
    for j in range(m):
        Ui[j, j] = 1 / U[j, j]
        for i in range(j - 1, -1, -1):
            Ui[i, j] = -np.dot(U[i, i + 1:j + 1], Ui[i + 1:j + 1, j]) / U[i, i]
    return Ui


def _ld_matmul(a, b):
    """a @ b for longdouble matrices, the rows of a split over a few threads (numpy's longdouble matmul has no BLAS behind it
    and releases the GIL); every entry is the same dot product as in a @ b, so the result is bit-identical to it.  Its only
    purpose is the run time of the CPU suite: a 800 x 1100 by 1100 x 1100 product takes 7.8 s in one thread and 1.0 s in eight,
    the restatement of the n = 800, m = 1100 case 68 s and 16 s."""
    rows = a.shape[0]
    nt = max(1, min(8, os.cpu_count() or 1))
    if a.ndim != 2 or b.ndim != 2 or nt == 1 or rows * a.shape[1] * b.shape[1] < 2e6:
        return a @ b
    cuts = np.linspace(0, rows, min(rows, 4 * nt) + 1).astype(int)
    with ThreadPoolExecutor(nt) as ex:
        parts = list(ex.map(lambda i: a[cuts[i]:cuts[i + 1]] @ b, range(len(cuts) - 1)))
    return np.vstack(parts)


def longdouble_operands(km_full, knm, sf2, y, sigma2, variational=False, jitter=1e-6):
    """An 80-bit restatement of what the oracle's model_calc_with_kn_diag, cm_calc, deriv_trained_calc, trained_prepare_hyper
    and model_prepare_hyper compute, from the SAME K_m (full symmetric, heteroskedastic noise included, no jitter) and K_nm --
    taken as exact -- through textbook formulas instead of the reference's QR:
        U = chol(K_m + jitter I), V = K_nm U^-1, r = sf2 - |V_i|^2, s = r + sigma2, R^T R = K_m + jitter I + K_mn S^-1 K_nm,
        Q = S^-1/2 K_nm R^-1, T = (U^T U)^-1 - (R^T R)^-1, v1 = (1 - |Q_i|^2) / s  [variational: (2 - r/s - |Q_i|^2) / s],
        t = R^-1 Q^T S^-1/2 y, w = (S^-1/2 y - Q Q^T S^-1/2 y) / sqrt s, v = v1 - w^2,
        Um = K_nm (U^T U)^-1, Sm = S^-1 K_nm (R^T R)^-1,
        W = T - t t^T - Um^T diag(v) Um, X = Sm - diag(v) Um - w t^T;  model only: W1 = T - Um^T diag(v1) Um, X1 = Sm - diag(v1) Um.
    Cholesky and triangular inverses are plain loops in longdouble.  Returns a dict of float64 arrays (W, W1 full symmetric)."""
    LD = np.longdouble
    assert np.finfo(LD).eps < 1e-18, "numpy longdouble is not an extended type here"
    m = km_full.shape[0]
    A = np.asarray(km_full, LD) + LD(jitter) * np.eye(m, dtype=LD)
    K, yl = np.asarray(knm, LD), np.asarray(y, LD)
    mm = _ld_matmul
    Ui = _ld_triu_inverse(_ld_chol_upper(A))
    V = mm(K, Ui)
    r = LD(sf2) - (V * V).sum(1)
    s = r + LD(sigma2)
    is_ = 1 / s
    sq = np.sqrt(is_)
    Ri = _ld_triu_inverse(_ld_chol_upper(A + mm(K.T, K * is_[:, None])))
    Q = mm(K * sq[:, None], Ri)
    qd = (Q * Q).sum(1)
    inv_km, inv_b = mm(Ui, Ui.T), mm(Ri, Ri.T)
    T = inv_km - inv_b
    v1 = is_ * (2 - is_ * r - qd) if variational else is_ * (1 - qd)
    y_ = yl * sq
    qty = Q.T @ y_
    t = Ri @ qty
    w = (y_ - Q @ qty) * sq
    v = v1 - w * w
    Um = mm(V, Ui.T)
    Sm = mm(Q * sq[:, None], Ri.T)
    out = dict(r=r, is_=is_, v=v, w=w, t=t, v1=v1,
               W=T - np.outer(t, t) - mm(Um.T, Um * v[:, None]), X=Sm - Um * v[:, None] - np.outer(w, t),
               W1=T - mm(Um.T, Um * v1[:, None]), X1=Sm - Um * v1[:, None])
    return {k: np.asarray(a, np.float64) for k, a in out.items()}
