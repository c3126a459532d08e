"""gprhip_observe in 80 bits from a GIVEN pre-state: R~ (m x m upper), b (m), U^-1 (m x m upper), the kernel and the inducing
points (debug_fetch "rtil", "bvec", "uinv").  Imports nothing from the library or the oracle: the CPU and the GPU tests share it.

    V = K U^-1 at the new points,  r_i = sf2 - |v_i|^2,  s_i = r_i + sigma2,  W = diag(1/sqrt(s)) V,  eta = y / sqrt(s)
    by definition :  R~' = chol(R~^T R~ + W^T W) (upper),  b' = R~'^-T (R~^T b + W^T eta)
    by reflectors :  the sequence of gpr_amd/csrc/tp_reflect.h, one reflector per pivot column, in 80 bits
    rho = what the QR leaves of eta,  |eta|^2 + |b|^2 = |b'|^2 + |rho|^2
    dl1 = -1/2 (2 sum_j log(R~'_jj / R~_jj) + sum_i log s_i + k log 2 pi)   (-1/2 sum r_i / s_i more, variational)
    dl2 = -1/2 |rho|^2

The bound of the GPU test is column-wise, in Higham's form for Householder QR (Accuracy and Stability, Theorem 19.4): column
c of the factor is the product of c + 1 reflectors of k + 1 entries applied to (R~[:, c]; W[:, c]), so
    |dR~'[:, c]|_2 <= C (k + 1) (c + 1) u |(R~[:, c]; W[:, c])|_2 .
Theory does not fix C; profiles/observe_margins.txt holds the measured ratios it was taken from.
"""
import numpy as np

from tests import posterior_ref as PR

LD = np.longdouble
U = 2.0 ** -53
LOG_2PI = LD("1.8378770664093454835606594728112353")

DEFECTS = ("unstable_v1", "negative_diagonal", "s_without_sigma2", "skipped_column", "stale_b")


def _ld(a):
    return None if a is None else np.asarray(a, dtype=LD)


def rows(Xnew, Z, uinv, sigma2, y=None, defect=None, **kernel):
    """W (k x m), eta (k), s, r at the new points Xnew (D x k); kernel: the keywords of posterior_ref.geometry."""
    g = PR.geometry(Xnew, Z, **kernel)
    V = g["K"] @ np.triu(_ld(uinv))
    r = g["sf2"] - (V * V).sum(1)
    s = r + (LD(0) if defect == "s_without_sigma2" else LD(sigma2))
    rt = np.sqrt(s)
    return dict(W=V / rt[:, None], eta=None if y is None else _ld(y) / rt, s=s, r=r, V=V)


def chol_upper(A):
    A = np.array(A, dtype=LD)
    m = A.shape[0]
    R = np.zeros((m, m), LD)
    for j in range(m):
        d = A[j, j] - R[:j, j] @ R[:j, j]
        assert d > 0, "not positive definite"
        R[j, j] = np.sqrt(d)
        if j + 1 < m:
            R[j, j + 1:] = (A[j, j + 1:] - R[:j, j] @ R[:j, j + 1:]) / R[j, j]
    return R


def solve_upper_t(R, x):
    """R^-T x"""
    m = R.shape[0]
    y = np.zeros(m, LD)
    for i in range(m):
        y[i] = (x[i] - R[:i, i] @ y[:i]) / R[i, i]
    return y


def inv_upper(R):
    m = R.shape[0]
    X = np.zeros((m, m), LD)
    for j in range(m - 1, -1, -1):
        X[j, j] = LD(1) / R[j, j]
        if j + 1 < m:
            X[j, j + 1:] = -(R[j, j + 1:] @ X[j + 1:, j + 1:]) / R[j, j]
    return X


def update_definition(Rt, b, W, eta):
    R, Wl = np.triu(_ld(Rt)), _ld(W)
    Rn = chol_upper(R.T @ R + Wl.T @ Wl)
    out = dict(R=Rn, logdet=np.log(np.diag(Rn) / np.diag(R)).sum())
    if b is not None:
        bl, el = _ld(b), _ld(eta)
        out["b"] = solve_upper_t(Rn, R.T @ bl + Wl.T @ el)
        out["rho2"] = (el @ el + bl @ bl) - out["b"] @ out["b"]
    return out


def update_reflectors(Rt, b, W, eta, dtype=LD, defect=None, skip=None):
    """The sequence of tp_reflect.h in `dtype` (float64: what a correct device computes up to the order of its sums).
    defect: one of DEFECTS planted into it (skip: the column the "skipped_column" defect leaves alone)."""
    T = dtype
    R = np.triu(np.asarray(Rt, dtype=T))
    Wl = np.array(W, dtype=T)
    k, m = Wl.shape
    bl = None if b is None else np.array(b, dtype=T)
    el = None if b is None else np.array(eta, dtype=T)
    ld = T(0)
    for j in range(m):
        w = Wl[:, j].copy()
        sigma = w @ w
        alpha = R[j, j]
        if not sigma > T(2.0 ** -120) * alpha * alpha:      # the identity, as tp_reflect.h takes it
            continue
        mu = np.sqrt(alpha * alpha + sigma)
        v1 = alpha - mu if defect == "unstable_v1" else -sigma / (alpha + mu)
        if v1 == 0:
            continue
        beta = T(-1) / (mu * v1)
        ld += T(0.5) * np.log1p(sigma / (alpha * alpha))
        R[j, j] = -mu if defect == "negative_diagonal" else mu
        if j + 1 < m:
            cols = np.arange(j + 1, m)
            if defect == "skipped_column":
                cols = cols[cols != (m - 1 if skip is None else skip)]
            t = beta * (v1 * R[j, cols] + w @ Wl[:, cols])
            R[j, cols] -= t * v1
            Wl[:, cols] -= np.outer(w, t)
        if bl is not None and defect != "stale_b":
            t = beta * (v1 * bl[j] + w @ el)
            bl[j] -= t * v1
            el -= t * w
    out = dict(R=R, logdet=ld)
    if bl is not None:
        out["b"] = bl
        out["rho"] = el
        out["rho2"] = el @ el
    return out


def dlog_evidence(s, r, logdet, rho2, variational):
    s, r = _ld(s), _ld(r)
    dl1 = -LD(0.5) * (2 * LD(logdet) + np.log(s).sum() + s.shape[0] * LOG_2PI)
    if variational:
        dl1 += -LD(0.5) * (r / s).sum()
    return dl1 + (LD(0) if rho2 is None else -LD(0.5) * LD(rho2))


def column_scale(Rt, W, b=None, eta=None):
    """|(R~[:, c]; W[:, c])|_2 per column, the b | eta column last when given"""
    R, Wl = np.triu(_ld(Rt)), _ld(W)
    sc = np.sqrt((R * R).sum(0) + (Wl * Wl).sum(0))
    if b is not None:
        sc = np.append(sc, np.sqrt(_ld(b) @ _ld(b) + _ld(eta) @ _ld(eta)))
    return sc


def column_ratios(got_R, ref_R, Rt, W, got_b=None, ref_b=None, b=None, eta=None):
    """Per column c: |got[:, c] - ref[:, c]|_2 / ((k + 1) (c + 1) u |(R~[:, c]; W[:, c])|_2); the b column counts as column m.
    The bound of the test is C times the denominator."""
    k, m = np.asarray(W).shape
    err = np.sqrt(((_ld(got_R) - _ld(ref_R)) ** 2).sum(0))
    if got_b is not None:
        err = np.append(err, np.sqrt(((_ld(got_b) - _ld(ref_b)) ** 2).sum()))
    sc = column_scale(Rt, W, b if got_b is not None else None, eta)
    den = (k + 1) * np.arange(1, err.shape[0] + 1) * U * sc
    return np.asarray(np.where(err > 0, err / np.where(den > 0, den, LD(1e-300)), 0), np.float64)


def inverse_bound(Rn, X):
    """|X_dev - R~'^-1| <= (m + 8) u |X| |R~'| |X| entry by entry (Higham, section 14.1: triangular inversion by any of the
    blocked methods), with the 80-bit inverse X of the device's own R~'.  Where a product lies below the smallest normal
    number the device holds a subnormal or zero: each of the m products behind an entry carries the absolute allowance
    eta = 2^-1022 times the row's |X| besides, as the K entries of posterior_ref do."""
    aX, aR = np.abs(_ld(X)), np.abs(np.triu(_ld(Rn)))
    m = Rn.shape[0]
    return np.asarray(PR.FIRST_ORDER * (m + 8) * U * (aX @ aR @ aX) + m * PR.ETA * (1 + aX.sum(1))[:, None], np.float64)


def coeff_bound(X, uinv, b):
    """t = U^-1 (R~'^-1 b') from the device's own operands: two mat-vecs of length <= m, the first one's error carried
    through the second"""
    m = X.shape[0]
    aX, aU, ab = np.abs(_ld(X)), np.abs(np.triu(_ld(uinv))), np.abs(_ld(b))
    return np.asarray(PR.FIRST_ORDER * (2 * m + 4) * U * (aU @ (aX @ ab)) + m * PR.ETA * (1 + aU.sum(1)), np.float64)


def posterior_from_scratch(X, y, Z, Xt, sigma2, jitter=1e-6, log_het=None, variational=False, **kernel):
    """The FITC posterior of a training set from nothing but its definition, in 80 bits (lib/fitc_gp.ml:151-182, :285-294,
    :418-425, :498-518): means and variances (without sigma2) at Xt, the log evidence, and the state (R~, b, U^-1, t)."""
    gz = PR.geometry(Z, Z, **dict(kernel, tproj=None))   # (the inducing points live in the projected space)
    m = gz["m"]
    Km = np.array(gz["K"], dtype=LD)
    Km[np.diag_indices(m)] += LD(jitter) + (0 if log_het is None else np.exp(_ld(log_het)))
    Um = chol_upper(Km)
    Ui = inv_upper(Um)
    g = PR.geometry(X, Z, **kernel)
    V = g["K"] @ Ui
    r = g["sf2"] - (V * V).sum(1)
    s = r + LD(sigma2)
    Rt = chol_upper(np.eye(m, dtype=LD) + V.T @ (V / s[:, None]))
    out = dict(R=Rt, uinv=Ui)
    n = V.shape[0]
    l1 = -LD(0.5) * (2 * np.log(np.diag(Rt)).sum() + np.log(s).sum() + n * LOG_2PI)
    if variational:
        l1 += -LD(0.5) * (r / s).sum()
    gt = PR.geometry(Xt, Z, **kernel)
    Vt = gt["K"] @ Ui
    Qt = Vt @ inv_upper(Rt)
    out["variances"] = g["sf2"] - (Vt * Vt).sum(1) + (Qt * Qt).sum(1)
    out["l1"] = l1
    if y is not None:
        yl = _ld(y)
        b = solve_upper_t(Rt, V.T @ (yl / s))
        t = Ui @ (inv_upper(Rt) @ b)
        out.update(b=b, t=t, means=gt["K"] @ t, l=l1 - LD(0.5) * ((yl * yl / s).sum() - b @ b))
    return out
