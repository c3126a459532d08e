"""Posterior sample paths (gprhip_sample_paths): what can be checked without a GPU -- the longdouble reference the GPU tests
use (tests/sample_paths_ref.py) against the oracle's own posterior (predict_means, predict_variances, fic_covariances) and
central differences of itself, and the host-side argument checks and cross-chunk merge under the address and
undefined-behaviour sanitizers (tests/cpp/sample_paths_check.cpp, a program of its own)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import fitc_oracle as O
from tests.sample_paths_ref import path_state, sample_paths_from_state, sample_paths_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
N, M, NT, SIGMA2 = 12, 4, 5, 0.3
H = 2.0 ** -13
KINDS = ["iso", "fat", "fat_proj", "fat_proj_het"]


def _case(kind):
    rng = np.random.default_rng(5)
    D = 3 if kind in ("fat_proj", "fat_proj_het") else 2
    X = np.asfortranarray(rng.normal(size=(D, N)))
    Xt = np.asfortranarray(rng.normal(size=(D, NT)))
    if kind == "iso":
        k = O.SeIsoKernel(0.2, 0.1)
    elif kind == "fat":
        k = O.SeFatKernel(2, 0.1, None)
    else:
        het = rng.uniform(-3.0, -1.0, size=M) if kind == "fat_proj_het" else None
        k = O.SeFatKernel(2, 0.1, np.asfortranarray(0.7 * rng.normal(size=(3, 2))), het)
    Z = np.asfortranarray(rng.normal(size=(2, M)))
    y = np.sin(X.sum(0)) + 0.1 * rng.normal(size=N)
    return k, Z, X, y, Xt


@pytest.mark.parametrize("variational", [False, True], ids=["standard", "variational"])
@pytest.mark.parametrize("kind", KINDS)
def test_reference_is_the_oracles_posterior(kind, variational):
    """With Z = I_m the columns of L = F - mu 1^T are the factor of the posterior covariance: (L L^T)_rs equals the oracle's
    fic_covariances off the diagonal, sum_j L_rj^2 + resid_r its predict_variances (predictive=False), and z = 0 gives its
    predict_means -- to 1e-11 of the largest entry (two evaluation orders of a small, well-conditioned case, one of them fp64)."""
    k, Z, X, y, Xt = _case(kind)
    out = O.evaluate(k, Z, X, y, SIGMA2, variational=variational, want_grad=False, keep=True)
    model, coeffs = out["model"], out["coeffs"]
    mu = O.predict_means(k, Z, coeffs, Xt)
    zero = sample_paths_ref(k, Z, X, y, SIGMA2, Xt, np.zeros((M, 1)))
    assert np.max(np.abs(zero["paths"][:, 0] - mu)) <= 1e-11 * np.max(np.abs(mu))
    ident = sample_paths_ref(k, Z, X, y, SIGMA2, Xt, np.eye(M))
    L = ident["paths"] - zero["paths"]
    cov = O.fic_covariances(k, Z, model, Xt)
    cov = np.triu(cov) + np.triu(cov, 1).T
    LLt = L @ L.T
    off = ~np.eye(NT, dtype=bool)
    assert np.max(np.abs(cov[off])) > 1e-4
    assert np.max(np.abs(LLt[off] - cov[off])) <= 1e-11 * np.max(np.abs(cov))
    var = O.predict_variances(k, Z, model, Xt, predictive=False)
    assert np.max(np.abs((L * L).sum(1) + ident["resid"] - var)) <= 1e-11 * np.max(np.abs(var))
    assert np.all(ident["resid"] > 0)
    pred = sample_paths_ref(k, Z, X, y, SIGMA2, Xt, np.zeros((M, 1)), predictive=True)
    assert np.allclose(pred["resid"], ident["resid"] + SIGMA2, rtol=0, atol=1e-15)
    # samples = paths + sqrt(resid) eps
    rng = np.random.default_rng(3)
    z, eps = rng.normal(size=(M, 3)), rng.normal(size=(NT, 3))
    got = sample_paths_ref(k, Z, X, y, SIGMA2, Xt, z, eps=eps)
    assert np.allclose(got["samples"], got["paths"] + np.sqrt(got["resid"])[:, None] * eps, rtol=0, atol=1e-14)
    # a draw is linear in z around the mean
    assert np.allclose(got["paths"] - zero["paths"], L @ z, rtol=0, atol=1e-13)


@pytest.mark.parametrize("kind", KINDS)
def test_reference_gradient_against_central_differences(kind):
    """Every entry of the gradient of the path part against D(h) = (F(x + h) - F(x - h)) / 2h of the reference's own F, the
    steps formed in 80-bit arithmetic and rounded (h = 2^-13).  Bound per entry, as tests/test_predict_grad_host.py derives it:
    2 T + 256 * 2^-53 scale / h with T = |D(2h) - D(h)| / 3 (the third-derivative term, measured) and scale = sum |K| |A| (the
    oracle's K_tm is an fp64 quantity)."""
    k, Z, X, y, Xt = _case(kind)
    rng = np.random.default_rng(4)
    z = rng.normal(size=(M, 2))
    state = path_state(k, Z, X, y, SIGMA2)
    D = Xt.shape[0]
    pairs = [(r, j) for r in range(NT) for j in range(2)]
    got = sample_paths_from_state(k, Z, state, Xt, z, SIGMA2, grad_at=pairs)["grads"]
    assert got.shape == (D, len(pairs)) and np.max(np.abs(got)) > 1e-3
    ktm, _ = O.spec_calc_shared_cross(k, Xt, Z)
    from tests.sample_paths_ref import weights
    scale = float(np.max(np.abs(ktm) @ np.abs(weights(state, z).astype(np.float64))))
    worst = 0.0
    for e, (r, j) in enumerate(pairs):
        for b in range(D):
            vals = {}
            for step in (-2, -1, 1, 2):
                Xs = np.array(Xt, dtype=LD)
                Xs[b, r] = Xs[b, r] + LD(step) * LD(H)
                vals[step] = sample_paths_from_state(k, Z, state, np.asfortranarray(Xs.astype(np.float64)), z, SIGMA2)["paths"][r, j]
            d1 = (vals[1] - vals[-1]) / (2 * H)
            d2 = (vals[2] - vals[-2]) / (4 * H)
            bound = 2.0 * abs(d2 - d1) / 3.0 + 256 * 2.0 ** -53 * scale / H
            err = abs(got[b, e] - d1)
            worst = max(worst, err / bound)
            assert err <= bound, (kind, r, j, b, got[b, e], d1, err, bound)
    print("path-gradient reference vs central differences (%s): worst error / bound %.3f" % (kind, worst))


def test_host_side_checks_and_merge_under_the_sanitizers(tmp_path):
    """tests/cpp/sample_paths_check.cpp: every argument refusal of the entry point and the cross-chunk merge of the best-k
    lists (ties, NaN, -0, both directions, k beyond the count) against a stable sort, compiled with
    -fsanitize=address,undefined as a program of its own and run here."""
    exe = tmp_path / "sample_paths_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "sample_paths_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "sample_paths_check: ok" in out.stdout, out.stderr[-2000:]
