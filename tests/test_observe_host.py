"""tests/observe_ref.py on the CPU: its two routes to the updated factor agree, its evidence difference is the oracle's, the
entry-wise check of tests/test_gpu_observe.py catches planted defects, and the reflector text the device compiles
(gpr_amd/csrc/tp_reflect.h) holds the same bound in double against long double under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import fitc_oracle as FO
from tests import observe_ref as O
from tests.test_gpu_input_grad import _case
from tests.test_gpu_input_grads import Case, data, hypers_of
from tests.test_gpu_parity import TOL_L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA2 = 0.1
N = 120
C_BOUND = 4.0   # tests/test_gpu_observe.py
LD = np.longdouble


@pytest.fixture(scope="module")
def state():
    """an 80-bit pre-state of n = 120 rows, m = 40, rounded to double as the device would hold it, and k = 5 new points"""
    c = Case("iso", N + 5, 40, 3)
    X, y, Z, args = data(c)
    kern = hypers_of(c, args)
    Xt = np.asfortranarray(X[:, :4])
    pre = O.posterior_from_scratch(np.asfortranarray(X[:, :N]), y[:N], Z, Xt, SIGMA2, **kern)
    f64 = lambda a: np.asarray(a, np.float64)
    return dict(c=c, X=X, y=y, Z=Z, args=args, kern=kern, Rt=f64(pre["R"]), b=f64(pre["b"]), uinv=f64(pre["uinv"]),
                Xn=np.asfortranarray(X[:, N:N + 5]), yn=y[N:N + 5].copy())


def test_the_two_references_agree(state):
    s = state
    rw = O.rows(s["Xn"], s["Z"], s["uinv"], SIGMA2, s["yn"], **s["kern"])
    a = O.update_definition(s["Rt"], s["b"], rw["W"], rw["eta"])
    r = O.update_reflectors(s["Rt"], s["b"], rw["W"], rw["eta"])
    ratios = O.column_ratios(r["R"], a["R"], s["Rt"], rw["W"], r["b"], a["b"], s["b"], rw["eta"])
    assert ratios.max() < 1e-2            # 80 bits against 80 bits, in units of the 53-bit bound
    assert abs(float(a["logdet"] - r["logdet"])) < 1e-17 * 40 and abs(float(a["rho2"] - r["rho2"])) < 1e-16


@pytest.mark.parametrize("variational", [False, True])
def test_the_evidence_difference_is_the_oracles(state, variational):
    s = state
    c = s["c"]
    ok = _case(c.kind, c.n, c.m, c.d, c.D, c.het, c.offset)[4]
    X, y = s["X"], s["y"]
    l0 = FO.evaluate_fast(ok, s["Z"], np.asfortranarray(X[:, :N]), y[:N], SIGMA2, variational=variational)["l"]
    l1 = FO.evaluate_fast(ok, s["Z"], np.asfortranarray(X[:, :N + 5]), y[:N + 5], SIGMA2, variational=variational)["l"]
    rw = O.rows(s["Xn"], s["Z"], s["uinv"], SIGMA2, s["yn"], **s["kern"])
    a = O.update_definition(s["Rt"], s["b"], rw["W"], rw["eta"])
    dl = float(O.dlog_evidence(rw["s"], rw["r"], a["logdet"], a["rho2"], variational))
    assert abs(dl - (l1 - l0)) <= TOL_L * abs(l1), (dl, l1 - l0)


@pytest.mark.parametrize("defect", O.DEFECTS)
def test_the_entry_wise_check_catches_a_planted_defect(state, defect):
    """the sequence in double passes the check of the GPU test; with one defect planted it does not"""
    s = state
    rw = O.rows(s["Xn"], s["Z"], s["uinv"], SIGMA2, s["yn"], **s["kern"])
    ref = O.update_definition(s["Rt"], s["b"], rw["W"], rw["eta"])
    W64, e64 = np.asarray(rw["W"], np.float64), np.asarray(rw["eta"], np.float64)

    def worst(**kw):
        W, e = W64, e64
        if kw.get("defect") == "s_without_sigma2":
            bad = O.rows(s["Xn"], s["Z"], s["uinv"], SIGMA2, s["yn"], defect="s_without_sigma2", **s["kern"])
            W, e, kw = np.asarray(bad["W"], np.float64), np.asarray(bad["eta"], np.float64), {}
        got = O.update_reflectors(s["Rt"], s["b"], W, e, dtype=np.float64, **kw)
        return O.column_ratios(got["R"], ref["R"], s["Rt"], rw["W"], got["b"], ref["b"], s["b"], rw["eta"]).max()

    assert worst() <= C_BOUND
    assert worst(defect=defect) > C_BOUND     # (beyond the bound: the check fails)


def test_the_unstable_reflector_is_caught_where_it_cancels():
    """v1 = R~_jj - R~'_jj cancels when |W[:, j]| is small against R~_jj: a new point far from most inducing points"""
    rng = np.random.default_rng(4)
    m, k = 30, 3
    Rt = np.triu(rng.normal(size=(m, m)) * 0.3) + np.diag(2.0 + rng.uniform(size=m))
    W = rng.normal(size=(k, m)) * 1e-5
    b, eta = rng.normal(size=m), rng.normal(size=k)
    ref = O.update_definition(Rt, b, W, eta)
    good = O.update_reflectors(Rt, b, W, eta, dtype=np.float64)
    bad = O.update_reflectors(Rt, b, W, eta, dtype=np.float64, defect="unstable_v1")
    r = lambda g: O.column_ratios(g["R"], ref["R"], Rt, W, g["b"], ref["b"], b, eta).max()
    assert r(good) <= C_BOUND < r(bad)


def test_reflector_text_under_the_sanitizers(tmp_path):
    """tests/cpp/tp_reflect_check.cpp: the blocked update of tp_reflect.h in double against long double on the GPU test's
    shapes, sigma = 0 columns, a pivot of 1e-150 under W entries of 1e150; its worst normalised ratio stays within C."""
    exe = tmp_path / "tp_reflect_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "tp_reflect_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "tp_reflect_check: ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    worst = float(re.search(r"worst ratio \S+ normalised (\S+)", out.stdout).group(1))
    print(out.stdout[-200:])
    assert worst <= C_BOUND
