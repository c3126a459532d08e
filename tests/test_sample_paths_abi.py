"""gprhip_sample_paths in every layer: declared in the header, exported by the library, bound in gpr_amd/_lib.py, named by the
C++ mirror, the OCaml stubs and the OCaml module; the Python layers carry it; the refusals that need no device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gprhip_sample_paths"


def test_symbol_is_declared_in_every_layer_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gprhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gprhip_problem\s*\*\s*p,\s*const\s+double\s*\*\s*z,\s*int64_t\s+ldz,\s*int\s+ns,"
                     r"\s*const\s+double\s*\*\s*test_inputs,\s*int64_t\s+ld,\s*int64_t\s+nt,\s*const\s+double\s*\*\s*eps,"
                     r"\s*int64_t\s+lde,\s*int\s+predictive,\s*double\s*\*\s*samples,\s*int64_t\s+lds,\s*int\s+maximise,"
                     r"\s*int\s+top_k,\s*int64_t\s*\*\s*top_index,\s*double\s*\*\s*top_values,\s*double\s*\*\s*top_dvalues,"
                     r"\s*int\s+on_device\s*\)" % NAME, header)
    assert re.search(r"#define\s+GPRHIP_MAX_DRAWS\s+64\b", header)
    from gpr_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 18 and _lib.MAX_DRAWS == 64
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "libgprhip.so does not export %s" % NAME
    assert NAME + "(" in open(os.path.join(ROOT, "include", "gprhip.hpp")).read()
    assert NAME + "(" in open(os.path.join(ROOT, "bindings", "gpr_hip_stubs.c")).read()
    ml = open(os.path.join(ROOT, "bindings", "gpr_hip.ml")).read()
    assert '"gprhip_ml_sample_paths"' in ml and "module Path_sampler = struct" in ml


def test_python_layers_carry_the_feature():
    from gpr_amd import cov_se_fat, cov_se_iso, fitc_gp
    from gpr_amd.problem import Problem
    assert callable(Problem.sample_paths)
    for spec in (cov_se_iso, cov_se_fat):
        GP = fitc_gp.Make_deriv(spec)
        for variant in (GP.FITC, GP.Variational_FITC):
            ps = variant.Eval.Path_sampler
            assert callable(ps.calc) and callable(ps.samples) and callable(ps.best)
    code = "import sys, gpr_amd; assert 'torch' not in sys.modules; assert callable(gpr_amd.Problem.sample_paths)"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_refusals_that_need_no_device():
    """Every refusal that does not look at the problem comes before anything touches it: checked with a NULL problem (itself
    refused, last) -- the status, the function's name and the reason in gprhip_last_error()."""
    from gpr_amd import _lib
    from gpr_amd.problem import Problem
    lib = _lib.load()
    buf = np.zeros(8)
    idx = np.zeros(64, dtype=np.int64)
    vp = ctypes.c_void_p
    dp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def call(ns=1, samples=True, top_k=0, top_index=None):
        return lib.gprhip_sample_paths(None, dp, 1, ns, vp(buf.ctypes.data), 1, 1, None, 0, 0,
                                       vp(buf.ctypes.data) if samples else None, 1, 1, top_k, top_index, None, None, 0)

    cases = [(dict(ns=0), b"ns"), (dict(ns=65), b"ns"), (dict(top_k=-1, top_index=ip), b"top_k"),
             (dict(top_k=65, top_index=ip), b"top_k"), (dict(top_k=3), b"top_index"),
             (dict(samples=False), b"nothing is requested"), (dict(), b"invalid arguments"),
             (dict(ns=64, top_k=64, top_index=ip), b"invalid arguments")]
    for kw, reason in cases:
        assert call(**kw) == _lib.EBADARG, kw
        msg = lib.gprhip_last_error()
        assert msg.startswith(NAME.encode()) and reason in msg, (kw, msg)
    p = Problem.__new__(Problem)
    p._h = ctypes.c_void_p()  # (nothing to destroy)
    p.D, p.m = 2, 3
    with pytest.raises(ValueError):
        Problem.sample_paths(p, np.zeros((2, 3)), np.zeros((4, 2)))           # z is not m x ns
    with pytest.raises(ValueError):
        Problem.sample_paths(p, np.zeros((3, 3)), np.zeros((3, 2)))           # test inputs are not D x nt
    with pytest.raises(ValueError):
        Problem.sample_paths(p, np.zeros((2, 3)), np.zeros((3, 2)), eps=np.zeros((2, 2)))   # eps is not nt x ns
    with pytest.raises(ValueError):
        Problem.sample_paths(p, 0, np.zeros((3, 2)), out_device_ptrs={})      # device buffers need nt
    with pytest.raises(TypeError):                                            # device buffers: eps is an address, not an array
        Problem.sample_paths(p, 0, np.zeros((3, 2)), eps=np.zeros((2, 2)), out_device_ptrs={}, nt=2)
    with pytest.raises(ValueError):                                           # eps is no output
        Problem.sample_paths(p, 0, np.zeros((3, 2)), out_device_ptrs={"eps": 1}, nt=2)


def test_cpp_mirror_methods_build(tmp_path):
    """Path_sampler of include/gprhip.hpp compiles and links against the library (no device call)."""
    src = tmp_path / "use.cpp"
    src.write_text('#include "gprhip.hpp"\n'
                   "using GP = gpr::Make_deriv<gpr::Cov_se_iso>;\n"
                   "int main(int argc, char**) {\n"
                   "  if (argc < 2) return 2;\n"
                   "  auto* calc = &GP::FITC::Path_sampler::calc;\n"
                   "  auto* samples = &GP::FITC::Path_sampler::samples;\n"
                   "  auto* best = &GP::FITC::Path_sampler::best;\n"
                   "  return calc && samples && best ? 0 : 1;\n"
                   "}\n")
    exe = tmp_path / "use"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", libdir, "-lgprhip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    assert subprocess.run([str(exe)], timeout=60).returncode == 2
