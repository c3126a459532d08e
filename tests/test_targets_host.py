"""Several target vectors on one model: the host-visible side, without a GPU -- the C header declares the three entry
points, the built library exports them, the ctypes table and the Python layers carry them, a program against the C++ mirror's new calls
builds."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gprhip_set_targets_many", "gprhip_eval_targets", "gprhip_predict_targets")


def _header():
    return open(os.path.join(ROOT, "include", "gprhip.h")).read()


def test_header_declares_the_three_entry_points():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*gprhip_problem\s*\*" % name, text), name
    assert re.search(r"#define\s+GPRHIP_MAX_TARGETS\s+16\b", text)
    fields = re.search(r"typedef struct \{([^}]*)\} gprhip_targets_result;", text).group(1)
    assert re.findall(r"(\w+);", fields) == ["l1", "l_sum", "dl_dsigma2_sum", "n_hypers", "k"]
    # gprhip_hypers keeps its 11 fields
    assert len(re.findall(r"(\w+);", re.search(r"typedef struct \{([^}]*)\} gprhip_hypers;", text).group(1))) == 11


def test_library_exports_them_and_the_binding_table_matches():
    from gpr_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), "libgprhip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    assert _lib.MAX_TARGETS == 16
    assert [f for f, _ in _lib.TargetsResult._fields_] == ["l1", "l_sum", "dl_dsigma2_sum", "n_hypers", "k"]
    assert ctypes.sizeof(_lib.TargetsResult) == 40  # three doubles, one int64, one int padded to 8


def test_python_layers_carry_the_feature():
    from gpr_amd import cov_se_iso, fitc_gp
    from gpr_amd.problem import Problem, TargetsEvaluation
    for name in ("set_targets_many", "eval_targets", "predict_targets"):
        assert callable(getattr(Problem, name))
    assert [f for f in TargetsEvaluation.__dataclass_fields__] == ["l1", "l2", "l", "l_sum", "dl_dsigma2_sum", "grad_sum", "coeffs"]
    GP = fitc_gp.Make_deriv(cov_se_iso)
    for variant in (GP.FITC, GP.Variational_FITC):
        assert callable(variant.Deriv.Trained.calc_many)
        for name in ("calc_many", "calc_log_evidence", "calc_log_evidences", "calc_mean_coeffs", "calc_means_many"):
            assert callable(getattr(variant.Eval.Trained, name)), name


def test_cpp_mirror_names_the_calls_and_still_builds(tmp_path):
    hpp = open(os.path.join(ROOT, "include", "gprhip.hpp")).read()
    for name in NEW:
        assert name + "(" in hpp, name
    src = tmp_path / "many.cpp"
    src.write_text('#include "gprhip.hpp"\n'
                   "int main() {\n"
                   "  gpr::Evaluation_many e;\n"
                   "  auto f = &gpr::Make_deriv<gpr::Cov_se_iso>::run_many;   // (instantiates the templates)\n"
                   "  auto g = &gpr::Make_deriv<gpr::Cov_se_fat>::means_many;\n"
                   "  return (int)e.l.size() + GPRHIP_MAX_TARGETS - 16 + (f == nullptr) + (g == nullptr);\n"
                   "}\n")
    exe = tmp_path / "many"
    libdir = os.path.join(ROOT, "gpr_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-lgprhip", "-Wl,-rpath," + libdir, "-o", str(exe)])
