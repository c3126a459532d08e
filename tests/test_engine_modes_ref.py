"""The reference and bound code of tools/engine_modes_check.hip (tools/engine_modes_ref.h) on the CPU: an emulated launch
passes its check; one dropped k-term, a wrong-signed beta, a shifted batch window, a write below the diagonal of an
upper_only launch and one read from a skipped operand block each fail it (tests/cpp/engine_modes_selftest.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_and_bound_selftest(tmp_path):
    exe = str(tmp_path / "engine_modes_selftest")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "tools"),
                    os.path.join(ROOT, "tests", "cpp", "engine_modes_selftest.cpp"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("selftest f64 ", "selftest f32 "))]
    assert out.returncode == 0 and len(lines) == 20, out.stdout[-3000:]
    assert all(ln.endswith(" OK") for ln in lines), out.stdout[-3000:]
    assert sum("unperturbed" in ln and "-> passes" in ln for ln in lines) == 6
    for what in ("one k-term dropped", "beta with the wrong sign", "second batch window shifted",
                 "a tile below the diagonal written", "one element of a skipped operand block read"):
        hit = [ln for ln in lines if what in ln]
        assert hit and all("-> fails" in ln for ln in hit), what
    assert out.stdout.strip().splitlines()[-1] == "selftest failed: 0"
