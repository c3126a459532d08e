"""The chunk plan of the calls that evaluate the model at test points (gpr_amd/csrc/predict_plan.h), checked without a GPU:
tests/cpp/predict_plan_check.cpp pins the rule to a table and sweeps random call sequences, as a program of its own under the
address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_plan_table_and_sweep_under_the_sanitizers(tmp_path):
    """The table: training chunk 2048 (and 131072), nt from 100 to 1 000 000, with and without the chunk's matrices in memory,
    at several sizes of the buffers kept from earlier calls.  The sweep: a call of at most 131072 points that does not fit the
    training chunk is one chunk, the chunk never exceeds the buffers the plan says will exist, and no buffer shrinks."""
    exe = tmp_path / "predict_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "predict_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "predict_plan_check: ok" in out.stdout, out.stderr[-2000:]
