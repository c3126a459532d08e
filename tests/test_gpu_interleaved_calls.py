"""The calls that evaluate a model at test points share their chunk buffers on the problem (gprhip_predict,
_predict_input_grad, _acquire, _sample_paths: one chunk plan, one allocation step, one walk over the chunks).  Here they run
one after the other on ONE problem, through both growths of the buffers and back to a size in between, and every output must
be bit for bit what the same call gives on a freshly created and evaluated problem: what a call computes does not depend on
what ran before it, on which buffers it found or on where they lie.

Models (n = 300, so the training chunk is 384 rows): m = 8, d = 2 on the one-kernel path; m = 130 (two tile columns) on the
engine path; and the engine model behind a D x d projection, whose host gradients keep both staging areas live."""
import functools

import numpy as np
import pytest

from tests.test_gpu_input_grad import _case
from tests.test_gpu_predict_grad import _problem, _test_points

gpu = pytest.mark.gpu
N = 300
CHUNK = 384                      # the training chunk of n = 300: n rounded up to the 128-row tile
NT_SMALL = 100                   # inside the training chunk
NT_GROW1 = 8 * CHUNK + 1         # the first growth: 3200 rows (3073 rounded up; more than 8 training chunks)
NT_GROW2 = 5000                  # the second growth: 5120 rows
NT_PATHS = 200
NT_BETWEEN = 4000                # 4096 rows: between the two growths, served by the buffers of the second
MODELS = {"one_kernel": ("iso", N, 8, 2), "engine": ("iso", N, 130, 2), "engine_proj": ("proj", N, 130, 2, 4)}
STEPS = ["predict", "predict_input_grad", "acquire", "sample_paths", "predict_between"]


def _call(p, key, step):
    """One step of the sequence on p: a dict of its output arrays"""
    if step in ("predict", "predict_between"):
        means, variances = p.predict(_test_points(key, NT_SMALL if step == "predict" else NT_BETWEEN))
        return dict(means=means, variances=variances)
    if step == "predict_input_grad":
        return p.predict_input_grad(_test_points(key, NT_GROW1))
    if step == "acquire":
        return p.acquire(_test_points(key, NT_GROW2), "ei", maximise=True, best=0.0, want=("values", "dvalues"), top_k=5)
    m = _case(*key)[2].shape[1]
    rng = np.random.default_rng(77)
    z, eps = rng.standard_normal((m, 4)), rng.standard_normal((NT_PATHS, 4))
    return p.sample_paths(_test_points(key, NT_PATHS), z, eps=eps, top_k=3)


@functools.lru_cache(maxsize=None)
def _fresh(name, step):
    """the step on a problem of its own, created and evaluated for it: computed once, read only"""
    key = MODELS[name]
    p = _problem(key)
    try:
        out = _call(p, key, step)
    finally:
        p.close()
    for a in out.values():
        a.setflags(write=False)
    return out


@gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_interleaved_calls_equal_fresh_problems_bit_for_bit(name):
    key = MODELS[name]
    p = _problem(key)
    try:
        p.set_timing(2)
        for step in STEPS:
            got, ref = _call(p, key, step), _fresh(name, step)
            stages = p.last_timings()
            if step in ("predict_input_grad", "acquire"):  # the path the model was chosen for
                assert ("pg_cov" in stages) == (name != "one_kernel"), (name, step, stages)
            assert set(got) == set(ref), (name, step)
            for what in sorted(ref):
                same = np.array_equal(got[what], ref[what], equal_nan=True)
                differ = 0 if same else int(np.sum(~((got[what] == ref[what]) | (np.isnan(got[what]) & np.isnan(ref[what])))))
                print("%s.%s.%s: %d of %d entries differ" % (name, step, what, differ, ref[what].size))
                assert same, (name, step, what, differ)
            if step == "acquire":
                assert np.all(ref["top_index"] >= 0) and np.all(np.isfinite(ref["top_dvalues"]))
            if step == "sample_paths":
                assert np.all(ref["top_index"] >= 0) and np.all(np.isfinite(ref["top_dvalues"]))
    finally:
        p.close()
