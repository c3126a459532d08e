"""The two refinement calls share their arena (the box, the state and trial points of the starts, the staging of host
outputs), the pinned count of starts that go on, and -- with gprhip_sample_paths -- the pinned draws and the weight buffers.
Here gprhip_acquire_refine, gprhip_sample_paths and gprhip_sample_paths_refine run one after the other on ONE problem:
through the growth of the arena (5 starts, then 70: more than one workgroup of 64), the switch from three integer vectors
to four and back, a count of starts inside the grown arena, and a last call with fewer draws.  Every output must be bit for
bit what the same call gives on a freshly created and evaluated problem, the weights the last call left behind included.

Models (n = 300): m = 8, d = 2 -- the one-kernel route of both calls; m = 130 -- the library-side loop of the acquisition
call and the one-kernel path call; the same behind a D x d projection -- the library-side loop of both calls."""
import functools

import numpy as np
import pytest

import gpr_amd
from tests.test_gpu_input_grad import _case
from tests.test_gpu_predict_grad import _problem, _test_points

gpu = pytest.mark.gpu
N = 300
NT_PATHS = 200
MAX_EVALS = 12
NAMES = gpr_amd.Problem.REFINE_OUTPUTS
MODELS = {"one_kernel": ("iso", N, 8, 2), "engine": ("iso", N, 130, 2), "engine_proj": ("proj", N, 130, 2, 4)}
# step: (call, draws, starts)
STEPS = {"acquire_refine_5": ("acquire_refine", 0, 5), "sample_paths": ("sample_paths", 4, NT_PATHS),
         "paths_refine_70": ("sample_paths_refine", 3, 70), "acquire_refine_33": ("acquire_refine", 0, 33),
         "paths_refine_5": ("sample_paths_refine", 1, 5), "sp_a": ("sp_a", 1, 0)}
# the stage that tells the route of a refinement call, per model
ROUTE = {"acquire_refine": {"one_kernel": "rf_small", "engine": "rf_step", "engine_proj": "rf_step"},
         "sample_paths_refine": {"one_kernel": "prf_kernel", "engine": "prf_kernel", "engine_proj": "prf_eval"}}


def _call(p, key, step):
    """One step of the sequence on p: a dict of its output arrays"""
    call, nd, ns = STEPS[step]
    Xs, Zs = _case(*key)[0], _case(*key)[2]
    m = Zs.shape[1]
    box = dict(lower=Xs.min(1), upper=Xs.max(1), max_evals=MAX_EVALS, want=NAMES)
    z = np.random.default_rng(77 + nd).standard_normal((m, max(nd, 1)))
    if call == "acquire_refine":
        return p.acquire_refine(_test_points(key, ns, seed=1), "ei", maximise=True, best=0.0, var_floor=1e-10, **box)
    if call == "sample_paths":
        return p.sample_paths(_test_points(key, ns), z, eps=np.random.default_rng(78).standard_normal((ns, nd)), top_k=3)
    if call == "sample_paths_refine":
        return p.sample_paths_refine(_test_points(key, ns, seed=2), z, (np.arange(ns) % nd).astype(np.int32), **box)
    return dict(sp_a=p.debug_fetch_matrix("sp_a"))


@functools.lru_cache(maxsize=None)
def _fresh(name, step):
    """the step on a problem of its own, created and evaluated for it: computed once, read only.  The weights are those the
    last call of the sequence leaves behind."""
    key = MODELS[name]
    p = _problem(key)
    try:
        if step == "sp_a":
            _call(p, key, "paths_refine_5")
        out = _call(p, key, step)
    finally:
        p.close()
    for a in out.values():
        a.setflags(write=False)
    return out


@gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_interleaved_refinement_calls_equal_fresh_problems_bit_for_bit(name):
    key = MODELS[name]
    p = _problem(key)
    try:
        p.set_timing(2)
        for step in STEPS:
            got, ref = _call(p, key, step), _fresh(name, step)
            call = STEPS[step][0]
            if call in ROUTE:  # the route the model was chosen for
                assert ROUTE[call][name] in p.last_timings(), (name, step, p.last_timings())
            assert set(got) == set(ref), (name, step)
            for what in sorted(ref):
                same = np.array_equal(got[what], ref[what], equal_nan=True)
                differ = 0 if same else int(np.sum(~((got[what] == ref[what]) | (np.isnan(got[what]) & np.isnan(ref[what])))))
                print("%s.%s.%s: %d of %d entries differ" % (name, step, what, differ, ref[what].size))
                assert same, (name, step, what, differ)
            if call in ROUTE:  # the call did some work: no start ends at its first evaluation everywhere
                assert np.all(np.isfinite(ref["values"])) and np.max(ref["evals"]) > 1, (name, step)
            if step == "sample_paths":
                assert np.all(ref["top_index"] >= 0) and np.all(np.isfinite(ref["top_dvalues"]))
            if step == "sp_a":
                assert ref["sp_a"].shape == (_case(*key)[2].shape[1], 1) and np.all(np.isfinite(ref["sp_a"]))
    finally:
        p.close()
