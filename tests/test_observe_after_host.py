"""tests/observe_after_cases.py on the CPU: HostDevice plays the device in float64 -- the pre-observation factors of each case
updated by observe_ref.update_reflectors(dtype=np.float64), every output formed in double from the updated factors -- and
  (a) the honest outputs pass every check of ratios(), the checks of tests/test_gpu_observe_after.py: cases and checks agree;
  (b) with one fault of FAULTS planted, every output the fault can reach (REACH) misses its bound by a factor of at least 100,
      on every case: the GPU tests can fail.  The 100 is a condition on the cases (new rows close enough to the test points),
      not a tolerance: honest error sits below 1.
Part (b) prints the smallest violation factor per fault and output over the cases."""
import numpy as np
import pytest

from tests import observe_after_cases as OA

# (case, the observe calls of the route) -- routes A / B (k = 1, 64), C (64 then 3) and D (k = 3: the state before is the restored one)
HOST = [OA.State(r, "base", c, k, path) for c, path in OA.SHAPES for r, k in (("A", 1), ("A", 64), ("C", 3), ("D", 3))] + \
    [OA.State("A", v, c, 3, "mid") for v, c in OA.VARIANTS if v == "fat-proj-het"]
WORST = {}


def states_of(s):
    """(the state the calls read, the state a fault reads instead)"""
    pre = OA.host_pre_state(s.c)
    post = pre
    for Xn, yn in OA.rows_of(s):
        before, post = post, OA.host_observe(s.c, post, Xn, yn)
    if s.route == "D":
        return pre, post          # restored: the factors of before; what a restore may leave behind is the observed state
    return post, before


@pytest.mark.parametrize("s", HOST, ids=OA.state_id)
def test_new_rows_sit_where_the_test_points_look(s):
    for Xn, yn in OA.rows_of(s):
        assert OA.near_share(s.c, Xn) >= 1.0 / 3.0, OA.near_share(s.c, Xn)


@pytest.mark.parametrize("s", HOST, ids=OA.state_id)
def test_honest_outputs_pass_every_check(s):
    st, _ = states_of(s)
    dev = OA.HostDevice(s.c, st)
    r = OA.ratios(dev, s.c, dev.fetch())
    print({k: "%.3g" % v for k, v in r.items()})
    assert set(r) == set(OA.OUTPUTS) and max(r.values()) <= 1.0, r


# (the restore fault belongs to route D, the others to the observed states)
@pytest.mark.parametrize("s,fault", [(s, f) for f in OA.FAULTS for s in HOST if (f == "restore_keeps_m") == (s.route == "D")], ids=OA.state_id)
def test_a_planted_fault_misses_the_bound_of_every_output_it_reaches_by_100(s, fault):
    st, stale = states_of(s)
    dev = OA.HostDevice(s.c, st, fault, stale)
    r = OA.ratios(dev, s.c, dev.fetch(), only=OA.REACH[fault])
    for name in OA.REACH[fault]:
        WORST[fault, name] = min(WORST.get((fault, name), np.inf), r[name])
        print("%s -> %s: %.3g x its bound (smallest so far %.3g)" % (fault, name, r[name], WORST[fault, name]))
        assert r[name] >= 100.0, (fault, name, r[name])


def test_smallest_violation_factors():
    """(runs last: the table of part (b))"""
    for (fault, name), v in sorted(WORST.items()):
        print("%-24s %-18s smallest violation factor %.3g" % (fault, name, v))
    assert WORST and min(WORST.values()) >= 100.0
