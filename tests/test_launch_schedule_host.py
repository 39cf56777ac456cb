"""The launch schedules of tests/launch_schedule.py on the CPU oracle alone: the boundaries sit where the GPU tests
(tests/test_gpu_launch_boundaries.py) need them and no launch is idle.  A schedule that has lost its edges fails here, without a GPU."""
import numpy as np
import pytest

import launch_schedule as ls
from optical_networking_gym import _native as nat

POLICIES = {"nsfnet96": ls.LEAN_POLICIES, "nobeleu128": (ls.FF, ls.LB), "alpha": (ls.FF, ls.GENERIC_ONLY_POLICY)}


@pytest.mark.parametrize("key", sorted(POLICIES))
def test_chopped_schedule_on_the_oracle(key):
    """Built from first fit's terminal steps; every policy the partition test runs has the same terminal steps, passes the
    placement asserts in every replica and sees an accepted request, a blocked request and a departure in every launch of 60 steps
    or more."""
    recs, _ = ls.oracle_run(key, ls.FF)
    lengths = ls.build_chopped(recs)
    terms = ls.terminal_indices(recs)
    assert len(terms) == 6 and sum(lengths) == ls.T
    for pol in POLICIES[key]:
        precs, _ = ls.oracle_run(key, pol)
        assert ls.terminal_indices(precs) == terms, pol
        where = ls.check_chopped(lengths, precs)
        ls.check_activity(precs, lengths, None, f"{key} policy {pol}")
        assert precs["active"].max() > 60
    rel = [where[t][1] for t in terms]
    assert (rel[0], rel[2], rel[3], rel[4], rel[5]) == (62, 62, 63, 64, 0) and lengths[where[terms[0]][0]] == 63
    # pops, not steps, move the ring: the 63-step launch that ends with t1 drains it exactly; 63 / 64 / 65 make 63 / 65 / 65
    pops = ls.launch_pops(lengths, terms)
    i = next(j for j in range(len(lengths)) if lengths[j:j + 3] == [63, 64, 65])
    assert pops[i:i + 3] == [63, 65, 65] and pops[where[terms[0]][0]] == ls.RING
    assert {ls.RING - 1, ls.RING, ls.RING + 1} <= set(pops)
    # the wide lean build is pinned by services of 40 slots
    if key == "nobeleu128":
        assert recs["nslots"].max() == 40


def test_every_edge_launch_runs_recorded_and_unrecorded():
    """Launches with a terminal step or the ring's edge are recorded by one partition case and unrecorded by another of the same
    kernel family, and every step is recorded by one of them."""
    groups = {}
    for key, pol, parity, generic, kind in ls.PARTITION_CASES:
        lean = ls.CONFIGS[key]["lean"] and not generic and pol in ls.LEAN_POLICIES
        groups.setdefault((key, lean, generic, kind), set()).add(parity)
    assert all(p == {0, 1} for p in groups.values()), groups
    recs, _ = ls.oracle_run("nsfnet96", ls.FF)
    lengths = ls.build_chopped(recs)
    edges = ls.edge_launches(lengths, ls.terminal_indices(recs))
    assert len(edges) >= 7             # one per terminal step, and the launch of 65 steps
    for i in range(len(lengths)):
        assert {ls.recorded(i, 0), ls.recorded(i, 1)} == {True, False}


@pytest.mark.parametrize("kind", ["edge", "inside"])
def test_trace_schedules_on_the_oracle(kind):
    """Replica 0's first no-op step on launch boundaries ('edge') or inside a launch, its failing pop being the one that first
    refills the ring ('inside': launch-relative step 64 for this trace, a terminal step in the launch pops twice); three no-op
    launches behind it; some other replica's trace runs out inside a launch."""
    lengths, recs, valid, rel = ls.partition_schedule("trace", kind)
    terms = ls.terminal_indices(recs, int(valid.min()))
    assert ls.TRACE_N - 6 <= valid.min() and valid.max() <= ls.TRACE_N
    st = ls.starts_of(lengths)
    if kind == "inside":
        assert rel == 64 and ls.pops_before_exhaustion(int(valid[0]) - rel, int(valid[0]), terms) == ls.RING
        inside = [r for r in range(1, ls.B) if int(valid[r]) not in st]
        assert inside, "no other replica's trace runs out inside a launch"
    else:
        assert rel == 0
    ls.check_activity(recs, lengths, valid, f"trace {kind}")
    assert sum(lengths) < ls.TRACE_STEPS
    for r in range(ls.B):               # the oracle was not stepped past the end of the trace
        assert not recs[int(valid[r]):, r]["accepted"].any()


@pytest.mark.parametrize("key", ["nsfnet96", "nobeleu128", "nsfnet96_ids"])
def test_mixed_schedule_on_the_oracle(key):
    """The mixed plan holds a retry, a QoT error, an accepted external action, a terminal step in an action segment, one masked
    reset and one counters-only reset mid-episode (mixed_plan asserts these), and every kind of segment."""
    plan = ls.mixed_plan(key)
    kinds = [s.kind for s in plan]
    assert set(ls.KINDS) <= set(kinds) and kinds[0] == "start"
    assert ("counters" in kinds) == (key == "nsfnet96_ids") and ("counters_refused" in kinds) == (key != "nsfnet96_ids")
    ls.check_mixed(plan, key)
    bundle = [s for s in plan if s.kind == "bundle_lb"]
    assert any(s.want["terminated"].any() for s in bundle)          # the auto-reset inside action-then-policy
    for s in bundle:                                                # the bundle's next action is the next call's action
        assert np.array_equal(s.next_actions[:-1], s.actions[1:])
    after_reset = plan[kinds.index("reset")].after.stats
    assert all(after_reset[r]["episode_services_processed"] == 1 and after_reset[r]["active"] == 0 for r in ls.RESET_REPLICAS)
    assert all(after_reset[r]["active"] > 0 for r in range(ls.B) if r not in ls.RESET_REPLICAS)
    if key == "nsfnet96_ids":
        st = plan[kinds.index("counters")].after.stats
        assert all(st[r]["episode_services_processed"] == 0 and st[r]["active"] > 0 for r in ls.COUNTERS_REPLICAS)
    assert not any((s.after.stats["flags"] & nat.F_OVERFLOW).any() for s in plan)
