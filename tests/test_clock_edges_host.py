"""The conditions that keep tests/test_gpu_clock_edges.py from passing emptily, on the oracle alone (no GPU).

For every pattern of tests/clock_edges.py the `<=` model (rel = float32(at + ht); after step t everything with rel <= at[t + 1]
has left) is the oracle's `active` at every step, and the traces hold what they are there for: enough steps on which a release
time equals the clock, enough arrivals that do not advance it, enough steps on which a strict `<` would leave another `active`.
The minimum counts are conditions on the traces, fixed before any kernel ran; with another seed that misses one, the seed changes,
not the count.
"""
import numpy as np
import pytest

import clock_edges as ce
from optical_networking_gym import _native as nat
from oracle_lib import OracleEnv

ALL_CONFIGS = tuple(ce.CONFIGS)


@pytest.mark.parametrize("key", ALL_CONFIGS)
def test_model_is_the_oracle_on_every_pattern(key):
    """First fit (and load balancing where a lean kernel runs it) on every configuration the GPU tests use: the <= model gives
    the oracle's `active` at every step of every pattern, and the strict twin does not on the patterns built for it."""
    for policy in (ce.FF, ce.LB) if key in ce.LEAN_CONFIGS else (ce.FF,):
        run = ce.trace_run(key, ce.schedule_of(policy))
        for r, name in enumerate(ce.PATTERNS):
            c = ce.edge_counts(run.at[r], run.ht[r], run.recs[:, r])
            assert c["model_ok"], (key, policy, name)
            assert not run.recs["terminated"][:, r].any() and not (run.recs["flags"][:, r] & nat.F_NO_REQUEST).any(), (key, name)
            if name in ("grid", "late_trace") or name.startswith("drain"):
                assert c["strict_differs"] >= 2, (key, policy, name, c["strict_differs"])


@pytest.mark.parametrize("key", ce.GRID_CONFIGS)
def test_grid_counts(key):
    run = ce.trace_run(key)
    r = ce.row("grid")
    at, ht = run.at[r], run.ht[r]
    assert np.array_equal(at, np.round(at)) and np.array_equal(ht, np.round(ht)) and at.max() + ht.max() < 2 ** 24   # exact in float32
    c = ce.edge_counts(at, ht, run.recs[:, r])
    assert c["model_ok"]
    assert c["equalities"] >= 100 and c["zero_advances"] >= 100 and c["strict_differs"] >= 100, c


@pytest.mark.parametrize("key", ce.LEAN_CONFIGS)
def test_late_trace_counts(key):
    run = ce.trace_run(key)
    r = ce.row("late_trace")
    assert run.at[r].min() >= 2.0 ** 28 and np.spacing(run.at[r][0]) == 32.0
    c = ce.edge_counts(run.at[r], run.ht[r], run.recs[:, r])
    assert c["model_ok"]
    assert c["equalities"] >= 100 and c["zero_advances"] >= 100 and c["strict_differs"] >= 100, c


def test_late_gen_counts():
    """The generator from a late clock: orc_seed keeps the state, the clock and the pending request of the trace step."""
    run = ce.late_gen_run()
    assert (run.first["accepted"] == 1).all() and (run.first["active"] == 0).all()      # the first service left at the late draw
    for r, (base, least) in enumerate(zip(ce.LATE_BASES, (80, 20))):
        assert run.at[r][0] == np.float32(base) and run.ht[r][0] == 7.0                 # the pending request was the trace's second
        assert (np.diff(run.at[r]) >= 0).all() and run.at[r][-1] > base
        c = ce.edge_counts(run.at[r], run.ht[r], run.recs[:, r])
        assert c["model_ok"], r
        assert c["equalities"] >= least and c["zero_advances"] >= least and c["strict_differs"] >= least, (r, c)
        assert run.oracles[r].stats()["current_time"] == float(run.at[r][-1])


@pytest.mark.parametrize("key", ce.LEAN_CONFIGS + ("offtable", "alpha"))
def test_drain_counts(key):
    """All m requests are accepted, one step releases m minus the keepers, and `active` drops from m - 1 to at most 7 on it."""
    run = ce.trace_run(key)
    for m in ce.DRAIN_M:
        r = ce.row(f"drain{m}")
        rec = run.recs[:, r]
        le = ce.edge_counts(run.at[r], run.ht[r], rec)["le"]
        keep = ce.keepers_of(m)
        assert rec["accepted"][:m].all(), (key, m)
        assert (rec["active"][:m - 1] == np.arange(1, m)).all()          # nothing left before: record index = request index
        assert le["departures"][m - 1] == m - len(keep) and le["equalities"][m - 1] == m - len(keep)
        assert rec["active"][m - 2] == m - 1 and rec["active"][m - 1] == len(keep) <= 7
        assert le["zero_advance"][m] == 1 and run.ht[r][m] == 0.0        # the arrival at 1000 leaves at the second arrival at 1000
        assert le["equalities"][m] == 1 and le["departures"][m] == 1
        assert len(run.at[r]) - (m + 3) >= 40
    assert ce.keepers_of(330) == [0, 63, 64, 255, 256, 329] and 330 - 6 == 324
    assert [len(ce.keepers_of(m)) for m in ce.DRAIN_M] == [2, 3, 4, 5, 6]


def test_zero_and_infinite_holding_times():
    """An accepted zero-holding service is gone at the very next arrival; an accepted infinite one is there at the end."""
    key, r = "nsfnet320", ce.row("zero_inf")
    trace = ce.traces(key)[r]
    o = OracleEnv(ce.holder_of(key), replica=r)
    o.set_trace(trace)
    o.reset()
    zeros = infs = 0
    acc = np.zeros(ce.N - 1, bool)
    for t in range(ce.N - 1):
        before = o.stats()["active"]
        rec = o.run_policy(ce.FF, 1)[0]
        acc[t] = bool(rec["accepted"])
        if acc[t] and trace["holding_time"][t] == 0.0:
            zeros += 1
            svc = o.services()
            assert not (svc["release_time"] == trace["arrival_time"][t]).any(), t
            assert rec["active"] <= before                               # it came and went within the step
        infs += int(acc[t] and np.isinf(trace["holding_time"][t]))
    assert zeros >= 40, zeros
    end = o.services()
    assert infs >= 40 and int(np.isinf(end["release_time"]).sum()) == infs
    run = ce.trace_run(key)
    assert np.array_equal(run.recs["accepted"][:, r].astype(bool), acc)
    assert len(ce.edge_counts(run.at[r], run.ht[r], run.recs[:, r])["le"]["running"]) == len(end)


def test_backsteps_release_nothing():
    run = ce.trace_run("nsfnet320")
    r = ce.row("backsteps")
    le = ce.edge_counts(run.at[r], run.ht[r], run.recs[:, r])["le"]
    back = np.flatnonzero(np.diff(run.at[r]) < 0)                        # step t draws request t + 1 at an earlier time
    assert len(back) >= 10
    assert (le["departures"][back] == 0).all()
    prev = np.concatenate([[0], run.recs["active"][:-1, r]])
    assert (run.recs["active"][back, r] == prev[back] + run.recs["accepted"][back, r]).all()
    assert le["departures"].sum() > 100                                  # and the other steps do release


@pytest.mark.parametrize("key,policy", [("nsfnet320", ce.HSNR), ("nobeleu256", ce.LF)])
def test_windows_of_the_costly_policies_hold_the_edges(key, policy):
    """Highest SNR and lowest fragmentation take only the windows of schedule_of: every drain step lies in one, and the
    windows hold equalities and zero advances of grid and late_trace."""
    sch = ce.schedule_of(policy)
    assert sum(n for _, n in sch) == ce.N - 1
    mine = ce.schedule_steps(sch, policy)
    assert 25 <= mine.sum() <= 40
    run = ce.trace_run(key, sch)
    for r, name in enumerate(ce.PATTERNS):
        c = ce.edge_counts(run.at[r], run.ht[r], run.recs[:, r])
        assert c["model_ok"], name
        if name.startswith("drain"):
            m = int(name[5:])
            assert mine[m - 2:m + 1].all()
            assert c["le"]["departures"][m - 1] >= m - 12                # (lowest fragmentation's step refuses some of its own choices)
        if name in ("grid", "late_trace"):
            assert c["le"]["equalities"][mine].sum() >= 10 and c["le"]["zero_advance"][mine].sum() >= 4
        if name == "backsteps":
            assert (np.diff(run.at[r])[mine] < 0).any()
        if name == "zero_inf":
            assert (run.ht[r][mine] == 0).any() and np.isinf(run.ht[r][mine]).any()
