"""Departures on the edges of the clock in every step kernel (patterns, host model and oracle runs: tests/clock_edges.py).

A service leaves when float32(arrival + holding) <= float32(clock).  The rule is written in release_due (k_run, step(), playout),
in release_due_defrag and in the lean scan of k_fast, and each copy is compiled into many instantiations; the traces of
tests/clock_edges.py put equalities, zero advances, drains across the scan's chunk borders, zero and infinite holding times and a
clock that steps back in front of each of them, as replicas of one environment.  Every leg holds the device to the oracle:
step records (`active`, `flags` and `reward` exact, GSNR to 1e-9), the final grid, stats() (clock and counters), services() by
(path_id, slot, nslots, modulation, release_time) and spectrum_map(records=True): a clean audit and the oracle's release times.
tests/test_clock_edges_host.py asserts, without a GPU, that the traces hold the edges in the numbers they are there for.

Highest SNR and lowest fragmentation take the windows of clock_edges.schedule_of (their oracle restatements take 0.1 s per step
on these loads) and first fit walks between the windows.  A counters-only reset needs track_service_ids, which rules the lean
kernels out (ongym_reset_episode_counters refuses without it), so that leg runs on k_run alone: no call of the library brings a
release time of copysignf(inf) in front of k_fast.
"""
import numpy as np
import pytest

import clock_edges as ce
from common import record_bytes
from launch_schedule import force_generic
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from oracle_lib import OracleEnv
from test_gpu_parity import GSNR_RTOL, assert_records_equal

pytestmark = pytest.mark.gpu


def make_env(key, rows=ce.PATTERNS, generic=False, trace=None, **over):
    """The device environment of a configuration on the traces of `rows`, reset."""
    if trace is None:
        trace = np.ascontiguousarray(ce.traces(key)[[ce.row(n) for n in rows]])
    with force_generic(generic):
        env = BatchedQRMSAEnv(tables=ce.tables_of(key), batch_size=len(trace), **ce.config_kw(key, **over))
    env.set_requests(trace)
    env.reset()
    return env


def run_schedule(env, schedule):
    return np.concatenate([env.step_policy(n, policy=p) for p, n in schedule])


def check_final(env, oracles, ctx, ids=False, dropped=False):
    """The final state against the oracles': stats() (clock, counters; the GSNR sums to 1e-9), grids, services and the records
    and audit of spectrum_map.  ids: service ids and the OSNR defragmentation rewrites are compared too.  dropped: the services
    a counters-only reset left running for good (+inf on the device, off the oracle's heap) are held to the oracle by the grid."""
    bad = []
    st = env.stats()
    sm = env.spectrum_map(owners=False, records=True)
    if sm["audit"][:, 0].any():
        bad.append(f"audit: {sm['audit'].tolist()}")
    for r, o in enumerate(oracles):
        so = o.stats()
        for f in ce.COUNTERS:
            if not np.array_equal(st[r][f], so[f]):
                bad.append(f"replica {r}: stats {f} {st[r][f]} != {so[f]}")
        for f in ce.APPROX:
            if st[r][f] != pytest.approx(so[f], rel=GSNR_RTOL):
                bad.append(f"replica {r}: stats {f} {st[r][f]!r} != {so[f]!r}")
        if not np.array_equal(env.grid(r), o.grid()):
            bad.append(f"replica {r}: grid")
        got, want = env.services(r), o.services()
        n = len(got)
        rel = sm["release"][r]
        if not (np.array_equal(rel[:n], got["release_time"]) and np.isnan(rel[n:]).all() and (sm["records"][r, n:] == -1).all()):
            bad.append(f"replica {r}: spectrum_map's release times are not services()'s")
        if dropped:
            got = got[np.isfinite(got["release_time"])]
        order = ["service_id"] if ids else ["release_time", "path_id", "slot"]
        got, want = np.sort(got, order=order), np.sort(want, order=order)
        if len(got) != len(want):
            bad.append(f"replica {r}: {len(got)} services, the oracle has {len(want)}")
            continue
        for f in ce.SERVICE_FIELDS + (("service_id",) if ids else ()):
            if not np.array_equal(got[f], want[f]):
                bad.append(f"replica {r}: services {f}")
        if ids and not np.allclose(got["osnr"], want["osnr"], rtol=GSNR_RTOL, atol=0):
            bad.append(f"replica {r}: services osnr")
    assert not bad, f"{ctx}: {len(bad)} mismatches, the first:\n" + "\n".join(bad[:20])


def edges_in(run, policy, rows=ce.PATTERNS):
    """From the oracle's records: the steps `policy` takes hold equalities and zero advances of grid and late_trace and every
    drain step, and the <= model is the oracle's `active` everywhere (no leg passes emptily)."""
    mine = ce.schedule_steps(run.schedule, policy)
    for r, name in enumerate(rows):
        c = ce.edge_counts(run.at[r], run.ht[r], run.recs[:, r])
        assert c["model_ok"], name
        if name in ("grid", "late_trace"):
            assert c["le"]["equalities"][mine].sum() >= 10 and c["le"]["zero_advance"][mine].sum() >= 4, name
        if name.startswith("drain"):
            m = int(name[5:])
            assert mine[m - 1] and c["le"]["departures"][m - 1] >= m - 12, name


# ---- lean kernels, trace instantiations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ce.LEAN_POLICIES)
@pytest.mark.parametrize("key", ce.LEAN_CONFIGS)
def test_lean_kernels_replay_the_edges(key, policy):
    """k_fast<TRACE> of the four lean policies (the `depart` lambda carries lowest fragmentation's dirty-row bookkeeping):
    narrow at capacity 512 and 448 (the straight record scans), the wide build, and two mask words (nobel-eu, 41 links)."""
    sch = ce.schedule_of(policy)
    run = ce.trace_run(key, sch)
    edges_in(run, policy)
    env = make_env(key)
    for p in {p for p, _ in sch}:
        assert env.occupancy(p)["lean_kernel"]
    got = run_schedule(env, sch)
    for r, name in enumerate(ce.PATTERNS):
        assert_records_equal(got[:, r], run.recs[:, r], f"{key} policy {policy} {name}")
    check_final(env, run.oracles, f"{key} policy {policy}")


# ---- lean kernels, generator instantiations ----------------------------------------------------------------------------------------
def late_gen_env(key, first_policy):
    env = make_env(key, trace=ce.late_gen_trace(key))
    first = env.step_policy(1, policy=first_policy)
    env.seed(ce.GEN_SEED)                       # the generator takes over: state, clock and pending request stay
    return env, first


@pytest.mark.parametrize("policy", [ce.FF, ce.HSNR])
def test_lean_generator_from_a_late_clock(policy):
    """k_fast<TRACE = false>, the benchmark's instantiations, from a clock of 2^27 (replica 1: 2^25) - with records, and for
    first fit without them (the instantiation the benchmark times) against the same final state."""
    key = "nsfnet320"
    sch = ce.late_gen_schedule(policy)
    run = ce.late_gen_run(key, sch)
    mine = ce.schedule_steps(sch, policy)
    for r, least in enumerate((80, 20) if policy == ce.FF else (20, 4)):
        c = ce.edge_counts(run.at[r], run.ht[r], run.recs[:, r])
        assert c["model_ok"]
        assert c["le"]["equalities"][mine].sum() >= least and (c["le"]["zero_advance"][mine] > 0).sum() >= least, (r, c)
    env, first = late_gen_env(key, sch[0][0])
    assert env.occupancy(policy)["lean_kernel"] and env.occupancy(ce.FF)["lean_kernel"]
    assert_records_equal(first, run.first, "the trace step")
    got = run_schedule(env, sch)
    assert_records_equal(got, run.recs, f"late_gen policy {policy}")
    check_final(env, run.oracles, f"late_gen policy {policy}")
    assert env.stats()["current_time"].tolist() == [float(run.at[r][-1]) for r in range(2)]
    if policy == ce.FF:
        norec, _ = late_gen_env(key, ce.FF)
        assert norec.step_policy(ce.GEN_STEPS, record=False) is None
        check_final(norec, run.oracles, "late_gen first fit without records")


# ---- launch splits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["nsfnet320", "nobeleu256"])
def test_launch_splits_give_the_same_records(key):
    """next_rel is rebuilt at every launch start: launches of 1 step, of 7 steps and one launch write the same records."""
    run = ce.trace_run(key)
    whole = make_env(key).step_policy(run.steps)
    for r, name in enumerate(ce.PATTERNS):
        assert_records_equal(whole[:, r], run.recs[:, r], f"{key} {name}")
    for split in (1, 7):
        env = make_env(key)
        lengths = [split] * (run.steps // split) + ([run.steps % split] if run.steps % split else [])
        got = np.concatenate([env.step_policy(n) for n in lengths])
        assert record_bytes(got) == record_bytes(whole), f"{key}: launches of {split} steps"
        check_final(env, run.oracles, f"{key}: launches of {split} steps")


# ---- generic kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,generic,policy", [("nsfnet320", True, ce.FF), ("nsfnet320", True, ce.GENERIC_ONLY_POLICY),
                                                ("nobeleu256", True, ce.FF), ("offtable", False, ce.FF), ("alpha", False, ce.FF)],
                         ids=["forced", "forced-policy5", "forced-two-words", "off-table-bit-rates", "per-link-attenuation"])
def test_generic_kernel_replays_the_edges(key, generic, policy):
    """release_due in k_run: ONGYM_FORCE_GENERIC=1 (both record codecs), bit rates outside the table, per-link attenuation."""
    sch = ce.schedule_of(policy)
    run = ce.trace_run(key, sch)
    edges_in(run, policy)
    env = make_env(key, generic=generic)
    assert not env.occupancy(policy)["lean_kernel"]
    got = run_schedule(env, sch)
    for r, name in enumerate(ce.PATTERNS):
        assert_records_equal(got[:, r], run.recs[:, r], f"{key} policy {policy} {name}")
    check_final(env, run.oracles, f"{key} generic policy {policy}")


# ---- defragmentation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_defrag", [0, 3])
def test_defragmentation_on_ties(n_defrag):
    """release_due_defrag: services due at one instant leave in (float32 release time, service id) order, and a
    defragmentation runs after each of them, so the order shows in the moves: ids, rewritten OSNR and the defrag counters."""
    key, rows = "nsfnet320", ("grid", "late_trace")
    over = (("defragmentation", True), ("n_defrag_services", n_defrag))
    run = ce.trace_run(key, ce.schedule_of(ce.FF), over, rows)
    edges_in(run, ce.FF, rows)
    for r in range(len(rows)):
        le = ce.edge_counts(run.at[r], run.ht[r], run.recs[:, r])["le"]
        assert (le["departures"] >= 2).sum() >= 50                       # steps on which the order of the departures matters
        assert run.oracles[r].stats()["episode_service_reallocations"] > 100
    env = make_env(key, rows, **dict(over))
    got = env.step_policy(run.steps)
    for r, name in enumerate(rows):
        assert_records_equal(got[:, r], run.recs[:, r], f"n_defrag_services {n_defrag} {name}")
    check_final(env, run.oracles, f"n_defrag_services {n_defrag}", ids=True)


# ---- measure_disruptions ---------------------------------------------------------------------------------------------------------------
def test_disrupted_services_leave_on_time():
    """The sign bit of a stored release time is the 'disrupted' flag: a flagged service leaves on the equality like any other."""
    key, rows = "nsfnet320", ("grid", "zero_inf")
    over = (("measure_disruptions", True),)
    run = ce.trace_run(key, ce.schedule_of(ce.FF), over, rows)
    edges_in(run, ce.FF, rows)
    env = make_env(key, rows, **dict(over))
    got = env.step_policy(run.steps)
    st = env.stats()
    for r, name in enumerate(rows):
        assert_records_equal(got[:, r], run.recs[:, r], name)
        so = run.oracles[r].stats()
        assert so["disrupted_services"] >= 50
        assert st[r]["disrupted_services"] == so["disrupted_services"]
        assert st[r]["episode_disrupted_services"] == so["episode_disrupted_services"]
        assert int(env.services(r)["reserved"].sum()) <= so["disrupted_services"]      # some disrupted services have left
    check_final(env, run.oracles, "measure_disruptions")


# ---- external actions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bundle", [False, True], ids=["step", "step_bundle"])
def test_external_actions_release_on_the_edges(bundle):
    """The oracle's first-fit actions through step() and step_bundle() (k_run's action modes), on grid and the drains."""
    key, rows = "nsfnet320", ("grid",) + tuple(f"drain{m}" for m in ce.DRAIN_M)
    run = ce.external_run(key, rows)
    edges_in(run, ce.FF, rows)
    actions = np.ascontiguousarray(run.recs["action"])
    env = make_env(key, rows)
    got = np.zeros((run.steps, len(rows)), nat.STEP_DTYPE)
    for t in range(run.steps):
        if bundle:
            got[t], req, st, na, _ = env.step_bundle(actions[t], next_policy=ce.FF)
            if t + 1 < run.steps:
                np.testing.assert_array_equal(na, actions[t + 1], err_msg=f"next action after step {t}")
        else:
            got[t] = env.step(actions[t])
    for r, name in enumerate(rows):
        assert_records_equal(got[:, r], run.recs[:, r], name)
    if bundle:
        assert st.tobytes() == env.stats().tobytes()
    check_final(env, run.oracles, "external actions")


# ---- playout ----------------------------------------------------------------------------------------------------------------------------
def test_playout_across_the_drain():
    """playout(own_stream=True) from the state two steps before each drain step, with a horizon across it, against the oracle's
    own continuation; the playouts leave the replicas as they were."""
    key, H = "nsfnet320", 8
    run = ce.trace_run(key)
    acc, active = run.recs["accepted"].astype(np.int64), run.recs["active"].astype(np.int64)
    env = make_env(key)
    done, got = 0, []
    col = {n: i for i, n in enumerate(nat.PLAYOUT)}
    for m in ce.DRAIN_M:
        s = m - 3                                   # the playout decides request s, then H more: the drain step is m - 1
        got.append(env.step_policy(s - done))
        done = s
        out = env.playout(None, horizon=H, policy=ce.FF, own_stream=True)[:, 0, 0]
        r = ce.row(f"drain{m}")
        assert active[s - 1, r] == m - 3 and active[s + H, r] <= 7 + H             # the horizon crosses the drain
        assert (out[:, col["status"]] == 1).all()
        np.testing.assert_array_equal(out[:, col["first_accepted"]], acc[s])
        np.testing.assert_array_equal(out[:, col["steps"]], H)
        np.testing.assert_array_equal(out[:, col["accepted"]], acc[s + 1:s + 1 + H].sum(axis=0))
        np.testing.assert_array_equal(out[:, col["blocked"]], H - acc[s + 1:s + 1 + H].sum(axis=0))
        np.testing.assert_array_equal(out[:, col["active_end"]], active[s + H])
    got.append(env.step_policy(run.steps - done))
    got = np.concatenate(got)
    for r, name in enumerate(ce.PATTERNS):
        assert_records_equal(got[:, r], run.recs[:, r], name)
    check_final(env, run.oracles, "after the playouts")


# ---- counters-only reset ----------------------------------------------------------------------------------------------------------------
def test_counters_only_reset_in_the_middle_of_the_grid():
    """After reset_episode_counters the running services hold copysignf(inf) and never leave, and the run goes on over the
    grid's equalities.  Replica 1 (the same trace) is not reset.  k_run only: see the module docstring."""
    key, rows, at = "nsfnet320", ("grid", "grid"), 300
    holder = ce.holder_of(key, batch=2, track_service_ids=True)
    trace = np.ascontiguousarray(ce.traces(key)[[ce.row(n) for n in rows]])
    oracles, want = [], []
    for r in range(2):
        o = OracleEnv(holder, replica=r)
        o.set_trace(trace[r])
        o.reset()
        a = o.run_policy(ce.FF, at)
        if r == 0:
            o.reset_counters()
        want.append(np.concatenate([a, o.run_policy(ce.FF, ce.N - 1 - at)]))
        oracles.append(o)
    kept = int(want[0]["active"][at - 1])
    assert kept > 50 and (want[0]["active"][at:] >= kept).all() and want[1]["active"][at:].min() < kept
    c = ce.edge_counts(trace[1]["arrival_time"], trace[1]["holding_time"][:-1], want[1])
    assert c["model_ok"] and c["le"]["equalities"][at:].sum() >= 50
    env = make_env(key, rows, track_service_ids=True)
    assert not env.occupancy()["lean_kernel"]
    got = [env.step_policy(at)]
    env.reset_episode_counters(np.array([1, 0], np.uint8))
    assert int(np.isinf(env.services(0)["release_time"]).sum()) == kept
    got = np.concatenate(got + [env.step_policy(ce.N - 1 - at)])
    for r in range(2):
        assert_records_equal(got[:, r], want[r], f"replica {r}")
    assert int(np.isinf(env.services(0)["release_time"]).sum()) == kept and np.isfinite(env.services(1)["release_time"]).all()
    check_final(env, oracles, "counters-only reset", dropped=True)
