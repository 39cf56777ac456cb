"""Request traces that put the departure rule on its edges, and a host model of that rule - TEST INFRASTRUCTURE.

Every step kernel releases the running services with `float32(arrival + holding) <= float32(now)` when it draws the next request:
release_due and release_due_defrag (csrc/ongym_device.hpp) and the lean scan of k_fast (csrc/ongym_fast.hpp: the `v_at >= next_rel`
shortcut, trips of four chunks of 64 records and a tail, next_rel kept between steps and rebuilt at launch start).  Random traffic
that starts at time 0 meets `release == now` a couple of times in thousands of requests and never two arrivals at one instant, so
the edges are reached on purpose here:

  grid        arrivals cumsum(integers{0, 1, 2}), holding integers[0, 400): every time exact in float32, equalities and zero
              advances on a third of the steps
  late_trace  arrivals from 2^28 on (one ulp is 32 s against a 36 s mean inter-arrival time), holding Exp(10800)
  late_gen    a trace of two requests whose second arrives at 2^27 (replica 1: 2^25), one policy step, then seed(): the device
              generator goes on from the late clock with the state and the pending request kept (the lean kernels' generator
              instantiations, which are the benchmark's, see no trace otherwise)
  drain       m arrivals at t = 1..m of 10 Gb/s that all leave at t = 1000 except keepers at requests 0, 63, 64, 255, 256 and m - 1
              (record index = request index while nothing has left: the keepers sit on the borders of the scan's chunks), then
              arrivals at 1000, 1000 and 1001 and ordinary requests (the 40 that belong to the pattern, then more up to the
              common length: the replicas of one environment share the trace length).  m in 64, 65, 256, 257, 330: a tail-only
              scan, one trip of four chunks, a trip and a tail, and the second mask word's clamped loop at every size.
  zero_inf    exponential times, holding 0 on every 11th request and +inf on every 7th
  backsteps   exponential times with 500 s taken from every 40th arrival: the clock steps back and nothing leaves

The host model (`model`) knows a trace and which requests were accepted, nothing else: rel = float32(at + ht), and after step t
the running set is what is left after removing every rel <= at[t + 1] (`strict`: <).  tests/test_clock_edges_host.py holds it
to the oracle at every step and asserts the counts that keep the GPU tests from passing emptily.  This module imports no GPU library.
"""
from __future__ import annotations

import copy
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from oracle_lib import OracleEnv, lib as oracle_library

FF, LB, HSNR, LF = (nat.POLICY_FIRST_FIT, nat.POLICY_LOAD_BALANCING, nat.POLICY_HIGHEST_SNR,
                    nat.POLICY_LOWEST_FRAGMENTATION)
LEAN_POLICIES = (FF, LB, HSNR, LF)
GENERIC_ONLY_POLICY = nat.POLICY_BEST_MOD_LB      # policy 5: no lean kernel
CHEAP_ORACLE = (FF, LB, GENERIC_ONLY_POLICY)      # policies whose 600 oracle steps take well under a second
N = 600                      # requests per trace
GEN_STEPS = 800              # generator steps of late_gen after the hand-over
SEED = 1                     # the traces' seed
GEN_SEED = 5                 # late_gen: the generator's seed
ORACLE_THREADS = 12
DRAIN_M = (64, 65, 256, 257, 330)
DRAIN_T = 1000.0
KEEPERS = (0, 63, 64, 255, 256)          # and m - 1
LATE_BASES = (2.0 ** 27, 2.0 ** 25)      # late_gen, replica 0 and 1
PATTERNS = ("grid", "late_trace") + tuple(f"drain{m}" for m in DRAIN_M) + ("zero_inf", "backsteps")
B = len(PATTERNS)            # 9 replicas, one pattern each

_COMMON = dict(modulations=jocn_modulations(), load=300.0, bit_rate_selection="discrete", auto_reset=True,
               episode_length=100000, margin=0.0)
RATES = (10, 40, 100, 400)
CONFIGS = {
    "nsfnet320": dict(topo="nsfnet", kw=dict(num_spectrum_resources=320, capacity=512, bit_rates=RATES)),
    "nsfnet320_c448": dict(topo="nsfnet", kw=dict(num_spectrum_resources=320, capacity=448, bit_rates=RATES)),
    "nsfnet320_wide": dict(topo="nsfnet", kw=dict(num_spectrum_resources=320, capacity=512, bit_rates=RATES + (1000,))),
    "nobeleu256": dict(topo="nobel-eu", kw=dict(num_spectrum_resources=256, capacity=512, bit_rates=RATES)),
    "cost239_192": dict(topo="cost239", kw=dict(num_spectrum_resources=192, capacity=512, bit_rates=RATES)),
    # the generic kernel's own instantiations: bit rates outside the table, and per-link attenuation (as tests/threshold_ladder.py)
    "offtable": dict(topo="nsfnet", kw=dict(num_spectrum_resources=320, capacity=512, bit_rates=RATES), offtable=True),
    "alpha": dict(topo="nsfnet", kw=dict(num_spectrum_resources=320, capacity=512, bit_rates=RATES), alpha=True),
}
LEAN_CONFIGS = ("nsfnet320", "nsfnet320_c448", "nsfnet320_wide", "nobeleu256")
GRID_CONFIGS = ("nsfnet320", "nobeleu256", "cost239_192", "nsfnet320_wide")


def tables_of(key):
    cfg = CONFIGS[key]
    tb = golden_tables(cfg["topo"])
    if cfg.get("alpha"):
        tb = copy.deepcopy(tb)
        tb.link_alpha = tb.link_alpha * np.linspace(0.85, 1.2, tb.n_links)
    return tb


def config_kw(key, **over) -> dict:
    return dict(_COMMON, **CONFIGS[key]["kw"], **over)


def holder_of(key, batch=B, **over):
    return nat.ConfigHolder(tables_of(key), batch=batch, **config_kw(key, **over))


# ---- trace builders ----------------------------------------------------------------------------------------------------------
def _requests(key, rng, at, ht, first_10g=0):
    """A trace of the given times: random node pairs, bit rates from the configured table (`offtable`: integers in [5, 500)),
    the first `first_10g` requests at 10 Gb/s."""
    tb, n = tables_of(key), len(at)
    reqs = np.zeros(n, nat.REQUEST_DTYPE)
    reqs["arrival_time"], reqs["holding_time"] = np.asarray(at, np.float32), np.asarray(ht, np.float32)
    src = rng.integers(0, tb.n_nodes, n)
    reqs["source"], reqs["destination"] = src, (src + rng.integers(1, tb.n_nodes, n)) % tb.n_nodes
    table = rng.choice(np.array(CONFIGS[key]["kw"]["bit_rates"]), n)
    other = rng.integers(5, 500, n)
    reqs["bit_rate"] = other if CONFIGS[key].get("offtable") else table
    reqs["bit_rate"][:first_10g] = 10.0
    return reqs


def grid(key, rng, n=N):
    return _requests(key, rng, np.cumsum(rng.integers(0, 3, n)), rng.integers(0, 400, n))


def late_trace(key, rng, n=N):
    at = (np.float64(2.0 ** 28) + np.cumsum(rng.exponential(36.0, n))).astype(np.float32)
    return _requests(key, rng, at, rng.exponential(10800.0, n).astype(np.float32))


def keepers_of(m) -> list:
    return sorted({k for k in KEEPERS if k < m} | {m - 1})


def drain(key, rng, m, n=N):
    at = np.arange(1, m + 1, dtype=np.float64)
    ht = DRAIN_T - at
    ht[keepers_of(m)] = 1e6
    rest = n - m - 3
    assert rest >= 40
    at = np.concatenate([at, [DRAIN_T, DRAIN_T, DRAIN_T + 1.0], DRAIN_T + 1.0 + np.cumsum(rng.exponential(36.0, rest))])
    ht = np.concatenate([ht, [0.0, 5.0, 1.0], rng.exponential(10800.0, rest)])
    return _requests(key, rng, at, ht, first_10g=m)


def zero_inf(key, rng, n=N):
    at, ht = np.cumsum(rng.exponential(36.0, n)), rng.exponential(3000.0, n)
    ht[::7] = np.inf
    ht[3::11] = 0.0
    return _requests(key, rng, at, ht)


def backsteps(key, rng, n=N):
    at = np.cumsum(rng.exponential(36.0, n)).astype(np.float32)
    at[50::40] -= np.float32(500.0)
    return _requests(key, rng, at, rng.exponential(3000.0, n))


@functools.lru_cache(maxsize=None)
def traces(key) -> np.ndarray:
    """REQUEST_DTYPE [B, N]: row r holds PATTERNS[r] for the configuration (node pairs and bit rates are the configuration's)."""
    out = np.zeros((B, N), nat.REQUEST_DTYPE)
    for r, name in enumerate(PATTERNS):
        rng = np.random.default_rng(1000 * SEED + r)
        out[r] = drain(key, rng, int(name[5:])) if name.startswith("drain") else globals()[name](key, rng)
    out.setflags(write=False)
    return out


def row(name) -> int:
    return PATTERNS.index(name)


# ---- the host model ------------------------------------------------------------------------------------------------------------
def model(at, ht, accepted, strict=False) -> dict:
    """The departure rule on a trace.  at: float32 [n + 1], the arrival of the request step t decides and, last, of the request
    pending after the run; ht: float32 [n]; accepted: [n] from the oracle.  Per step t: `active` after it, `departures` at the
    draw of request t + 1, `equalities` (running services with rel == at[t + 1]) and `zero_advance` (at[t + 1] == at[t])."""
    at, ht = np.asarray(at, np.float32), np.asarray(ht, np.float32)
    n = len(ht)
    assert len(at) == n + 1 and len(accepted) == n
    rel = at[:-1] + ht                                  # float32 + float32, as `_add_release` adds them
    assert rel.dtype == np.float32
    out = {k: np.zeros(n, np.int64) for k in ("active", "departures", "equalities", "zero_advance")}
    running = np.zeros(0, np.int64)
    for t in range(n):
        if accepted[t]:
            running = np.append(running, t)
        now = at[t + 1]
        due = rel[running] < now if strict else rel[running] <= now
        out["equalities"][t] = int((rel[running] == now).sum())
        out["departures"][t] = int(due.sum())
        running = running[~due]
        out["active"][t] = len(running)
        out["zero_advance"][t] = int(now == at[t])
    out["running"] = running                            # the requests still running at the end
    out["rel"] = rel
    return out


def edge_counts(at, ht, recs) -> dict:
    """What a host test asserts of a run: whether the <= model is the oracle's `active` at every step, the number of equalities
    and zero advances, and the number of steps on which the strict twin has another `active`."""
    le, lt = model(at, ht, recs["accepted"]), model(at, ht, recs["accepted"], strict=True)
    return dict(model_ok=bool(np.array_equal(le["active"], recs["active"])), equalities=int(le["equalities"].sum()),
                zero_advances=int(le["zero_advance"].sum()), strict_differs=int((lt["active"] != le["active"]).sum()),
                max_departures=int(le["departures"].max()), le=le)


# ---- the oracle's runs -----------------------------------------------------------------------------------------------------------
def threaded(fn, items):
    oracle_library()          # built and loaded here, on the calling thread: oracle_lib.lib() takes no lock
    with ThreadPoolExecutor(ORACLE_THREADS) as pool:          # the oracle's calls release the GIL; replicas are independent
        return list(pool.map(fn, items))


class Run:
    """An oracle run: records [steps, B'], the oracles in their final state (only read afterwards), and per replica the
    times (at [steps + 1], ht [steps]) of the requests it decided."""
    pass


WINDOW_TAIL = 20
# steps m - 2, m - 1 (the drain step) and m of every drain pattern, merged where they touch, and WINDOW_TAIL steps late in the
# run, where grid and late_trace release on an equality on every other step
EDGE_WINDOWS = ((62, 66), (254, 258), (328, 331), (340, 340 + WINDOW_TAIL))


def schedule_of(policy, steps=N - 1) -> tuple:
    """The launches of a trace run as ((policy, steps), ...).  A policy of CHEAP_ORACLE takes every step.  The oracle's
    restatements of highest SNR and lowest fragmentation take about 0.1 s per step at these loads (every candidate of every
    route is evaluated, and lowest fragmentation paints each), so these two take the steps of EDGE_WINDOWS - each drain step
    with the step before and after it, and WINDOW_TAIL steps for the other patterns - and first fit, the cheap one, walks
    between them.  Departures belong to the draw of the next request, so a step's policy is the one whose kernel releases."""
    if policy in CHEAP_ORACLE:
        return ((policy, steps),)
    cuts, done = [], 0
    for lo, hi in EDGE_WINDOWS:
        cuts += [(FF, lo - done), (policy, hi - lo)]
        done = hi
    cuts.append((FF, steps - done))
    return tuple(c for c in cuts if c[1] > 0)


def schedule_steps(schedule, policy) -> np.ndarray:
    """bool [steps]: the steps of a schedule that `policy` takes"""
    return np.concatenate([np.full(n, p == policy) for p, n in schedule])


@functools.lru_cache(maxsize=None)
def trace_run(key, schedule=((FF, N - 1),), over=(), rows=PATTERNS) -> Run:
    """The launches of `schedule` on the oracle, one replica per pattern of `rows`, each on its trace (N - 1 steps in all: the
    last request stays pending, so no step finds the trace empty).  over: extra configuration as a tuple of (name, value)."""
    holder = holder_of(key, batch=len(rows), **dict(over))
    steps = sum(n for _, n in schedule)
    run = Run()
    run.holder, run.steps, run.rows, run.schedule = holder, steps, rows, schedule
    run.trace = np.ascontiguousarray(traces(key)[[row(n) for n in rows]])
    run.trace.setflags(write=False)

    def one(r):
        o = OracleEnv(holder, replica=r)
        o.set_trace(run.trace[r])
        o.reset()
        return o, np.concatenate([o.run_policy(p, n) for p, n in schedule])

    res = threaded(one, range(len(rows)))
    run.oracles = [x[0] for x in res]
    run.recs = np.stack([x[1] for x in res], axis=1)
    run.recs.setflags(write=False)
    run.at = [run.trace[r]["arrival_time"][:steps + 1] for r in range(len(rows))]
    run.ht = [run.trace[r]["holding_time"][:steps] for r in range(len(rows))]
    return run


@functools.lru_cache(maxsize=None)
def external_run(key, rows) -> Run:
    """First fit's choices applied from outside: per step the oracle's policy answers and its step() takes the action, as a
    caller of step() / step_bundle() does.  The records are those of the fused run except for the blocking flags, which the
    fused policy sets and an external reject action does not carry."""
    fused = trace_run(key, schedule_of(FF), (), rows)
    run = Run()
    run.holder, run.steps, run.rows, run.schedule, run.trace, run.at, run.ht = (fused.holder, fused.steps, rows, fused.schedule,
                                                                                fused.trace, fused.at, fused.ht)

    def one(r):
        o = OracleEnv(run.holder, replica=r)
        o.set_trace(run.trace[r])
        o.reset()
        recs = np.zeros(run.steps, nat.STEP_DTYPE)
        for t in range(run.steps):
            rc, recs[t] = o.step(o.policy(FF)[0])
            assert rc == 0 and not recs[t]["terminated"]
        return o, recs

    res = threaded(one, range(len(rows)))
    run.oracles = [x[0] for x in res]
    run.recs = np.stack([x[1] for x in res], axis=1)
    for f in ("action", "accepted", "active", "slot", "reward"):
        assert np.array_equal(run.recs[f], fused.recs[f]), f
    run.recs.setflags(write=False)
    return run


def late_gen_trace(key, batch=len(LATE_BASES)) -> np.ndarray:
    """REQUEST_DTYPE [batch, 2]: a 10 Gb/s request at t = 1, then one at the replica's late clock."""
    reqs = np.zeros((batch, 2), nat.REQUEST_DTYPE)
    reqs["arrival_time"] = [[1.0, LATE_BASES[r % len(LATE_BASES)]] for r in range(batch)]
    reqs["holding_time"] = [5.0, 7.0]
    reqs["source"], reqs["destination"] = [0, 1], [3, 4]
    reqs["bit_rate"] = [10.0, 40.0]
    return reqs


def late_gen_schedule(policy, steps=GEN_STEPS) -> tuple:
    """The generator launches of late_gen: a costly policy (schedule_of) takes the last GEN_TAIL steps, first fit the others."""
    return ((policy, steps),) if policy in CHEAP_ORACLE else ((FF, steps - GEN_TAIL), (policy, GEN_TAIL))


GEN_TAIL = 120


@functools.lru_cache(maxsize=None)
def late_gen_run(key="nsfnet320", schedule=((FF, GEN_STEPS),)) -> Run:
    """late_gen on the oracle: one step of the schedule's first policy on the two-request trace, then the generator's stream
    (GEN_SEED, r) - orc_seed keeps state, clock and the pending request, as ongym_seed_base does - stepped one request at a
    time so that the generator's requests are known to the host model."""
    run = Run()
    run.steps = steps = sum(n for _, n in schedule)
    run.schedule = schedule
    policies = np.concatenate([np.full(n, p) for p, n in schedule])
    holder = holder_of(key, batch=len(LATE_BASES))

    def one(r):
        o = OracleEnv(holder, replica=r)
        o.set_trace(late_gen_trace(key)[r])
        o.reset()
        first = o.run_policy(int(policies[0]), 1)
        o.seed(GEN_SEED)
        recs, at, ht = np.zeros(steps, nat.STEP_DTYPE), np.zeros(steps + 1, np.float32), np.zeros(steps, np.float32)
        for t in range(steps):
            q = o.request()
            at[t], ht[t] = q["arrival_time"], q["holding_time"]
            recs[t] = o.run_policy(int(policies[t]), 1)[0]
        at[steps] = o.request()["arrival_time"]
        return o, first, recs, at, ht

    res = threaded(one, range(len(LATE_BASES)))
    run.oracles = [x[0] for x in res]
    run.first = np.stack([x[1] for x in res], axis=1)          # [1, B']: the trace step before the hand-over
    run.recs = np.stack([x[2] for x in res], axis=1)
    run.recs.setflags(write=False)
    run.at, run.ht = [x[3] for x in res], [x[4] for x in res]
    return run


def sort_services(svc):
    return np.sort(svc, order=["release_time", "path_id", "slot"])


SERVICE_FIELDS = ("path_id", "slot", "nslots", "modulation", "release_time")
# stats() fields the GPU tests hold exactly to the oracle: all but the work counters (the device settles evaluations by a lower
# bound; tests/test_gpu_launch_boundaries.py holds them to inequalities) and the two GSNR sums, which are compared to 1e-9.
WORK = ("total_gn_evals", "total_gn_shortcuts", "total_interferer_terms", "total_paths_tried", "total_path_hops")
APPROX = ("episode_osnr_sum", "last_mean_gsnr")
COUNTERS = tuple(f for f in nat.STATS_DTYPE.names if f not in WORK + APPROX)
