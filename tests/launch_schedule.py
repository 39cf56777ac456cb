"""Launch schedules for tests/test_gpu_launch_boundaries.py and tests/test_launch_schedule_host.py - TEST INFRASTRUCTURE.

A replica's state crosses every launch boundary through memory, and the two step kernels keep it in different forms while they run
(k_fast: the lean record codec, a 64-entry request ring restarted at req_index, next_rel, osnr_prod / osnr_flushed, per-lane histograms
and launch deltas; k_run: load_state / store_state).  This module places launch boundaries where that hand-over can go wrong and
says, from the CPU oracle alone, that the placement is what it claims to be:

  chopped   launch lengths summing to T, built around the indices of the oracle's `terminated` records (never from arithmetic):
            1, 1, 2 from the reset state; 63, 64, 65 in a row and launches of exactly 63, 64 and 65 POPS of the 64-entry ring (a
            terminal step pops twice: see build_chopped); a terminal step (auto-reset and a second pop of the ring) as the last and as the first step of a launch and at launch-relative index 62, 63 and 64 of launches of
            130 steps or more; a launch of one step on a loaded network; a launch of 200 steps or more.
  coarse    the same steps in one launch.
  trace     two chopped schedules over a replayed trace: "edge" has boundaries one step before, at and one step after the first
            no-op step; "inside" has the trace run out inside a launch, at the pop that would first refill the ring.  Both go on
            with launches of 1, 64 and 5 steps of no-ops.
  mixed     the chopped lengths again, the segments cycling through step_policy of four lean policies and one generic-only policy,
            step(actions) with first fit's / the reject / uniformly random actions and step_bundle, with one masked reset and one
            counters-only reset in between.  The oracle mirrors every segment; the plan (actions included) is made by the oracle alone.

`record=True` and `record=False` are different kernel instantiations: launch i of a chopped schedule is recorded when (i + parity) is
even, and every (configuration, policy group) is run with both parities.
"""
from __future__ import annotations

import contextlib
import copy
import functools
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from oracle_lib import OracleEnv

B, T, SEED = 8, 900, 5
ORACLE_THREADS = 8
RING = 64                        # requests drawn per ring refill (kWave, csrc/ongym_fast.hpp)
TRACE_N, TRACE_SEED = 500, 46
FF, LB, HSNR, LF = (nat.POLICY_FIRST_FIT, nat.POLICY_LOAD_BALANCING, nat.POLICY_HIGHEST_SNR,
                    nat.POLICY_LOWEST_FRAGMENTATION)
GENERIC_ONLY_POLICY = nat.POLICY_BEST_MOD_LB      # policy 5: no lean kernel
LEAN_POLICIES = (FF, LB, HSNR, LF)

_COMMON = dict(modulations=jocn_modulations(), capacity=256, episode_length=150, auto_reset=True, launch_power_dbm=0.0,
               margin=0.0, bit_rate_selection="discrete")
CONFIGS = {
    "nsfnet96": dict(topo="nsfnet", lean=True, kw=dict(num_spectrum_resources=96, load=150.0, bit_rates=(10, 40, 100, 400))),
    "nobeleu128": dict(topo="nobel-eu", lean=True, kw=dict(num_spectrum_resources=128, load=200.0, bit_rates=(40, 100, 400, 1000))),
    "trace": dict(topo="nsfnet", lean=True, trace=True,
                  kw=dict(num_spectrum_resources=96, load=150.0, bit_rates=(10, 40, 100, 400))),
    "alpha": dict(topo="nsfnet", lean=False, alpha=True,
                  kw=dict(num_spectrum_resources=96, load=150.0, bit_rates=(10, 40, 100, 400))),
    # nsfnet96 with service ids tracked: k_run only, and the only form in which the library takes a counters-only reset
    # (ongym_reset_episode_counters refuses without cfg.track_service_ids, which in turn rules out the lean kernels)
    "nsfnet96_ids": dict(topo="nsfnet", lean=False,
                         kw=dict(num_spectrum_resources=96, load=150.0, bit_rates=(10, 40, 100, 400), track_service_ids=True)),
}


def tables_of(key):
    cfg = CONFIGS[key]
    tb = golden_tables(cfg["topo"])
    if cfg.get("alpha"):
        tb = copy.deepcopy(tb)
        tb.link_alpha = tb.link_alpha * np.linspace(0.85, 1.2, tb.n_links)
    return tb


def config_kw(key) -> dict:
    return dict(_COMMON, **CONFIGS[key]["kw"])


@functools.lru_cache(maxsize=None)
def holder_of(key):
    return nat.ConfigHolder(tables_of(key), batch=B, **config_kw(key))


@functools.lru_cache(maxsize=None)
def trace_of(key):
    """TRACE_N requests per replica from the configured bit-rate table (as make_trace of tests/playout_child.py)."""
    tb, kw = tables_of(key), config_kw(key)
    rng = np.random.default_rng(TRACE_SEED)
    reqs = np.zeros((B, TRACE_N), nat.REQUEST_DTYPE)
    for r in range(B):
        reqs[r]["arrival_time"] = np.cumsum(rng.exponential(10800.0 / kw["load"], TRACE_N)).astype(np.float32)
        reqs[r]["holding_time"] = rng.exponential(10800.0, TRACE_N).astype(np.float32)
        src = rng.integers(0, tb.n_nodes, TRACE_N)
        reqs[r]["source"], reqs[r]["destination"] = src, (src + rng.integers(1, tb.n_nodes, TRACE_N)) % tb.n_nodes
        reqs[r]["bit_rate"] = rng.choice(np.array(kw["bit_rates"]), TRACE_N)
    return reqs


def make_oracles(key):
    """One reset oracle per replica on the configuration's request source."""
    out = []
    for r in range(B):
        o = OracleEnv(holder_of(key), replica=r)
        if CONFIGS[key].get("trace"):
            o.set_trace(trace_of(key)[r])
        else:
            o.seed(SEED)
        o.reset()
        out.append(o)
    return out


@contextlib.contextmanager
def force_generic(on: bool):
    """ONGYM_FORCE_GENERIC set to 1 (on) or unset (off) while an environment is created (it is read at create), then put back."""
    old = os.environ.get("ONGYM_FORCE_GENERIC")
    if on:
        os.environ["ONGYM_FORCE_GENERIC"] = "1"
    else:
        os.environ.pop("ONGYM_FORCE_GENERIC", None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("ONGYM_FORCE_GENERIC", None)
        else:
            os.environ["ONGYM_FORCE_GENERIC"] = old


def make_env(key, generic=False):
    """The device environment of a configuration, reset."""
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    with force_generic(generic):
        env = BatchedQRMSAEnv(tables=tables_of(key), batch_size=B, **config_kw(key))
    if CONFIGS[key].get("trace"):
        env.set_requests(trace_of(key))
    else:
        env.seed(SEED)
    env.reset()
    return env


# ---- the oracle's trajectory ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_run(key, policy, nsteps=T):
    """(records [nsteps, B], valid [B]) of `nsteps` fused policy steps on the oracle.  `valid` is the index of a replica's first
    no-op step (nsteps where its request source never runs out); the oracle is not stepped past it (the device's steps from there
    on are flagged no-ops) and its records from there on are zero."""
    recs = np.zeros((nsteps, B), nat.STEP_DTYPE)
    valid = np.full(B, nsteps, np.int64)
    def run(ro):
        r, o = ro
        if not CONFIGS[key].get("trace"):
            recs[:, r] = o.run_policy(policy, nsteps)
            return
        for i in range(nsteps):                      # step by step: the flag appears with the last valid step
            recs[i, r] = o.run_policy(policy, 1)[0]
            if o.stats()["flags"] & nat.F_NO_REQUEST:
                valid[r] = i + 1
                break

    with ThreadPoolExecutor(ORACLE_THREADS) as pool:  # the oracle's calls release the GIL; replicas are independent
        list(pool.map(run, enumerate(make_oracles(key))))
    recs.setflags(write=False)
    valid.setflags(write=False)
    return recs, valid


def terminal_indices(recs, upto=None) -> list:
    """Indices of the terminal steps; the same in every replica (each step of a fused policy decides one request)."""
    t0 = np.flatnonzero(recs["terminated"][:upto, 0])
    for r in range(1, recs.shape[1]):
        assert np.array_equal(np.flatnonzero(recs["terminated"][:upto, r]), t0), f"replica {r}: other terminal steps than replica 0"
    return [int(t) for t in t0]


def starts_of(lengths) -> list:
    return [int(s) for s in np.concatenate([[0], np.cumsum(lengths)[:-1]])]


def recorded(i: int, parity: int) -> bool:
    return (i + parity) % 2 == 0


# ---- chopped schedule ------------------------------------------------------------------------------------------------------------
# The auto-reset of a terminal step empties the network, and first fit blocks nothing in the first 65 or so steps of an episode
# of these configurations.  So that every launch of 60 steps or more sees a blocked request, the long launches are placed over the
# late part of an episode and the early parts are cut into launches of fewer than 60 steps.
def launch_pops(lengths, terms) -> list:
    """Pops of the request ring per launch: one per step, two per terminal step (its auto-reset draws a request of its own)."""
    return [n + sum(s <= t < s + n for t in terms) for s, n in zip(starts_of(lengths), lengths)]


def build_chopped(recs, total=T) -> list:
    """Launch lengths around the terminal indices t1..t6 of the oracle's records (see the module docstring), asserted by
    check_chopped.  k_fast refills its ring lazily, at the first pop that finds it drained, so what a boundary can expose is a
    launch that ENDS with the ring exactly drained (RING pops: the refill is still owed when req_index is stored).  Three
    consecutive launches of 63, 64 and 65 steps span more than an episode and the middle one must hold the terminal step (each
    needs the late part of an episode to see a blocked request), so they make RING - 1, RING + 1 and RING + 1 pops; the launch
    with exactly RING pops is the one of 63 steps that ends with t1."""
    terms = terminal_indices(recs)
    assert len(terms) >= 6, f"need six terminal steps in {total}, the oracle has {terms}"
    t1, t2, t3, t4, t5, t6 = terms[:6]
    a = t1 + 1 - 63                                   # t1 is the last step of a launch of 63 steps: RING pops
    c = t3 - 62 - (63 + 64 + 65)                      # 63, 64, 65 end where t3's launch begins; t2 falls into the 64
    cuts = [0, 1, 2, 4, 4 + (a - 4) // 2, a, t1 + 1,
            t1 + 1 + (c - t1 - 1) // 2, t1 + 2 + (c - t1 - 1) // 2,      # one step on a loaded network
            c, c + 63, c + 63 + 64,
            t3 - 62, t3 - 62 + 130,                   # t3 at launch-relative 62: both pops before the ring's edge
            t4 - 63, t4 - 63 + 130,                   # t4 at 63: the edge between its two pops
            t5 - 64,                                  # t5 at 64: the edge before its first pop, in a launch of 200 steps or more
            t6,                                       # t6 is the first step of its launch
            total]
    assert all(y > x for x, y in zip(cuts, cuts[1:])), f"terminal steps {terms} leave no room for the schedule: cuts {cuts}"
    lengths = [y - x for x, y in zip(cuts, cuts[1:])]
    check_chopped(lengths, recs, total)
    return lengths


def check_chopped(lengths, recs, total=T):
    """The placement the module docstring promises, asserted for every replica (the terminal steps are the same in all)."""
    terms = terminal_indices(recs)
    st = starts_of(lengths)
    assert sum(lengths) == total and min(lengths) >= 1
    assert lengths[:3] == [1, 1, 2], lengths
    assert any(lengths[i:i + 3] == [63, 64, 65] for i in range(len(lengths))), lengths
    pops = launch_pops(lengths, terms)
    for want in (RING - 1, RING, RING + 1):          # no refill; the ring drained with the launch's last pop; a refill on the last pop
        assert want in pops, f"no launch with exactly {want} pops of the ring: {pops}"
    where = {}                                       # terminal step -> (launch, launch-relative index)
    for t in terms:
        i = max(j for j, s in enumerate(st) if s <= t)
        where[t] = (i, t - st[i])
    assert any(rel == lengths[i] - 1 and lengths[i] > 1 for i, rel in where.values()), "no terminal step ends a launch"
    assert any(rel == 0 and lengths[i] > 1 for i, rel in where.values()), "no terminal step begins a launch"
    for want in (62, 63, 64):
        assert any(rel == want and lengths[i] >= 130 for i, rel in where.values()), f"no terminal step at launch-relative {want}"
    assert any(n == 1 and s > 0 and (recs["active"][s - 1] > 0).all() and not recs["terminated"][s - 1].any()
               for n, s in zip(lengths, st)), "no one-step launch on a loaded network"
    assert max(lengths) >= 200
    return where


def edge_launches(lengths, terms) -> list:
    """Launches that hold a terminal step or reach the ring's edge (RING pops or more: a terminal step pops twice)."""
    st = starts_of(lengths)
    return [i for i, (s, n, p) in enumerate(zip(st, lengths, launch_pops(lengths, terms)))
            if any(s <= t < s + n for t in terms) or p >= RING]


# ---- trace schedules -------------------------------------------------------------------------------------------------------------
TRACE_HEAD = [1, 1, 2, 40, 40]
NOOP_TAIL = [1, 64, 5]


def pops_before_exhaustion(start, valid, terms) -> int:
    """Pops of the request ring in a launch that begins at step `start`, before the pop that finds the trace empty: one per step,
    two per terminal step.  The failing pop is the last valid step's."""
    return (valid - 1 - start) + sum(start <= t < valid - 1 for t in terms)


def build_trace(kind, valid0, terms) -> tuple:
    """(lengths, rel).  'edge': boundaries at valid0 - 1, valid0, valid0 + 1.  'inside': replica 0's first no-op step at
    launch-relative index rel, chosen among 63, 64 and 65 as the one whose failing pop is launch-relative pop RING, i.e. the pop
    that first refills the ring (a terminal step inside the launch pops twice and moves it by one)."""
    head = TRACE_HEAD
    if kind == "edge":
        rel = 0
        lengths = head + [valid0 - 1 - sum(head), 1, 1] + NOOP_TAIL
    else:
        fits = [rel for rel in (63, 64, 65) if pops_before_exhaustion(valid0 - rel, valid0, terms) == RING]
        assert fits, f"no start among valid - 63/64/65 puts the failing pop on the ring's edge (valid {valid0}, terminal steps {terms})"
        rel = fits[0]
        lengths = head + [valid0 - rel - sum(head), rel + 6] + NOOP_TAIL
    assert min(lengths) >= 1, lengths
    st = starts_of(lengths)
    if kind == "edge":
        assert {valid0 - 1, valid0, valid0 + 1} <= set(st)
    else:
        i = max(j for j, s in enumerate(st) if s <= valid0)
        assert valid0 - st[i] == rel and lengths[i] > rel
    assert lengths[-3:] == NOOP_TAIL and st[-3] > valid0
    return lengths, rel


# ---- "no test passes emptily": conditions on the oracle's records -------------------------------------------------------------
def launch_activity(recs, lengths, valid=None) -> list:
    """Per launch: int array [3, B] of (accepted, blocked, departures) per replica, from the oracle's records.  A departure is a
    step after which `active` is lower than after the step before (the auto-reset of a terminal step does not count)."""
    out = []
    for s, n in zip(starts_of(lengths), lengths):
        act = np.zeros((3, recs.shape[1]), np.int64)
        for r in range(recs.shape[1]):
            e = min(s + n, int(valid[r])) if valid is not None else s + n
            if e <= s:
                continue
            w = recs[s:e, r]
            act[0, r] = (w["accepted"] == 1).sum()
            act[1, r] = ((w["accepted"] == 0) & (w["retry"] == 0)).sum()
            a = recs["active"][max(s - 1, 0):e, r].astype(np.int64)
            term = recs["terminated"][max(s - 1, 0):e, r]
            act[2, r] = ((np.diff(a) < 0) & (term[:-1] == 0) & (term[1:] == 0)).sum()
        out.append(act)
    return out


def check_activity(recs, lengths, valid=None, what=""):
    """Every launch of 60 valid steps or more sees an accepted request in EVERY replica, and a blocked request and a departure in
    some replica.  A launch of 130 steps or more covers the whole late part of an episode, where first fit's 2-5 % of blocked
    requests fall: it sees a departure in every replica and a blocked request in at least half of them."""
    act = launch_activity(recs, lengths, valid)
    for i, (s, n) in enumerate(zip(starts_of(lengths), lengths)):
        nvalid = n if valid is None else int(min(s + n, valid.min())) - s
        if nvalid >= 60:
            ctx = f"{what}: launch {i} ({n} steps from {s}) has per replica (accepted, blocked, departures) =\n{act[i]}"
            assert (act[i][0] > 0).all() and (act[i][1] > 0).any() and (act[i][2] > 0).any(), ctx
            if nvalid >= 130:
                assert (act[i][2] > 0).all() and (act[i][1] > 0).sum() * 2 >= recs.shape[1], ctx
    return act


# ---- mixed schedule --------------------------------------------------------------------------------------------------------------
KINDS = ("policy_ff", "actions_ff", "policy_lb", "reject", "policy_hsnr_norec", "bundle_lb", "policy_lf", "random", "policy_generic")
KIND_POLICY = {"policy_ff": FF, "policy_lb": LB, "policy_hsnr_norec": HSNR, "policy_lf": LF, "policy_generic": GENERIC_ONLY_POLICY}
ACTION_SEED = {"nsfnet96": 8101, "nobeleu128": 8102, "nsfnet96_ids": 8103}      # the random-action segments' streams
KIND_OFFSET = 2              # the cycle starts at its third entry: then the fused launches of 60 steps or more lie over late parts of
                             # an episode (accepted, blocked and departing requests) and the masked reset falls mid-episode
N_REJECT = 3                 # "a few": more in a row would drain the network
RESET_AFTER, RESET_REPLICAS = 6, (1, 5)              # reset(mask) after segment 6
COUNTERS_AFTER, COUNTERS_REPLICAS = 10, (2, 6)       # reset_episode_counters(mask) after segment 10


@dataclass
class Snapshot:
    stats: np.ndarray                  # STATS_DTYPE [B]
    grids: list                        # int32 [n_links, S] per replica
    requests: list                     # bytes per replica
    services: list                     # SERVICE_DTYPE arrays per replica, sorted by (release_time, path_id, slot)


@dataclass
class Segment:
    kind: str
    n: int                             # steps (calls for the action kinds)
    policy: int = -1
    record: bool = True
    actions: Optional[np.ndarray] = None           # int32 [n, B] for the action kinds
    next_actions: Optional[np.ndarray] = None      # int32 [n, B]: bundle_lb, the oracle's policy(1) after each step
    want: Optional[np.ndarray] = None              # STEP_DTYPE [n, B] from the oracle
    rc: Optional[np.ndarray] = None                # int32 [n, B]: the oracle's step return code (non-zero: QoT error, nothing applied)
    mask: Optional[np.ndarray] = None              # uint8 [B] for reset / counters
    after: Optional[Snapshot] = field(default=None, repr=False)


def sort_services(svc):
    return np.sort(svc, order=["release_time", "path_id", "slot"])


def oracle_snapshot(oracles) -> Snapshot:
    st = np.zeros(len(oracles), nat.STATS_DTYPE)
    for r, o in enumerate(oracles):
        st[r] = o.stats()
    return Snapshot(st, [o.grid() for o in oracles], [o.request().tobytes() for o in oracles],
                    [sort_services(o.services()) for o in oracles])


def _oracle_step(o, action):
    rc, rec = o.step(int(action))
    if rc == 0 and rec["terminated"]:
        o.reset()                                   # auto_reset (orc_run_policy does the same)
    return rc, rec


@functools.lru_cache(maxsize=None)
def mixed_plan(key) -> tuple:
    """The mixed schedule of a configuration with everything the oracle says about it: one Segment per operation, in order."""
    lengths = build_chopped(oracle_run(key, FF)[0])
    oracles = make_oracles(key)
    reject = oracles[0].reject_action
    rng = np.random.default_rng(ACTION_SEED[key])
    plan = [Segment("start", 0, after=oracle_snapshot(oracles))]      # the reset state: the baseline of segment 0's deltas
    for i, n in enumerate(lengths):
        kind = KINDS[(i + KIND_OFFSET) % len(KINDS)]
        if kind in KIND_POLICY:
            seg = Segment(kind, n, policy=KIND_POLICY[kind], record=kind != "policy_hsnr_norec")
            with ThreadPoolExecutor(ORACLE_THREADS) as pool:
                seg.want = np.stack(list(pool.map(lambda o: o.run_policy(seg.policy, n), oracles)), axis=1)
        else:
            n = min(n, N_REJECT) if kind == "reject" else n
            seg = Segment(kind, n, actions=np.zeros((n, B), np.int32), want=np.zeros((n, B), nat.STEP_DTYPE),
                          rc=np.zeros((n, B), np.int32))
            if kind == "bundle_lb":
                seg.next_actions = np.zeros((n, B), np.int32)
            for j in range(n):
                for r, o in enumerate(oracles):
                    if kind == "actions_ff":
                        a = o.policy(FF)[0]
                    elif kind == "reject":
                        a = reject
                    elif kind == "bundle_lb":       # load balancing's choice: the first from the policy, then the bundle's own
                        a = o.policy(LB)[0]
                    else:
                        a = int(rng.integers(0, reject + 1))
                    seg.actions[j, r] = a
                    seg.rc[j, r], seg.want[j, r] = _oracle_step(o, a)
                    if kind == "bundle_lb":
                        seg.next_actions[j, r] = o.policy(LB)[0]
        seg.after = oracle_snapshot(oracles)
        plan.append(seg)
        for at, name, reps in ((RESET_AFTER, "reset", RESET_REPLICAS), (COUNTERS_AFTER, "counters", COUNTERS_REPLICAS)):
            if i == at:
                mask = np.zeros(B, np.uint8)
                mask[list(reps)] = 1
                for r in reps:
                    st = oracles[r].stats()
                    assert st["active"] > 0 and st["episode_services_processed"] > 10, f"{name} of replica {r} is not mid-episode"
                supported = name == "reset" or bool(config_kw(key).get("track_service_ids"))
                op = Segment(name if supported else "counters_refused", 0, mask=mask)
                if supported:
                    for r in reps:
                        oracles[r].reset() if name == "reset" else oracles[r].reset_counters()
                op.after = oracle_snapshot(oracles)
                plan.append(op)
    check_mixed(plan, key)
    return tuple(plan)


def check_mixed(plan, key=""):
    """The mixed schedule holds what it is there for: a retry, a QoT error, an accepted external action and a terminal step in an
    action segment, and accepted / blocked / departing requests in every fused launch of 60 steps or more."""
    acts = [s for s in plan if s.actions is not None]
    ok = [s.want[s.rc == 0] for s in acts]
    assert sum(int(w["retry"].sum()) for w in ok) > 0, f"{key}: no retry"
    assert sum(int((s.rc != 0).sum()) for s in acts) > 0, f"{key}: no QoT error"
    assert sum(int((s.want[s.rc == 0]["accepted"] == 1).sum()) for s in acts if s.kind == "random") > 0, f"{key}: no accepted random action"
    assert sum(int(w["terminated"].sum()) for w in ok) > 0, f"{key}: no terminal step in an action segment"
    assert [s.kind for s in plan].count("reset") == 1
    assert sum(s.kind in ("counters", "counters_refused") for s in plan) == 1
    for i, s in enumerate(plan):
        if s.kind in KIND_POLICY and s.n >= 60:
            act = launch_activity(s.want, [s.n])[0].sum(axis=1)
            assert min(act) > 0, f"{key}: segment {i} ({s.kind}, {s.n} steps) has (accepted, blocked, departures) = {act}"


# ---- the partition test's cases -------------------------------------------------------------------------------------------------
# (configuration, policy, parity, ONGYM_FORCE_GENERIC, trace schedule).  Within a group that shares its kernel family the parities
# alternate, and a group of one policy runs with both: every launch is recorded by one case and unrecorded by another.
PARTITION_CASES = (
    [("nsfnet96", p, i % 2, False, None) for i, p in enumerate(LEAN_POLICIES)]
    + [("nobeleu128", FF, 0, False, None), ("nobeleu128", LB, 1, False, None)]
    + [("trace", FF, 0, False, "edge"), ("trace", FF, 1, False, "edge"), ("trace", FF, 0, False, "inside"), ("trace", FF, 1, False, "inside")]
    + [("alpha", FF, 0, False, None), ("alpha", GENERIC_ONLY_POLICY, 1, False, None)]
    + [(k, FF, par, True, None) for k in ("nsfnet96", "nobeleu128") for par in (0, 1)])
TRACE_STEPS = 600            # more than the trace holds: the oracle stops at the first no-op step


def partition_schedule(key, kind=None) -> tuple:
    """(lengths, oracle records of first fit, valid, trace-schedule rel) of a partition case.  The terminal steps do not depend on
    the policy (every fused step decides one request; tests/test_launch_schedule_host.py asserts it for every policy used)."""
    if CONFIGS[key].get("trace"):
        recs, valid = oracle_run(key, FF, TRACE_STEPS)
        assert (valid < TRACE_STEPS).all()
        lengths, rel = build_trace(kind, int(valid[0]), terminal_indices(recs, int(valid.min())))
        return lengths, recs, valid, rel
    recs, valid = oracle_run(key, FF)
    return build_chopped(recs), recs, None, None
