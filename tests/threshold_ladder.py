"""A ladder of margins that puts the admission threshold on one candidate's GSNR, one replica per rung.

The rule `GSNR >= minimum_osnr[m] + margin` is restated by hand in every kernel ("Decision exactness"): a compare
in the linear domain, the reference's dB expression inside a 1e-9 relative band (4.34e-9 dB either side), and an early refusal
from the ASE bound outside it.  Random traffic never comes nearer than about 1e-2 dB to a threshold, so the band is reached on
purpose here:

  1. one oracle run of a fused policy (replica stream 0, base margin m0) for FIND requests;
  2. among its accepted steps, t* is the one whose chosen candidate lies closest to its threshold, g its GSNR (fp64, the oracle's),
     m its format;
  3. 21 replicas get margin_r = (g - thr[m]) + delta_r, delta = +-{0, 1, 2, 8 ulp(g), 1e-13, 1e-12, 1e-11, 4e-10, 2e-9, 1e-8,
     4.3e-8} dB: on the equality, a few ulp off it, deep inside the band, near its edges, just outside, ten band widths away.

All margins lie above m0 by the distance d of the closest decision (give or take 4.3e-8 dB), every decision before t* was farther
than d from its threshold, so the history before t* is the same on every rung; at t* the low rungs accept format m and the high
rungs fall through.  All rungs see one request stream: either the device generator after fork(src=[0]*B, keep_params=True)
(every rung has replica 0's stream key and its own margin; the oracle of rung r is seeded as replica 0), or a host trace
captured from the base run and installed for every replica.

This module imports no GPU library; tests/test_threshold_ladder_host.py holds the conditions that keep the GPU tests from being
vacuous, on the oracle alone.
"""
from __future__ import annotations

import copy
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from common import golden_tables, jocn_modulations, record_bytes
from optical_networking_gym import _native as nat
from oracle_lib import OracleEnv

B = 21
S = 128
SEED = 5
FIND = 300          # requests searched for the closest accepted decision
AFTER = 40          # diverged steps run after t*
HALF_BAND_DB = 10.0 * np.log10(1.0 + 1e-9)      # 4.34e-9 dB
ZONE_DB = 1e-11     # rungs closer than this to g are exempt from oracle parity (the device sums in another order)
QUIET_DB = 1e-6     # no other accepted decision of a run lies this close to its threshold
DELTAS_DB = (1e-13, 1e-12, 1e-11, 4e-10, 2e-9, 1e-8, 4.3e-8)
ULPS = (1, 2, 8)

FF, LB, HSNR = nat.POLICY_FIRST_FIT, nat.POLICY_LOAD_BALANCING, nat.POLICY_HIGHEST_SNR

_KW = dict(num_spectrum_resources=S, capacity=192, load=120.0, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400),
           episode_length=1000, auto_reset=True)

# name: topology, fused policy, base margin, request source ("fork": device generator, "trace": host trace), per-link attenuation
CASES = {
    "ff_nsfnet_m0": dict(topo="nsfnet", policy=FF, m0=0.0, source="fork"),
    "ff_nsfnet_m1": dict(topo="nsfnet", policy=FF, m0=1.0, source="fork"),
    "ff_nobeleu": dict(topo="nobel-eu", policy=FF, m0=0.5, source="fork"),
    "ff_trace": dict(topo="nsfnet", policy=FF, m0=0.0, source="trace"),
    "ff_alpha": dict(topo="nsfnet", policy=FF, m0=0.0, source="fork", alpha=True),
    "lb_nsfnet": dict(topo="nsfnet", policy=LB, m0=0.5, source="fork"),
    "hsnr_nsfnet": dict(topo="nsfnet", policy=HSNR, m0=0.5, source="fork"),
    "hsnr_cost239": dict(topo="cost239", policy=HSNR, m0=0.5, source="fork"),
}
# first-fit ladders found by a search on the oracle (seeds 1..20, m0 in {0, 0.5, 1}, NSFNET / COST239 / nobel-eu) for pending
# states on which the answers of policies 1, 11 (seed 2) and 2 (seed 13) change along the ladder; see POLICY_CASES
CASES["ff_nsfnet_s2"] = dict(topo="nsfnet", policy=FF, m0=0.5, source="fork", seed=2)
CASES["ff_nsfnet_s13"] = dict(topo="nsfnet", policy=FF, m0=1.0, source="fork", seed=13)
# the ASE-bound case: a trace whose first request is a 400 Gb/s demand on a long NSFNET pair, decided on the empty network
EMPTY = "ff_empty"
CASES[EMPTY] = dict(topo="nsfnet", policy=FF, m0=0.0, source="trace", empty=True)


def tables_of(name):
    """Per-link attenuation as tests/playout_child.py builds it (the generic kernel's non-uniform instantiation)."""
    c = CASES[name]
    tb = golden_tables(c["topo"])
    if c.get("alpha"):
        tb = copy.deepcopy(tb)
        tb.link_alpha = tb.link_alpha * np.linspace(0.85, 1.2, tb.n_links)
    return tb


def config_kw(name, **over) -> dict:
    return dict(_KW, modulations=jocn_modulations(), margin=CASES[name]["m0"], **over)


def thresholds() -> np.ndarray:
    return np.array([m.minimum_osnr for m in jocn_modulations()], np.float64)


def ladder(g: float, thr_m: float):
    """(margins, T): the 21 margins (g - thr_m) + delta and T_r = thr_m + margin_r, added in fp64 as the oracle and the device add
    them, both ordered by T_r (then by delta: thr + (g - thr + delta) need not round-trip, so delta alone does not order them)."""
    u = float(np.spacing(g))
    mags = [k * u for k in ULPS] + list(DELTAS_DB)
    deltas = np.array([0.0] + [s * x for x in mags for s in (-1.0, 1.0)], np.float64)
    assert len(deltas) == B
    margins = (np.float64(g) - np.float64(thr_m)) + deltas
    T = np.float64(thr_m) + margins
    order = np.lexsort((deltas, T))
    return margins[order], T[order]


class Case:
    """What find_case returns; everything is computed once and only read afterwards."""
    pass


def _request_source(o, c, seed, trace):
    if trace is not None:
        o.set_trace(trace)
    else:
        o.L.orc_seed(o.h, seed, 0)          # every rung draws replica 0's stream
    o.reset()


def _run(o, pid, steps):
    """Step records and the request of every step (the pending request before it)."""
    recs = np.zeros(steps, nat.STEP_DTYPE)
    reqs = np.zeros(steps, nat.REQUEST_DTYPE)
    for t in range(steps):
        reqs[t] = o.request()
        recs[t] = o.run_policy(pid, 1)[0]
    return recs, reqs


def distances(recs, thr, margin):
    """osnr - thr[m] - margin of the accepted steps (inf elsewhere), evaluated as the decision evaluates it."""
    acc = recs["accepted"].astype(bool)
    m = np.clip(recs["modulation"].astype(np.int64), 0, len(thr) - 1)
    return np.where(acc, recs["osnr"] - (thr[m] + margin), np.inf)


def rung_oracle(case, r):
    """A fresh reset oracle of rung r on the case's request stream."""
    o = OracleEnv(case.holder, replica=r)
    _request_source(o, case.cfg, case.seed, case.trace)
    return o


def pending_oracle(case, r):
    """The oracle of rung r with t* steps done and the critical request undecided."""
    o = rung_oracle(case, r)
    if case.t:
        o.run_policy(case.policy, case.t)
    return o


def ulps_of(x, ref) -> float:
    return abs(float(x) - float(ref)) / float(np.spacing(abs(float(ref))))


def threaded(fn, n):
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        return list(pool.map(fn, range(n)))


def build_case(name, seed, base_trace=None, find=FIND) -> Case:
    """The recipe of the module docstring; raises ValueError where the construction does not hold."""
    c = CASES[name]
    tb, thr, pid = tables_of(name), thresholds(), c["policy"]
    holder0 = nat.ConfigHolder(tb, batch=1, **config_kw(name))
    o = OracleEnv(holder0, replica=0)
    _request_source(o, c, seed, base_trace)
    # the search covers `find` requests; the base run goes on so that a trace case has requests for the steps after t*
    base, reqs = _run(o, pid, find + AFTER + 2 if base_trace is None else len(base_trace) - 1)
    d = distances(base[:find], thr, c["m0"])
    t = int(np.argmin(d))
    if not np.isfinite(d[t]):
        raise ValueError(f"{name}: no accepted step")
    g, m = float(base["osnr"][t]), int(base["modulation"][t])
    q = reqs[t]
    path = int(tb.pair_paths[int(q["source"]), int(q["destination"]), int(base["route"][t])])
    margins, T = ladder(g, thr[m])

    case = Case()
    case.name, case.cfg, case.seed, case.tables, case.policy = name, c, seed, tb, pid
    case.t, case.g, case.m, case.d = t, g, m, float(d[t])
    case.cand = (path, int(base["slot"][t]), int(base["nslots"][t]))
    case.route = int(base["route"][t])
    case.action = int(base["action"][t])
    case.margins, case.T, case.thr = margins, T, thr
    case.steps = t + 1 + AFTER
    case.trace = None
    if c["source"] == "trace":
        # the base run's own requests, and a tail so that no launch runs off the trace's end
        case.trace = np.ascontiguousarray(reqs if base_trace is None else base_trace)
        if len(case.trace) < case.steps + 1:
            raise ValueError(f"{name}: trace of {len(case.trace)} requests shorter than the run of {case.steps}")
    case.base = base[:case.steps]
    case.kw = config_kw(name, replica_margin=[float(x) for x in margins])
    case.holder = nat.ConfigHolder(tb, batch=B, **case.kw)

    case.oracles = [rung_oracle(case, r) for r in range(B)]          # left in their final state, after case.steps steps

    def run(r):
        return case.oracles[r].run_policy(pid, case.steps)

    case.recs = np.stack(threaded(run, B), axis=1)          # [steps, B]
    # the refusals: history before t* bit-identical to the base run, decision at t* exactly g >= T_r
    for r in range(B):
        if record_bytes(case.recs[:t, r]) != record_bytes(base[:t]):
            first = next(i for i in range(t) if record_bytes(case.recs[i:i + 1, r]) != record_bytes(base[i:i + 1]))
            raise ValueError(f"{name}: rung {r} leaves the base history at step {first} < t* = {t}")
    case.accepts = accepted_m(case, case.recs[t])
    want = np.float64(g) >= T
    if not np.array_equal(case.accepts, want):
        raise ValueError(f"{name}: oracle decisions at t* {case.accepts.astype(int)} are not g >= T_r {want.astype(int)}")
    return case


def accepted_m(case, rec_t):
    """Per rung: the step at t* took the ladder's candidate (same route, format and slot as the base run)."""
    path_ok = rec_t["route"] == case.route
    return (rec_t["accepted"].astype(bool) & path_ok & (rec_t["modulation"] == case.m) & (rec_t["slot"] == case.cand[1])
            & (rec_t["nslots"] == case.cand[2]))


def empty_trace(name):
    """ASE-bound case: a 400 Gb/s demand at the reset state, followed by ordinary requests of a seeded generator.  The pair is
    chosen on the oracle: among all pairs whose (route 0, top format, slot 0) is accepted on the empty network (g - thr[top] >= 0),
    the one that lies closest to the threshold, i.e. the longest such route."""
    c = CASES[name]
    tb, thr = tables_of(name), thresholds()
    holder0 = nat.ConfigHolder(tb, batch=1, **config_kw(name))
    rng = np.random.default_rng(4600 + SEED)
    n = 48
    reqs = np.zeros(n, nat.REQUEST_DTYPE)
    reqs["arrival_time"] = np.cumsum(rng.exponential(10800.0 / _KW["load"], n)).astype(np.float32)
    reqs["holding_time"] = rng.exponential(10800.0, n).astype(np.float32)
    src = rng.integers(0, tb.n_nodes, n)
    reqs["source"], reqs["destination"] = src, (src + rng.integers(1, tb.n_nodes, n)) % tb.n_nodes
    reqs["bit_rate"] = rng.choice(np.array(_KW["bit_rates"]), n)
    reqs["bit_rate"][0] = 400.0
    best = None
    for a in range(tb.n_nodes):
        for b in range(tb.n_nodes):
            if a == b:
                continue
            reqs["source"][0], reqs["destination"][0] = a, b
            o = OracleEnv(holder0, replica=0)
            o.set_trace(reqs)
            o.reset()
            rec = o.run_policy(c["policy"], 1)[0]
            if not rec["accepted"] or rec["route"] != 0 or rec["slot"] != 0 or rec["modulation"] != len(thr) - 1:
                continue
            d = float(rec["osnr"] - thr[int(rec["modulation"])] - c["m0"])
            if best is None or d < best[0]:
                best = (d, a, b)
    reqs["source"][0], reqs["destination"][0] = best[1], best[2]
    return reqs


@functools.lru_cache(maxsize=None)
def find_case(name) -> Case:
    """The case of the table: base records, t*, g, m, the candidate (path, slot, n), the ladder, and the 21 rungs' oracle runs.
    Refuses (ValueError) a case whose rungs' histories are not bit-identical before t*, or whose oracle decisions at t* are not
    g >= thr[m] + margin_r on every rung.  Seed 5 unless the table says otherwise."""
    c = CASES[name]
    if c.get("empty"):
        case = build_case(name, SEED, base_trace=empty_trace(name), find=1)
    else:
        case = build_case(name, c.get("seed", SEED))
    return case


# The pending states on which every fused policy 0..11 is compared with the oracle.  Together they give every policy id a ladder
# on which its answer changes, except lowest fragmentation (10): the search above (180 first-fit ladders) found none.  It scores
# every candidate of every route and takes the best score; the ladder's candidate was never the one whose refusal moved it.
POLICY_CASES = ("ff_nsfnet_m0", "ff_nsfnet_m1", "ff_nobeleu", "ff_nsfnet_s2", "ff_nsfnet_s13", "lb_nsfnet", "hsnr_nsfnet")
NO_CHANGING_LADDER = (10,)


@functools.lru_cache(maxsize=None)
def changing_policies(name) -> tuple:
    """The fused policies whose oracle answer in the pending state differs between the lowest and the highest rung."""
    case = find_case(name)
    lo, hi = pending_oracle(case, 0), pending_oracle(case, B - 1)
    return tuple(p for p in range(12) if lo.policy(p) != hi.policy(p))


def exact_rungs(case) -> np.ndarray:
    """Rungs held to their own oracle: |T_r - g| >= 1e-11 dB.  The exempt set is fixed by the ladder: at most 13 of 21."""
    ex = np.abs(case.T - case.g) >= ZONE_DB
    assert B - int(ex.sum()) <= 13
    return ex


def one_change(flags) -> int:
    """Index of the first rung that fell through when `flags` (accepted at format m, along T_r) changes exactly once from
    accepted to fallen through; -1 otherwise."""
    f = np.asarray(flags, bool)
    k = int(f.sum())
    return k if 0 < k < len(f) and f[:k].all() and not f[k:].any() else -1


# ---- ladders on a state that was reached under another margin -----------------------------------------------------------------
# The device builds them with B + 1 replicas: replica 0 keeps the base margin and runs the history, replicas 1..B hold the ladder
# and take replica 0's state by fork(src=[0]*(B+1), keep_params=True).  The oracle runs the history at the base margin and then
# takes the rung's margin (orc_set_margin).  The history is the first-fit run of ff_nsfnet_m0 (seed 5, margin 0).
STATE_CASE = "ff_nsfnet_m0"
MMI_T, MMI_MTC = 245, 3             # max_modulation_idx: found by a search over t on the oracle (4 on the low rungs, 3 on the high)
SERVICE_T = 200                     # running lightpaths: service_qot and action_impact
LF_T = 198                          # lowest fragmentation: a state in which the step accepts the policy's choice on both ends (in
                                    # most states the reference's step refuses it: the policy evaluates it one slot wider)


def state_kw(margins, **over) -> dict:
    return config_kw(STATE_CASE, replica_margin=[CASES[STATE_CASE]["m0"]] + [float(x) for x in margins], **over)


def state_oracles(t, margins=None, **over):
    """B oracles in the state after t first-fit steps at the base margin (one when margins is None), each with its rung's margin.
    With fewer formats in the window than there are, every step follows an observation, which moves the window (the codec of the
    step decodes the action under the window the observation left)."""
    holder = nat.ConfigHolder(tables_of(STATE_CASE), batch=1, **config_kw(STATE_CASE, **over))
    c = holder.struct
    pl = np.ctypeslib.as_array(c.path_len_norm, shape=(c.n_paths,))

    def make(r):
        o = OracleEnv(holder, replica=0)
        o.L.orc_seed(o.h, SEED, 0)
        o.reset()
        if "modulations_to_consider" in over:
            for _ in range(t):
                o.observe(pl, c.max_bit_rate)
                o.run_policy(FF, 1)
        elif t:
            o.run_policy(FF, t)
        if margins is not None:
            o.set_margin(margins[r])
        return o

    return holder, (threaded(make, B) if margins is not None else [make(0)])


def deciding_candidate(o, tb, thr, margin):
    """get_max_modulation_index's scan (envs/qrmsa.pyx:543-581) on the oracle's queries: path-major, best format first,
    candidates ascending; (route, path, format, slot, n, GSNR) of the first candidate that reaches thr + margin, or None."""
    q = o.request()
    for k in range(tb.k_paths):
        p = int(tb.pair_paths[int(q["source"]), int(q["destination"]), k])
        if p < 0:
            break
        avail = o.available(p)
        for m in range(len(thr) - 1, -1, -1):
            n = o.number_slots(float(q["bit_rate"]), m)
            for s in o.candidates(avail, n):
                g = float(o.gn(p, s, n)[0])
                if g >= thr[m] + margin:
                    return k, p, m, int(s), int(n), g
    return None


def _state_case(t, g, thr_m, **over) -> Case:
    case = Case()
    case.t, case.g, case.thr = t, float(g), thresholds()
    case.margins, case.T = ladder(case.g, thr_m)
    case.tables, case.seed = tables_of(STATE_CASE), SEED
    case.kw = state_kw(case.margins, **over)
    case.holder, case.oracles = state_oracles(t, case.margins, **over)
    return case


@functools.lru_cache(maxsize=None)
def mmi_case() -> Case:
    """The ladder on the candidate that decides max_modulation_idx of the request pending after MMI_T steps, with three formats in
    the window (the generic kernel, and the scan of the observation)."""
    tb, thr = tables_of(STATE_CASE), thresholds()
    holder, (o,) = state_oracles(MMI_T, modulations_to_consider=MMI_MTC)
    o.observe(np.ctypeslib.as_array(holder.struct.path_len_norm, shape=(holder.struct.n_paths,)), holder.struct.max_bit_rate)
    k, p, m, s, n, g = deciding_candidate(o, tb, thr, CASES[STATE_CASE]["m0"])
    case = _state_case(MMI_T, g, thr[m], modulations_to_consider=MMI_MTC)
    case.cand, case.route, case.m = (p, s, n), k, m
    return case


def oracle_mmi(case, o):
    """(max_modulation_idx after observation(), the mask, first fit's action under that window) of one rung's oracle."""
    c = case.holder.struct
    pl = np.ctypeslib.as_array(c.path_len_norm, shape=(c.n_paths,))
    _, mask = o.observe(pl, c.max_bit_rate)
    return int(o.max_modulation_idx), mask, o.policy_first_fit()


@functools.lru_cache(maxsize=None)
def service_case() -> Case:
    """The ladder on the lowest GSNR - minimum_osnr of the lightpaths running after SERVICE_T steps (service_qot's count of
    services below minimum_osnr + margin), restated with the oracle's literal GN (tests/test_gpu_service_qot.py)."""
    from test_gpu_service_qot import restate_gn
    tb, thr = tables_of(STATE_CASE), thresholds()
    holder, (o,) = state_oracles(SERVICE_T)
    svcs = o.services()
    want = restate_gn(o, tb, holder.mod_se, svcs)
    d = want[:, 0] - thr[svcs["modulation"]]
    y = int(np.argmin(d))
    case = _state_case(SERVICE_T, want[y, 0], thr[svcs["modulation"][y]])
    case.svcs, case.want, case.y, case.d = svcs, want, y, d
    return case


@functools.lru_cache(maxsize=None)
def impact_case() -> Case:
    """The ladder on a running lightpath's GSNR after a candidate action that shares a link with it (action_impact's count of
    victims newly below minimum_osnr + margin), restated as tests/test_gpu_action_impact.py restates it: first fit's action for
    the pending request if it has victims, else the first free placement (route-major, best format first) that has; the victim
    is the one with the lowest margin after."""
    from test_gpu_action_impact import restate_replica
    tb, thr = tables_of(STATE_CASE), thresholds()
    holder, (o,) = state_oracles(SERVICE_T)
    svcs, q = o.services(), o.request()
    actions = [o.policy_first_fit()[0]]
    for k in range(tb.k_paths):
        p = int(tb.pair_paths[int(q["source"]), int(q["destination"]), k])
        for m in range(len(thr) - 1, -1, -1):
            starts = o.candidates(o.available(p), o.number_slots(float(q["bit_rate"]), m)) if p >= 0 else []
            if starts:
                actions.append(o.encode(k, m, int(starts[0])))
    for action in actions:
        status, pairs = restate_replica(o, tb, holder, svcs, [action])
        if status[0] == 0 and len(pairs):
            break
    else:
        raise ValueError("no candidate action with victims")
    i = int(np.argmin(pairs[:, 3] - pairs[:, 4]))
    case = _state_case(SERVICE_T, pairs[i, 3], pairs[i, 4])
    case.svcs, case.action, case.status, case.pairs, case.i = svcs, int(action), status, pairs, i
    return case


@functools.lru_cache(maxsize=None)
def policy_state_case(pid, t=LF_T) -> Case:
    """A ladder for a policy that evaluates every candidate (lowest fragmentation: a history at the ladder's margins would leave
    the base history early).  On the state after t first-fit steps at the base margin, the candidate the policy chooses for the
    pending request is refused from some margin on; that margin is found on the oracle by bisection down to neighbouring
    doubles, and g = thr[m] + that margin is the GSNR the policy's own evaluation of the candidate reached."""
    thr, m0 = thresholds(), CASES[STATE_CASE]["m0"]
    _, (o,) = state_oracles(t)
    first = o.policy(pid)
    m = o.decode(first[0])[1]
    lo, hi = m0, m0 + 8.0
    o.set_margin(hi)
    if o.policy(pid) == first:
        raise ValueError(f"policy {pid}: the answer does not change up to margin {hi}")
    while True:
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        o.set_margin(mid)
        if o.policy(pid) == first:
            lo = mid
        else:
            hi = mid
    case = _state_case(t, thr[m] + lo, thr[m])
    case.policy, case.m, case.first = pid, m, first
    return case
