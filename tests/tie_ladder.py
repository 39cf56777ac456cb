"""A ladder of near-ties between two equal routes, for the winner's choice of highest SNR (policy 2), one environment per rung.

heuristic_highest_snr keeps the first candidate and replaces it only on a strict `osnr > best_osnr` (heuristics.py:316, the
oracle's oracle/ongym_oracle.c policy_highest_snr).  The kernels widen that comparison by a tie band (kTieBandDb,
csrc/ongym_device.hpp; DESIGN section 2, "Decision exactness") that absorbs the rounding noise between the sums of two equal
routes.  Random traffic meets exact ties (equal routes on an empty network) and differences of 1e-3 dB and more, nothing between,
so the differences between are built here:

  topology   a four-node diamond a, b, c, d with links 0: a-b, 1: b-d, 2: a-c, 3: c-d, all four the link of
             tests/golden/tables_ring4.json (250 km, 4 spans of 62.5 km, its alpha and nf), two routes per pair; for (a, d) route 0 is
             links [0, 1] and route 1 links [2, 3]: link-disjoint and equal in every parameter.
  lever      link_nf of one link times (1 + eps).  It enters the route's ASE linearly and leaves uniform_alpha alone
             (csrc/ongym_tables.hpp), so the lean kernels stay eligible.  Ladder "route1" turns link 3 (route 1 is read from
             path_ase), ladder "route0" link 1 (the first route goes through the pre_* / first-route record).  eps > 0 makes the
             ladder's own route the worse one.
  rungs      eps in {0, +-1e-15, +-1e-13, +-2e-12, +-3e-11, +-1e-10, +-2e-10, +-4e-10, +-1e-9, +-1e-8, +-1e-6}: 21 environments, each with
             its own tables and its own oracles.
  replicas   B = 3 at launch powers -3, 0, +2 dBm, margin 0: the difference delta between the routes' best candidates is about
             2.1 |eps|, 1.8 |eps| and 1.1 |eps| dB, and at +2 dBm some winners are the second-best format.
  requests   one host trace for every replica: identical requests a -> d at 400 Gb/s, arrivals 1, 2, 3, ..., holding time 1e6 (nothing
             departs).  Case "s64": S = 64, 9 requests; case "s160": S = 160, 21 requests (several 64-slot passes per format).  The
             trace carries one request more, which stays pending after the last step.  Decision 2j (0-based; the issue's request
             2j + 1) meets j services on each route and is the laddered one; decision 2j + 1 restores the symmetry.

For every rung, replica and decision the builder restates the policy on the oracle's queries (candidates, available, gn): the best
passing candidate of each route, delta = best GSNR of route 1 - best of route 0, and the distance of every evaluated candidate from
its admission threshold.  A decision is exact when |delta| >= 1e-11 dB (ZONE_DB, the project's exempt zone) and exempt otherwise.

This module imports no GPU library; tests/test_tie_ladder_host.py holds, on the oracle alone, the conditions that keep
tests/test_gpu_tie_ladder.py from passing emptily.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from common import jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym._tables import StaticTables
from oracle_lib import OracleEnv

B = 3
POWERS_DBM = (-3.0, 0.0, 2.0)
ZONE_DB = 1e-11             # decisions whose routes differ by less are exempt from oracle parity (tests/threshold_ladder.py)
EPS_MAGS = (1e-15, 1e-13, 2e-12, 3e-11, 1e-10, 2e-10, 4e-10, 1e-9, 1e-8, 1e-6)
EPS = (0.0,) + tuple(s * x for x in EPS_MAGS for s in (-1.0, 1.0))
MAY_BE_EXEMPT = 2e-12       # rungs with |eps| above this hold only exact laddered decisions
CASES = {"s64": dict(S=64, n=9), "s160": dict(S=160, n=21)}
LADDERS = {"route1": 3, "route0": 1}        # name -> the link whose nf is turned
SRC, DST, BIT_RATE = 0, 3, 400.0
HSNR = nat.POLICY_HIGHEST_SNR

# the link of tests/golden/tables_ring4.json
_LINK = dict(length=250.0, nspans=4, span_km=62.5, alpha=2.3025850929940457e-05, nf=2.818382931264454)
_EDGES = ((0, 1), (1, 3), (0, 2), (2, 3))                   # a-b, b-d, a-c, c-d
# node pair -> its two routes as (nodes, links), the shorter first
_ROUTES = {
    (0, 1): (((0, 1), (0,)), ((0, 2, 3, 1), (2, 3, 1))),
    (0, 2): (((0, 2), (2,)), ((0, 1, 3, 2), (0, 1, 3))),
    (0, 3): (((0, 1, 3), (0, 1)), ((0, 2, 3), (2, 3))),
    (1, 2): (((1, 0, 2), (0, 2)), ((1, 3, 2), (1, 3))),
    (1, 3): (((1, 3), (1,)), ((1, 0, 2, 3), (0, 2, 3))),
    (2, 3): (((2, 3), (3,)), ((2, 0, 1, 3), (2, 0, 1))),
}


def diamond() -> dict:
    """The topology as a tests/golden/tables_*.json-shaped dict (StaticTables.from_golden)."""
    pairs, pid = {}, 0
    for (i, j), routes in _ROUTES.items():
        lst = []
        for k, (nodes, links) in enumerate(routes):
            lst.append(dict(id=pid, k=k, nodes=list(nodes), links=list(links), hops=len(links), length=_LINK["length"] * len(links)))
            pid += 1
        pairs[f"{i},{j}"] = lst
    return dict(name="diamond4", k_paths=2, node_names=["a", "b", "c", "d"],
                edges=[dict(index=e, a=a, b=b, **_LINK) for e, (a, b) in enumerate(_EDGES)], pairs=pairs)


@functools.lru_cache(maxsize=None)
def base_tables() -> StaticTables:
    return StaticTables.from_golden(diamond())


def rung_tables(link: int, eps: float) -> StaticTables:
    tb = base_tables()
    nf = tb.link_nf.copy()
    nf[link] = nf[link] * (1.0 + eps)
    return dataclasses.replace(tb, link_nf=nf)


def rung_topology(directory, link: int, eps: float):
    """The rung as the annotated graph the compatibility view (envs/qrmsa.py) takes: the diamond written as a topology file, read
    by get_topology, the lever on the noise figure of every span of `link`.  StaticTables.from_topology of it is rung_tables'."""
    import os
    from optical_networking_gym.topology import get_topology
    name = os.path.join(str(directory), "diamond4.txt")
    with open(name, "w", encoding="utf-8") as f:
        f.write("4\n4\n" + "".join(f"{a + 1} {b + 1} 250\n" for a, b in _EDGES))
    topology = get_topology(name, None, jocn_modulations(), 80, 0.2, 4.5, 2)
    nf = rung_tables(link, eps).link_nf         # the fixture's digits (10 ** 0.45 here is one ulp off them), and the lever
    for _, _, d in topology.edges(data=True):
        for span in d["link"].spans:
            span.noise_figure_normalized = float(nf[int(d["index"])])
    return topology


def trace(n: int) -> np.ndarray:
    """n identical requests and the one that stays pending after them."""
    reqs = np.zeros(n + 1, nat.REQUEST_DTYPE)
    reqs["arrival_time"] = np.arange(1, n + 2, dtype=np.float32)
    reqs["holding_time"] = 1e6
    reqs["source"], reqs["destination"], reqs["bit_rate"] = SRC, DST, BIT_RATE
    return reqs


def config_kw(case: str) -> dict:
    return dict(modulations=jocn_modulations(), num_spectrum_resources=CASES[case]["S"], capacity=64, load=10.0,
                bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), episode_length=1000, auto_reset=True, margin=0.0,
                replica_launch_power_dbm=POWERS_DBM)


def thresholds() -> np.ndarray:
    return np.array([m.minimum_osnr for m in jocn_modulations()], np.float64)


def laddered(t: int) -> bool:
    return t % 2 == 0


# per route of a decision: its best passing candidate, restated from the oracle's queries
BEST_DTYPE = np.dtype([("path", np.int32), ("modulation", np.int32), ("slot", np.int32), ("nslots", np.int32), ("osnr", np.float64)])


def restate_decision(o: OracleEnv, tb: StaticTables, thr: np.ndarray, margin: float = 0.0):
    """The policy's candidate walk on the pending request (route, format best first, slot ascending), from the oracle's queries:
    (best[2] in BEST_DTYPE, path -1 where no candidate of the route passes; the least |GSNR - threshold| over every candidate)."""
    q = o.request()
    cands, fmt, route = [], [], []
    for k in range(tb.k_paths):
        p = int(tb.pair_paths[int(q["source"]), int(q["destination"]), k])
        avail = o.available(p)
        for m in range(len(thr) - 1, -1, -1):
            n = o.number_slots(float(q["bit_rate"]), m)
            if n <= 0:
                continue
            for s in o.candidates(avail, n):
                cands.append((p, s, n)); fmt.append(m); route.append(k)
    best = np.zeros(tb.k_paths, BEST_DTYPE)
    best["path"], best["osnr"] = -1, -np.inf
    if not cands:
        return best, np.inf
    cands, fmt, route = np.array(cands, np.int32), np.array(fmt), np.array(route)
    g = o.gn_many(cands)[:, 0]
    T = thr[fmt] + margin
    ok = g >= T
    for k in range(tb.k_paths):
        idx = np.flatnonzero(ok & (route == k))
        if len(idx):
            i = idx[int(np.argmax(g[idx]))]                     # the first maximum: strict `>` keeps the earlier candidate
            best[k] = (cands[i, 0], fmt[i], cands[i, 1], cands[i, 2], g[i])
    return best, float(np.min(np.abs(g - T)))


class Rung:
    """One environment of a ladder: tables, configuration and, per replica, the oracle's run with the restated decisions.
    Everything is computed once and only read afterwards."""

    def exact(self) -> np.ndarray:
        """[n, B]: the decision's routes differ by at least ZONE_DB."""
        return np.abs(self.delta) >= ZONE_DB


def build_rung(case: str, ladder: str, eps: float) -> Rung:
    n, thr = CASES[case]["n"], thresholds()
    r = Rung()
    r.case, r.ladder, r.eps, r.n = case, ladder, eps, n
    r.tables = rung_tables(LADDERS[ladder], eps)
    r.kw = config_kw(case)
    r.holder = nat.ConfigHolder(r.tables, batch=B, **r.kw)
    r.trace = trace(n)
    r.recs = np.zeros((n, B), nat.STEP_DTYPE)
    r.best = np.zeros((n, B, 2), BEST_DTYPE)
    r.delta = np.zeros((n, B))
    r.dist = np.zeros((n, B))
    r.oracles = []
    for b in range(B):
        o = OracleEnv(r.holder, replica=b)
        o.set_trace(r.trace)
        o.reset()
        for t in range(n):
            r.best[t, b], r.dist[t, b] = restate_decision(o, r.tables, thr)
            r.delta[t, b] = r.best[t, b, 1]["osnr"] - r.best[t, b, 0]["osnr"]
            r.recs[t, b] = o.run_policy(HSNR, 1)[0]
        r.oracles.append(o)             # left in the final state
    return r


@functools.lru_cache(maxsize=None)
def find_ladder(case: str, ladder: str) -> tuple:
    """The 21 rungs of one ladder of one case, in the order of EPS."""
    return tuple(build_rung(case, ladder, eps) for eps in EPS)


def pending_oracles(rung: Rung, t: int) -> list:
    """Fresh oracles of the rung's replicas with t decisions taken and decision t pending."""
    out = []
    for b in range(B):
        o = OracleEnv(rung.holder, replica=b)
        o.set_trace(rung.trace)
        o.reset()
        if t:
            o.run_policy(HSNR, t)
        out.append(o)
    return out


def better_route(ladder: str, eps: float) -> int:
    """The route the sign of eps makes better (route 0, which leads, at eps = 0)."""
    if eps == 0.0:
        return 0
    own = 1 if ladder == "route1" else 0
    return own if eps < 0 else 1 - own
