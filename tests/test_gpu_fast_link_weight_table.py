"""The lean kernels (csrc/ongym_fast.hpp) take an interferer's shared-link weight sums (sum w1, sum w2 over the links it shares
with the candidate route) from a table built at create (csrc/ongym_lwtab.hpp) instead of summing them link by link: one 16-byte
entry per (route, subset of the route's links), found by a per-route multiplicative hash of the shared-link mask.  Environments
whose link masks need two words (M64) and environments created under ONGYM_FAST_NO_LWTAB=1 keep the link loop.

1. The table, read back through ongym_query_link_weight_entry, equals a restatement: fp64, the link weights of
   ongym_hip.hip's create added in ascending link order starting from 0.0; the index is injective per route.
2. Table path and loop path of the same library give the same statistics, grids and step records (NSFNET, S = 320, the benchmark's
   load and table size, 64 replicas x 1200 requests with episodes of 1000: every replica is reset once).  First fit reads the
   table; load balancing is run the same way although fast_lw_policy() leaves it on the loop (it gained nothing from the table):
   the switch must then change nothing.
3. First fit against the CPU oracle on NSFNET (one and two cache groups both occur) and on a three-node line whose two-hop route
   shares a link with every service: with more than 128 services running its interferers overflow the register cache, and the
   loop beyond the cache reads the table too.  The line also has one-hop routes and node pairs with a single route.
4. nobel-eu (41 links, M64) reports no table and runs.
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym._tables import StaticTables
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from optical_networking_gym.topology import get_topology
from oracle_lib import OracleEnv

pytestmark = pytest.mark.gpu

POLICIES = {"first_fit": nat.POLICY_FIRST_FIT, "load_balancing": nat.POLICY_LOAD_BALANCING}
SEED = 5
CACHE = 128         # interferers of a route held in registers by the one-mask-word kernels (2 groups of 64)


def config(S, capacity, load, episode_length):
    return dict(modulations=jocn_modulations(), num_spectrum_resources=S, capacity=capacity, load=load,
                bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), auto_reset=True, episode_length=episode_length)


def link_weights(t):
    """(w1, w2) per link as ongym_create computes them (ongym_hip.hip: nspans * l_eff, nspans * l_eff * (l_eff / span length))."""
    w1, w2 = [], []
    for e in range(t.n_links):
        a, L, ns = float(t.link_alpha[e]), float(t.link_span_km[e]), float(int(t.link_nspans[e]))
        l_eff = (1.0 - math.exp(-2.0 * a * L * 1e3)) / (2.0 * a)
        w1.append(ns * l_eff)
        w2.append(ns * l_eff * (l_eff / (L * 1e3)))
    return w1, w2


# ---- 1. the table against a restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nsfnet", "cost239"])
def test_table_equals_restatement_and_index_is_injective(name):
    t = golden_tables(name)
    env = BatchedQRMSAEnv(tables=t, batch_size=1, **config(320, 64, 100.0, 1000))
    env.seed(SEED); env.reset()
    assert env.occupancy()["lean_kernel"]
    w1, w2 = link_weights(t)
    entries = 0
    for p in range(t.n_paths):
        links = sorted(int(l) for l in t.path_links[p, :t.path_hops[p]])
        H = len(links)
        seen = set()
        mult = bits = None
        for sub in range(1 << H):
            chosen = [links[i] for i in range(H) if sub >> i & 1]           # ascending link order
            mask = sum(1 << l for l in chosen)
            got = env.link_weight_entry(p, mask)
            assert got is not None, "no table"
            a = b = 0.0
            for l in chosen:
                a = a + w1[l]
                b = b + w2[l]
            assert (got["w1"], got["w2"]) == (a, b), (name, p, chosen, got, a, b)
            if mult is None:
                mult, bits = got["mult"], got["bits"]
            assert (got["mult"], got["bits"]) == (mult, bits) and mult != 0
            assert H <= bits <= H + 2 and 0 <= got["index"] < (1 << bits)
            seen.add(got["index"])
            entries += 1
        assert len(seen) == 1 << H, (name, p, "index not injective")
        # links that are not on the route do not matter; no shared link is the empty subset: index 0, entry (0, 0)
        route = sum(1 << l for l in links)
        other = ~route & ((1 << t.n_links) - 1)
        empty = env.link_weight_entry(p, other)
        assert (empty["index"], empty["w1"], empty["w2"]) == (0, 0.0, 0.0)
        assert env.link_weight_entry(p, route | other) == env.link_weight_entry(p, route)
    print(f"{name}: {t.n_paths} routes, {entries} entries checked ({entries * 16} bytes can be read by a kernel)")


# ---- 2. table path against loop path ---------------------------------------------------------------------------------------
NSF = dict(B=64, S=320, capacity=448, load=300.0, episode_length=1000)       # the benchmark's NSFNET workload
LAUNCHES = (250, 250, 250, 250, 200)                                         # 1200 requests: crosses the reset at 1000


def run_nsfnet(pid, record, table, monkeypatch):
    if table:
        monkeypatch.delenv("ONGYM_FAST_NO_LWTAB", raising=False)
    else:
        monkeypatch.setenv("ONGYM_FAST_NO_LWTAB", "1")          # read at ongym_create
    t = golden_tables("nsfnet")
    env = BatchedQRMSAEnv(tables=t, batch_size=NSF["B"], **config(NSF["S"], NSF["capacity"], NSF["load"], NSF["episode_length"]))
    env.seed(SEED); env.reset()
    assert env.occupancy(pid)["lean_kernel"]
    assert (env.link_weight_entry(0, 0) is not None) == table
    recs = [env.step_policy(n, record=record, policy=pid) for n in LAUNCHES]
    grids = np.stack([env.grid(r) for r in range(NSF["B"])])
    return env.stats(), grids, (np.concatenate(recs) if record else None)


@pytest.mark.parametrize("record", [False, True], ids=["norecord", "record"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("policy", list(POLICIES))
def test_table_path_equals_loop_path(policy, wide, record, monkeypatch):
    if wide:
        monkeypatch.setenv("ONGYM_FORCE_WIDE", "1")
    pid = POLICIES[policy]
    st_t, grid_t, rec_t = run_nsfnet(pid, record, True, monkeypatch)
    st_l, grid_l, rec_l = run_nsfnet(pid, record, False, monkeypatch)
    assert (st_t["episodes_completed"] >= 1).all()              # the run crossed an episode reset in every replica
    for f in st_t.dtype.names:
        assert np.array_equal(st_t[f], st_l[f]), f
    assert np.array_equal(grid_t, grid_l)
    if record:
        for f in rec_t.dtype.names:
            assert np.array_equal(rec_t[f], rec_l[f]), f


# ---- 3. against the CPU oracle ---------------------------------------------------------------------------------------------
STATS = ("services_processed", "services_accepted", "episode_services_processed", "episode_services_accepted",
         "bit_rate_requested", "bit_rate_provisioned", "episode_bit_rate_provisioned", "rejected", "episodes_completed",
         "total_steps", "total_accepted", "total_paths_tried", "total_path_hops", "total_active_sum", "current_time", "active")
ORACLE_B, ORACLE_STEPS = 32, 600


def first_fit_vs_oracle(t, cfg):
    """First fit on the device and on one oracle per replica: every final state equal.  Returns (device stats, oracle records)."""
    holder = nat.ConfigHolder(t, batch=ORACLE_B, **cfg)
    want = np.zeros((ORACLE_STEPS, ORACLE_B), nat.STEP_DTYPE)
    oracles = [OracleEnv(holder, replica=r) for r in range(ORACLE_B)]

    def run(r):
        oracles[r].seed(SEED); oracles[r].reset()
        want[:, r] = oracles[r].run_policy(nat.POLICY_FIRST_FIT, ORACLE_STEPS)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(run, range(ORACLE_B)))
    env = BatchedQRMSAEnv(tables=t, batch_size=ORACLE_B, **cfg)
    env.seed(SEED); env.reset()
    assert env.occupancy()["lean_kernel"] and env.link_weight_entry(0, 0) is not None
    for n in (1, 99, 250, 250):
        env.step_policy(n, record=False)
    st = env.stats()
    for r in range(ORACLE_B):
        o = oracles[r]
        np.testing.assert_array_equal(env.grid(r), o.grid(), err_msg=f"replica {r}: grid")
        a = np.sort(env.services(r), order=["release_time", "path_id", "slot"])
        b = np.sort(o.services(), order=["release_time", "path_id", "slot"])
        assert a.tobytes() == b.tobytes(), f"replica {r}: services"
        so = o.stats()
        for f in STATS:
            assert st[r][f] == so[f], (r, f, st[r][f], so[f])
        np.testing.assert_array_equal(st[r]["episode_modulation_hist"], so["episode_modulation_hist"])
    return st, want


def test_first_fit_nsfnet_vs_oracle():
    st, want = first_fit_vs_oracle(golden_tables("nsfnet"), config(320, 448, 300.0, 4000))
    print(f"nsfnet: services running at the end {int(st['active'].min())}..{int(st['active'].max())}")
    # a route's interferers are a share of the running services: with up to ~300 of them, routes with at most 64 interferers
    # (one cache group) and routes with more (two) both occur
    assert st["active"].max() > 2 * 64


def test_first_fit_line_beyond_the_cache_vs_oracle(tmp_path):
    # nodes 1 - 2 - 3: routes 1-2 and 2-3 have one link, route 1-3 both, and every node pair has this one route (k = 5 asked for).
    # Every running service shares a link with route 1-3, so that route's interferer count is the number of running services.
    path = tmp_path / "line3.txt"
    path.write_text("3\n2\n1 2 400\n2 3 600\n")
    t = StaticTables.from_topology(get_topology(str(path), None, jocn_modulations(), 80, 0.2, 4.5, 5))
    assert sorted(t.path_hops.tolist()) == [1, 1, 2] and (t.pair_paths[:, :, 1:] == -1).all()
    # load 200: the CPU oracle ends 600 requests with 141..167 services running in each of the 32 replicas (seed 5)
    st, want = first_fit_vs_oracle(t, config(320, 320, 200.0, 4000))
    over = (want["active"] > CACHE).sum(0)
    print(f"line: services running at the end {int(st['active'].min())}..{int(st['active'].max())}; steps with more than {CACHE} "
          f"per replica {int(over.min())}..{int(over.max())}")
    # (a third of the requests ask for 1-3, so hundreds of its evaluations per replica run past the register cache)
    assert st["active"].min() > CACHE and over.min() >= 100


# ---- 4. two-word masks keep the loop ---------------------------------------------------------------------------------------
def test_m64_environment_has_no_table_and_runs():
    t = golden_tables("nobel-eu")
    assert t.n_links > 32
    env = BatchedQRMSAEnv(tables=t, batch_size=8, **config(320, 256, 200.0, 1000))
    env.seed(SEED); env.reset()
    assert env.occupancy()["lean_kernel"]
    assert env.link_weight_entry(0, 1) is None
    env.step_policy(200, record=False)
    st = env.stats()
    assert (st["total_steps"] == 200).all() and (st["total_accepted"] > 0).all()
