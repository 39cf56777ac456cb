"""First fit without step records (csrc/ongym_fast.hpp) enters the walk over a pair's routes with the route id that came with the
request, fetches the next id only behind a route that failed, and provisions a request where its format passes, inside the
format loop; the kernels that write records keep the plain loop and provision after it.  Most requests never see a second
route, so the cases below are loaded until the later routes serve a good share of the traffic and many requests are rejected
(every route failed: the exact blocking flags of the reject path).

Every case runs first fit on 64 replicas, seed 5, in launches of uneven length, in the narrow and the wide build
(ONGYM_FORCE_WIDE=1), with and without step records, against the CPU oracle: the step records where they are written, final
grids, services (sorted) and statistics.  One case runs on the instantiation that sums link weights in a loop
(ONGYM_FAST_NO_LWTAB=1), one resets the network while later routes are in use, and one runs on nobel-eu (41 links: the kernels
with two mask words, which walk the routes the same way).

The inputs were chosen on the CPU oracle ("accepted by route" over all 64 replicas of the run of the test):

    case            topology  S    capacity  load  bit rates        requests  episode
    later_routes    nsfnet    160    448     400   10,40,100,400      1500     4000
    mostly_blocked  nsfnet     80    256     300   100,400            1500     4000
    reset           nsfnet    160    448     400   10,40,100,400      2100      700
    two_words       nobel-eu  160    512     600   10,40,100,400      1500     4000
    single_route    ring4      80    256      60   100,400            1500     4000

                    accepted  accepted by route 0..4               most services
    later_routes     82.9 %   67 321 / 7 376 / 3 171 / 1 134 / 605      348
    mostly_blocked   54.0 %   41 899 / 5 880 / 2 309 / 1 008 / 710      180
    reset            87.0 %   100 108 / 9 904 / 4 262 / 1 677 / 915     314
    two_words        73.5 %   58 868 / 6 312 / 2 767 / 1 532 / 1 047    423
    single_route     56.3 %   54 008 / 0 / 0 / 0 / 0                     49

Each case but the last recomputes its counts from the oracle's records and prints them, and asserts what keeps it from passing
vacuously: at least 10 % of the accepted requests are served by a route >= 1, every route index 0..4 serves at least 20
requests, at least 10 % of the requests are rejected, no F_OVERFLOW, and some change of route index lies away from every launch
boundary.

ring4 (three links in a line) has one route per node pair, so the walk ends at the -1 that follows it in the pair's list
whenever that route fails: the case asserts that and a rejection rate of at least 10 %.

No table these tests can reach has a pair of distinct nodes without a route (nsfnet, nobel-eu and cost239 have k = 5 routes for
every pair, ring4 one), so the reject of a request whose first route id is already -1 is not exercised here.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from oracle_lib import OracleEnv

pytestmark = pytest.mark.gpu

GSNR_RTOL = 1e-9
EXACT = ("action", "route", "modulation", "slot", "nslots", "accepted", "terminated", "retry", "flags", "active", "reward")
STATS = ("services_processed", "services_accepted", "episode_services_processed", "episode_services_accepted",
         "bit_rate_requested", "bit_rate_provisioned", "episode_bit_rate_provisioned", "rejected", "episodes_completed",
         "total_steps", "total_accepted", "total_paths_tried", "total_path_hops", "total_active_sum", "current_time", "active")
PID = nat.POLICY_FIRST_FIT
SEED = 5
B = 64
LAUNCHES_1500 = (1, 63, 250, 7, 500, 129, 550)
LAUNCHES_2100 = LAUNCHES_1500 + (600,)

CASES = {
    "later_routes": dict(topo="nsfnet", S=160, capacity=448, load=400.0, bit_rates=(10, 40, 100, 400), launches=LAUNCHES_1500,
                         episode_length=4000),
    "mostly_blocked": dict(topo="nsfnet", S=80, capacity=256, load=300.0, bit_rates=(100, 400), launches=LAUNCHES_1500,
                           episode_length=4000),
    "reset": dict(topo="nsfnet", S=160, capacity=448, load=400.0, bit_rates=(10, 40, 100, 400), launches=LAUNCHES_2100,
                  episode_length=700),
    "two_words": dict(topo="nobel-eu", S=160, capacity=512, load=600.0, bit_rates=(10, 40, 100, 400), launches=LAUNCHES_1500,
                      episode_length=4000),
    "single_route": dict(topo="ring4", S=80, capacity=256, load=60.0, bit_rates=(100, 400), launches=LAUNCHES_1500,
                         episode_length=4000),
}


def config(c):
    return dict(modulations=jocn_modulations(), num_spectrum_resources=c["S"], capacity=c["capacity"], load=c["load"],
                bit_rate_selection="discrete", bit_rates=c["bit_rates"], auto_reset=True, episode_length=c["episode_length"])


_oracle = {}


def oracle_run(name):
    """Step records [steps, B] and the oracles (final state) of one case: computed once, only read afterwards."""
    if name not in _oracle:
        c = CASES[name]
        steps = sum(c["launches"])
        holder = nat.ConfigHolder(golden_tables(c["topo"]), batch=B, **config(c))
        recs = np.zeros((steps, B), nat.STEP_DTYPE)
        envs = [OracleEnv(holder, replica=r) for r in range(B)]

        def run(r):         # one oracle per replica, no shared state: the C calls run side by side (ctypes drops the GIL)
            envs[r].seed(SEED); envs[r].reset()
            recs[:, r] = envs[r].run_policy(PID, steps)

        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            list(pool.map(run, range(B)))
        _oracle[name] = (holder, recs, envs)
    return _oracle[name]


def assert_records_equal(got, want, ctx):
    for f in EXACT:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(got[f] != want[f])[0]
            raise AssertionError(f"{ctx}: field {f} differs first at {tuple(bad)}: {got[f][tuple(bad)]} != {want[f][tuple(bad)]}")
    for f in ("osnr", "ase", "nli"):
        np.testing.assert_allclose(got[f], want[f], rtol=GSNR_RTOL, err_msg=f"{ctx}: {f}")


def check_routes(name, want):
    """The counts of the case, printed, then the conditions that keep it from passing vacuously."""
    c = CASES[name]
    acc = want["accepted"].astype(bool)
    route = want["route"].astype(np.int64)
    by_route = [int((acc & (route == k)).sum()) for k in range(5)]
    n_acc, n_all = int(acc.sum()), acc.size
    overflow = int((want["flags"] & nat.F_OVERFLOW).astype(bool).sum())
    edges = np.cumsum(c["launches"])[:-1]
    # a change of the serving route between two consecutive requests of a replica, both accepted
    both = acc[1:] & acc[:-1] & (route[1:] != route[:-1])
    change = np.unique(np.argwhere(both)[:, 0] + 1)
    print(f"{name}: requests {n_all} accepted {n_acc / n_all:.3f} by route " + " / ".join(str(x) for x in by_route)
          + f" rejected {1 - n_acc / n_all:.3f} overflow {overflow} most services {int(want['active'].max())} "
          f"steps with a change of route {change.size}")
    assert overflow == 0
    assert 10 * (n_acc - by_route[0]) >= n_acc, (name, by_route)
    assert min(by_route) >= 20, (name, by_route)
    assert 10 * (n_all - n_acc) >= n_all, (name, n_acc, n_all)
    assert np.setdiff1d(change, edges).size > 0, name


def run_and_compare(name, wide, record, table, monkeypatch):
    c = CASES[name]
    if wide:
        monkeypatch.setenv("ONGYM_FORCE_WIDE", "1")       # read at ongym_create
    if table:
        monkeypatch.delenv("ONGYM_FAST_NO_LWTAB", raising=False)
    else:
        monkeypatch.setenv("ONGYM_FAST_NO_LWTAB", "1")    # read at ongym_create
    holder, want, oracles = oracle_run(name)
    env = BatchedQRMSAEnv(tables=golden_tables(c["topo"]), batch_size=B, **config(c))
    env.seed(SEED); env.reset()
    assert env.occupancy(PID)["lean_kernel"]
    if c["topo"] == "nsfnet":
        assert (env.link_weight_entry(0, 0) is not None) == table
    got = [env.step_policy(n, record=record, policy=PID) for n in c["launches"]]
    ctx = f"{name} wide {wide} record {record} table {table}"
    if record:
        assert_records_equal(np.concatenate(got), want, ctx)
    st = env.stats()
    for r in range(B):
        o = oracles[r]
        np.testing.assert_array_equal(env.grid(r), o.grid(), err_msg=f"{ctx} replica {r}: grid")
        a = np.sort(env.services(r), order=["release_time", "path_id", "slot"])
        b = np.sort(o.services(), order=["release_time", "path_id", "slot"])
        assert a.tobytes() == b.tobytes(), f"{ctx} replica {r}: services"
        so = o.stats()
        for f in STATS:
            assert st[r][f] == so[f], (ctx, r, f, st[r][f], so[f])
        np.testing.assert_array_equal(st[r]["episode_modulation_hist"], so["episode_modulation_hist"])
        # the device settles some evaluations by the ASE bound (see test_gpu_parity.test_random_traffic_vs_oracle)
        assert st[r]["total_gn_evals"] <= so["total_gn_evals"] <= st[r]["total_gn_evals"] + st[r]["total_gn_shortcuts"]
    if name != "single_route":
        check_routes(name, want)
    return want


@pytest.mark.parametrize("record", [False, True], ids=["norecord", "record"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("name", ["later_routes", "mostly_blocked"])
def test_later_routes_and_rejections_vs_oracle(name, wide, record, monkeypatch):
    run_and_compare(name, wide, record, True, monkeypatch)


def test_later_routes_on_the_link_loop_instantiation_vs_oracle(monkeypatch):
    run_and_compare("later_routes", False, False, False, monkeypatch)


@pytest.mark.parametrize("record", [False, True], ids=["norecord", "record"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_episode_reset_while_later_routes_are_in_use_vs_oracle(wide, record, monkeypatch):
    want = run_and_compare("reset", wide, record, True, monkeypatch)
    term = want["terminated"].astype(bool)
    assert (term.sum(0) == 3).all()
    # later routes serve requests in the last hundred requests before every reset
    at = np.argwhere(term)
    for t, r in at:
        w = want[max(0, t - 100):t + 1, r]
        assert (w["accepted"].astype(bool) & (w["route"] >= 1)).any(), (int(t), int(r))


@pytest.mark.parametrize("wide,record", [(False, False), (True, False), (False, True)], ids=["narrow", "wide", "narrow-record"])
def test_later_routes_with_two_mask_words_vs_oracle(wide, record, monkeypatch):
    run_and_compare("two_words", wide, record, True, monkeypatch)


@pytest.mark.parametrize("record", [False, True], ids=["norecord", "record"])
def test_pairs_with_a_single_route_vs_oracle(record, monkeypatch):
    want = run_and_compare("single_route", False, record, True, monkeypatch)
    pairs = np.asarray(golden_tables("ring4").pair_paths).reshape(-1, golden_tables("ring4").k_paths)
    assert (pairs[:, 1:] < 0).all()                 # nothing follows a pair's first route
    acc = want["accepted"].astype(bool)
    print(f"single_route: accepted {acc.mean():.3f} by route 0 {int((acc & (want['route'] == 0)).sum())} "
          f"most services {int(want['active'].max())}")
    assert not (want["flags"] & nat.F_OVERFLOW).any()
    assert 10 * int((~acc).sum()) >= acc.size
    assert (want["route"][acc] == 0).all()
