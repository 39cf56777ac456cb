"""The interferer list build of the lean first-fit kernels (csrc/ongym_fast.hpp: build_cache) exists twice: straight-line code over
chunks 0..3 of 64 records while at most 256 services run in a table of at least 256 entries (four_chunks), and the chunk loop
for everything else, which is also what the other policies run.  A replica changes from one to the other and back whenever its
number of running services crosses 256, in the middle of a launch.  The format loop, the wave sum and the wave minimum that
every lean policy shares were rewritten in the same change (same results, fewer instructions) and are held to the oracle by
the same runs.

First fit and load balancing on NSFNET, S = 320, capacity 320, 64 replicas, 1500 requests per replica in launches of uneven
length, in the narrow and the wide build (ONGYM_FORCE_WIDE=1), with and without step records, against the CPU oracle: final
grids, services (sorted), statistics, and the step records where they are written.

The case proves from the oracle's step records (`active` after every step) that both paths ran and that the hand-over
happened in both directions: at least a quarter of the replicas must cross 256 upwards and downwards.  The load was chosen
with exactly this count on the CPU (seed 5, 64 replicas, 1500 steps; episodes longer than the run, so no reset empties the
network):

    load   policy           replicas crossing up and down   crossings per replica (up + down)   steps with active > 256   most services
     275   first fit        62 of 64                        1..68                               0.06..0.61                318
     275   load balancing   50 of 64                        0..44                               0.00..0.41                290

(the test prints these figures before it asserts).  The table never fills at this load (the library reports a full table as an
error of the statistics call); at load 280 first fit fills it in three steps.  Load balancing rejects 9 % of the requests, so
it runs fewer services than first fit: at load 285 the counts are 60 and 54 of 64.

A second, small configuration has a table of 192 entries: it can only take the chunk loop, with up to three chunks in use, and
must agree with the oracle all the same.
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
POLICIES = {"first_fit": nat.POLICY_FIRST_FIT, "load_balancing": nat.POLICY_LOAD_BALANCING}
FOUR = 256                                          # the straight-line scans cover records 0..255
LAUNCHES = (1, 63, 250, 7, 500, 129, 550)           # 1500 requests, split unevenly
SEED = 5

BIG = dict(B=64, S=320, capacity=320, load=275.0)
SMALL = dict(B=4, S=320, capacity=192, load=130.0)
SMALL_LAUNCHES = (3, 200, 64, 333)


def config(c):
    return dict(modulations=jocn_modulations(), num_spectrum_resources=c["S"], capacity=c["capacity"], load=c["load"],
                bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), auto_reset=True, episode_length=4000)


_oracle = {}


def oracle_run(name, pid, c, steps):
    """Step records [steps, B] and the oracles (final state) of one configuration and policy: computed once, only read afterwards."""
    key = (name, pid)
    if key not in _oracle:
        holder = nat.ConfigHolder(golden_tables("nsfnet"), batch=c["B"], **config(c))
        recs = np.zeros((steps, c["B"]), nat.STEP_DTYPE)
        envs = [OracleEnv(holder, replica=r) for r in range(c["B"])]

        def run(r):         # one oracle per replica, no shared state: the C calls run side by side (ctypes drops the GIL)
            envs[r].seed(SEED); envs[r].reset()
            recs[:, r] = envs[r].run_policy(pid, steps)

        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            list(pool.map(run, range(c["B"])))
        _oracle[key] = (holder, recs, envs)
    return _oracle[key]


def crossings(active):
    """Per replica: times the running services went from <= FOUR to > FOUR and back (the network starts empty)."""
    above = np.concatenate([np.zeros((1, active.shape[1]), bool), active > FOUR])
    up = (~above[:-1] & above[1:]).sum(0)
    down = (above[:-1] & ~above[1:]).sum(0)
    return up, down


def assert_records_equal(got, want, ctx):
    for f in EXACT:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(got[f] != want[f])[0]
            raise AssertionError(f"{ctx}: field {f} differs first at {tuple(bad)}: {got[f][tuple(bad)]} != {want[f][tuple(bad)]}")
    for f in ("osnr", "ase", "nli"):
        np.testing.assert_allclose(got[f], want[f], rtol=GSNR_RTOL, err_msg=f"{ctx}: {f}")


def run_and_compare(name, c, launches, pid, wide, record, monkeypatch):
    if wide:
        monkeypatch.setenv("ONGYM_FORCE_WIDE", "1")       # read at ongym_create
    steps = sum(launches)
    holder, want, oracles = oracle_run(name, pid, c, steps)
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=c["B"], **config(c))
    env.seed(SEED); env.reset()
    assert env.occupancy(pid)["lean_kernel"]
    got = [env.step_policy(n, record=record, policy=pid) for n in launches]
    ctx = f"{name} policy {pid} wide {wide} record {record}"
    if record:
        assert_records_equal(np.concatenate(got), want, ctx)
    st = env.stats()
    for r in range(c["B"]):
        o = oracles[r]
        np.testing.assert_array_equal(env.grid(r), o.grid(), err_msg=f"{ctx} replica {r}: grid")
        a = np.sort(env.services(r), order=["release_time", "path_id", "slot"])
        b = np.sort(o.services(), order=["release_time", "path_id", "slot"])
        assert a.tobytes() == b.tobytes(), f"{ctx} replica {r}: services"
        so = o.stats()
        for f in STATS:
            assert st[r][f] == so[f], (ctx, r, f, st[r][f], so[f])
        np.testing.assert_array_equal(st[r]["episode_modulation_hist"], so["episode_modulation_hist"])
        # first fit: the device settles some evaluations by the ASE bound (see test_gpu_parity.test_random_traffic_vs_oracle);
        # load balancing examines the routes in ascending load order and stops at the first that serves, so its effort counters
        # are not the oracle's
        if pid == nat.POLICY_FIRST_FIT:
            assert st[r]["total_gn_evals"] <= so["total_gn_evals"] <= st[r]["total_gn_evals"] + st[r]["total_gn_shortcuts"]
    return want


@pytest.mark.parametrize("record", [False, True], ids=["norecord", "record"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("policy", list(POLICIES))
def test_scans_change_paths_at_256_services_vs_oracle(policy, wide, record, monkeypatch):
    pid = POLICIES[policy]
    want = run_and_compare("big", BIG, LAUNCHES, pid, wide, record, monkeypatch)
    assert not (want["flags"] & nat.F_OVERFLOW).any()
    up, down = crossings(want["active"].astype(np.int64))
    both = int(((up > 0) & (down > 0)).sum())
    share = (want["active"] > FOUR).mean(0)
    print(f"{policy}: {both} of {BIG['B']} replicas cross {FOUR} up and down; crossings per replica {int((up + down).min())}.."
          f"{int((up + down).max())}; share of steps above {share.min():.2f}..{share.max():.2f}; most services "
          f"{int(want['active'].max())}; rejected {int((want['accepted'] == 0).sum())}")
    assert 4 * both >= BIG["B"], (both, BIG["B"])
    # the hand-over also happens inside launches, not only between them: some crossing lies away from every launch boundary
    edges = np.cumsum(LAUNCHES)[:-1]
    above = want["active"] > FOUR
    change = np.argwhere(above[1:] != above[:-1])[:, 0] + 1
    assert np.setdiff1d(change, edges).size > 0


@pytest.mark.parametrize("policy", list(POLICIES))
def test_table_smaller_than_256_keeps_the_chunk_loops_vs_oracle(policy, monkeypatch):
    pid = POLICIES[policy]
    want = run_and_compare("small", SMALL, SMALL_LAUNCHES, pid, False, True, monkeypatch)
    most = int(want["active"].max())
    print(f"{policy}: most services {most} of {SMALL['capacity']}")
    assert 2 * 64 < most <= SMALL["capacity"] < FOUR      # three chunks of 64 records in use, and never the straight-line path
