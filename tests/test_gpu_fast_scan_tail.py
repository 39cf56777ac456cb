"""The lean first-fit kernels (csrc/ongym_fast.hpp) scan the records of the running services in three ways, chosen per request by
the number of running services:

  * interferer list build (build_cache): chunks 0..3 of 64 records straight, then, above 256 services, chunks 4..6 one at a time
    (the tail, up to 448 services in a table that holds the chunk), and the chunk loop for everything beyond;
  * release scan (one mask word): whole trips over four chunks, highest first, while four chunks are left, then the remaining
    chunks (at most three) one at a time: with five chunks in use, one trip over chunks 4..1 and chunk 0 on its own.

A replica moves between these whenever its number of running services crosses 256, 320, 384 or 448, in the middle of a launch.
Every case below runs first fit on NSFNET, S = 320, 64 replicas, in launches of uneven length, in the narrow and the wide build
(ONGYM_FORCE_WIDE=1), with and without step records, against the CPU oracle: final grids, services (sorted), statistics, and the
step records where they are written.  The headline mix also runs on the instantiation that sums link weights in a loop
(ONGYM_FAST_NO_LWTAB=1).

The inputs were chosen on the CPU oracle (seed 5, 64 replicas, episodes longer than the run, so no reset empties the network);
"cross N" = the replica went above N running services and came back at least once:

    case        capacity  load  bit rates        requests  most  overflow  cross 256  cross 320  cross 384  cross 448  steps > 256
    headline       448     300  10,40,100,400      1500     342     0         47         12          0          0         0.58
    seven          448     385  10,40              2000     443     0         29         48         54          0         0.79
    table384       384     330  10,40              2000     380     0         48         64          0          0         0.75
    beyond         576     450  10,40              2000     502     0         26         35         55         45         0.81

Each case recomputes and prints these counts from the oracle's step records and asserts, for every boundary it is there for, that
at least a quarter of the replicas cross it in both directions, that some crossing lies away from every launch boundary, and that
the table never fills (the library reports a full table as an error of the statistics call).

The last case resets the episode while the tail is in use: capacity 448, load 385, bit rates (10, 40), episodes of 700 requests,
2100 requests: three resets per replica, 266 to 361 services in the record of each terminal step (most 361, no overflow).
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
B, S = 64, 320
BOUNDS = (256, 320, 384, 448)
LAUNCHES_1500 = (1, 63, 250, 7, 500, 129, 550)          # the launch lengths of test_gpu_fast_four_chunk
LAUNCHES_2000 = LAUNCHES_1500 + (500,)
LAUNCHES_2100 = LAUNCHES_2000 + (100,)

# name: capacity, load, bit rates, launches, episode length, boundaries that at least a quarter of the replicas must cross
CASES = {
    "headline": dict(capacity=448, load=300.0, bit_rates=(10, 40, 100, 400), launches=LAUNCHES_1500, episode_length=4000, cross=(256,)),
    "seven": dict(capacity=448, load=385.0, bit_rates=(10, 40), launches=LAUNCHES_2000, episode_length=4000, cross=(256, 320, 384)),
    "table384": dict(capacity=384, load=330.0, bit_rates=(10, 40), launches=LAUNCHES_2000, episode_length=4000, cross=(256, 320)),
    "beyond": dict(capacity=576, load=450.0, bit_rates=(10, 40), launches=LAUNCHES_2000, episode_length=4000, cross=(256, 320, 384, 448)),
    "reset": dict(capacity=448, load=385.0, bit_rates=(10, 40), launches=LAUNCHES_2100, episode_length=700, cross=()),
}


def config(c):
    return dict(modulations=jocn_modulations(), num_spectrum_resources=S, capacity=c["capacity"], load=c["load"],
                bit_rate_selection="discrete", bit_rates=c["bit_rates"], auto_reset=True, episode_length=c["episode_length"])


_oracle = {}


def oracle_run(name):
    """Step records [steps, B] and the oracles (final state) of one case: computed once, only read afterwards."""
    if name not in _oracle:
        c = CASES[name]
        steps = sum(c["launches"])
        holder = nat.ConfigHolder(golden_tables("nsfnet"), batch=B, **config(c))
        recs = np.zeros((steps, B), nat.STEP_DTYPE)
        envs = [OracleEnv(holder, replica=r) for r in range(B)]

        def run(r):         # one oracle per replica, no shared state: the C calls run side by side (ctypes drops the GIL)
            envs[r].seed(SEED); envs[r].reset()
            recs[:, r] = envs[r].run_policy(PID, steps)

        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            list(pool.map(run, range(B)))
        _oracle[name] = (holder, recs, envs)
    return _oracle[name]


def crossings(active, bound):
    """Per replica: times the running services went from <= bound to > bound and back (the network starts empty)."""
    above = np.concatenate([np.zeros((1, active.shape[1]), bool), active > bound])
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


def run_and_compare(name, wide, record, table, monkeypatch):
    c = CASES[name]
    if wide:
        monkeypatch.setenv("ONGYM_FORCE_WIDE", "1")       # read at ongym_create
    if table:
        monkeypatch.delenv("ONGYM_FAST_NO_LWTAB", raising=False)
    else:
        monkeypatch.setenv("ONGYM_FAST_NO_LWTAB", "1")    # read at ongym_create
    holder, want, oracles = oracle_run(name)
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **config(c))
    env.seed(SEED); env.reset()
    assert env.occupancy(PID)["lean_kernel"]
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
    return want


def check_crossings(name, want):
    """The counts of the table in the module docstring, printed, then the conditions that keep the case from passing vacuously."""
    c = CASES[name]
    active = want["active"].astype(np.int64)
    assert not (want["flags"] & nat.F_OVERFLOW).any()
    edges = np.cumsum(c["launches"])[:-1]
    both = {}
    for bound in BOUNDS:
        up, down = crossings(active, bound)
        both[bound] = int(((up > 0) & (down > 0)).sum())
    print(f"{name}: capacity {c['capacity']} load {c['load']} requests {active.shape[0]} most services {int(active.max())} "
          f"overflow {int((want['flags'] & nat.F_OVERFLOW).astype(bool).sum())} replicas crossing up and down "
          + " ".join(f"{b}: {both[b]}" for b in BOUNDS) + f" share of steps > 256 {(active > 256).mean():.2f}")
    assert int(active.max()) <= c["capacity"]
    for bound in c["cross"]:
        assert 4 * both[bound] >= B, (name, bound, both[bound])
        # the hand-over also happens inside launches, not only between them
        above = active > bound
        change = np.argwhere(above[1:] != above[:-1])[:, 0] + 1
        assert np.setdiff1d(change, edges).size > 0, (name, bound)


@pytest.mark.parametrize("record", [False, True], ids=["norecord", "record"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("name", ["headline", "seven", "table384", "beyond"])
def test_record_scans_above_256_services_vs_oracle(name, wide, record, monkeypatch):
    want = run_and_compare(name, wide, record, True, monkeypatch)
    check_crossings(name, want)
    most = int(want["active"].max())
    if name == "beyond":
        assert most > 448                       # the chunk loop takes over above the tail, and hands back
    else:
        assert 256 < most <= 448


@pytest.mark.parametrize("record", [False, True], ids=["norecord", "record"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_headline_mix_on_the_link_loop_instantiation_vs_oracle(wide, record, monkeypatch):
    want = run_and_compare("headline", wide, record, False, monkeypatch)
    check_crossings("headline", want)


@pytest.mark.parametrize("record", [False, True], ids=["norecord", "record"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_episode_reset_while_the_tail_is_in_use_vs_oracle(wide, record, monkeypatch):
    want = run_and_compare("reset", wide, record, True, monkeypatch)
    check_crossings("reset", want)
    term = want["terminated"].astype(bool)
    before = want["active"][term].astype(np.int64)
    print(f"reset: resets per replica {int(term.sum(0).min())}..{int(term.sum(0).max())}; services running just before a reset "
          f"{int(before.min())}..{int(before.max())}; most services {int(want['active'].max())}")
    assert (term.sum(0) == 3).all()
    assert (before > 256).all()                 # every reset clears a table whose tail chunks are in use
