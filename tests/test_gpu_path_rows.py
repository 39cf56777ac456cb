"""First fit without step records and with one mask word (csrc/ongym_fast.hpp, path_and) reads the free-slot rows of all links of a
route of up to four hops in one LDS trip: lane 16 r + w reads word w of the row of the route's r-th link, and two lane swaps with
an AND each combine the four rows.  The links come from dword 0 of the route's record in a first-fit copy of the record table
(csrc/ongym_tables.hpp, path_rows_word): hop count | four link fields, unused fields = the first link; routes of more than four
hops, and every route when S >= 512 (the row with the virtual slot S does not fit 16 lanes), carry the long mark and take the
link loop, as every kernel with records, two mask words or another policy does.

Every run is first fit on 64 replicas, seed 5, in launches of uneven length, against the CPU oracle: final grids, services
(sorted) and statistics, and the step records where they are written.  The oracle of a case runs once, one step at a time, so
that the node pair of every request is known and with it the route (path id) behind the route index of a step record.

The inputs were chosen on the CPU oracle (all 64 replicas, 1500 requests each, no F_OVERFLOW anywhere):

    case      topology  S    capacity  load   bit rates       accepted  most services
    hops      nsfnet    160    448      400   10,40,100,400    82.9 %      348
    full_480  nsfnet    480    768     4000   400              42.9 %      542
    full_511  nsfnet    511    768     4000   400              44.6 %      561
    long_512  nsfnet    512    768     4000   400              44.5 %      560
    ring      ring4      80    256       60   100,400          56.3 %       49
    two_words nobel-eu  160    512      600   10,40,100,400    73.5 %      423

    hops: accepted requests by hop count of the serving route, 1 / 2 / 3 / 4 / 5 / 6 / 7: 22 430 / 28 901 / 18 981 / 8 084 /
    1 139 / 69 / 3 (the same run as test_gpu_first_route's later_routes: by route index 67 321 / 7 376 / 3 171 / 1 134 / 605)
    full_480, full_511, long_512: by hop count 1 .. 6: 19 201 / 13 157 / 5 789 / 2 510 / 477 / 11 (S = 480; the others within 6 %)
    ring: by hop count 1 / 2 / 3: 37 376 / 12 832 / 3 800

Word 15.  With S = 480 a row has 15 words of slots and word 15 holds nothing but the virtual free slot S (bit 0), with S = 511 it
holds slots 480 .. 510 and S at bit 31.  An allocation "lies in word 15" here when the slot behind its last one - its guard slot,
or S itself when it ends at S - is in word 15: the run of n + 1 free bits that admitted it then reached into that word.  Accepted
allocations of that kind: 187 (S = 480, all of them end at S), 1 908 (S = 511), 1 793 (S = 512, where word 15 is an ordinary word).
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
LAUNCHES = (1, 63, 250, 7, 500, 129, 550)
STEPS = sum(LAUNCHES)

CASES = {
    "hops": dict(topo="nsfnet", S=160, capacity=448, load=400.0, bit_rates=(10, 40, 100, 400)),
    "full_480": dict(topo="nsfnet", S=480, capacity=768, load=4000.0, bit_rates=(400,)),
    "full_511": dict(topo="nsfnet", S=511, capacity=768, load=4000.0, bit_rates=(400,)),
    "long_512": dict(topo="nsfnet", S=512, capacity=768, load=4000.0, bit_rates=(400,)),
    "ring": dict(topo="ring4", S=80, capacity=256, load=60.0, bit_rates=(100, 400)),
    "two_words": dict(topo="nobel-eu", S=160, capacity=512, load=600.0, bit_rates=(10, 40, 100, 400)),
}


def config(c):
    return dict(modulations=jocn_modulations(), num_spectrum_resources=c["S"], capacity=c["capacity"], load=c["load"],
                bit_rate_selection="discrete", bit_rates=c["bit_rates"], auto_reset=True, episode_length=4000)


_oracle = {}


def oracle_run(name):
    """Step records [steps, B], the path ids of the routes of every request's node pair [steps, B, K] and the oracles (final
    state) of one case: computed once, only read afterwards."""
    if name not in _oracle:
        c = CASES[name]
        tables = golden_tables(c["topo"])
        holder = nat.ConfigHolder(tables, batch=B, **config(c))
        recs = np.zeros((STEPS, B), nat.STEP_DTYPE)
        pair = np.zeros((STEPS, B, 2), np.int64)
        envs = [OracleEnv(holder, replica=r) for r in range(B)]

        def run(r):         # one oracle per replica, no shared state
            o = envs[r]
            o.seed(SEED); o.reset()
            for t in range(STEPS):
                q = o.request()
                pair[t, r] = (q["source"], q["destination"])
                recs[t, r] = o.run_policy(PID, 1)[0]

        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            list(pool.map(run, range(B)))
        paths = np.asarray(tables.pair_paths)[pair[..., 0], pair[..., 1]]       # [steps, B, K]
        _oracle[name] = (holder, recs, paths, envs)
    return _oracle[name]


def serving_hops(name):
    """Hop count of the route that served each accepted request [n_accepted]."""
    _, want, paths, _ = oracle_run(name)
    acc = want["accepted"].astype(bool)
    pid = np.take_along_axis(paths, want["route"].astype(np.int64)[..., None].clip(0), axis=2)[..., 0][acc]
    assert (pid >= 0).all()
    return np.asarray(golden_tables(CASES[name]["topo"]).path_hops)[pid]


def assert_records_equal(got, want, ctx):
    for f in EXACT:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(got[f] != want[f])[0]
            raise AssertionError(f"{ctx}: field {f} differs first at {tuple(bad)}: {got[f][tuple(bad)]} != {want[f][tuple(bad)]}")
    for f in ("osnr", "ase", "nli"):
        np.testing.assert_allclose(got[f], want[f], rtol=GSNR_RTOL, err_msg=f"{ctx}: {f}")


def run_and_compare(name, monkeypatch, wide=False, record=False, table=True):
    c = CASES[name]
    if wide:
        monkeypatch.setenv("ONGYM_FORCE_WIDE", "1")       # read at ongym_create
    if table:
        monkeypatch.delenv("ONGYM_FAST_NO_LWTAB", raising=False)
    else:
        monkeypatch.setenv("ONGYM_FAST_NO_LWTAB", "1")    # read at ongym_create
    holder, want, _, oracles = oracle_run(name)
    env = BatchedQRMSAEnv(tables=golden_tables(c["topo"]), batch_size=B, **config(c))
    env.seed(SEED); env.reset()
    assert env.occupancy(PID)["lean_kernel"]
    if c["topo"] == "nsfnet":
        assert (env.link_weight_entry(0, 0) is not None) == table
    got = [env.step_policy(n, record=record, policy=PID) for n in LAUNCHES]
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
        assert st[r]["total_gn_evals"] <= so["total_gn_evals"] <= st[r]["total_gn_shortcuts"] + st[r]["total_gn_evals"]
    assert not (want["flags"] & nat.F_OVERFLOW).any()
    return env, want


# ---- table contents ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("topo", ["nsfnet", "cost239", "ring4"])
def test_route_rows_table_spells_out_every_route(topo):
    tables = golden_tables(topo)
    hops, links = np.asarray(tables.path_hops), np.asarray(tables.path_links)
    kw = config(dict(S=160, capacity=256, load=100.0, bit_rates=(100, 400)))
    env = BatchedQRMSAEnv(tables=tables, batch_size=B, **kw)
    env.seed(SEED); env.reset()
    assert env.occupancy(PID)["lean_kernel"]
    n_long = 0
    for p in range(len(hops)):
        got = env.path_rows(p)
        h = int(hops[p])
        assert got["hops"] == h, (topo, p, got)
        assert got["long"] == (h > 4), (topo, p, got)
        if h > 4:
            n_long += 1
            assert got["word"] == (h | 1 << 31), (topo, p, got)
        else:
            want = [int(links[p, r]) if r < h else int(links[p, 0]) for r in range(4)]
            assert got["links"] == want, (topo, p, got, want)
            assert got["word"] == h | sum(l << (8 + 6 * r) for r, l in enumerate(want)), (topo, p, got)
    print(f"{topo}: {len(hops)} routes, {n_long} long, longest {int(hops.max())} hops")
    assert n_long == {"nsfnet": 181, "cost239": 1, "ring4": 0}[topo]      # (the longest routes: 9, 5 and 3 hops)


@pytest.mark.parametrize("S", [511, 512, 513, 640])
def test_every_route_is_long_from_512_slots(S):
    tables = golden_tables("nsfnet")
    hops = np.asarray(tables.path_hops)
    env = BatchedQRMSAEnv(tables=tables, batch_size=B, **config(dict(S=S, capacity=256, load=100.0, bit_rates=(100, 400))))
    env.seed(SEED); env.reset()
    assert env.occupancy(PID)["lean_kernel"]
    rows = [env.path_rows(p) for p in range(len(hops))]
    assert [r["hops"] for r in rows] == hops.tolist()
    if S >= 512:
        assert all(r["long"] and r["word"] == (int(h) | 1 << 31) for r, h in zip(rows, hops))
    else:
        assert [r["long"] for r in rows] == (hops > 4).tolist()


# ---- every hop count ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["narrow", "wide", "no_lwtab"])
def test_routes_of_every_hop_count_vs_oracle(variant, monkeypatch):
    env, want = run_and_compare("hops", monkeypatch, wide=variant == "wide", table=variant != "no_lwtab")
    h = serving_hops("hops")
    by_hops = [int((h == n).sum()) for n in (1, 2, 3, 4)] + [int((h >= 5).sum())]
    print(f"hops: accepted {want['accepted'].mean():.3f} by hop count 1 / 2 / 3 / 4 / >= 5: " + " / ".join(map(str, by_hops)))
    assert min(by_hops) >= 20, by_hops
    # the table the kernel read gives the same hop counts and sends exactly the >= 5 hops to the loop
    paths = np.unique(oracle_run("hops")[2])
    hops = np.asarray(golden_tables("nsfnet").path_hops)
    for p in paths[paths >= 0]:
        r = env.path_rows(int(p))
        assert r["hops"] == hops[p] and r["long"] == (hops[p] > 4)


# ---- a full row, and one word too many ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["full_480", "full_511", "long_512"])
def test_sixteen_words_and_the_virtual_slot_vs_oracle(name, monkeypatch):
    env, want = run_and_compare(name, monkeypatch)
    S = CASES[name]["S"]
    acc = want["accepted"].astype(bool)
    last = want["slot"].astype(np.int64) + want["nslots"]              # the slot behind the allocation: its guard slot, or S
    in15 = int((acc & (last >> 5 == 15)).sum())
    print(f"{name}: accepted {acc.mean():.3f} most services {int(want['active'].max())} allocations reaching word 15: {in15}")
    assert 10 * int((~acc).sum()) >= acc.size, name                    # the network fills
    assert env.path_rows(0)["long"] == (S >= 512)
    if S < 512:
        assert (S >> 5, S & 31) == ((15, 0) if S == 480 else (15, 31))  # where the virtual slot S falls
        assert in15 > 0


# ---- short routes only -----------------------------------------------------------------------------------------------

def test_one_hop_routes_read_one_row_four_times_vs_oracle(monkeypatch):
    env, want = run_and_compare("ring", monkeypatch)
    h = serving_hops("ring")
    print(f"ring: accepted {want['accepted'].mean():.3f} by hop count 1 / 2 / 3: " + " / ".join(str(int((h == n).sum())) for n in (1, 2, 3)))
    assert (h == 1).sum() >= 20 and h.max() <= 3
    assert 10 * int((~want["accepted"].astype(bool)).sum()) >= want.size


# ---- kernels that keep the loop ---------------------------------------------------------------------------------------

def test_record_kernel_keeps_the_loop_vs_oracle(monkeypatch):
    run_and_compare("hops", monkeypatch, record=True)


def test_two_mask_words_keep_the_loop_vs_oracle(monkeypatch):
    env, _ = run_and_compare("two_words", monkeypatch)
    assert all(env.path_rows(p)["long"] for p in range(0, 40))           # 41 links: no route is spelled out
