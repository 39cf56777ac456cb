"""The parts of a request that DESIGN.md section 5, "Scalar issue slots of a request", rewrites in the lean first-fit kernel
(csrc/ongym_fast.hpp), each against the CPU oracle, exactly: final grids, services (sorted), statistics, and step records where
they are written.

  * The interferer list build (build_cache, the straight form): one ballot per chunk of 64 records, list positions on top of a
    running count, one store per chunk.  The count and the stores are what the section moves between the pipes, so the case
    holds every chunk edge: a request evaluated with 63, 64, 65, 128, 129, 256, 257, 320 and 321 running services.  The traffic
    is case "seven" of tests/test_gpu_fast_scan_tail.py (first fit, NSFNET, S = 320, capacity 448, 64 replicas); the edges are
    asserted from the oracle's step records within the first 1500 requests (`active` before a request that was accepted: an
    accepted request was evaluated at least once, and the list of that evaluation was built over that many records).
    A table of 192 records always takes the loop form of the build, which the section leaves alone.
  * The departures of a four-chunk trip of the release scan (chunks top .. top - 3 read together, then `depart` per chunk that
    holds a departure).  Fixed arrival and holding times through set_requests: 256 requests of 10 Gb/s one second apart fill
    records 0..255, and the request after them arrives when the chosen ones are due.  One replica per combination: each of the
    four chunks alone, all four, two in one chunk, the last record (the hole IS the last record), the last record with another
    chunk.  A host model of the record table (append on accept, the last record into the hole, highest index first) turns the
    oracle's `accepted` into the chunk of every departure; the model's `active` must be the oracle's at every step.
  * Instantiations that keep the parent's code behind `if constexpr`: two mask words (nobel-eu, S = 768), and step records.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import clock_edges as ce
import test_gpu_fast_four_chunk as four
import test_gpu_fast_scan_tail as tail
from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from oracle_lib import OracleEnv
from test_gpu_clock_edges import check_final
from test_gpu_parity import assert_records_equal

pytestmark = pytest.mark.gpu

FF = nat.POLICY_FIRST_FIT
EDGES = (63, 64, 65, 128, 129, 256, 257, 320, 321)
EDGE_STEPS = 1500


# ---- the list build ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_list_build_on_every_chunk_edge_vs_oracle(wide, monkeypatch):
    want = tail.run_and_compare("seven", wide, False, True, monkeypatch)
    active, accepted = want["active"].astype(np.int64)[:EDGE_STEPS], want["accepted"][:EDGE_STEPS].astype(bool)
    before = np.concatenate([np.zeros((1, active.shape[1]), np.int64), active[:-1]])        # the network starts empty
    on_edge = {e: int(((before == e) & accepted).sum()) for e in EDGES}
    print("accepted requests evaluated with N running services, N: count " + " ".join(f"{e}: {n}" for e, n in on_edge.items()))
    assert all(n > 0 for n in on_edge.values()), on_edge
    assert not (want["flags"] & nat.F_OVERFLOW).any()


def test_table_of_192_records_keeps_the_loop_form_vs_oracle(monkeypatch):
    want = four.run_and_compare("small", four.SMALL, four.SMALL_LAUNCHES, FF, False, False, monkeypatch)
    most = int(want["active"].max())
    assert 2 * 64 < most <= four.SMALL["capacity"] < four.FOUR


# ---- departures of a four-chunk trip ---------------------------------------------------------------------------------------------
KEY = "nsfnet320_c448"      # first fit, NSFNET, S = 320, capacity 448: the benchmark's table
FILL = 256                  # records 0..255: top = 3, one trip over chunks 3, 2, 1, 0
DUE_AT = 1000.0
TAIL_REQUESTS = 40
# name: (records that are due when request FILL + 1 is drawn, the chunks below `top` that must hold a departure)
COMBOS = {
    "top": ((200,), {0}),
    "top-1": ((130,), {1}),
    "top-2": ((70,), {2}),
    "top-3": ((5,), {3}),
    "all_four": ((250, 140, 100, 10), {0, 1, 2, 3}),
    "two_in_one_chunk": ((20, 40), {3}),
    "two_in_top": ((210, 230), {0}),
    "hole_is_last": ((255,), {0}),
    "last_and_lowest": ((255, 3), {0, 3}),
}


def combo_trace(name, r):
    rng = np.random.default_rng(2700 + r)
    at = np.arange(1, FILL + 1, dtype=np.float64)
    ht = np.full(FILL, 1e6)
    due = np.array(COMBOS[name][0])
    ht[due] = DUE_AT - at[due]
    at = np.concatenate([at, [DUE_AT, DUE_AT + 1.0], DUE_AT + 1.0 + np.cumsum(rng.exponential(36.0, TAIL_REQUESTS))])
    ht = np.concatenate([ht, [1e6, 1e6], rng.exponential(10800.0, TAIL_REQUESTS)])
    return ce._requests(KEY, rng, at, ht, first_10g=FILL)


def table_model(at, ht, accepted):
    """The record table of k_fast on a trace: a service takes the entry behind the last one; the services due at the draw of the
    next request leave highest entry first, and the last record fills the hole.  Returns `active` after every step and, per
    step, the (entry, number of records) of every departure as the scan's ballots saw them (before any move of that step)."""
    at, ht = np.asarray(at, np.float32), np.asarray(ht, np.float32)
    rel = at[:-1] + ht
    table, active, left = [], [], []
    for t in range(len(ht)):
        if accepted[t]:
            table.append(t)
        due = sorted((i for i, q in enumerate(table) if rel[q] <= at[t + 1]), reverse=True)
        left.append([(i, len(table)) for i in due])
        for i in due:
            table[i] = table[-1]
            table.pop()
        active.append(len(table))
    return np.array(active), left


_combo = {}


def combo_run():
    if not _combo:
        names = list(COMBOS)
        trace = np.ascontiguousarray(np.stack([combo_trace(n, r) for r, n in enumerate(names)]))
        holder = ce.holder_of(KEY, batch=len(names))
        steps = trace.shape[1] - 1          # the last request stays pending

        def one(r):
            o = OracleEnv(holder, replica=r)
            o.set_trace(trace[r])
            o.reset()
            return o, o.run_policy(FF, steps)

        with ThreadPoolExecutor(max_workers=min(len(names), os.cpu_count() or 1)) as pool:
            res = list(pool.map(one, range(len(names))))
        _combo.update(names=names, trace=trace, holder=holder, steps=steps, oracles=[x[0] for x in res],
                      recs=np.stack([x[1] for x in res], axis=1))
    return _combo


@pytest.mark.parametrize("record", [False, True], ids=["norecord", "record"])
def test_departures_in_every_combination_of_a_four_chunk_trip_vs_oracle(record):
    run = combo_run()
    for r, name in enumerate(run["names"]):
        tr, recs = run["trace"][r], run["recs"][:, r]
        active, left = table_model(tr["arrival_time"], tr["holding_time"][:-1], recs["accepted"])
        assert np.array_equal(active, recs["active"]), name             # the model is the oracle's
        assert recs["accepted"][:FILL].all(), name                      # so request i holds record i when the trip runs
        trip = left[FILL - 1]                                           # the departures at the draw of request FILL + 1
        entries, chunks = COMBOS[name]
        assert sorted(i for i, _ in trip) == sorted(entries) and all(n == FILL for _, n in trip), (name, trip)
        top = (FILL - 1) // 64
        assert top == 3 and {top - i // 64 for i, _ in trip} == chunks, (name, trip)
        if "last" in name:
            assert (FILL - 1, FILL) in trip
        print(f"{name}: departures (entry, records) {trip}; chunks below top {sorted(chunks)}; active after the trip {active[FILL - 1]}")
    env = BatchedQRMSAEnv(tables=ce.tables_of(KEY), batch_size=len(run["names"]), **ce.config_kw(KEY))
    env.set_requests(run["trace"])
    env.reset()
    assert env.occupancy(FF)["lean_kernel"]
    got = [env.step_policy(n, record=record, policy=FF) for n in (FILL - 2, 3, run["steps"] - FILL - 1)]   # the trip inside a launch
    if record:
        got = np.concatenate(got)
        for r, name in enumerate(run["names"]):
            assert_records_equal(got[:, r], run["recs"][:, r], name)
    check_final(env, run["oracles"], f"four-chunk trip, record {record}")


# ---- the instantiations that keep the parent's code --------------------------------------------------------------------------------
M64 = dict(B=8, steps=(1, 250, 149), kw=dict(modulations=jocn_modulations(), num_spectrum_resources=768, capacity=704, load=600.0,
                                              bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), auto_reset=True,
                                              episode_length=4000))


def test_two_mask_words_nobel_eu_768_vs_oracle():
    tables, B, steps = golden_tables("nobel-eu"), M64["B"], sum(M64["steps"])
    holder = nat.ConfigHolder(tables, batch=B, **M64["kw"])
    oracles = [OracleEnv(holder, replica=r) for r in range(B)]

    def one(r):
        oracles[r].seed(tail.SEED); oracles[r].reset()
        return oracles[r].run_policy(FF, steps)

    with ThreadPoolExecutor(max_workers=min(B, os.cpu_count() or 1)) as pool:
        want = np.stack(list(pool.map(one, range(B))), axis=1)
    env = BatchedQRMSAEnv(tables=tables, batch_size=B, **M64["kw"])
    env.seed(tail.SEED); env.reset()
    occ = env.occupancy(FF)
    assert occ["lean_kernel"] and tables.n_links > 32           # two mask words
    for n in M64["steps"]:
        env.step_policy(n, record=False, policy=FF)
    st = env.stats()
    print(f"nobel-eu S = 768: {tables.n_links} links, most services {int(want['active'].max())}, accepted {want['accepted'].mean():.3f}")
    assert int(want["active"].max()) > 64
    for r, o in enumerate(oracles):
        np.testing.assert_array_equal(env.grid(r), o.grid(), err_msg=f"replica {r}: grid")
        a = np.sort(env.services(r), order=["release_time", "path_id", "slot"])
        b = np.sort(o.services(), order=["release_time", "path_id", "slot"])
        assert a.tobytes() == b.tobytes(), f"replica {r}: services"
        so = o.stats()
        for f in tail.STATS:
            assert st[r][f] == so[f], (r, f, st[r][f], so[f])


def test_record_kernel_on_every_chunk_edge_vs_oracle(monkeypatch):
    tail.run_and_compare("seven", False, True, True, monkeypatch)
