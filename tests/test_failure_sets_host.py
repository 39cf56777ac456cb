"""Failures of link sets without a GPU: ongym_failure_sets is declared with its exact parameter list, exported and typed;
BatchedQRMSAEnv.failure_sets checks its arguments before it calls the library; pack_link_sets, node_link_sets and link_pair_sets
equal a direct construction from link_nodes; the restatement that tests/test_gpu_failure_sets.py holds the device to
(restate_set, tests/failure_sets_child.py) equals restate_scenario of tests/failure_impact_child.py on every one-element set;
and for the seeds of the GPU cases (every node's links and 12 dual cuts per replica, on the CPU oracles) no evaluation lies
inside the band where a decision could differ, while the cases exercise what the GPU module claims."""
import ctypes
import os
import re
from itertools import combinations

import numpy as np
import pytest
import torch

import common
from failure_impact_child import BAND, CASES, drive, oracle_records, replica_margin, restate_scenario
from failure_sets_child import COVER, as_words, coverage, node_lists, pair_lists, restate_set, restate_sets, scenario_lists, words
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()


def test_header_declares_failure_sets():
    m = re.search(r"int ongym_failure_sets\s*\(([^)]*)\);", HEADER)
    assert m
    assert " ".join(m.group(1).split()) == ("ongym_env *env, int32_t n_sets, const uint64_t *sets, int32_t per_replica, "
                                            "double *set_out, int32_t *svc_out")
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4 == nat.ABI_VERSION
    assert nat.FAILURE_SETS == ("status", "victims", "victim_capacity", "restored", "restored_capacity", "lost_no_spectrum",
                                "lost_qot", "extra_hops", "extra_slot_hops", "lowest_margin", "lost_no_route", "failed_links")
    assert nat.FAILURE_SETS[:10] == nat.FAILURE_IMPACT


def test_library_exports_and_native_declares_it():
    lib = nat.load_library()
    assert "ongym_failure_sets" in nat.EXPORTED_SYMBOLS
    f = lib.ongym_failure_sets
    assert f.restype is ctypes.c_int32
    assert f.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.ongym_failure_sets(None, 1, None, 0, None, None) == -1


class _StubLib:
    """records ongym_failure_sets calls"""
    def __init__(self):
        self.calls = []

    def ongym_failure_sets(self, h, n, sets, per_replica, out, svc):
        self.calls.append((int(n), int(per_replica), svc is not None))
        return 0


def _env(io_device, B=4, **kw):
    env = object.__new__(BatchedQRMSAEnv)
    env.holder = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                                  capacity=128, io_device=io_device, **kw)
    env.batch_size, env.lib, env._h, env.stream_handle = B, _StubLib(), None, None
    return env


def test_host_environment_checks_its_arguments_before_the_call():
    env = _env(False)
    c = env.holder.struct
    out = env.failure_sets(np.ones((3, 2), np.uint64))
    assert out.shape == (4, 3, 12) and out.dtype == np.float64
    row, svc = env.failure_sets(np.ones((4, 5, 2), np.uint64), detail=True)
    assert row.shape == (4, 5, 12) and svc.shape == (4, 5, c.capacity) and svc.dtype == np.int32
    assert env.failure_sets([[0, 1], (2,), range(3), []]).shape == (4, 4, 12)
    assert env.failure_sets(env.node_link_sets()).shape == (4, c.n_nodes, 12)
    assert env.lib.calls == [(3, 0, False), (5, 1, True), (4, 0, False), (c.n_nodes, 0, False)]
    for bad, kw, match in ((np.ones((0, 2), np.uint64), {}, "lie in"), (np.ones((65536, 2), np.uint64), {}, "lie in"),
                           (np.ones((3, 2), np.int64), {}, "uint64"), (np.ones((3, 3), np.uint64), {}, "shape"),
                           (np.ones((3, 5, 2), np.uint64), {}, "shape"), (np.ones(2, np.uint64), {}, "shape"),
                           ([[0, c.n_links]], {}, "outside"), ([[-1]], {}, "outside"), (None, {}, "uint64"),
                           (np.ones((3, 2), np.uint64), {"out": out}, "io_device")):
        with pytest.raises(ValueError, match=match):
            env.failure_sets(bad, **kw)
    assert len(env.lib.calls) == 4


def test_a_format_window_is_refused_before_the_call():
    env = _env(False, modulations_to_consider=3)
    with pytest.raises(ValueError, match="modulations_to_consider"):
        env.failure_sets(np.ones((3, 2), np.uint64))
    assert env.lib.calls == []


def test_io_device_environment_checks_its_arguments_before_the_call():
    env = _env(True)
    sets, out = torch.ones((3, 2), dtype=torch.int64), torch.empty((4, 3, 12), dtype=torch.float64)
    for a, kw, match in ((np.ones((3, 2), np.uint64), {"out": out}, "sets must be"),      # not a tensor
                         (sets, {"out": out}, "sets must be"),                           # a host tensor: not on the device
                         (sets.int(), {"out": out}, "sets must be"),
                         ([[0, 1]], {"out": out}, "sets must be")):
        with pytest.raises(ValueError, match=match):
            env.failure_sets(a, **kw)
    assert env.lib.calls == []


@pytest.mark.parametrize("topo", ["ring4", "nsfnet", "nobel-eu"])
def test_the_generators_equal_a_direct_construction_from_link_nodes(topo):
    tb = common.golden_tables(topo)
    env = object.__new__(BatchedQRMSAEnv)
    env.holder = nat.ConfigHolder(tb, modulations=common.jocn_modulations(), batch=1, load=100, capacity=64)
    E, N = tb.n_links, tb.n_nodes
    nodes = env.node_link_sets()
    assert nodes.dtype == np.uint64 and nodes.shape == (N, 2)
    for v in range(N):
        bits = sum(1 << e for e in range(E) if v in tb.link_nodes[e].tolist())
        assert [int(nodes[v, 0]), int(nodes[v, 1])] == [bits & (2 ** 64 - 1), bits >> 64] == words(node_lists(tb)[v])
    assert sum(bin(int(x)).count("1") for x in nodes.reshape(-1)) == 2 * E          # every link ends at two nodes
    pairs = env.link_pair_sets()
    assert pairs.dtype == np.uint64 and pairs.shape == (E * (E - 1) // 2, 2)
    for i, (a, b) in enumerate(combinations(range(E), 2)):
        bits = (1 << a) | (1 << b)
        assert [int(pairs[i, 0]), int(pairs[i, 1])] == [bits & (2 ** 64 - 1), bits >> 64]
    packed = BatchedQRMSAEnv.pack_link_sets([[0, E - 1, 0], [], np.array([1], np.int32), range(E)], E)
    assert np.array_equal(packed, as_words([[0, E - 1], [], [1], list(range(E))]))
    big = BatchedQRMSAEnv.pack_link_sets([[63, 64, 127]], 128)
    assert big.tolist() == [[1 << 63, 1 | (1 << 63)]]
    assert pairs.tolist() == BatchedQRMSAEnv.pack_link_sets(combinations(range(E), 2), E).tolist()


_RESTATED = {}


def restated(key):
    """a GPU case's configuration driven on CPU oracles with the GPU module's seed (computed once): per replica the restated
    rows of every node's link set and the replica's dual cuts, with the log of every evaluation's distance to its limit"""
    if key in _RESTATED:
        return _RESTATED[key]
    tb, kw, holder, ors = drive(key)
    reps = []
    for r, o in enumerate(ors):
        svcs = oracle_records(o)
        if len(svcs) and key == "ids":
            svcs = svcs.copy()                  # the oracle lists no ids: an id per record, namesakes by construction
            svcs["service_id"] = np.arange(len(svcs)) % max(1, len(svcs) - 3)
        log, cover = [], dict.fromkeys(COVER, 0)
        ws = as_words(node_lists(tb) + pair_lists(tb, r))
        want, act = restate_sets(o, tb, holder, replica_margin(kw, r), svcs, o.grid(), ws, key == "ids", log, cover)
        reps.append(dict(o=o, svcs=svcs, want=want, act=act, log=np.array(log), cond=coverage(want, cover),
                         margin=replica_margin(kw, r)))
    _RESTATED[key] = key, tb, holder, reps
    return _RESTATED[key]


@pytest.fixture(params=CASES)
def case(request):
    return restated(request.param)


def test_a_one_element_set_is_the_single_link_scenario(case):
    """restate_set on {e} equals restate_scenario of link e: row columns 0-9 and the record actions, for every link of every
    replica; column 11 is 1 and column 10 the victims that lost every route"""
    key, tb, holder, reps = case
    victims = 0
    for rep in reps:
        for e in range(tb.n_links):
            args = (rep["o"], tb, holder, rep["margin"], rep["svcs"], rep["o"].grid())
            row, act = restate_set(*args, as_words([[e]])[0], key == "ids")
            want, want_act, _ = restate_scenario(*args, e, key == "ids")
            assert np.array_equal(row[:10], want, equal_nan=True), (key, e)
            assert np.array_equal(act, want_act), (key, e)
            assert row[11] == 1 and 0 <= row[10] <= row[5]
            victims += int(row[1])
    assert victims > 0


def test_skipped_sets_and_the_scenario_list(case):
    key, tb, holder, reps = case
    E, N = tb.n_links, tb.n_nodes
    rep = reps[0]
    args = (rep["o"], tb, holder, rep["margin"], rep["svcs"], rep["o"].grid())
    for w in (as_words([[]])[0], as_words([[E]])[0], as_words([[0, E + 3]])[0], np.array([0, 1 << 63], np.uint64)):
        row, act = restate_set(*args, w)
        assert row[0] == 1 and np.all(np.isnan(row[1:])) and np.all(act == -1)
    lists = scenario_lists(tb, 1)
    npairs = min(E * (E - 1) // 2, 12)
    assert len(lists) == N + npairs + E + 3
    assert lists[:N] == node_lists(tb) and lists[N + npairs:N + npairs + E] == [[e] for e in range(E)]
    assert lists[-3:] == [node_lists(tb)[0], [], [E]]
    assert all(len(p) == 2 and p[0] < p[1] < E for p in lists[N:N + npairs]) and len({tuple(p) for p in lists[N:N + npairs]}) == npairs


def test_no_evaluation_lies_in_the_band_for_the_seeds_of_the_gpu_cases(case):
    key, _, _, reps = case
    logs = np.concatenate([rep["log"] for rep in reps])
    print(f"{key}: {len(logs)} evaluated (candidate, format) pairs, closest to its limit {logs.min() if len(logs) else np.nan:.2e}")
    assert len(logs) > 0
    assert int(np.sum(logs < BAND)) == 0


def total(reps):
    out = {}
    for rep in reps:
        for k, v in rep["cond"].items():
            out[k] = out.get(k, 0) + v
    return out


def test_rows_are_consistent_and_the_cases_are_not_empty(case):
    key, tb, holder, reps = case
    for rep in reps:
        w = rep["want"]
        assert np.all(w[:, 0] == 0) and np.array_equal(w[:, 1], w[:, 3] + w[:, 5] + w[:, 6])
        assert np.all(w[:, 10] <= w[:, 5]) and np.array_equal(np.isnan(w[:, 9]), w[:, 3] == 0)
        assert np.array_equal(w[:, 11], [len(set(l)) for l in node_lists(tb)] + [2] * (len(w) - tb.n_nodes))
    t = total(reps)
    print(key, t)
    assert 4 * t["no_victim"] <= t["evaluated"]                 # at most a quarter of the scenarios without a victim
    assert t["restored"] > 0 and t["no_route"] > 0


def test_the_cases_together_exercise_every_condition():
    """what tests/test_gpu_failure_sets.py asserts on the values restated from the device's records, on the oracles' here: a
    victim lost on QoT, one lost for spectrum although a route is left, victims that cross two or more failed links, and
    victims restored on a later route because their first route clear of their own failed links crosses another failed
    link - what single-link answers cannot give"""
    t = {}
    for key in CASES:
        for k, v in total(restated(key)[3]).items():
            t[k] = t.get(k, 0) + v
    print(t)
    assert t["lost_qot"] > 0 and t["lost_ns"] - t["no_route"] > 0 and t["multi"] > 0 and t["skip_restored"] > 0
