"""Failure impact without a GPU: ongym_failure_impact is declared with its exact parameter list, exported and typed;
BatchedQRMSAEnv.failure_impact checks its arguments before it calls the library; and the restatement that
tests/test_gpu_failure_impact.py holds the device to (tests/failure_impact_child.py) is pinned to the CPU oracle: its search,
called with the current request's slot counts and every route eligible, is the oracle's own first-fit decision; its release
rule leaves the grid of the surviving records; and, for the seeds of the GPU cases, no evaluation lies inside the band where a
decision could differ, while the cases exercise what the GPU module claims."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from failure_impact_child import (BAND, CASES, conditions, drive, explicit_links, fail_link, gn_running, oracle_records, provision, replica_margin,
                                  restate_replica, search)
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from test_gpu_service_qot import insertion_order

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()


def test_header_declares_failure_impact():
    m = re.search(r"int ongym_failure_impact\s*\(([^)]*)\);", HEADER)
    assert m
    assert " ".join(m.group(1).split()) == "ongym_env *env, int32_t n_fail, const int32_t *links, double *link_out, int32_t *svc_out"
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4
    assert nat.FAILURE_IMPACT == ("status", "victims", "victim_capacity", "restored", "restored_capacity", "lost_no_spectrum",
                                  "lost_qot", "extra_hops", "extra_slot_hops", "lowest_margin")


def test_library_exports_and_native_declares_it():
    lib = nat.load_library()
    assert "ongym_failure_impact" in nat.EXPORTED_SYMBOLS
    f = lib.ongym_failure_impact
    assert f.restype is ctypes.c_int32
    assert f.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.ongym_failure_impact(None, 1, None, None, None) == -1


class _StubLib:
    """records ongym_failure_impact calls"""
    def __init__(self):
        self.calls = []

    def ongym_failure_impact(self, h, n, links, out, svc):
        self.calls.append((int(n), links is not None, svc is not None))
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
    E = c.n_links
    out = env.failure_impact()
    assert out.shape == (4, E, 10) and out.dtype == np.float64
    assert env.failure_impact(np.zeros(4, np.int32)).shape == (4, 1, 10)
    link, svc = env.failure_impact(np.zeros((4, E), np.int32), detail=True)
    assert link.shape == (4, E, 10) and svc.shape == (4, E, c.capacity) and svc.dtype == np.int32
    assert env.lib.calls == [(E, False, False), (1, True, False), (E, True, True)]
    for bad, kw, match in ((np.zeros((4, 0), np.int32), {}, "lie in"), (np.zeros((4, E + 1), np.int32), {}, "lie in"),
                           (np.zeros((4, 3), np.int64), {}, "int32"), (np.zeros((3, 3), np.int32), {}, "shape"),
                           (np.zeros((4, 3, 1), np.int32), {}, "shape"), ([[0]] * 4, {}, "int32"),
                           (None, {"out": out}, "io_device")):
        with pytest.raises(ValueError, match=match):
            env.failure_impact(bad, **kw)
    assert len(env.lib.calls) == 3


def test_a_format_window_is_refused_before_the_call():
    env = _env(False, modulations_to_consider=3)
    with pytest.raises(ValueError, match="modulations_to_consider"):
        env.failure_impact()
    assert env.lib.calls == []


def test_io_device_environment_checks_its_arguments_before_the_call():
    env = _env(True)
    E = env.holder.struct.n_links
    links, out = torch.zeros((4, 3), dtype=torch.int32), torch.empty((4, 3, 10), dtype=torch.float64)
    for a, kw, match in ((np.zeros((4, 3), np.int32), {"out": out}, "links must be"),     # not a tensor
                         (links, {"out": out}, "links must be"),                          # a host tensor: not on the device
                         (links.long(), {"out": out}, "links must be"),
                         (None, {}, "needs out")):
        with pytest.raises(ValueError, match=match):
            env.failure_impact(a, **kw)
    assert env.lib.calls == [] and E > 3


@pytest.mark.parametrize("topo,power,S,load", [("nsfnet", 0.0, 128, 120.0), ("cost239", 5.0, 96, 110.0)])
def test_the_search_is_the_oracles_first_fit(topo, power, S, load):
    """the restatement's search with the CURRENT REQUEST's slot counts and every route of its node pair eligible, on the
    oracle's own state (records in the order of the links' lists, its grid), is policy_first_fit() on every state of a run; at
    the high launch power QoT refusals occur"""
    from oracle_lib import OracleEnv
    tb = common.golden_tables(topo)
    kw = dict(modulations=common.jocn_modulations(), bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), load=load,
              num_spectrum_resources=S, capacity=256, episode_length=10 ** 6, margin=0.5, launch_power_dbm=power)
    holder = nat.ConfigHolder(tb, batch=1, **kw)
    c = holder.struct
    se, thr = np.asarray(holder.mod_se), np.asarray(holder.mod_thr)
    o = OracleEnv(holder)
    o.seed(5)
    o.reset()
    o.run_first_fit(120)
    states = refusals = rejects = 0
    for _ in range(150):
        want = o.policy_first_fit()[0]
        q = o.request()
        svcs = o.services()
        svcs = svcs[insertion_order(svcs)]
        running = [(int(s["path_id"]), int(s["slot"]), int(s["nslots"]), int(s["modulation"]), -1) for s in svcs]
        nslots = [o.number_slots(float(q["bit_rate"]), m) for m in range(c.n_mods)]
        routes = []
        for k in range(c.k_paths):
            p = int(tb.pair_paths[int(q["source"]), int(q["destination"]), k])
            if p < 0:
                break
            routes.append((k, p))
        log = []
        hit, _ = search(o, tb, thr, c.margin, nslots, routes, o.grid(),
                        lambda p, a, n: gn_running(o, tb, se, running, p, a, n)[0], log)
        got = o.reject_action if hit is None else o.encode(hit[0], hit[1], hit[2])
        assert got == want
        assert not np.any(np.array(log) < BAND)
        refusals += len(log) - (hit is not None)
        rejects += hit is None
        states += 1
        o.step(int(want))
    print(f"{topo}: {states} states, {refusals} evaluations refused on QoT, {rejects} rejects")
    assert states == 150
    assert refusals > 0 or power < 1.0


_RESTATED = {}


def restated(key):
    """a GPU case's configuration driven on CPU oracles with the GPU module's seed (computed once): per replica the restated
    rows for every link (sequential and independent), with the log of every evaluation's distance to its limit"""
    if key in _RESTATED:
        return _RESTATED[key]
    tb, kw, holder, ors = drive(key)
    E = tb.n_links
    reps = []
    for r, o in enumerate(ors):
        svcs = oracle_records(o)
        if len(svcs) and key == "ids":
            svcs = svcs.copy()                  # the oracle lists no ids: an id per record, namesakes by construction
            svcs["service_id"] = np.arange(len(svcs)) % max(1, len(svcs) - 3)
        log = []
        margin = replica_margin(kw, r)
        want, act, wide = restate_replica(o, tb, holder, margin, svcs, o.grid(), np.arange(E), key == "ids", True, log)
        _, indep, _ = restate_replica(o, tb, holder, margin, svcs, o.grid(), np.arange(E), key == "ids", False)
        want_l, _, _ = restate_replica(o, tb, holder, margin, svcs, o.grid(), explicit_links(E, len(ors))[r], key == "ids")
        cond = conditions(tb, holder, svcs, want, act, indep)
        cond["wide"], cond["wide_seen"] = wide
        reps.append(dict(o=o, svcs=svcs, want=want, log=np.array(log), want_l=want_l, cond=cond))
    _RESTATED[key] = key, tb, holder, reps
    return _RESTATED[key]


@pytest.fixture(params=CASES)
def case(request):
    return restated(request.param)


def test_release_rule_leaves_the_grid_of_the_survivors(case):
    key, tb, holder, reps = case
    checked = 0
    for rep in reps:
        grid = rep["o"].grid()
        for link in range(tb.n_links):
            _, victims, running, freed = fail_link(tb, rep["svcs"], grid, link)
            rebuilt = np.ones_like(grid)
            for p, s, n, _, _ in running:
                provision(rebuilt, tb, p, s, n)
            assert np.array_equal(freed != 0, rebuilt != 0), (key, link)
            checked += len(victims)
    assert checked > 0


def test_no_evaluation_lies_in_the_band_for_the_seeds_of_the_gpu_cases(case):
    key, _, _, reps = case
    logs = np.concatenate([rep["log"] for rep in reps])
    print(f"{key}: {len(logs)} evaluated (candidate, format) pairs, closest to its limit {logs.min() if len(logs) else np.nan:.2e}")
    assert len(logs) > 0
    assert int(np.sum(logs < BAND)) == 0


def test_rows_are_consistent_and_the_cases_are_not_empty(case):
    key, tb, holder, reps = case
    total = {}
    for rep in reps:
        w = rep["want"]
        assert np.all(w[:, 0] == 0) and np.array_equal(w[:, 1], w[:, 3] + w[:, 5] + w[:, 6])
        assert np.array_equal(np.isnan(w[:, 9]), w[:, 3] == 0)
        wl = rep["want_l"]
        assert wl[:, 0].tolist()[-2:] == [1, 1] and np.all(np.isnan(wl[-2:, 1:])) and np.all(wl[:-2, 0] == 0)
        assert np.array_equal(wl[-3], wl[0], equal_nan=True)             # the duplicate: an independent scenario, the same row
        for k, v in rep["cond"].items():
            total[k] = total.get(k, 0) + v
    print(key, total)
    assert total["restored"] > 0
    assert 4 * total["no_victim"] <= total["evaluated"]
    if key == "ring4":
        assert total["route2"] == 0
    if key == "nobeleu":
        assert total["wide"] > 0 and total["wide_seen"] > 0
    if key == "odd":
        assert total["ends_at_S"] > 0


def test_the_cases_together_exercise_every_condition():
    """what tests/test_gpu_failure_impact.py asserts on the values restated from the device's records, on the oracles' here"""
    total = {}
    for key in CASES:
        for rep in restated(key)[3]:
            for k, v in rep["cond"].items():
                total[k] = total.get(k, 0) + v
    print(total)
    for k in ("down", "route2", "lost_ns", "lost_qot", "sequential", "no_victim", "wide", "wide_seen", "ends_at_S"):
        assert total[k] > 0, k
