"""Cutting and repairing links on live replicas without a GPU: the three calls are declared with their exact parameter lists,
exported and typed; BatchedQRMSAEnv checks its arguments before it calls the library; and on the CPU oracles of the GPU cases
(tests/link_cut_child.py, same configurations, seeds and sets)
  (a) every oracle's grid is the union of its records' provisioned ranges, the premise of the derived "failed" rule (a failed
      link is a row without a free slot that no record crosses), and stays so through the restated cut;
  (b) the sets exercise what tests/test_gpu_link_cut.py claims: a restored victim, a victim lost on QoT, one lost for spectrum
      with a route left, one with no route left, one that crosses two failed links; at most a quarter of the non-empty sets
      have no victim;
  (c) no evaluation of the restated cut or of the restated first decision after it lies inside the band where a decision
      could differ."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from failure_impact_child import BAND, CASES, drive, oracle_records, replica_margin
from failure_sets_child import as_words
from link_cut_child import (COVER, FIELDS, coverage, crossing, expected_cut, first_fit_restated, grid_of_records, links_of,
                            replica_links, svc_rows)
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()
VP, I32 = ctypes.c_void_p, ctypes.c_int32


def params(name):
    m = re.search(r"int %s\s*\(([^)]*)\);" % name, HEADER)
    assert m, name
    return " ".join(m.group(1).split())


def test_header_declares_the_three_calls():
    assert params("ongym_cut_links") == ("ongym_env *env, const uint64_t *sets, int32_t per_replica, int32_t flags, "
                                         "double *cut_out, int32_t *svc_out, int32_t *index_out")
    assert params("ongym_repair_links") == "ongym_env *env, const uint64_t *sets, int32_t per_replica, int32_t *repaired_out"
    assert params("ongym_failed_links") == "ongym_env *env, uint64_t *failed_out"
    assert re.search(r"enum\s*\{\s*ONGYM_CUT_NO_RESTORE\s*=\s*1\s*\}", HEADER) and nat.CUT_NO_RESTORE == 1
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4 == nat.ABI_VERSION
    assert nat.CUT_LINKS == nat.FAILURE_SETS + ("dropped",) and len(nat.CUT_LINKS) == 13


def test_library_exports_and_native_declares_them():
    lib = nat.load_library()
    for name, args in (("ongym_cut_links", [VP, VP, I32, I32, VP, VP, VP]), ("ongym_repair_links", [VP, VP, I32, VP]),
                       ("ongym_failed_links", [VP, VP])):
        assert name in nat.EXPORTED_SYMBOLS
        f = getattr(lib, name)
        assert f.restype is I32 and f.argtypes == args, name
    assert lib.ongym_cut_links(None, None, 0, 0, None, None, None) == -1
    assert lib.ongym_repair_links(None, None, 0, None) == -1
    assert lib.ongym_failed_links(None, None) == -1


class _StubLib:
    """records the calls"""
    def __init__(self):
        self.calls = []

    def ongym_cut_links(self, h, sets, per_replica, flags, out, svc, index):
        self.calls.append(("cut", int(per_replica), int(flags), svc is not None, index is not None))
        return 0

    def ongym_repair_links(self, h, sets, per_replica, out):
        self.calls.append(("repair", int(per_replica)))
        return 0

    def ongym_failed_links(self, h, out):
        self.calls.append(("failed",))
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
    out = env.cut_links(np.ones(2, np.uint64))
    assert out.shape == (4, 13) and out.dtype == np.float64
    row, (svc, index) = env.cut_links(np.ones((4, 2), np.uint64), restore=False, detail=True)
    assert row.shape == (4, 13) and svc.shape == index.shape == (4, c.capacity) and svc.dtype == index.dtype == np.int32
    assert env.cut_links([[0, 1], (2,), range(3), []]).shape == (4, 13)
    n = env.repair_links(np.ones((4, 2), np.uint64))
    assert n.shape == (4,) and n.dtype == np.int32
    f = env.failed_links()
    assert f.shape == (4, 2) and f.dtype == np.uint64
    assert env.lib.calls == [("cut", 0, 0, False, False), ("cut", 1, nat.CUT_NO_RESTORE, True, True), ("cut", 1, 0, False, False),
                             ("repair", 1), ("failed",)]
    for bad, kw, match in ((np.ones((3, 2), np.uint64), {}, "shape"), (np.ones((4, 3), np.uint64), {}, "shape"),
                           (np.ones((4, 2), np.int64), {}, "uint64"), ([[0], [1]], {}, "one link-index iterable per replica"),
                           ([[0], [1], [2], [c.n_links]], {}, "outside"), (None, {}, "uint64"),
                           (np.ones(2, np.uint64), {"out": out}, "io_device")):
        with pytest.raises(ValueError, match=match):
            env.cut_links(bad, **kw)
    with pytest.raises(ValueError, match="shape"):
        env.repair_links(np.ones((5, 2), np.uint64))
    with pytest.raises(ValueError, match="io_device"):
        env.failed_links(out=f)
    assert len(env.lib.calls) == 5


def test_a_format_window_is_refused_before_the_call():
    env = _env(False, modulations_to_consider=3)
    with pytest.raises(ValueError, match="modulations_to_consider"):
        env.cut_links(np.ones(2, np.uint64))
    assert env.lib.calls == []


def test_io_device_environment_checks_its_arguments_before_the_call():
    env = _env(True)
    sets, out = torch.ones((4, 2), dtype=torch.int64), torch.empty((4, 13), dtype=torch.float64)
    for a in (np.ones((4, 2), np.uint64), sets, sets.int(), [[0], [1], [2], [3]]):       # not a tensor, a host tensor, dtype, lists
        with pytest.raises(ValueError, match="sets must be"):
            env.cut_links(a, out=out)
        with pytest.raises(ValueError, match="sets must be"):
            env.repair_links(a, out=torch.empty(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs out"):
        env.failed_links()
    assert env.lib.calls == []


# ---- the oracle-driven states of the GPU cases ------------------------------------------------------------------------------
_RESTATED = {}


def restated(key):
    """a GPU case's configuration driven on CPU oracles with the GPU module's seed (computed once): per replica the pre-cut
    state, its set, the restated cut and the restated first decision after it, with the log of every evaluation's distance
    to its limit"""
    if key in _RESTATED:
        return _RESTATED[key]
    tb, kw, holder, ors = drive(key)
    ids = key == "ids"
    reps = []
    for r, o in enumerate(ors):
        svcs = oracle_records(o)
        if len(svcs) and ids:
            svcs = svcs.copy()                  # the oracle lists no ids: an id per record, namesakes by construction
            svcs["service_id"] = np.arange(len(svcs)) % max(1, len(svcs) - 3)
        links = replica_links(tb, svcs, r)
        w = as_words([links])[0]
        log, cover = [], dict.fromkeys(COVER, 0)
        margin = replica_margin(kw, r)
        row, act, index, post, grid = expected_cut(o, tb, holder, margin, svcs, o.grid(), w, ids, True, log, cover)
        cur_id = int(o.stats()["episode_services_processed"]) - 1 if ids else None
        ff = first_fit_restated(o, tb, holder, margin, post, grid, o.request(), cur_id, log)
        reps.append(dict(o=o, svcs=svcs, links=links, w=w, row=row, act=act, index=index, post=post, grid=grid, ff=ff,
                         log=np.array(log), cond=coverage(row, cover), margin=margin))
    _RESTATED[key] = key, tb, holder, reps
    return _RESTATED[key]


@pytest.fixture(params=CASES)
def case(request):
    return restated(request.param)


def test_the_grid_is_the_union_of_the_records_provisioned_ranges(case):
    """(a): n slots plus the guard slot unless the range ends at S, on every oracle; so a row without a free slot that no
    record crosses cannot be a healthy link"""
    key, tb, holder, reps = case
    S, records = holder.struct.n_slots, 0
    for rep in reps:
        rows = svc_rows(rep["svcs"])
        assert np.array_equal(rep["o"].grid(), grid_of_records(tb, tb.n_links, S, rows)), key
        records += len(rows)
    assert records > 0


def test_the_restated_cut_keeps_the_invariant_and_its_row_is_consistent(case):
    key, tb, holder, reps = case
    c = holder.struct
    reject = c.k_paths * c.n_mods * c.n_slots
    for r, rep in enumerate(reps):
        row, act, index, post, n = rep["row"], rep["act"], rep["index"], rep["post"], len(rep["svcs"])
        if r % 4 == 3:
            assert rep["links"] == [] and row[0] == 1 and np.all(np.isnan(row[1:])) and np.all(act == -1) and np.all(index == -1)
            assert np.array_equal(post, svc_rows(rep["svcs"])) and np.array_equal(rep["grid"], rep["o"].grid())
            continue
        assert row[0] == 0 and row[12] == 0 and row[1] == row[3] + row[5] + row[6] + row[12] and row[11] == len(set(rep["links"]))
        assert links_of(rep["w"]) == sorted(set(rep["links"]))
        assert np.array_equal(rep["grid"], grid_of_records(tb, tb.n_links, c.n_slots, post, rep["links"]))
        assert crossing(tb, post, rep["links"]) == 0
        assert len(post) == n - row[5] - row[6]
        kept = index >= 0
        assert sorted(index[kept].tolist()) == list(range(len(post)))
        assert np.array_equal(kept, act < reject)                                                  # survivors and restored victims
        assert np.array_equal(act >= 0, [crossing(tb, [x], rep["links"]) == 1 for x in svc_rows(rep["svcs"])])
        own = [FIELDS.index(f) for f in ("reserved", "release_time", "service_id")]
        assert np.array_equal(post[index[kept]][:, own], svc_rows(rep["svcs"])[kept][:, own])      # what a record owns travels with it
        dropped = expected_cut(rep["o"], tb, holder, rep["margin"], rep["svcs"], rep["o"].grid(), rep["w"], key == "ids", False)
        assert dropped[0][12] == dropped[0][1] == row[1] and np.all(dropped[0][3:9] == 0) and dropped[0][10] == 0
        assert np.array_equal(dropped[3], svc_rows(rep["svcs"])[act < 0])
        assert np.array_equal(dropped[4], grid_of_records(tb, tb.n_links, c.n_slots, dropped[3], rep["links"]))


def test_no_evaluation_lies_in_the_band_for_the_seeds_of_the_gpu_cases(case):
    """(c)"""
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


def test_the_sets_exercise_every_condition():
    """(b), over all cases together"""
    t = {}
    for key in CASES:
        for k, v in total(restated(key)[3]).items():
            t[k] = t.get(k, 0) + v
    print(t)
    assert t["restored"] > 0 and t["lost_qot"] > 0 and t["lost_ns_route"] > 0 and t["no_route"] > 0 and t["multi"] > 0
    assert 4 * t["no_victim"] <= t["evaluated"]
