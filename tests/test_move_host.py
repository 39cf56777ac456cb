"""Moving running lightpaths on live replicas without a GPU: the call is declared with its exact parameter list, exported and
typed; BatchedQRMSAEnv checks its arguments before it calls the library; and on the CPU oracles of the GPU cases
(tests/move_child.py, same configurations, seeds and moves)
  (a) the restated moves keep the grid equal to the union of the records' provisioned ranges, and a record keeps its index,
      release time and id;
  (b) the drawn moves reach every status 0-4 and what tests/test_gpu_move.py claims: a move to another route, one to another
      format with another slot count, a one-slot shift down that overlaps the old range, a moved record that ended at S (case
      `odd`), a moved namesake (case `ids`), a TOP pick that skips an attempted record;
  (c) no evaluation of the restated moves lies inside the band where a decision could differ."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from failure_impact_child import BAND, CASES, drive, oracle_records, replica_margin
from link_cut_child import FIELDS, grid_of_records, svc_rows
from move_child import COVER, FIRST_FIT, LEAN, TOP, draw_moves, expected_moves, top_record, width_limit
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()
VP, I32 = ctypes.c_void_p, ctypes.c_int32


def test_header_declares_the_call():
    m = re.search(r"int ongym_move_services\s*\(([^)]*)\);", HEADER)
    assert m and " ".join(m.group(1).split()) == ("ongym_env *env, int32_t n_moves, const int32_t *moves, int32_t flags, "
                                                  "double *move_out")
    for name, value in (("ONGYM_MOVE_TOP", -1), ("ONGYM_MOVE_FIRST_FIT", -1), ("ONGYM_MOVE_OWN_ROUTE", 1)):
        assert re.search(r"enum\s*\{\s*%s\s*=\s*%d\s*\}" % (name, value), HEADER), name
    assert (nat.MOVE_TOP, nat.MOVE_FIRST_FIT, nat.MOVE_OWN_ROUTE) == (-1, -1, 1)
    assert nat.MOVE_COLUMNS == ("status", "record", "old_action", "new_action", "margin", "slot_hops_delta")
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4 == nat.ABI_VERSION


def test_library_exports_and_native_declares_it():
    lib = nat.load_library()
    assert "ongym_move_services" in nat.EXPORTED_SYMBOLS
    f = lib.ongym_move_services
    assert f.restype is I32 and f.argtypes == [VP, I32, VP, I32, VP]
    assert f(None, 1, None, 0, None) == -1


class _StubLib:
    """records the calls"""
    def __init__(self):
        self.calls = []

    def ongym_move_services(self, h, n_moves, moves, flags, out):
        self.calls.append((int(n_moves), int(flags)))
        return 0


def _env(io_device, B=4, **kw):
    env = object.__new__(BatchedQRMSAEnv)
    env.holder = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                                  capacity=128, io_device=io_device, **kw)
    env.batch_size, env.lib, env._h, env.stream_handle = B, _StubLib(), None, None
    return env


def test_host_environment_checks_its_arguments_before_the_call():
    env = _env(False)
    out = env.move_services(np.zeros((3, 2), np.int32))
    assert out.shape == (4, 3, 6) and out.dtype == np.float64
    assert env.move_services(np.zeros((4, 5, 2), np.int32), own_route=True).shape == (4, 5, 6)
    assert env.move_services(np.zeros((4, 8, 2), np.int32)[:, ::2]).shape == (4, 4, 6)            # made contiguous
    assert env.defragment(7).shape == (4, 7, 6)
    assert env.defragment(2, own_route=False).shape == (4, 2, 6)
    assert env.lib.calls == [(3, 0), (5, nat.MOVE_OWN_ROUTE), (4, 0), (7, nat.MOVE_OWN_ROUTE), (2, 0)]
    for bad, kw, match in ((np.zeros((3, 2, 2), np.int32), {}, "shape"), (np.zeros((4, 3, 3), np.int32), {}, "shape"),
                           (np.zeros((0, 2), np.int32), {}, "shape"), (np.zeros(2, np.int32), {}, "shape"),
                           (np.zeros((3, 2), np.int64), {}, "int32"), ([[0, -1]], {}, "int32"), (None, {}, "int32"),
                           (np.zeros((3, 2), np.int32), {"out": out}, "io_device")):
        with pytest.raises(ValueError, match=match):
            env.move_services(bad, **kw)
    with pytest.raises(ValueError, match="at least 1"):
        env.defragment(0)
    assert len(env.lib.calls) == 5


def test_a_format_window_is_refused_before_the_call():
    env = _env(False, modulations_to_consider=3)
    with pytest.raises(ValueError, match="modulations_to_consider"):
        env.move_services(np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError, match="modulations_to_consider"):
        env.defragment(3)
    assert env.lib.calls == []


def test_io_device_environment_checks_its_arguments_before_the_call():
    env = _env(True)
    moves, out = torch.zeros((4, 3, 2), dtype=torch.int32), torch.empty((4, 3, 6), dtype=torch.float64)
    for a in (np.zeros((4, 3, 2), np.int32), moves, moves.long(), [[0, -1]]):       # not a tensor, a host tensor, dtype, a list
        with pytest.raises(ValueError, match="moves must be"):
            env.move_services(a, out=out)
    with pytest.raises(ValueError, match="io_device"):
        env.defragment(3)
    assert env.lib.calls == []


# ---- the oracle-driven states of the GPU cases ------------------------------------------------------------------------------
_RESTATED = {}


def restated(key):
    """a GPU case's configuration driven on CPU oracles with the GPU module's seed (computed once): per replica the pre-call
    state, its moves, the restated call and the restated own-route sweep, with the log of every evaluation's distance to its
    limit"""
    if key in _RESTATED:
        return _RESTATED[key]
    tb, kw, holder, ors = drive(key)
    ids = key == "ids"
    sweep = np.tile(np.array([TOP, FIRST_FIT], np.int32), (6, 1))
    limit = width_limit(holder, key in LEAN)    # what the device applies where a lean step kernel can run the configuration
    reps = []
    for r, o in enumerate(ors):
        svcs = oracle_records(o)
        if len(svcs) and ids:
            svcs = svcs.copy()                  # the oracle lists no ids: an id per record, namesakes by construction
            svcs["service_id"] = np.arange(len(svcs)) % max(1, len(svcs) - 3)
        moves = draw_moves(o, tb, holder, svcs, o.grid(), r, ids)
        log, cover = [], {}
        margin = replica_margin(kw, r)
        want, post, grid = expected_moves(o, tb, holder, margin, svcs, o.grid(), moves, ids, False, log, cover, limit)
        s_want, s_post, s_grid = expected_moves(o, tb, holder, margin, svcs, o.grid(), sweep, ids, True, log, limit=limit)
        reps.append(dict(o=o, svcs=svcs, moves=moves, want=want, post=post, grid=grid, log=np.array(log), cover=cover,
                         s_want=s_want, s_post=s_post, s_grid=s_grid))
    _RESTATED[key] = key, tb, holder, reps
    return _RESTATED[key]


@pytest.fixture(params=CASES)
def case(request):
    return restated(request.param)


def test_the_restated_moves_keep_the_grid_the_union_of_the_records_ranges(case):
    """(a), for the drawn moves and for the own-route sweep"""
    key, tb, holder, reps = case
    c = holder.struct
    S, moved = c.n_slots, 0
    own = [FIELDS.index(f) for f in ("reserved", "release_time", "service_id")]
    se = np.asarray(holder.mod_se)
    for rep in reps:
        pre = svc_rows(rep["svcs"])
        assert np.array_equal(rep["o"].grid(), grid_of_records(tb, tb.n_links, S, pre)), key
        for want, post, grid in ((rep["want"], rep["post"], rep["grid"]), (rep["s_want"], rep["s_post"], rep["s_grid"])):
            assert np.array_equal(grid, grid_of_records(tb, tb.n_links, S, post)), key
            assert post.shape == pre.shape and np.array_equal(post[:, own], pre[:, own]), key
            assert np.all(post[:, 2] <= np.maximum(pre[:, 2], width_limit(holder, key in LEAN))), key      # no move widens beyond the limit
            cap = lambda x: x[:, 2] * se[x[:, 3].astype(int)]     # noqa: E731
            assert np.all(cap(post) >= cap(pre)), key                      # slot counts are rounded up, move after move
            ok = want[:, 0] == 0
            changed = np.flatnonzero(np.any(post[:, :4] != pre[:, :4], axis=1))
            assert set(changed.tolist()) <= set(want[ok, 1].astype(int).tolist()), key
            assert np.all(want[~ok, 2] == want[~ok, 3]) and np.all(want[~ok, 5] == 0) and np.all(np.isnan(want[~ok, 4])), key
            assert np.all(want[ok, 2] != want[ok, 3]) and np.all(want[ok, 4] >= 0), key
            assert np.all((want[:, 1] == -1) == (want[:, 2] == -1)) and np.all(want[want[:, 1] == -1, 0] == 1), key
            moved += int(ok.sum())
        sw = rep["s_want"]                               # the sweep: every pick is a different record, in descending order of last slot
        picked = sw[sw[:, 1] >= 0, 1].astype(int)
        assert len(set(picked.tolist())) == len(picked) == min(6, len(pre)), key
        if len(pre):
            assert picked[0] == top_record(pre, set()), key
    assert moved > 0


def test_no_evaluation_lies_in_the_band_for_the_seeds_of_the_gpu_cases(case):
    """(c)"""
    key, _, _, reps = case
    logs = np.concatenate([rep["log"] for rep in reps])
    print(f"{key}: {len(logs)} evaluated (candidate, format) pairs, closest to its limit {logs.min() if len(logs) else np.nan:.2e}")
    assert len(logs) > 0
    assert int(np.sum(logs < BAND)) == 0


def total(key):
    out = dict.fromkeys(COVER, 0)
    for rep in restated(key)[3]:
        for k, v in rep["cover"].items():
            out[k] += v
    return out


def test_the_moves_exercise_every_status_and_condition():
    """(b): over all cases together, and the two that belong to a case in that case"""
    t = dict.fromkeys(COVER, 0)
    for key in CASES:
        for k, v in total(key).items():
            t[k] += v
    print(t)
    assert all(t[k] > 0 for k in ("moved", "invalid", "unchanged", "no_spectrum", "qot")), t
    assert all(t[k] > 0 for k in ("other_route", "other_format", "shift_down", "top_skips", "to_S")), t
    assert total("odd")["ends_at_S"] > 0 and total("ids")["namesake"] > 0
