"""The admission map without a GPU: ongym_admission_map is declared with its exact parameter list, exported and typed; both
environment flavours check their arguments before they call the library; the "traffic" weights are the two-stage draw's; the
slot formula is the oracle's number_slots for the configured rates; and, for the seeds of the GPU cases driven on CPU oracles,
no evaluation of the restatement (tests/admission_map_child.py) lies inside the band where a decision could differ, while the
cases exercise what tests/test_gpu_admission_map.py claims."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from admission_map_child import (BAND, CASES, drive, drive_full, oracle_records, pairs_of, restate_case, slot_counts,
                                 traffic_weights)
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()


def test_header_declares_admission_map():
    m = re.search(r"int ongym_admission_map\s*\(([^)]*)\);", HEADER)
    assert m
    assert " ".join(m.group(1).split()) == ("ongym_env *env, int32_t n_actions, const int32_t *actions, int32_t n_rates, const float *rates, "
                                            "const double *weights, double *summary_out, int32_t *map_out, float *margin_out")
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4 == nat.ABI_VERSION
    assert nat.ADMISSION_MAP == ("status", "admitted", "blocked_no_spectrum", "blocked_qot", "blocking_probability",
                                 "bit_rate_blocking", "lowest_margin", "detoured")
    assert nat.MAX_ADMISSION_RATES == 16
    assert "4 A Q R bytes per replica" in HEADER                   # the header says that map_out is large


def test_library_exports_and_native_declares_it():
    lib = nat.load_library()
    assert "ongym_admission_map" in nat.EXPORTED_SYMBOLS
    f = lib.ongym_admission_map
    vp = ctypes.c_void_p
    assert f.restype is ctypes.c_int32
    assert f.argtypes == [vp, ctypes.c_int32, vp, ctypes.c_int32, vp, vp, vp, vp, vp]
    assert f(None, 1, None, 4, None, None, None, None, None) == -1


class _StubLib:
    """records ongym_admission_map calls"""
    def __init__(self):
        self.calls = []

    def ongym_admission_map(self, h, a, actions, r, rates, weights, out, amap, margin):
        self.calls.append((int(a), actions is not None, int(r), rates is not None, weights is not None, amap is not None,
                           margin is not None))
        return 0


def _env(io_device, B=4, **kw):
    env = object.__new__(BatchedQRMSAEnv)
    kw.setdefault("bit_rate_selection", "discrete")
    env.holder = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                                  capacity=128, io_device=io_device, bit_rates=(10, 40, 100, 400), **kw)
    env.batch_size, env.lib, env._h, env.stream_handle = B, _StubLib(), None, None
    return env


def test_host_environment_checks_its_arguments_before_the_call():
    env = _env(False)
    Q = 91
    assert env.admission_pairs.shape == (Q, 2) and env.admission_pairs.dtype == np.int32
    assert env.admission_pairs.tolist() == [list(p) for p in pairs_of(14)]
    out = env.admission_map()
    assert out.shape == (4, 1, 8) and out.dtype == np.float64
    assert env.admission_map(np.zeros(4, np.int32), weights=None).shape == (4, 1, 8)
    s, m, g = env.admission_map(np.zeros((4, 5), np.int32), rates=(10, 100, 1000), weights=np.ones((Q, 3)), detail=True)
    assert s.shape == (4, 5, 8) and m.shape == (4, 5, Q, 3) and m.dtype == np.int32 and g.shape == m.shape and g.dtype == np.float32
    assert env.lib.calls == [(1, False, 4, False, True, False, False), (1, True, 4, False, False, False, False),
                             (5, True, 3, True, True, True, True)]
    a = np.zeros((4, 3), np.int32)
    for args, kw, match in (((np.zeros((4, 0), np.int32),), {}, "lie in"), ((np.zeros((4, 257), np.int32),), {}, "lie in"),
                            ((a.astype(np.int64),), {}, "int32"), ((np.zeros((3, 3), np.int32),), {}, "shape"),
                            ((np.zeros((4, 3, 1), np.int32),), {}, "shape"), (([[0]] * 4,), {}, "int32"),
                            ((a,), {"rates": (10, 40)}, "traffic"), ((a,), {"rates": (), "weights": None}, "number of rates"),
                            ((a,), {"rates": [1.0] * 17, "weights": None}, "number of rates"),
                            ((a,), {"rates": (10, np.nan), "weights": None}, "finite"),
                            ((a,), {"rates": (10, 0), "weights": None}, "positive"), ((a,), {"weights": "uniform"}, "traffic"),
                            ((a,), {"weights": np.ones((Q, 3))}, "shape"), ((a,), {"weights": np.ones((Q, 4), np.float32)}, "float64"),
                            ((), {"out": out}, "io_device")):
        with pytest.raises(ValueError, match=match):
            env.admission_map(*args, **kw)
    assert len(env.lib.calls) == 3


def test_a_format_window_and_continuous_rates_are_refused_before_the_call():
    env = _env(False, modulations_to_consider=3)
    with pytest.raises(ValueError, match="modulations_to_consider"):
        env.admission_map()
    cont = _env(False, bit_rate_selection="continuous")
    with pytest.raises(ValueError, match="discrete"):
        cont.admission_map(weights=None)
    assert cont.admission_map(rates=(50.0,), weights=None).shape == (4, 1, 8)
    assert env.lib.calls == [] and cont.lib.calls == [(1, False, 1, True, False, False, False)]


def test_io_device_environment_checks_its_arguments_before_the_call():
    env = _env(True)
    acts, out = torch.zeros((4, 3), dtype=torch.int32), torch.empty((4, 3, 8), dtype=torch.float64)
    for a, kw, match in ((np.zeros((4, 3), np.int32), {"out": out}, "actions must be"),   # not a tensor
                         (acts, {"out": out}, "actions must be"),                         # a host tensor: not on the device
                         (acts.long(), {"out": out}, "actions must be"),
                         (None, {"weights": None}, "needs out"),
                         (None, {"weights": np.ones((91, 4)), "out": out}, "weights must be")):
        with pytest.raises(ValueError, match=match):
            env.admission_map(a, **kw)
    assert env.lib.calls == []


def test_traffic_weights_are_the_two_stage_draw():
    p = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14], float)
    for kw in ({}, {"node_request_probabilities": p / p.sum(), "bit_rate_probabilities": (0.1, 0.2, 0.3, 0.4)}):
        env = _env(False, **kw)
        w = env.admission_weights()
        assert w.shape == (91, 4) and abs(w.sum() - 1.0) < 1e-12
        np.testing.assert_allclose(w, traffic_weights(env.holder), rtol=1e-12, atol=0)
    rng = np.random.default_rng(0)                                  # the enumeration against the draw itself
    q = p / p.sum()
    hits = np.zeros((14, 14))
    for _ in range(40000):
        s = rng.choice(14, p=q)
        rest = q.copy()
        rest[s] = 0
        hits[s, rng.choice(14, p=rest / rest.sum())] += 1
    emp = np.array([(hits[s, d] + hits[d, s]) / 40000 for s, d in pairs_of(14)])
    assert np.max(np.abs(emp - w.sum(axis=1))) < 5 * np.sqrt(0.05 / 40000)      # five sigma of the likeliest pair (p < 0.05)


@pytest.mark.parametrize("width", [0.0, 25.0])
def test_slot_formula_is_the_oracles_number_slots(width):
    from oracle_lib import OracleEnv
    env = _env(False, nslots_channel_width=width)
    o = OracleEnv(env.holder)
    n = slot_counts(env.holder, env.holder.bit_rates)
    for r, rate in enumerate(env.holder.bit_rates):
        for m in range(env.holder.struct.n_mods):
            assert n[r, m] == o.number_slots(float(rate), m)


_RESTATED = {}


def restated(key):
    """a GPU case's configuration driven on CPU oracles with the GPU module's seed (computed once)"""
    if key not in _RESTATED:
        tb, kw, holder, ors = drive_full() if key == "full" else drive(key)
        state = lambda r: (oracle_records(ors[r]), ors[r].grid(), ors[r].request())      # noqa: E731
        _RESTATED[key] = restate_case(key, tb, kw, holder, ors, state, lambda r: ors[r].policy_first_fit()[0])
    return _RESTATED[key]


@pytest.mark.parametrize("key", CASES + ("full",))
def test_no_evaluation_lies_in_the_band_and_no_case_is_empty(key):
    rates, weights, reps, band, evaluated = restated(key)
    tot = {}
    for rep in reps:
        for k, v in rep["cond"].items():
            tot[k] = tot.get(k, 0) + v
        for rows in (rep["null"][0], rep["list"][0]):
            ok = rows[:, 0] < 2
            assert np.all(rows[ok, 1] + rows[ok, 2] + rows[ok, 3] == weights.size)
            assert np.all(np.isnan(rows[~ok, 1:]))
    print(key, evaluated, "evaluations", tot)
    assert evaluated > 0 and band == 0
    assert abs(weights.sum() - 1.0) < 1e-12
    assert 4 * tot["none_blocked"] <= tot["scenarios"]             # at most a quarter of the scenarios without a blocked cell
    if key == "full":
        assert tot["status3"] > 0
    else:
        assert tot["status0"] > 0 and tot["status1"] > 0


def test_the_cases_together_exercise_every_condition():
    tot = {}
    for key in CASES + ("full",):
        for rep in restated(key)[2]:
            for k, v in rep["cond"].items():
                tot[k] = tot.get(k, 0) + v
    print(tot)
    for k in ("status0", "status1", "status2", "status3", "ns", "qot", "detoured", "below_top", "changed", "newly_blocked", "qot_alone"):
        assert tot[k] > 0, k
