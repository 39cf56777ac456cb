"""ongym_score_actions without a GPU: the header text and the ctypes mirror, every argument check of
BatchedQRMSAEnv.score_actions against a recording fake library, the presets, and the numpy restatement of tests/score_child.py
held to the CPU oracle: its highest-SNR preset is the oracle's highest-SNR policy, its first_feasible preset never lies above
first fit's action, and the conditions under which tests/test_gpu_score.py may compare a device to the restatement hold on
these states (no margin within 1e-8 dB of zero, no two distinct deciding scores within 1e-9 dB)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from batched_calls import make_env
from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym import rl
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from oracle_lib import OracleEnv
from score_child import (F, PRESETS, candidate_table, expected_scores, load_of, oracle_table, scores_of, touch_of, weight_rows)
from test_abi_mirror_host import parse_constants, parse_prototypes, prototype_problems

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = open(os.path.join(REPO, "include", "ongym_score.h")).read()
TEXT = re.sub(r"/\*.*?\*/", "", RAW, flags=re.S)


# ---- header, export, argtypes ---------------------------------------------------------------------------------------------
def test_header_declares_the_call_and_the_mirror_matches_it():
    assert '#include "ongym_score.h"' in open(os.path.join(REPO, "include", "ongym.h")).read()
    protos = parse_prototypes(TEXT)
    assert [p[0] for p in protos] == list(nat.SCORE_SIGNATURES) == ["ongym_score_actions"]
    assert [(a[0], a[1], a[2]) for a in protos[0][2]] == [("env", "ongym_env", 1), ("weights", "double", 1), ("per_replica", "int32_t", 0),
                                                          ("actions", "int32_t", 1), ("best_out", "double", 1), ("count_out", "int32_t", 1)]
    assert prototype_problems(protos, nat.SCORE_SIGNATURES, {}) == []
    doctored = {"ongym_score_actions": (C.c_int32, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p))}
    assert prototype_problems(protos, doctored, {}) == ["ongym_score_actions: parameter 2 (per_replica): header int32_t, python c_void_p"]
    assert parse_constants(TEXT) == {"ONGYM_SCORE_FEATURES": len(nat.SCORE_FEATURES)} and len(nat.SCORE_FEATURES) == 10
    assert nat.SCORE_FEATURES == ("route", "hops", "format_rank", "slots", "slot_hops", "start", "load", "touch", "gsnr", "margin")
    assert nat.SCORE_COUNT_COLUMNS == ("with_spectrum", "feasible", "flags")
    for i, name in enumerate(nat.SCORE_FEATURES):                  # the header names the features in the mirror's order
        assert re.search(rf"\bx{i} {name}\b", RAW), name
    assert not set(nat.SCORE_SIGNATURES) & set(nat.SIGNATURES)


def test_library_exports_the_call_and_refuses_a_null_environment():
    lib = nat.load_library()
    fn = lib.ongym_score_actions
    assert fn.restype is C.c_int32 and list(fn.argtypes) == list(nat.SCORE_SIGNATURES["ongym_score_actions"][1])
    assert fn(None, None, 0, None, None, None) == nat.E_ARG


def test_a_library_without_the_call_does_not_load(monkeypatch):
    class Old:
        _name = "old.so"
    monkeypatch.delenv("ONGYM_HIP_LIB", raising=False)
    with pytest.raises(RuntimeError, match="does not export ongym_score_actions"):
        nat._declare(Old())


# ---- BatchedQRMSAEnv.score_actions against a recording library ---------------------------------------------------------------
B = 4


class FakeLib:
    """ongym_score_actions that records its arguments, reads the weights at the size the scalars imply and fills the outputs"""

    def __init__(self):
        self.calls = []

    def ongym_score_actions(self, handle, weights, per_replica, actions, best, counts):
        adr = lambda p: (p.value or 0) if isinstance(p, C.c_void_p) else int(p or 0)           # noqa: E731
        n = (B if per_replica else 1) * F
        w = np.frombuffer(C.string_at(adr(weights), 8 * n), np.float64).copy()
        C.memset(adr(actions), 0x01, 4 * B)
        if adr(best):
            C.memset(adr(best), 0x02, 8 * B * (1 + F))
        if adr(counts):
            C.memset(adr(counts), 0x03, 4 * B * 3)
        self.calls.append(dict(handle=handle, weights=w, per_replica=per_replica, best=bool(adr(best)), counts=bool(adr(counts))))
        return 0


def stub(kind):
    env = make_env(BatchedQRMSAEnv, kind)
    env.lib = FakeLib()
    return env


def test_host_arguments():
    env = stub("host")
    w = np.arange(F, dtype=np.float64)
    a = env.score_actions(w)
    assert a.dtype == np.int32 and a.shape == (B,) and np.all(a == 0x01010101)
    call = env.lib.calls[-1]
    assert call["per_replica"] == 0 and not call["best"] and not call["counts"] and np.array_equal(call["weights"], w)
    W = np.arange(B * F, dtype=np.float64).reshape(B, F)
    a, best, counts = env.score_actions(W, detail=True)
    call = env.lib.calls[-1]
    assert call["per_replica"] == 1 and call["best"] and call["counts"] and np.array_equal(call["weights"], W.ravel())
    assert best.dtype == np.float64 and best.shape == (B, 1 + F) and counts.dtype == np.int32 and counts.shape == (B, 3)
    assert np.all(counts == 0x03030303)
    env.score_actions(W[:, ::-1][:, ::-1][::1])                                     # a view
    env.score_actions(np.asfortranarray(W))                                          # made contiguous
    assert np.array_equal(env.lib.calls[-1]["weights"], W.ravel())
    env.score_actions(list(w))                                                       # a list, as cut_links takes lists
    assert np.array_equal(env.lib.calls[-1]["weights"], w)
    n = len(env.lib.calls)
    for bad, what in ((w.astype(np.float32), "float64"), (torch.from_numpy(w), "float64"), (None, "float64"), (w[:9], "shape"),
                      (W[:3], "shape"), (W.reshape(2, 2, F), "shape"), (np.zeros((B, F + 1)), "shape")):
        with pytest.raises(ValueError, match=what):
            env.score_actions(bad)
    for v in (np.nan, np.inf, -np.inf):
        Wb = W.copy()
        Wb[B - 1, F - 1] = v
        with pytest.raises(ValueError, match="finite"):
            env.score_actions(Wb)
    with pytest.raises(ValueError, match="out is for io_device"):
        env.score_actions(w, out=np.zeros(B, np.int32))
    with pytest.raises(ValueError, match="every format"):
        stub("host_window").score_actions(w)
    assert len(env.lib.calls) == n                                                   # every refusal before the library


def test_device_arguments(monkeypatch):
    monkeypatch.setattr(rl, "_device", lambda env: torch.device("cpu"))
    monkeypatch.setattr(rl, "_check_stream", lambda env: None)
    env = stub("device")
    W = torch.arange(B * F, dtype=torch.float64).reshape(B, F)
    out = (torch.zeros(B, dtype=torch.int32), torch.zeros((B, 1 + F), dtype=torch.float64), torch.zeros((B, 3), dtype=torch.int32))
    assert env.score_actions(W[0].clone(), out=out[0]) is out[0]
    assert env.lib.calls[-1]["per_replica"] == 0 and not env.lib.calls[-1]["best"]
    ret = env.score_actions(W, out=out, detail=True)
    assert ret is out and env.lib.calls[-1]["per_replica"] == 1 and env.lib.calls[-1]["counts"]
    assert np.array_equal(env.lib.calls[-1]["weights"], W.numpy().ravel()) and torch.all(out[2] == 0x03030303)
    Wn = W.clone()
    Wn[0, 0] = float("nan")
    env.score_actions(Wn, out=out[0])                                                # a device array is not inspected
    n = len(env.lib.calls)
    for bad in (W.numpy(), W.float(), W[:, :9].contiguous(), W.t().contiguous().t(), None):
        with pytest.raises(ValueError, match="weights"):
            env.score_actions(bad, out=out[0])
    for bad_out, detail in ((None, False), (out[0].long(), False), (out[0][:3], False), (out[0].numpy(), False), (out[0], True),
                            (out[:2], True), ((out[0], out[1].float(), out[2]), True), ((out[0], out[1], out[2][:, :2]), True)):
        with pytest.raises(ValueError, match="out"):
            env.score_actions(W, out=bad_out, detail=detail)
    with pytest.raises(ValueError, match="every format"):
        stub("device_window").score_actions(W, out=out[0])
    assert len(env.lib.calls) == n
    monkeypatch.setattr(rl, "_check_stream", lambda env: (_ for _ in ()).throw(ValueError("stream")))
    with pytest.raises(ValueError, match="stream"):
        env.score_actions(W, out=out[0])
    assert len(env.lib.calls) == n


# ---- presets --------------------------------------------------------------------------------------------------------------
def test_presets():
    assert tuple(nat.SCORE_PRESETS) == PRESETS
    M, S = 6, 320
    ff = nat.score_preset("first_feasible", M, S)
    assert ff.tolist() == [M * S, 0, S, 0, 0, 1, 0, 0, 0, 0]
    x = np.array([[k, 3, r, 4, 12, s, 7.5, 1, 20.0, 1.0] for k in range(3) for r in range(M) for s in (0, 17, S - 1)], np.float64)
    assert scores_of(x, ff).tolist() == [k * M * S + r * S + s for k in range(3) for r in range(M) for s in (0, 17, S - 1)]
    assert nat.score_preset("highest_snr", M, S).tolist() == [0] * 8 + [-1, 0]
    assert nat.score_preset("lowest_margin", M, S).tolist() == [0] * 9 + [1]
    ls = nat.score_preset("least_slot_hops", M, S)
    assert ls[4] == 1 and ls[8] == ls[9] == 0 and np.count_nonzero(ls) == 3
    # the tie-breakers order equal slot-hops by route, then start, and never outweigh one slot-hop (k < 128, s < 1024)
    assert 0 < ls[5] * 1023 < ls[0] and ls[0] * 127 + ls[5] * 1023 < 1
    assert all(nat.score_preset(n, M, S) is not nat.score_preset(n, M, S) for n in PRESETS)       # copies
    env = stub("host")
    c = env.holder.struct
    assert np.array_equal(env.score_preset("first_feasible"), nat.first_feasible_weights(c.n_mods, c.n_slots))
    with pytest.raises(KeyError):
        nat.score_preset("no_such", M, S)
    assert nat.score_weights(touch=2.5).tolist() == [0] * 7 + [2.5, 0, 0]


# ---- hand-made rows: touch and load ---------------------------------------------------------------------------------------
def test_touch_and_load_on_hand_made_rows():
    S = 16
    row = np.ones(S, np.int32)
    row[[5, 6, 12]] = 0                                  # free runs [0, 5), [7, 12), [13, 16)
    assert touch_of(row, 0, 2) == 1                      # s = 0: the left edge; cell 3 behind the guard is free
    assert touch_of(row, 0, 3) == 1                      # cell 4 free
    assert touch_of(row, 0, 4) == 2                      # n + 1 = the whole free run: the edge and cell 5
    assert touch_of(row, 1, 2) == 0
    assert touch_of(row, 1, 3) == 1                      # e = 5 is used
    assert touch_of(row, 7, 4) == 2                      # n + 1 = the whole free run [7, 12): cell 6 and cell 12
    assert touch_of(row, 8, 2) == 0 and touch_of(row, 8, 3) == 1 and touch_of(row, 7, 2) == 1
    assert touch_of(row, 13, 3) == 2                     # the block ends at S (no guard): s + n + 1 > S, so e = S
    assert touch_of(row, 13, 2) == 2                     # the guard is the last cell: e = S
    assert touch_of(row, 14, 2) == 1                     # ends at S, cell 13 free
    assert touch_of(np.ones(S, np.int32), 3, 2) == 0 and touch_of(np.ones(S, np.int32), 0, S) == 2
    assert load_of(row, 2) == 1.5 and load_of(row, 3) == 1.0 and load_of(np.ones(S, np.int32), 4) == 0.0
    assert load_of(np.zeros(S, np.int32), 3) == S / 3

    # the table walks route, format best first, start ascending; formats that share a slot count share their GSNR
    h = nat.ConfigHolder(golden_tables("ring4"), modulations=jocn_modulations(), num_spectrum_resources=S, capacity=64, load=10)
    M = h.struct.n_mods

    class T:                                             # two routes between nodes 0 and 1, of two and three hops
        pair_paths = np.full((2, 2, h.struct.k_paths), -1)
        path_hops = np.array([2, 3])
    T.pair_paths[0, 1, :2] = T.pair_paths[1, 0, :2] = [0, 1]
    rows = {0: row, 1: np.ones(S, np.int32)}
    nslots = [0, 9, 4, 4, 2, 2][:M]

    def cands(r, n):
        return [s for s in range(S) if np.all(r[s:s + n]) and (s + n == S or (s + n < S and r[s + n]))]
    gn = lambda c: [30.0 - 0.5 * p - 0.01 * s for p, s, n in c]                    # noqa: E731
    t = candidate_table(T, h, 0.0, 0, 1, nslots, rows.__getitem__, cands, gn)
    x = t["x"]
    order = [tuple(v) for v in x[:, [0, 2, 5]].astype(int).tolist()]
    assert order == sorted(order) and t["empty_group"] is True        # nine slots find no start on route 0
    assert set(x[x[:, 0] == 0][:, 6]) == {1.5} and set(x[x[:, 0] == 1][:, 6]) == {0.0}
    assert np.array_equal(x[:, 4], x[:, 3] * x[:, 1]) and np.array_equal(x[:, 1], np.where(x[:, 0] == 0, 2, 3))
    nine = x[(x[:, 0] == 0) & (x[:, 3] == 9)]
    assert len(nine) == 0 and len(x[(x[:, 0] == 1) & (x[:, 3] == 9)]) == S - 9 + 1 - 1 + 1     # s = 0..6 with a guard, s = 7 ends at S
    thr = np.asarray(h.mod_thr)
    assert np.array_equal(x[:, 9], x[:, 8] - (thr[M - 1 - x[:, 2].astype(int)] + 0.0))
    same = x[(x[:, 0] == 0) & (x[:, 3] == 2) & (x[:, 5] == 2)]
    assert len(same) == 2 and same[0, 8] == same[1, 8] and same[0, 9] != same[1, 9]
    e = expected_scores(t, nat.score_preset("highest_snr", M, S))
    assert e["action"] == 0 * M * S + int(x[0, 2]) * S + 0 and e["best"][0] == -30.0 and e["counts"].tolist() == [len(x), len(x), 0]
    t2 = candidate_table(T, h, 40.0, 0, 1, nslots, rows.__getitem__, cands, gn)     # a margin nothing clears
    e = expected_scores(t2, nat.score_preset("highest_snr", M, S))
    assert e["action"] == h.reject_action and np.all(np.isnan(e["best"])) and e["counts"].tolist() == [len(x), 0, nat.F_BLOCKED_OSNR]
    t3 = candidate_table(T, h, 0.0, 0, 1, [0, 0, 0, 0, 0, S + 1][:M], rows.__getitem__, cands, gn)
    assert expected_scores(t3, np.zeros(F))["counts"].tolist() == [0, 0, nat.F_BLOCKED_RESOURCES]
    # strict `<` with exact scores: the first of equal scores wins; a NaN score never wins
    assert expected_scores(t, np.zeros(F))["index"] == 0
    assert expected_scores(t, nat.score_weights(start=-1))["index"] == int(np.flatnonzero(x[:, 5] == x[:, 5].max())[0])


# ---- the restatement on oracle states -------------------------------------------------------------------------------------
STATES = dict(ring4=("ring4", 64, 40.0, 250, 6), nsfnet100=("nsfnet", 100, 140.0, 250, 6), nobeleu320=("nobel-eu", 320, 300.0, 500, 3))
DECISIONS = 6


@pytest.fixture(scope="module")
def decisions():
    """per topology the decisions of its seeds: (table, first fit's action, the oracle's highest-SNR answer, reject action)"""
    out = {}
    for key, (tbname, S, load, warm, seeds) in STATES.items():
        tb = golden_tables(tbname)
        holder = nat.ConfigHolder(tb, modulations=jocn_modulations(), num_spectrum_resources=S, capacity=1024, load=load,
                                  bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), episode_length=10 ** 6)
        rows = []
        for seed in range(100, 100 + seeds):
            o = OracleEnv(holder)
            o.seed(seed)
            o.reset()
            o.run_first_fit(warm)
            for _ in range(DECISIONS):
                ff = o.policy_first_fit()
                rows.append((oracle_table(o, tb, holder, holder.struct.margin), ff[0], o.policy(nat.POLICY_HIGHEST_SNR), o.reject_action))
                o.step(ff[0])
        out[key] = (holder, rows)
    return out


@pytest.mark.parametrize("key", list(STATES))
def test_restatement_against_the_oracle(decisions, key):
    holder, rows = decisions[key]
    c = holder.struct
    hs, lm = nat.score_preset("highest_snr", c.n_mods, c.n_slots), nat.score_preset("lowest_margin", c.n_mods, c.n_slots)
    ffw = nat.score_preset("first_feasible", c.n_mods, c.n_slots)
    below = rejects = ties = 0
    closest_margin = closest_pair = np.inf
    for table, ff_action, (hs_action, hs_res, hs_osnr), reject in rows:
        assert reject == c.k_paths * c.n_mods * c.n_slots
        e = expected_scores(table, hs)
        assert e["action"] == hs_action
        assert (bool(e["counts"][2] & nat.F_BLOCKED_RESOURCES), bool(e["counts"][2] & nat.F_BLOCKED_OSNR)) == (hs_res, hs_osnr)
        f = expected_scores(table, ffw)
        assert f["action"] <= ff_action
        below += f["action"] < ff_action
        none = not table["feasible"].any()
        rejects += none
        for w in (hs, lm, ffw, *weight_rows(holder, 8)[4:]):
            r = expected_scores(table, w)
            assert (r["action"] == reject) == none and (r["index"] < 0) == none and np.isnan(r["best"][0]) == none
            assert r["counts"][:2].tolist() == [len(table["x"]), int(table["feasible"].sum())]
        if f["index"] >= 0:
            assert f["best"][0] == f["action"]                        # the score of first_feasible IS the action index
        # the conditions of the GPU comparison
        if len(table["x"]):
            closest_margin = min(closest_margin, float(np.min(np.abs(table["x"][:, 9]))))
        for w in (hs, lm):
            t = scores_of(table["x"], w)[table["feasible"]]
            u = np.unique(t)
            ties += len(t) - len(u)
            if len(u) > 1:
                closest_pair = min(closest_pair, float(u[1] - u[0]))
            assert not expected_scores(table, w)["near"]
    print(f"{key}: {len(rows)} decisions, first_feasible below first fit in {below}, no feasible candidate in {rejects}, "
          f"closest margin {closest_margin:.3g} dB, closest two distinct deciding scores {closest_pair:.3g} dB, {ties} exact ties")
    assert below >= 1
    assert rejects >= 1 or key == "nobeleu320"                          # the loaded small networks block; nobel-eu at 300 E does not here
    assert closest_margin > 1e-8 and closest_pair > 1e-9
    assert ties > 0                                                     # equal scores are exact ties, resolved by walk order
