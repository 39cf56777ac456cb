"""Action impact without a GPU: ongym_action_impact is declared with its exact parameter list, exported and typed;
BatchedQRMSAEnv.action_impact checks its arguments before it calls the library; QRMSABlockVecEnv(protect_running=True) masks by
column 3; and the restatement that tests/test_gpu_action_impact.py holds the device to equals, on the CPU oracle, the oracle's
own step: the state is built twice by replay, one copy steps the action, and where the step released nothing every victim's
restated GSNR-after is the stepped oracle's value for that service."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from optical_networking_gym.envs.block_vec_env import QRMSABlockVecEnv
from test_gpu_action_impact import (BAND_CAP, CASES, COLS, REPLICAS, SEED, candidate_actions, compare_rows, decode, drive, in_band,
                                    oracle_block_row, restate_replica, rows_from_pairs)
from test_gpu_service_qot import insertion_order, restate_gn

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()


def test_header_declares_action_impact():
    m = re.search(r"int ongym_action_impact\s*\(([^)]*)\);", HEADER)
    assert m
    assert " ".join(m.group(1).split()) == ("ongym_env *env, int32_t n_actions, const int32_t *actions, const double *svc_in, "
                                            "double *impact_out")
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4
    assert nat.ACTION_IMPACT == ("status", "affected", "below_minimum_after", "newly_below_minimum", "newly_below_margin",
                                 "lowest_margin_after", "largest_drop", "lowest_margin_record")
    assert nat.MAX_IMPACT_ACTIONS == 256


def test_library_exports_and_native_declares_it():
    lib = nat.load_library()
    assert "ongym_action_impact" in nat.EXPORTED_SYMBOLS
    f = lib.ongym_action_impact
    assert f.restype is ctypes.c_int32
    assert f.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.ongym_action_impact(None, 1, None, None, None) == -1


class _StubLib:
    """records ongym_action_impact calls"""
    def __init__(self):
        self.calls = []

    def ongym_action_impact(self, h, n, actions, svc, out):
        self.calls.append((int(n), svc is not None and getattr(svc, "value", svc) is not None))
        return 0


def _env(io_device, B=4):
    env = object.__new__(BatchedQRMSAEnv)
    env.holder = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                                  io_device=io_device)
    env.batch_size, env.lib, env._h, env.stream_handle = B, _StubLib(), None, None
    return env


def test_host_environment_checks_its_arguments_before_the_call():
    env = _env(False)
    c = env.holder.struct
    out = env.action_impact(np.zeros((4, 9), np.int32))
    assert out.shape == (4, 9, 8) and out.dtype == np.float64
    assert env.action_impact(np.zeros(4, np.int32)).shape == (4, 1, 8)
    env.action_impact(np.zeros((4, 256), np.int32), svc=np.zeros((4, c.capacity, 4)))
    assert env.lib.calls == [(9, False), (1, False), (256, True)]
    for bad, kw, match in ((np.zeros((4, 0), np.int32), {}, "lie in"), (np.zeros((4, 257), np.int32), {}, "lie in"),
                           (np.zeros((4, 9), np.int64), {}, "int32"), (np.zeros((3, 9), np.int32), {}, "shape"),
                           (np.zeros((4, 9, 1), np.int32), {}, "shape"), ([[0]] * 4, {}, "int32"),
                           (np.zeros((4, 9), np.int32), {"svc": np.zeros((4, c.capacity, 3))}, "svc must be"),
                           (np.zeros((4, 9), np.int32), {"svc": np.zeros((4, c.capacity, 4), np.float32)}, "svc must be"),
                           (np.zeros((4, 9), np.int32), {"out": out}, "io_device")):
        with pytest.raises(ValueError, match=match):
            env.action_impact(bad, **kw)
    assert len(env.lib.calls) == 3


def test_io_device_environment_checks_its_arguments_before_the_call():
    env = _env(True)
    c = env.holder.struct
    acts, out = torch.zeros((4, 9), dtype=torch.int32), torch.empty((4, 9, 8), dtype=torch.float64)
    for a, kw, match in ((np.zeros((4, 9), np.int32), {"out": out}, "actions must be"),     # not a tensor
                         (acts, {"out": out}, "actions must be"),                           # a host tensor: not on the device
                         (acts.long(), {"out": out}, "actions must be")):
        with pytest.raises(ValueError, match=match):
            env.action_impact(a, **kw)
    assert env.lib.calls == []
    assert c.io_device


class _FakeBatched:
    """observe_blocks / action_impact of two replicas, three block actions and reject"""
    def __init__(self):
        self.asked = []

    def observe_blocks(self, J):
        return (np.zeros((2, 4), np.float32), np.array([[1, 1, 0, 1], [1, 1, 1, 1]], np.uint8),
                np.array([[10, 20, 99, 99], [11, 21, 31, 99]], np.int32))

    def action_impact(self, actions):
        self.asked.append(actions.copy())
        out = np.full((2, 4, 8), np.nan)
        out[:, :3, 0], out[:, 3, 0] = 0, 1
        out[:, :3, 1:5] = 0
        out[0, 1, COLS["newly_below_minimum"]] = 2
        out[1, 2, COLS["newly_below_minimum"]] = 1
        out[0, 2, 0] = 2
        out[0, 2, 1:5] = np.nan
        return out


def test_protect_running_clears_the_disrupting_block_actions_only():
    v = object.__new__(QRMSABlockVecEnv)
    v.env, v.blocks, v.num_envs, v.protect_running = _FakeBatched(), 1, 2, True
    v._obs = v._mask = v._map = v._newly = None
    assert v.action_masks().tolist() == [[True, False, False, True], [True, True, False, True]]
    assert v._newly.tolist() == [[0, 2, 0, 0], [0, 0, 1, 0]]
    v.protect_running, v._mask = False, None
    assert v.action_masks().tolist() == [[True, True, False, True], [True, True, True, True]]
    assert len(v.env.asked) == 1


@pytest.mark.parametrize("key,B", [("disr_nsfnet_320", 12), ("ff_nsfnet_320", 6)])
def test_restated_after_equals_the_stepped_oracle(key, B):
    """the first-fit action after the case's traffic: restated GSNR-after of every victim within 1e-12 dB of the stepped
    oracle's restate_gn (3.6e-15 dB seen: the release-time order is a proxy of the reference's list order), and with
    measure_disruptions the restated newly-below count is the increase of the oracle's disrupted_services"""
    tb, kw, holder, stay = drive(key, B, SEED)
    _, _, _, moved = drive(key, B, SEED)
    pairs_seen = qualified = accepted = newly_total = 0
    worst = 0.0
    for o, o2 in zip(stay, moved):
        action = o.policy_first_fit()[0]
        if action == o.reject_action:
            continue
        svcs = o.services()
        svcs = svcs[insertion_order(svcs)]
        status, pairs = restate_replica(o, tb, holder, svcs, np.array([action]))
        assert status[0] == 0
        d0 = int(o2.stats()["disrupted_services"])
        rc, rec = o2.step(int(action))
        assert rc == 0 and rec["accepted"]
        accepted += 1
        if kw.get("measure_disruptions"):
            # the oracle does not list its disrupted set (`reserved` of services() is 0), so "not yet marked" is restated as
            # "not below before": a service below minimum_osnr is in the set (test_gpu_service_qot pins that invariant)
            newly = int(np.sum((pairs[:, 3] < pairs[:, 4]) & ~(pairs[:, 2] < pairs[:, 4])))
            assert newly == int(o2.stats()["disrupted_services"]) - d0
            newly_total += newly
        after = o2.services()
        after = after[insertion_order(after)]
        if len(after) != len(svcs) + 1:
            continue                                                # the step released something: another set of services
        qualified += 1
        want = restate_gn(o2, tb, holder.mod_se, after)
        at = {(int(p), int(s)): i for i, (p, s) in enumerate(zip(after["path_id"], after["slot"]))}
        for _, y, _, g_after, _ in pairs:
            y = int(y)
            worst = max(worst, abs(want[at[(int(svcs["path_id"][y]), int(svcs["slot"][y]))], 0] - g_after))
            pairs_seen += 1
    print(f"{key}: {accepted} accepted, {qualified} released nothing, {pairs_seen} pairs, largest difference {worst:.2e} dB, "
          f"{newly_total} newly below = the oracle's disrupted increase")
    assert qualified >= 2 and pairs_seen > 50
    assert worst <= 1e-12
    assert newly_total > 0 or not kw.get("measure_disruptions")


@pytest.mark.parametrize("key", [k for k in CASES if not k.startswith("ids_")])
def test_restated_pairs_near_a_limit_for_the_seeds_of_the_gpu_cases(key):
    """what the restatement alone puts inside the band where the GPU test may leave a count out: within the cap for the seeds
    used (ids_nsfnet_320 needs the device's service ids); and the disruption case is not trivial"""
    B = REPLICAS.get(key, 3)
    tb, kw, holder, oracles = drive(key, B, SEED)
    n_pairs = n_band = 0
    newly, seen = [], set()
    for o in oracles:
        svcs = o.services()
        svcs = svcs[insertion_order(svcs)]
        actions = candidate_actions(o, tb, holder, oracle_block_row(o, tb, holder))
        status, pairs = restate_replica(o, tb, holder, svcs, actions)
        seen |= set(status.tolist())
        rows = rows_from_pairs(len(actions), status, pairs, np.arange(len(svcs)), kw["margin"])
        compare_rows(rows, rows)
        n_pairs += len(pairs)
        n_band += int(in_band(pairs, kw["margin"]).sum())
        newly.append(rows[status == 0][:, COLS["newly_below_minimum"]])
    newly = np.concatenate(newly)
    print(f"{key}: {n_pairs} pairs, {n_band} in the band, {len(newly)} evaluated actions, {int(np.sum(newly > 0))} newly below")
    assert seen == {0, 1, 2}
    assert n_pairs > 0 and n_band <= BAND_CAP * n_pairs
    if key.startswith("disr_"):
        assert np.any(newly > 0) and np.any(newly == 0)


def test_decode_follows_the_step():
    tb, kw, holder, (o,) = drive("ff_nsfnet_320", 1, SEED)
    ff = o.policy_first_fit()[0]
    st, path, slot, n, m = decode(o, tb, holder, ff)
    assert st == 0 and o.is_path_free(path, slot, n)
    assert decode(o, tb, holder, -1)[0] == 1 and decode(o, tb, holder, o.reject_action)[0] == 1
    assert decode(o, tb, holder, o.reject_action + 5)[0] == 1
    _, rec = o.step(int(ff))
    assert rec["accepted"] and rec["slot"] == slot and rec["nslots"] == n and rec["modulation"] == m
