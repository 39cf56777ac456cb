"""The block action space without a GPU: ongym_observe_blocks is declared with its exact parameter list, exported and typed;
BatchedQRMSAEnv.observe_blocks checks every argument before it calls the library; decode_block_actions is one gather; and the
numpy restatement of the definition used by tests/test_gpu_blocks.py holds on hand-made rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from optical_networking_gym import _native as nat
from optical_networking_gym import rl
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from test_gpu_blocks import fitting_blocks, free_runs, restate

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()


def test_header_declares_observe_blocks():
    m = re.search(r"int ongym_observe_blocks\s*\(([^)]*)\);", HEADER)
    assert m
    assert " ".join(m.group(1).split()) == "ongym_env *env, int32_t blocks, float *obs, uint8_t *mask, int32_t *action_map"
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4
    assert nat.MAX_BLOCKS == 16


def test_library_exports_and_native_declares_it():
    lib = nat.load_library()
    assert "ongym_observe_blocks" in nat.EXPORTED_SYMBOLS
    f = lib.ongym_observe_blocks
    assert f.restype is ctypes.c_int32
    assert f.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.ongym_observe_blocks(None, 4, None, None, None) == -1


class _StubLib:
    """records ongym_observe_blocks calls"""
    def __init__(self):
        self.calls = []

    def ongym_observe_blocks(self, h, J, *ptrs):
        self.calls.append(J)
        return 0


def _env(io_device, B=4):
    env = object.__new__(BatchedQRMSAEnv)
    env.holder = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                                  io_device=io_device)
    env.batch_size, env.lib, env._h, env.stream_handle = B, _StubLib(), None, None
    return env


def test_blocks_out_of_range_are_refused_before_the_library():
    env = _env(False)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="blocks"):
            env.observe_blocks(bad)
    with pytest.raises(ValueError, match="out"):
        env.observe_blocks(4, out=(None, None, None))
    assert env.lib.calls == []
    obs, mask, amap = env.observe_blocks(4)
    K = env.holder.struct.k_paths
    assert obs.shape == (4, 3 + 3 * K + 24 * K) and obs.dtype == np.float32
    assert mask.shape == amap.shape == (4, 4 * K + 1) and mask.dtype == np.uint8 and amap.dtype == np.int32
    assert env.lib.calls == [4]


@pytest.fixture
def on_cpu(monkeypatch):
    monkeypatch.setattr(rl, "_device", lambda env: torch.device("cpu"))


def _tensors(B, K, J):
    n = K * J + 1
    return (torch.zeros((B, 3 + 3 * K + 6 * K * J), dtype=torch.float32), torch.zeros((B, n), dtype=torch.uint8),
            torch.zeros((B, n), dtype=torch.int32))


def test_device_environment_checks_its_tensors_then_the_stream(on_cpu):
    env = _env(True)
    K, J = env.holder.struct.k_paths, 8
    with pytest.raises(ValueError, match="out="):
        env.observe_blocks(J)
    with pytest.raises(ValueError, match="blocks"):
        env.observe_blocks(0, out=_tensors(4, K, J))
    good = _tensors(4, K, J)
    with pytest.raises(ValueError, match="tuple"):
        env.observe_blocks(J, out=good[:2])
    for i, name in enumerate(("obs", "mask", "action_map")):
        t = list(good)
        t[i] = good[i].to(torch.float64 if i != 0 else torch.float16)                 # dtype
        with pytest.raises(ValueError, match=name):
            env.observe_blocks(J, out=tuple(t))
        t[i] = good[i][:3]                                                             # shape
        with pytest.raises(ValueError, match=name):
            env.observe_blocks(J, out=tuple(t))
        t[i] = torch.zeros((good[i].shape[1], 4), dtype=good[i].dtype).t()           # not contiguous
        with pytest.raises(ValueError, match=name):
            env.observe_blocks(J, out=tuple(t))
        t[i] = good[i].numpy()                                                         # not a tensor
        with pytest.raises(ValueError, match=name):
            env.observe_blocks(J, out=tuple(t))
        flat = torch.zeros(good[i].numel() + 4, dtype=good[i].dtype)
        if good[i].dtype == torch.uint8:                                               # alignment
            t[i] = flat[1:1 + good[i].numel()].view(good[i].shape)
            with pytest.raises(ValueError, match="aligned"):
                env.observe_blocks(J, out=tuple(t))
    with pytest.raises(ValueError, match="stream"):                                    # all right: the stream is checked last
        env.observe_blocks(J, out=good)
    assert env.lib.calls == []


def test_device_environment_refuses_tensors_on_another_device(monkeypatch):
    monkeypatch.setattr(rl, "_device", lambda env: torch.device("meta"))
    env = _env(True)
    with pytest.raises(ValueError, match="obs"):
        env.observe_blocks(8, out=_tensors(4, env.holder.struct.k_paths, 8))
    assert env.lib.calls == []


def test_decode_block_actions_is_a_gather():
    amap = np.array([[5, 7, 9, 100], [11, 100, 100, 100]], np.int32)
    out = BatchedQRMSAEnv.decode_block_actions(np.array([2, 0]), amap)
    assert out.dtype == np.int32 and out.tolist() == [9, 11]
    with pytest.raises(ValueError):
        BatchedQRMSAEnv.decode_block_actions(np.array([4, 0]), amap)
    with pytest.raises(ValueError):
        BatchedQRMSAEnv.decode_block_actions(np.array([0]), amap)
    t = BatchedQRMSAEnv.decode_block_actions(torch.tensor([3, 1]), torch.from_numpy(amap))
    assert t.dtype == torch.int32 and t.tolist() == [100, 100]


def test_fitting_blocks_apply_the_guard_slot_except_at_the_row_end():
    row = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1], np.int8)
    assert free_runs(row) == [(0, 2), (3, 3), (7, 2)]
    assert fitting_blocks(row, 1) == [(0, 2), (3, 3), (7, 2)]
    assert fitting_blocks(row, 2) == [(3, 3), (7, 2)]          # [0, 2) would need its guard slot; the last run ends at S
    assert fitting_blocks(row, 3) == []


def test_restatement_decodes_best_format_first_and_falls_back():
    # route 0 of two links over S = 12 slots (route 1 absent), two formats: m = 1 needs 2 slots, m = 0 needs 4
    cfg = dict(K=2, M=2, S=12, pair_paths=np.array([[[-1, -1], [0, -1]], [[-1, -1], [-1, -1]]]),
               path_links=np.array([[0, 1]]), path_hops=np.array([2]), se=np.array([1, 2]), thr=np.array([3.0, 10.0]),
               width=25.0, margin=0.5)
    grid = np.ones((2, 12), np.int8)
    grid[0, 5] = 0                                             # free runs [0, 5) and [6, 12)
    req = dict(source=0, destination=1, bit_rate=np.float32(100.0), have=True)
    gsnr = {(0, 0, 2): 12.0, (0, 6, 2): 9.0, (0, 0, 4): 2.0, (0, 6, 4): 9.0}
    feat, mask, amap, near = restate(cfg, grid, req, 2, gsnr)
    assert mask.tolist() == [1, 1, 0, 0, 1] and near == 0
    assert amap.tolist() == [0, 1 * 12 + 6, 48, 48, 48]        # block 1 fails at 2 slots and falls back to the 4-slot format
    assert feat[:4].tolist() == [np.float32(11 / 12), np.float32(6 / 12), -1.0, -1.0]
    assert feat[4:10].tolist() == pytest.approx([1, 0, 5 / 12, 2 / 12, 1.0, (12 - 10 - 0.5) / 10])
    assert feat[10:16].tolist() == pytest.approx([1, 6 / 12, 6 / 12, 4 / 12, 0.5, (9 - 3 - 0.5) / 10])
    assert feat[16:].tolist() == [0, -1, -1, -1, -1, -1] * 2
