"""Link metrics without a GPU: ongym_link_metrics is declared with its exact parameter list, exported and typed;
BatchedQRMSAEnv.link_metrics checks every argument before it calls the library; and the numpy restatement used by
tests/test_gpu_link_metrics.py holds on hand-made rows and, replayed on the CPU oracle, equals the reference's fixture."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from common import GOLDEN, golden_tables, holder_for, traj_requests
from optical_networking_gym import _native as nat
from optical_networking_gym import rl
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from oracle_lib import OracleEnv
from test_gpu_link_metrics import (edge_index, linkstats_meta, restate_compactness, restate_link, restate_link_stats,
                                   runs)

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()


def test_header_declares_link_metrics():
    m = re.search(r"int ongym_link_metrics\s*\(([^)]*)\);", HEADER)
    assert m
    assert " ".join(m.group(1).split()) == "ongym_env *env, float *link_out, double *compactness, double *link_stats"
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4
    assert nat.LINK_METRICS == ("free_slots", "free_blocks", "largest_free_block", "used_blocks", "occupied_span",
                                "external_fragmentation", "entropy", "rss")
    assert nat.LINK_STATS == ("utilization", "external_fragmentation", "compactness", "last_update")


def test_library_exports_and_native_declares_it():
    lib = nat.load_library()
    assert "ongym_link_metrics" in nat.EXPORTED_SYMBOLS
    f = lib.ongym_link_metrics
    assert f.restype is ctypes.c_int32
    assert f.argtypes == [ctypes.c_void_p] * 4
    assert lib.ongym_link_metrics(None, None, None, None) == -1


class _StubLib:
    """records ongym_link_metrics calls"""
    def __init__(self):
        self.calls = []

    def ongym_link_metrics(self, h, link, comp, stats):
        self.calls.append(stats is not None)
        return 0


def _env(io_device, B=4):
    env = object.__new__(BatchedQRMSAEnv)
    env.holder = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                                  io_device=io_device)
    env.batch_size, env.lib, env._h, env.stream_handle = B, _StubLib(), None, None
    return env


def test_host_environment_checks_link_stats_before_the_library():
    env = _env(False)
    E = env.holder.struct.n_links
    for bad in (np.zeros((4, E, 4), np.float32), np.zeros((4, E, 3)), np.zeros((3, E, 4)), np.zeros((4, E, 8))[..., :4],
                torch.zeros((4, E, 4), dtype=torch.float64), [[0.0] * 4] * E):
        with pytest.raises(ValueError, match="link_stats"):
            env.link_metrics(link_stats=bad)
    ro = np.zeros((4, E, 4))
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="link_stats"):
        env.link_metrics(link_stats=ro)
    with pytest.raises(ValueError, match="out"):
        env.link_metrics(out=(None, None))
    assert env.lib.calls == []
    link, comp = env.link_metrics()
    assert link.shape == (4, E, 8) and link.dtype == np.float32 and comp.shape == (4,) and comp.dtype == np.float64
    env.link_metrics(link_stats=np.zeros((4, E, 4)))
    assert env.lib.calls == [False, True]


@pytest.fixture
def on_cpu(monkeypatch):
    monkeypatch.setattr(rl, "_device", lambda env: torch.device("cpu"))


def _tensors(B, E):
    return (torch.zeros((B, E, 8), dtype=torch.float32), torch.zeros((B,), dtype=torch.float64),
            torch.zeros((B, E, 4), dtype=torch.float64))


def test_device_environment_checks_its_tensors_then_the_stream(on_cpu):
    env = _env(True)
    E = env.holder.struct.n_links
    with pytest.raises(ValueError, match="out="):
        env.link_metrics()
    good = _tensors(4, E)
    with pytest.raises(ValueError, match="tuple"):
        env.link_metrics(out=good[:1])
    for i, name in enumerate(("link", "compactness", "link_stats")):
        t = list(good)
        t[i] = good[i].to(torch.float32 if i else torch.float64)                       # dtype
        with pytest.raises(ValueError, match=name):
            env.link_metrics(out=tuple(t[:2]), link_stats=t[2])
        t[i] = good[i][:3]                                                             # shape
        with pytest.raises(ValueError, match=name):
            env.link_metrics(out=tuple(t[:2]), link_stats=t[2])
        if good[i].dim() > 1:                                                          # not contiguous
            t[i] = good[i].transpose(0, 1).contiguous().transpose(0, 1)
            with pytest.raises(ValueError, match=name):
                env.link_metrics(out=tuple(t[:2]), link_stats=t[2])
        t[i] = good[i].numpy()                                                         # not a tensor
        with pytest.raises(ValueError, match=name):
            env.link_metrics(out=tuple(t[:2]), link_stats=t[2])
    with pytest.raises(ValueError, match="stream"):                                    # all right: the stream is checked last
        env.link_metrics(out=good[:2], link_stats=good[2])
    with pytest.raises(ValueError, match="stream"):
        env.link_metrics(out=good[:2])
    assert env.lib.calls == []


def test_device_environment_refuses_tensors_on_another_device(monkeypatch):
    monkeypatch.setattr(rl, "_device", lambda env: torch.device("meta"))
    env = _env(True)
    t = _tensors(4, env.holder.struct.n_links)
    with pytest.raises(ValueError, match="link"):
        env.link_metrics(out=t[:2], link_stats=t[2])
    assert env.lib.calls == []


# ---- the restatement on hand-made rows ----------------------------------------------------------------------------------
def _row(s):
    return np.array([int(c) for c in s], np.int8)


def test_runs_split_a_row_into_free_and_used_runs():
    assert runs(_row("1100111001")) == ([(0, 2), (4, 3), (9, 1)], [(2, 2), (7, 2)])
    assert runs(_row("0000")) == ([], [(0, 4)])
    assert runs(_row("1111")) == ([(0, 4)], [])


def test_link_features_on_hand_made_rows():
    S = 100
    free = restate_link(np.ones(S, np.int8))
    assert free.tolist() == [S, 1, S, 0, 0, 0.0, 0.0, 1.0]
    full = restate_link(np.zeros(S, np.int8))
    assert full.tolist() == [0, 0, 0, 1, S, 0.0, 0.0, 0.0]
    alt = restate_link(np.tile(np.array([1, 0], np.int8), S // 2))          # 50 free runs of 1, 50 used runs of 1
    assert alt[:5].tolist() == [50, 50, 1, 50, 99]
    assert alt[5] == pytest.approx(1 - 1 / 50) and alt[6] == pytest.approx(-50 * 0.01 * np.log(0.01))
    assert alt[7] == pytest.approx(np.sqrt(50) / 50)
    ends = np.zeros(S, np.int8)
    ends[:10] = 1
    ends[70:] = 1                                                              # free [0, 10) and [70, 100), used [10, 70)
    f = restate_link(ends)
    assert f[:5].tolist() == [40, 2, 30, 1, 60]
    assert f[5] == pytest.approx(1 - 30 / 40)
    assert f[6] == pytest.approx(-(0.1 * np.log(0.1) + 0.3 * np.log(0.3)))
    assert f[7] == pytest.approx(np.sqrt(100 + 900) / 40)
    mid = 1 - ends                                                             # used at both ends, free [10, 70)
    assert restate_link(mid)[:5].tolist() == [60, 1, 60, 2, 100]


def test_network_compactness_on_hand_made_rows():
    g = np.array([_row("1100110011"), _row("0011111111"), _row("1111111111")])
    # link 0: used runs [2, 4) and [6, 8): span 6, one free run inside; the others have at most one used run
    assert restate_compactness(g, 12) == (6 / 12) * (3 / 1)
    assert restate_compactness(g[1:], 2) == 1.0


def test_accumulator_restatement_keeps_the_reference_quirks():
    S = 100
    idle = np.ones(S, np.int8)
    ls = np.zeros(4)
    restate_link_stats(ls, idle, 0.0)                                          # current_time 0: only divisions by 0
    assert ls[0] == 0.0 and np.isnan(ls[1]) and np.isnan(ls[2]) and ls[3] == 0.0
    ls = np.zeros(4)
    restate_link_stats(ls, idle, 5.0)                                          # idle link: 0 / 0 in the fragmentation term
    assert ls[0] == 0.0 and np.isnan(ls[1]) and ls[2] == 1.0 and ls[3] == 5.0
    ends = np.ones(S, np.int8)
    ends[10:70] = 0                                                            # exactly free-used-free: max_empty = 0
    ls = np.zeros(4)
    restate_link_stats(ls, ends, 2.0)
    assert ls.tolist() == [0.6, 1.0, 1.0, 2.0]
    two = np.ones(S, np.int8)
    two[10:20] = 0
    two[30:40] = 0                                                             # 3 free runs (10, 10, 60), 20 used in 2 runs
    ls = np.array([0.5, 0.25, 0.75, 1.0])
    restate_link_stats(ls, two, 4.0)
    assert ls[0] == (0.5 * 1.0 + 0.2 * 3.0) / 4.0
    assert ls[1] == (0.25 * 1.0 + (1.0 - 60 / 20) * 3.0) / 4.0                # negative, as in the reference
    assert ls[2] == (0.75 * 1.0 + ((30 / 20) * (1.0 / 2)) * 3.0) / 4.0
    full = np.zeros(S, np.int8)
    ls = np.zeros(4)
    restate_link_stats(ls, full, 1.0)
    assert ls.tolist() == [1.0, 1.0, 1.0, 1.0]


def test_accumulator_restatement_on_the_oracle_equals_the_reference_fixture():
    meta = linkstats_meta()
    d = np.load(os.path.join(GOLDEN, "linkstats_nsfnet320.npz"))
    checks = {c["step"]: c for c in meta["checks"]}
    orc = OracleEnv(holder_for(meta))
    orc.set_trace(traj_requests(d))
    assert int(np.sum(d["req_kind"] == 0)) == meta["initial_resets"]
    for _ in range(meta["initial_resets"]):
        orc.reset()
    idx = edge_index(golden_tables("nsfnet"), meta["edges"])
    ls = np.zeros((orc.cfg.n_links, 4))
    seen = 0
    for i, a in enumerate(d["st_action"]):
        orc.step(int(a))
        if i in checks:
            now = float(orc.stats()["current_time"])
            assert now == checks[i]["current_time"]
            grid = orc.grid()
            for e in range(orc.cfg.n_links):
                restate_link_stats(ls[e], grid[e], now)
            want = np.array(checks[i]["links"], np.float64)
            assert np.array_equal(np.isnan(ls[idx]), np.isnan(want)), i
            np.testing.assert_allclose(ls[idx], want, rtol=1e-12, atol=1e-15, err_msg=str(i))
            seen += 1
    assert seen == len(checks) == 3
    assert np.any(ls[:, 1] < 0)                        # the fixture holds the reference's negative fragmentation values
