"""Service QoT without a GPU: ongym_service_qot is declared with its exact parameter list, exported and typed;
BatchedQRMSAEnv.service_qot checks its arguments before it calls the library; and the interferer-list restatement that
tests/test_gpu_service_qot.py holds the device to equals, on the CPU oracle, the oracle's own step bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from oracle_lib import OracleEnv
from test_gpu_service_qot import insertion_order, interferer_lists, restate_aggregates, restate_gn

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()


def test_header_declares_service_qot():
    m = re.search(r"int ongym_service_qot\s*\(([^)]*)\);", HEADER)
    assert m
    assert " ".join(m.group(1).split()) == "ongym_env *env, double *svc_out, double *replica_out, float *link_out"
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4
    assert nat.SERVICE_QOT == ("gsnr", "ase", "nli", "margin")
    assert nat.REPLICA_QOT == ("running", "below_minimum", "below_margin", "lowest_margin", "mean_gsnr", "lowest_margin_index")
    assert nat.LINK_QOT == ("lightpaths", "lowest_margin", "below_minimum")


def test_library_exports_and_native_declares_it():
    lib = nat.load_library()
    assert "ongym_service_qot" in nat.EXPORTED_SYMBOLS
    f = lib.ongym_service_qot
    assert f.restype is ctypes.c_int32
    assert f.argtypes == [ctypes.c_void_p] * 4
    assert lib.ongym_service_qot(None, None, None, None) == -1


class _StubLib:
    """records ongym_service_qot calls"""
    def __init__(self):
        self.calls = []

    def ongym_service_qot(self, h, svc, rep, link):
        self.calls.append((svc is not None, rep is not None, link is not None))
        return 0


def _env(io_device, B=4):
    env = object.__new__(BatchedQRMSAEnv)
    env.holder = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                                  io_device=io_device)
    env.batch_size, env.lib, env._h, env.stream_handle = B, _StubLib(), None, None
    return env


def test_host_environment_returns_arrays_of_the_documented_shapes():
    env = _env(False)
    c = env.holder.struct
    svc, rep, link = env.service_qot()
    assert svc.shape == (4, c.capacity, 4) and svc.dtype == np.float64
    assert rep.shape == (4, 6) and rep.dtype == np.float64
    assert link.shape == (4, c.n_links, 3) and link.dtype == np.float32
    assert env.lib.calls == [(True, True, True)]
    with pytest.raises(ValueError, match="io_device"):
        env.service_qot(out=(svc, rep, link))
    assert len(env.lib.calls) == 1


def test_io_device_environment_checks_out_before_the_call():
    env = _env(True)
    c = env.holder.struct
    ok = (torch.empty((4, c.capacity, 4), dtype=torch.float64), torch.empty((4, 6), dtype=torch.float64),
          torch.empty((4, c.n_links, 3), dtype=torch.float32))
    for bad, match in ((None, "needs out"), (ok[:2], "tuple"), ((None, None, None), "at least one"),
                       ((ok[0].float(), None, None), "svc must be"), ((None, ok[1][:, :5].contiguous(), None), "replica must be"),
                       ((None, None, ok[2]), "link must be")):           # a host tensor: not on the environment's device
        with pytest.raises(ValueError, match=match):
            env.service_qot(out=bad)
    assert env.lib.calls == []


def _trace(tables, n, rng, holding=1.0e5):
    """requests one time unit or more apart that all outlive the trace: no departures, and the release times (arrival + one
    holding time) keep the provisioning order"""
    reqs = np.zeros(n, nat.REQUEST_DTYPE)
    reqs["arrival_time"] = np.cumsum(rng.uniform(1.0, 3.0, n)).astype(np.float32)
    reqs["holding_time"] = np.float32(holding)
    src = rng.integers(0, tables.n_nodes, n)
    reqs["source"], reqs["destination"] = src, (src + rng.integers(1, tables.n_nodes, n)) % tables.n_nodes
    reqs["bit_rate"] = rng.choice(np.array([10, 40, 100, 400]), n)
    return reqs


@pytest.mark.parametrize("topo,S,lp", [("nsfnet", 320, 1.0), ("nobel-eu", 160, 3.0), ("cost239", 100, -1.0)])
def test_restated_gsnr_of_a_new_service_equals_the_oracle_step_bit_for_bit(topo, S, lp):
    """every accepted request of a trace without departures: the restatement (itself left out, lists in the links' order)
    evaluated on the state right after the step gives the step record's GSNR / ASE / NLI bit for bit"""
    tb = golden_tables(topo)
    rng = np.random.default_rng(S)
    n = 260
    holder = nat.ConfigHolder(tb, modulations=jocn_modulations(), num_spectrum_resources=S, capacity=1024, load=300,
                              bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), episode_length=10 ** 6,
                              launch_power_dbm=lp, margin=0.0)
    o = OracleEnv(holder)
    o.set_trace(_trace(tb, n + 10, rng))
    o.reset()
    accepted = 0
    for _ in range(n):
        a, _, _ = o.policy_first_fit()
        rc, rec = o.step(a)
        assert rc == 0
        if not rec["accepted"]:
            continue
        svcs = o.services()
        svcs = svcs[insertion_order(svcs)]
        y = len(svcs) - 1                                   # the newest service is the last one provisioned
        assert svcs["slot"][y] == rec["slot"] and svcs["nslots"][y] == rec["nslots"]
        counts, intf = interferer_lists(tb, holder.mod_se, svcs, y)
        want = o.gn_lists(int(svcs["path_id"][y]), int(svcs["slot"][y]), int(svcs["nslots"][y]), counts, intf)
        assert want.tobytes() == np.array([rec["osnr"], rec["ase"], rec["nli"]]).tobytes(), accepted
        if accepted % 25 == 0:                              # restate_gn over the whole state agrees on it
            assert restate_gn(o, tb, holder.mod_se, svcs)[y].tobytes() == want.tobytes()
        accepted += 1
    assert accepted > 150


def test_interferer_lists_leave_out_the_service_and_its_namesakes():
    tb = golden_tables("nsfnet")
    svcs = np.zeros(4, nat.SERVICE_DTYPE)
    p = int(tb.pair_paths.reshape(-1)[0])
    svcs["path_id"] = p
    svcs["slot"] = [0, 10, 20, 30]
    svcs["nslots"] = [2, 3, 4, 5]
    svcs["modulation"] = [0, 1, 2, 3]
    se = [1, 2, 3, 4, 5, 6]
    counts, intf = interferer_lists(tb, se, svcs, 1)
    assert counts.tolist() == [3] * int(tb.path_hops[p])
    assert intf[:3].tolist() == [[0, 2, 1], [20, 4, 3], [30, 5, 4]]
    counts, intf = interferer_lists(tb, se, svcs, 1, ids=np.array([7, 8, 8, 9]))
    assert counts.tolist() == [2] * int(tb.path_hops[p])
    assert intf[:2].tolist() == [[0, 2, 1], [30, 5, 4]]


def test_aggregate_restatement_on_a_hand_made_replica():
    tb = golden_tables("nsfnet")
    p0, p1 = int(tb.pair_paths[0, 1, 0]), int(tb.pair_paths[2, 5, 0])
    svcs = np.zeros(3, nat.SERVICE_DTYPE)
    svcs["path_id"] = [p0, p1, p0]
    svcs["modulation"] = [0, 1, 0]
    thr = np.array([3.71, 6.72, 10.84, 13.24, 16.16, 19.01])
    svc = np.full((8, 4), np.nan)
    svc[:3, 0] = [3.5, 8.0, 3.9]
    svc[:3, 3] = svc[:3, 0] - thr[svcs["modulation"]]
    rep, link = restate_aggregates(svc, svcs, tb.path_links, tb.path_hops, thr, 0.5, tb.n_links)
    assert rep[[0, 1, 2, 5]].tolist() == [3, 1, 2, 0]
    assert rep[3] == pytest.approx(3.5 - 3.71) and rep[4] == pytest.approx((3.5 + 8.0 + 3.9) / 3)
    for l in tb.path_links[p0, :tb.path_hops[p0]]:
        assert link[l, 0] >= 2 and link[l, 2] >= 1 and link[l, 1] == pytest.approx(3.5 - 3.71)
    untouched = np.setdiff1d(np.arange(tb.n_links), np.concatenate([tb.path_links[p, :tb.path_hops[p]] for p in (p0, p1)]))
    assert np.all(link[untouched, 0] == 0) and np.all(np.isnan(link[untouched, 1]))
    rep, _ = restate_aggregates(svc, svcs[:0], tb.path_links, tb.path_hops, thr, 0.5, tb.n_links)
    assert rep[0] == 0 and np.isnan(rep[3]) and np.isnan(rep[4]) and rep[5] == -1
