"""Block action space (ongym_observe_blocks through BatchedQRMSAEnv.observe_blocks / decode_block_actions, QRMSABlockVecEnv).
Every GPU computation runs in ONE fresh child process (tests/blocks_child.py); the tests assert on the .npz it writes.

The numpy restatement of the definition (include/ongym.h, ongym_observe_blocks) lives here; the child uses its block lists
only to ask the device's calculate_osnr query (gsnr_many, pinned to the oracle elsewhere) for the GSNR of every block start."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import load_traj
from optical_networking_gym import _native as nat

pytestmark = pytest.mark.gpu

TRAJ = ("traj_nsfnet320", "traj_cost239", "traj_nobeleu320", "traj_nsfnet768", "traj_nsfnet320_cont", "traj_ring4")
TRAJ_BLOCKS = (1, 4)
STATES = (("nsfnet", 320, 1), ("nsfnet", 320, 2), ("nobel-eu", 320, 1), ("nobel-eu", 320, 3), ("nsfnet", 768, 1))
STATE_BLOCKS = (1, 3, 8, 16)
GSNR_RTOL = 1e-9


# ---- the definition, restated -------------------------------------------------------------------------------------------
def free_runs(row):
    """maximal runs of free slots of a row: [(a, L)] in increasing a"""
    x = np.diff(np.concatenate(([0], (np.asarray(row) != 0).astype(np.int8), [0])))
    a, e = np.flatnonzero(x == 1), np.flatnonzero(x == -1)
    return list(zip(a.tolist(), (e - a).tolist()))


def fitting_blocks(row, n):
    """the free runs that hold a candidate of _get_candidates for n slots: L >= n at the row's end, else L >= n + 1"""
    S = len(row)
    return [(a, L) for a, L in free_runs(row) if (L >= n if a + L == S else L >= n + 1)]


def route_row(grid, path_links, path_hops, path):
    return np.logical_and.reduce(grid[path_links[path, :path_hops[path]]], axis=0)


def slots_needed(bit_rate, se, width):
    """get_number_slots as the step computes it (the request's float32 bit rate in double)"""
    return int(np.ceil(float(np.float32(bit_rate)) / (float(se) * float(width))))


def restate(cfg, grid, req, J, gsnr):
    """(obs[3 + K:], mask, action_map, near) of one replica; gsnr[(path, a, n)] = GSNR dB; near = decisions within 1e-9 dB"""
    K, M, S = cfg["K"], cfg["M"], cfg["S"]
    reject = K * M * S
    feat = np.full(2 * K + 6 * K * J, -1.0, np.float32)
    mask = np.zeros(K * J + 1, np.uint8)
    amap = np.full(K * J + 1, reject, np.int32)
    mask[-1] = 1
    for i in range(K * J):
        feat[2 * K + 6 * i] = 0.0
    near = 0
    if not req["have"]:
        return feat, mask, amap, near
    src, dst = int(req["source"]), int(req["destination"])
    n = [slots_needed(req["bit_rate"], cfg["se"][m], cfg["width"]) for m in range(M)]
    for k in range(K):
        path = int(cfg["pair_paths"][src, dst, k])
        if path < 0:
            continue
        row = route_row(grid, cfg["path_links"], cfg["path_hops"], path)
        runs = free_runs(row)
        feat[2 * k] = np.float32(int(row.sum()) / S)
        feat[2 * k + 1] = np.float32(max([L for _, L in runs], default=0) / S)
        blocks = [fitting_blocks(row, n[m])[:J] if n[m] > 0 else [] for m in range(M)]
        for j in range(J):
            for m in range(M - 1, -1, -1):
                if len(blocks[m]) <= j:
                    continue
                a, L = blocks[m][j]
                g = gsnr[(path, a, n[m])]
                lim = cfg["thr"][m] + cfg["margin"]
                near += abs(g - lim) < 1e-9
                if g >= lim:
                    i = k * J + j
                    f = feat[2 * K + 6 * i: 2 * K + 6 * i + 6]
                    f[:5] = np.float32(1.0), np.float32(a / S), np.float32(L / S), np.float32(n[m] / S), np.float32((m + 1) / M)
                    f[5] = np.float32((g - cfg["thr"][m] - cfg["margin"]) / 10.0)
                    mask[i] = 1
                    amap[i] = k * M * S + (M - 1 - m) * S + a
                    break
    return feat, mask, amap, near


def block_candidates(cfg, grid, req):
    """every (path, a, n) the restatement may evaluate: the first 16 fitting blocks of every route and format"""
    out = set()
    src, dst = int(req["source"]), int(req["destination"])
    for k in range(cfg["K"]):
        path = int(cfg["pair_paths"][src, dst, k])
        if path < 0:
            continue
        row = route_row(grid, cfg["path_links"], cfg["path_hops"], path)
        for m in range(cfg["M"]):
            n = slots_needed(req["bit_rate"], cfg["se"][m], cfg["width"])
            if n > 0:
                out.update((path, a, n) for a, _ in fitting_blocks(row, n)[:nat.MAX_BLOCKS])
    return sorted(out)


# ---- the child's results ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("blocks") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "blocks_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "blocks child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def assert_golden_by_actions(rec, d, ctx=""):
    """assert_golden of test_gpu_state.py for records of action steps: the blocked-resource / blocked-OSNR bits describe the
    heuristic's search, which an action step does not make, so they are compared where the golden step accepted (both 0)"""
    for f, g in (("action", "st_action"), ("accepted", "st_accepted"), ("terminated", "st_term"), ("reward", "st_reward"),
                 ("active", "st_active"), ("route", "st_route"), ("slot", "st_slot")):
        assert np.array_equal(rec[f], d[g]), (ctx, f, np.flatnonzero(rec[f] != d[g])[:5])
    acc = d["st_accepted"] == 1
    assert np.array_equal(rec["modulation"][acc], d["st_mod"][acc]), ctx
    assert np.array_equal(rec["nslots"][acc], d["st_n"][acc]), ctx
    assert not np.any(rec["flags"][acc] & (nat.F_BLOCKED_RESOURCES | nat.F_BLOCKED_OSNR | nat.F_QOT_ERROR)), ctx
    assert not np.any(rec["retry"]), ctx
    for f, g in (("osnr", "st_osnr"), ("ase", "st_ase"), ("nli", "st_nli")):
        want = d[g]
        known = np.isfinite(want)
        np.testing.assert_allclose(rec[f][known], want[known], rtol=GSNR_RTOL, err_msg=f"{ctx}: {f}")


@pytest.mark.parametrize("tag", TRAJ)
@pytest.mark.parametrize("J", TRAJ_BLOCKS)
def test_block_actions_replay_the_reference_first_fit(res, tag, J):
    """the smallest route whose block 0 is valid, decoded through the action map, is the reference's first-fit action"""
    _, d = load_traj(tag)
    rec = res[f"traj_{tag}_J{J}"].view(nat.STEP_DTYPE)[:, 0]
    assert_golden_by_actions(rec, d, ctx=f"{tag} J={J}")
    assert int(res[f"traj_{tag}_J{J}_valid"]) > 0


def _state_cfg(res, key):
    cfg = {k[len(key) + 5:]: res[k] for k in res if k.startswith(key + "_cfg_")}
    for k in ("K", "M", "S"):
        cfg[k] = int(cfg[k])
    cfg["width"], cfg["margin"] = float(cfg["width"]), float(cfg["margin"])
    return cfg


@pytest.mark.parametrize("topo,S,seed", STATES)
def test_blocks_equal_the_restated_definition(res, topo, S, seed):
    key = f"st_{topo}_{S}_{seed}"
    cfg = _state_cfg(res, key)
    grids, reqs = res[key + "_grids"], res[key + "_reqs"]
    cand, g = res[key + "_cand"], res[key + "_gsnr"]
    K = cfg["K"]
    near = valid = deep = 0
    for r in range(len(reqs)):
        sel = cand[:, 0] == r
        gsnr = {(int(p), int(a), int(n)): float(x) for (_, p, a, n), x in zip(cand[sel], g[sel])}
        for J in STATE_BLOCKS:
            obs, mask, amap = res[f"{key}_J{J}_obs"][r], res[f"{key}_J{J}_mask"][r], res[f"{key}_J{J}_map"][r]
            feat, wmask, wmap, nr = restate(cfg, grids[r], reqs[r], J, gsnr)
            near += nr
            ctx = f"{key} replica {r} J={J}"
            np.testing.assert_array_equal(mask, wmask, err_msg=ctx)
            np.testing.assert_array_equal(amap, wmap, err_msg=ctx)
            got = obs[3 + K:]
            m5 = np.zeros(len(got), bool)
            m5[2 * K + 5::6] = True
            assert np.array_equal(got[~m5].view(np.uint32), feat[~m5].view(np.uint32)), ctx
            np.testing.assert_allclose(got[m5], feat[m5], rtol=0, atol=1e-6, err_msg=ctx)
            valid += int(mask[:-1].sum())
            if J > 1:
                deep += int(mask[:-1].reshape(K, J)[:, 1:].sum())
    assert near == 0, f"{near} QoT decisions within 1e-9 dB of the threshold"
    assert valid > 0 and deep > 0                     # later blocks than the first are exercised


@pytest.mark.parametrize("topo,S,seed", STATES)
def test_header_equals_ongym_observe_on_device_states(res, topo, S, seed):
    key = f"st_{topo}_{S}_{seed}"
    K = int(res[key + "_cfg_K"])
    head = res[key + "_obs_head"]
    for J in STATE_BLOCKS:
        assert np.array_equal(res[f"{key}_J{J}_obs"][:, :3 + K].view(np.uint32), head.view(np.uint32)), J


def test_header_equals_ongym_observe_at_the_golden_observation(res):
    a, b = res["head_blocks"], res["head_observe"]
    assert a.shape == b.shape and a.shape[0] > 10
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_every_valid_block_action_is_accepted_as_decoded(res):
    checked = 0
    for r in res["fork_replicas"]:
        amap, mask = res[f"fork_{r}_map"], res[f"fork_{r}_mask"]
        rec = res[f"fork_{r}_rec"].view(nat.STEP_DTYPE)[:, 0]
        M, S = int(res["fork_M"]), int(res["fork_S"])
        nslots = res[f"fork_{r}_nslots"]
        assert mask[:-1].sum() > 1, r
        for i in range(len(amap)):
            x = rec[i]
            assert not x["retry"] and not (x["flags"] & nat.F_QOT_ERROR), (r, i)
            if mask[i] and i < len(amap) - 1:
                a = int(amap[i])
                assert x["accepted"] == 1, (r, i)
                assert (x["route"], x["modulation"], x["slot"], x["nslots"]) == \
                    (a // (M * S), M - 1 - (a // S) % M, a % S, nslots[i]), (r, i)
                checked += 1
            else:
                assert x["accepted"] == 0 and x["action"] == int(res["fork_reject"]), (r, i)
    assert checked >= 3


def test_observe_blocks_is_read_only(res):
    assert res["ro_blob_same"] and res["ro_stats_same"] and res["ro_traj_same"]


def test_device_io_runs_on_the_current_stream_and_equals_the_host_path(res):
    assert res["dev_obs_same"] and res["dev_mask_same"] and res["dev_map_same"] and res["dev_rec_same"]
    assert int(res["dev_accepted"]) > 0
    assert res["dev_stream_refused"]


def test_block_vec_env(res):
    assert tuple(res["vec_obs_shape"]) == (64, 3 + 3 * 5 + 6 * 5 * 8) and tuple(res["vec_mask_shape"]) == (64, 41)
    assert int(res["vec_n_actions"]) == 41 and int(res["vec_obs_dim"]) == 3 + 3 * 5 + 6 * 5 * 8
    assert int(res["vec_qot"]) == 0 and int(res["vec_retry"]) == 0
    assert int(res["vec_episodes"]) > 0 and int(res["vec_accepted"]) > 0 and int(res["vec_deep"]) > 0


def test_refusals(res):
    assert int(res["refuse_mtc_rc"]) == -1 and "format window" in str(res["refuse_mtc_msg"])
    assert int(res["refuse_j0_rc"]) == -1 and int(res["refuse_j17_rc"]) == -1
