"""Per-link spectrum fragmentation metrics (ongym_link_metrics through BatchedQRMSAEnv.link_metrics).  Every GPU computation runs
in ONE fresh child process (tests/link_metrics_child.py); the tests assert on the .npz it writes.

The numpy restatement of the definitions (include/ongym.h, ongym_link_metrics) lives here: the link features on the free runs
of a row, _get_network_compactness (qrmsa.pyx:1150-1186) and _update_link_stats (qrmsa.pyx:1353-1480) with the reference's
arithmetic.  tests/test_link_metrics_host.py pins the last one to the reference's fixture on the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from common import GOLDEN

pytestmark = pytest.mark.gpu

# (topology, S, stepping) of the definition states: S = 768 has 12 row words, 160 and 100 a partial last word; nobel-eu (41
# links) and germany50 (88 links: a second pass of the lanes) use the generic record codec
STATES = (("nsfnet", 320, "p0"), ("cost239", 320, "p0"), ("nobel-eu", 320, "p0"), ("nsfnet", 768, "p0"), ("nsfnet", 160, "p0"),
          ("germany50", 100, "p0"), ("nsfnet", 320, "p1"), ("nsfnet", 320, "p10"), ("nsfnet", 320, "defrag"),
          ("nsfnet", 320, "random"))
ACC_STEPS, ACC_REPLICAS = 40, 8
LINKSTATS_STEPS = (60, 200, 419)


def linkstats_meta():
    """the fixture's metadata with the settings test_gpu_compat.py::test_link_statistics_like_the_reference builds its env with;
    the trace's first two requests (req_kind 0) are drawn by the constructor's reset and env.reset()"""
    meta = json.load(open(os.path.join(GOLDEN, "linkstats_nsfnet320.json")))
    return dict(meta, mean_holding=10800.0, bit_rate_selection="discrete", launch_power_dbm=0.0, frequency_start=3e8 / 1565e-9,
                slot_bw=12.5e9, margin=0.0, k_paths=5, initial_resets=2)


def edge_index(tables, edges):
    """table link index of every fixture edge (node names)"""
    names = list(tables.node_names)
    by = {}
    for e, (u, v) in enumerate(tables.link_nodes):
        by[(names[u], names[v])] = by[(names[v], names[u])] = e
    return np.array([by[(str(u), str(v))] for u, v in edges])


# ---- the definitions, restated ------------------------------------------------------------------------------------------
def runs(row):
    """(free runs, used runs) of a row (1 = free) as lists of (start, length), in increasing start"""
    f = (np.asarray(row) != 0).astype(np.int8)
    out = []
    for v in (f, 1 - f):
        x = np.diff(np.concatenate(([0], v, [0])))
        a, e = np.flatnonzero(x == 1), np.flatnonzero(x == -1)
        out.append(list(zip(a.tolist(), (e - a).tolist())))
    return out[0], out[1]


def restate_link(row):
    """the eight link features (nat.LINK_METRICS) of one row, in float64"""
    S = len(row)
    free, used = runs(row)
    F = sum(L for _, L in free)
    lmax = max((L for _, L in free), default=0)
    span = used[-1][0] + used[-1][1] - used[0][0] if used else 0
    p = np.array([L / S for _, L in free], np.float64)
    ent = float(-np.sum(p * np.log(p))) if len(p) else 0.0
    rss = float(np.sqrt(sum(L * L for _, L in free)) / F) if F else 0.0
    return np.array([F, len(free), lmax, len(used), span, 1.0 - lmax / F if F else 0.0, ent, rss], np.float64)


def restate_compactness(grid, slot_hops):
    """_get_network_compactness: (occupied / slot_hops) * (E / inner free runs), over links with more than one used run"""
    occupied = inner = 0
    for row in grid:
        free, used = runs(row)
        if len(used) > 1:
            lo, hi = used[0][0], used[-1][0] + used[-1][1]
            occupied += hi - lo
            inner += sum(1 for a, L in free if a >= lo and a + L <= hi)
    return (occupied / slot_hops) * (len(grid) / inner) if inner else 1.0


def restate_link_stats(ls, row, now):
    """_update_link_stats of one link at time `now`, in place on ls = (utilization, external_fragmentation, compactness,
    last_update), with the reference's arithmetic and quirks"""
    S = len(row)
    free, used = runs(row)
    F = sum(L for _, L in free)
    util, frag, comp, last = (float(x) for x in ls)
    now = float(now)
    dt = now - last
    if now > 0:
        util = ((util * last) + (((S - F) / S) * dt)) / now
    ends_only = len(free) == 2 and row[0] != 0 and row[-1] != 0
    max_empty = max(L for _, L in free) if len(free) > 1 and not ends_only else 0
    with np.errstate(divide="ignore", invalid="ignore"):
        cf = float(1.0 - np.float64(max_empty) / np.float64(S - F)) if F > 0 else 1.0
        cc = 1.0
        if len(used) > 1:
            cc = ((used[-1][0] + used[-1][1] - used[0][0]) / (S - F)) * (1.0 / len(used))
        frag = float((np.float64(frag * last) + np.float64(cf * dt)) / np.float64(now))
        comp = float((np.float64(comp * last) + np.float64(cc * dt)) / np.float64(now))
    ls[:] = util, frag, comp, now
    return ls


def assert_stats_close(got, want, ctx=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), ctx
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15, err_msg=ctx)


# ---- the child's results ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("link_metrics") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_metrics_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "link metrics child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def test_link_stats_equal_the_reference_fixture(res):
    meta = linkstats_meta()
    checks = {c["step"]: c for c in meta["checks"]}
    idx = res["pin_edge_index"]
    for i in LINKSTATS_STEPS:
        ls = res[f"pin_{i}"]
        assert ls.shape[0] == 3
        want = np.array(checks[i]["links"], np.float64)
        for r in range(3):
            assert float(res[f"pin_{i}_time"][r]) == checks[i]["current_time"]
            assert_stats_close(ls[r][idx], want, ctx=f"step {i} replica {r}")


@pytest.mark.parametrize("topo,S,how", STATES)
def test_metrics_equal_the_restated_definition(res, topo, S, how):
    key = f"st_{topo}_{S}_{how}"
    grids, link, comp, hops = res[key + "_grids"], res[key + "_link"], res[key + "_comp"], res[key + "_hops"]
    B, E, _ = link.shape
    assert B == 256 and grids.shape == (B, E, S)
    fragmented = 0
    for r in range(B):
        want = np.stack([restate_link(row) for row in grids[r]])
        ctx = f"{key} replica {r}"
        np.testing.assert_array_equal(link[r][:, :5], want[:, :5].astype(np.float32), err_msg=ctx)
        np.testing.assert_allclose(link[r][:, 5:], want[:, 5:], rtol=1e-6, atol=1e-7, err_msg=ctx)
        assert comp[r] == restate_compactness(grids[r], int(hops[r])), ctx
        fragmented += int(np.sum(link[r][:, 1] > 1))
    assert fragmented > 0 and np.any(comp != 1.0)          # the states exercise multi-run rows and the compactness ratio


def test_accumulator_equals_the_restatement_at_every_step(res):
    grids, ls, times = res["acc_grids"], res["acc_stats"], res["acc_times"]
    T, R, E, S = grids.shape
    assert T == ACC_STEPS + 1 and R == ACC_REPLICAS
    want = np.zeros((R, E, 4), np.float64)
    for t in range(T):
        for r in range(R):
            for e in range(E):
                restate_link_stats(want[r, e], grids[t, r, e], times[t, r])
            assert_stats_close(ls[t, r], want[r], ctx=f"step {t} replica {r}")


def test_compat_env_agrees_with_its_host_methods(res):
    for i in LINKSTATS_STEPS:
        dev, host = res[f"compat_{i}_dev"], res[f"compat_{i}_host"]
        assert np.array_equal(dev, host, equal_nan=True), i
        assert float(res[f"compat_{i}_comp_dev"]) == float(res[f"compat_{i}_comp_host"]), i
    assert float(res[f"compat_{LINKSTATS_STEPS[-1]}_comp_host"]) != 1.0


def test_link_metrics_is_read_only(res):
    assert res["ro_blob_same"] and res["ro_stats_same"] and res["ro_traj_same"]


def test_empty_network_after_reset(res):
    link, comp, ls = res["empty_link"], res["empty_comp"], res["empty_stats"]
    S = int(res["empty_S"])
    want = np.array([S, 1, S, 0, 0, 0, 0, 1], np.float32)
    assert np.array_equal(link, np.broadcast_to(want, link.shape))
    assert np.all(comp == 1.0)
    # reset drew the first request, so current_time is its arrival (> 0): an idle link has utilization 0, fragmentation
    # 1 - 0/0 = NaN and compactness 1
    now = res["empty_time"]
    assert np.all(now > 0)
    assert np.all(ls[..., 0] == 0) and np.all(np.isnan(ls[..., 1])) and np.all(ls[..., 2] == 1.0)
    assert np.array_equal(ls[..., 3], np.broadcast_to(now[:, None], ls.shape[:2]))


def test_device_io_runs_on_the_current_stream_and_equals_the_host_path(res):
    assert res["dev_link_same"] and res["dev_comp_same"] and res["dev_stats_same"]
    assert res["dev_stream_refused"]


def test_refusals(res):
    assert int(res["refuse_null_rc"]) == -1 and "null" in str(res["refuse_null_msg"])
    assert res["refuse_dtype"] and res["refuse_shape"] and res["refuse_out"]
