"""Link failures on live replicas (ongym_cut_links, ongym_repair_links, ongym_failed_links through BatchedQRMSAEnv).  Every
GPU computation runs in ONE fresh child process (tests/link_cut_child.py); the tests assert on the .npz it writes.

The six configurations are those of tests/failure_impact_child.py.  Replica r's set is a node's links (r % 4 == 0), a dual
cut drawn with default_rng(300 + r) (1), the link most records cross (2) or the empty set (3).  The device is held to
expected_cut of the child, computed from the device's own services() and grid() before the cut: the post-cut records, grid,
index_out, svc_out and columns 0-8 and 10-12 exactly; lowest_margin, and under id tracking the Service.OSNR of a restored
record, at the tolerance tests/test_gpu_action_impact.py holds its dB columns to (rtol 1e-9 on the linear 1/GSNR, 4.4e-9 dB:
the device's sum order differs from the list order by a few ulp).  Exact counts need every decision to be the restatement's:
no evaluated (candidate, format) pair of a case may lie within 1e-8 relative of its limit, which the child counts on the
states it compares (and tests/test_link_cut_host.py on the CPU for the same seeds)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from failure_impact_child import CASES
from link_cut_child import BOTH, FIELDS, OSNR, TRAFFIC
from optical_networking_gym import _native as nat
from test_gpu_action_impact import DB_ATOL

pytestmark = pytest.mark.gpu
COLS = {k: i for i, k in enumerate(nat.CUT_LINKS)}
EXACT = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12]


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("link_cut") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_cut_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "link cut child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def compare_state(res, key, r, tag, cut, svc, index, ids):
    """the device's row, svc_out, index_out, records and grid of replica r against the restatement"""
    k, ctx = f"{key}_r{r}{tag}", f"{key} r{r}{tag}"
    want, act, idx, post, grid = (res[k + s] for s in ("_row", "_act", "_idx", "_post", "_grid"))
    n = len(act)
    assert np.array_equal(np.isnan(cut), np.isnan(want)), (ctx, cut, want)
    if want[0] == 1:
        assert cut[0] == 1 and np.all(np.isnan(cut[1:])), ctx
    else:
        assert np.array_equal(cut[EXACT], want[EXACT]), (ctx, cut, want)
        assert cut[1] == cut[3] + cut[5] + cut[6] + cut[12] and cut[10] <= cut[5], ctx
        if want[3] > 0:
            np.testing.assert_allclose(cut[9], want[9], rtol=0, atol=DB_ATOL, err_msg=ctx)
    assert np.array_equal(svc[:n], act) and np.all(svc[n:] == -1), ctx
    assert np.array_equal(index[:n], idx) and np.all(index[n:] == -1), ctx
    got_post, got_grid = res[k + "_got_post"], res[k + "_got_grid"]
    assert got_post.shape == post.shape, ctx
    rest = [i for i in range(len(FIELDS)) if i != OSNR]
    assert np.array_equal(got_post[:, rest], post[:, rest]), ctx
    new = np.zeros(len(post), bool)
    new[idx[(idx >= 0) & (act >= 0)]] = True                         # the restored victims
    assert np.array_equal(got_post[~new, OSNR], post[~new, OSNR]), ctx
    if ids:
        np.testing.assert_allclose(got_post[new, OSNR], post[new, OSNR], rtol=0, atol=DB_ATOL, err_msg=ctx)
    else:
        assert np.array_equal(got_post[new, OSNR], post[new, OSNR]), ctx
    assert np.array_equal(got_grid, grid), ctx
    return want


@pytest.mark.parametrize("key", CASES)
def test_the_state_after_the_cut_equals_the_restatement(res, key):
    """1: records, grid, index_out, svc_out and the row of every replica; the failed set is the cut set"""
    assert int(res[key + "_band"]) == 0                            # a condition of the exact comparison, not a tolerance
    B, ids = int(res[key + "_B"]), bool(res[key + "_ids"])
    victims = restored = 0
    for r in range(B):
        want = compare_state(res, key, r, "", res[key + "_cut"][r], res[key + "_svc"][r], res[key + "_index"][r], ids)
        if r % 4 == 3:
            assert want[0] == 1 and not np.any(res[key + "_failed"][r])
        else:
            assert want[0] == 0 and np.array_equal(res[key + "_failed"][r], res[key + "_W"][r])
            victims += int(want[1])
            restored += int(want[3])
        assert int(res[key + "_active_after"][r]) == len(res[f"{key}_r{r}_post"])
    print(f"{key}: {victims} victims, {restored} restored")
    assert victims > 0 and restored > 0
    if key == "nsfnet":
        assert res[key + "_rec32"]
    if key == "nobeleu":
        assert not res[key + "_rec32"] and int(res[key + "_E"]) > 32


def test_the_cases_together_exercise_every_condition(res):
    t = {n: sum(int(res[f"{key}_cond_{n}"]) for key in CASES)
         for n in ("evaluated", "no_victim", "restored", "lost_qot", "lost_ns_route", "no_route", "multi")}
    print(t)
    assert t["restored"] > 0 and t["lost_qot"] > 0 and t["lost_ns_route"] > 0 and t["no_route"] > 0 and t["multi"] > 0
    assert 4 * t["no_victim"] <= t["evaluated"]


@pytest.mark.parametrize("key", CASES)
def test_the_cut_reports_what_failure_sets_reports_on_a_twin(res, key):
    """2: columns 0-11 and svc_out are failure_sets' with F = 1 on the pre-cut state in a second environment"""
    cut, fs = res[key + "_cut"], res[key + "_fs"]
    exact = [c for c in range(12) if c != 9]
    assert np.array_equal(cut[:, exact], fs[:, exact], equal_nan=True)
    assert np.array_equal(np.isnan(cut[:, 9]), np.isnan(fs[:, 9]))
    some = ~np.isnan(fs[:, 9])
    assert some.any()
    np.testing.assert_allclose(cut[some, 9], fs[some, 9], rtol=0, atol=DB_ATOL)
    assert np.array_equal(res[key + "_svc"], res[key + "_fs_svc"])


@pytest.mark.parametrize("key", CASES)
def test_the_first_decision_on_the_degraded_network(res, key):
    """3: policy_actions(first fit) right after the cut equals first fit restated on the post-cut records, grid and request"""
    assert int(res[key + "_band"]) == 0
    assert np.array_equal(res[key + "_ff"], res[key + "_want_ff"]), (res[key + "_ff"], res[key + "_want_ff"])


@pytest.mark.parametrize("key", TRAFFIC)
def test_invariants_while_traffic_continues_and_after_the_repair(res, key):
    """4: six launches of 50 first-fit steps on the degraded network, the repair, 100 more steps"""
    assert np.all(res[key + "_run_steps"] == 300)
    assert res[key + "_run_grid_ok"].shape[0] == 6 and np.all(res[key + "_run_grid_ok"])
    assert np.all(res[key + "_run_cross"] == 0) and np.all(res[key + "_run_failed_same"])
    assert np.array_equal(res[key + "_repaired"], res[key + "_set_size"]) and int(res[key + "_set_size"].sum()) > 0
    assert res[key + "_rows_free"] and not np.any(res[key + "_failed_after_repair"])
    assert np.all(res[key + "_later_grid_ok"])
    print(key, "records on repaired links after 100 steps:", int(res[key + "_later_cross"]))
    assert int(res[key + "_later_cross"]) >= 1


@pytest.mark.parametrize("key", BOTH)
def test_both_step_kernels_agree_after_the_same_cut(res, key):
    """5: the lean and the generic kernel from the same seed, the same cut after the same launch, 250 recorded steps"""
    assert not res[f"{key}_both_lean1"]
    if key == "nsfnet":
        assert res[f"{key}_both_lean0"]
    assert res[key + "_both_same"] and res[key + "_both_failed_same"] and int(res[key + "_both_accepted"]) > 0
    a, b = res[key + "_both_osnr"]
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=0)


@pytest.mark.parametrize("key", CASES)
def test_statistics_and_untouched_replicas(res, key):
    """6: a status-1 replica keeps its bytes; no statistic but `active` moves (total_* included), and with ids
    episode_osnr_sum moves by the sum of new - old Service.OSNR over the restored"""
    B, ids = int(res[key + "_B"]), bool(res[key + "_ids"])
    same = res[key + "_noop_blob_same"]
    assert np.all(same[np.arange(B) % 4 == 3])
    assert res[key + "_stats_same"]
    before, after = res[key + "_osnr_sum"]
    if ids:
        assert np.any(res[key + "_osnr_delta"] != 0)
        np.testing.assert_allclose(after, before + res[key + "_osnr_delta"], rtol=1e-9, atol=0)
    else:
        assert np.array_equal(before, after)


def test_a_cut_without_victims_and_its_repair_give_the_start_back(res):
    """6: byte for byte; cutting a failed link again and repairing a healthy one change nothing"""
    assert np.all(res["noop_status"] == 0) and np.all(res["noop_victims"] == 0) and np.all(res["noop_again_victims"] == 0)
    assert res["noop_failed"] and np.all(res["noop_changed"]) and np.all(res["noop_recut_same"])
    assert np.all(res["noop_repaired"] == 1) and np.all(res["noop_back"])
    assert np.all(res["noop_repaired_twice"] == 0) and np.all(res["noop_still_back"])
    assert res["shared_same"] and int(res["shared_victims"]) > 0


def test_state_calls_carry_failures_and_a_reset_returns_the_fibre(res):
    """7"""
    assert res["state_failed_same"] and res["state_records_same"] and res["state_failed_kept"]
    assert res["fork_healthy_before"] and res["fork_copies"] and res["reset_clears"]


@pytest.mark.parametrize("key", CASES)
def test_without_restoration_every_victim_is_dropped(res, key):
    """8: restore=False"""
    B, ids = int(res[key + "_B"]), bool(res[key + "_ids"])
    cut, svc = res[key + "_nr_cut"], res[key + "_nr_svc"]
    dropped = 0
    for r in range(B):
        want = compare_state(res, key, r, "_nr", cut[r], svc[r], res[key + "_nr_index"][r], ids)
        if want[0] == 0:
            assert cut[r, 12] == cut[r, 1] == res[key + "_cut"][r, 1] and np.all(cut[r, 3:9] == 0) and cut[r, 10] == 0
            assert np.isnan(cut[r, 9])
            assert np.array_equal(res[key + "_nr_failed"][r], res[key + "_W"][r])
            dropped += int(cut[r, 12])
    assert dropped > 0
    reject = np.max(svc)
    assert np.all((svc == -1) | (svc == reject)) and int(np.sum(svc == reject)) == dropped


def test_device_io_on_the_current_stream_equals_the_host_path(res):
    """9"""
    assert res["dev_stream_refused"] and res["dev_same"] and res["dev_failed_same"] and res["dev_state_same"] and res["dev_repair_same"]
    assert np.all(res["dev_refusals"])


def test_library_refusals(res):
    """10"""
    for k in ("null_sets", "null_out", "flags", "repair_null_sets", "null_failed", "window", "pairs"):
        assert int(res["refuse_rc_" + k]) == -1, k
    for k in ("ok", "ok_shared", "ok_failed", "ok_repair"):
        assert int(res["refuse_rc_" + k]) == 0, (k, str(res["refuse_msg_" + k]))
    assert "sets" in str(res["refuse_msg_null_sets"]) and "sets" in str(res["refuse_msg_repair_null_sets"])
    assert "cut_out" in str(res["refuse_msg_null_out"]) and "failed_out" in str(res["refuse_msg_null_failed"])
    assert "flags" in str(res["refuse_msg_flags"])
    assert "modulations_to_consider" in str(res["refuse_msg_window"])
    assert "node pairs" in str(res["refuse_msg_pairs"])
    assert res["refuse_failed_between"][0, 0] == 1                   # link 0 was cut by the two accepted calls
