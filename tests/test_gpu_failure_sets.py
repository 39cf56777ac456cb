"""Failures of link sets and first-fit restoration (ongym_failure_sets through BatchedQRMSAEnv.failure_sets).  Every GPU
computation runs in ONE fresh child process (tests/failure_sets_child.py); the tests assert on the .npz it writes.

The six configurations are those of tests/failure_impact_child.py.  Replica r's list (per_replica = 1) is every node's link
set, up to 12 dual cuts drawn with default_rng(100 + r), the E one-link sets, the first node set once more, the empty set and
a set with bit E.  The device is held to restate_set of the child, computed from the device's own services() and grid() of
each replica: status, columns 1-8, 10 and 11 and svc_out exactly; lowest_margin at the tolerance tests/test_gpu_action_impact.py
holds its dB columns to (rtol 1e-9 on the linear 1/GSNR, 4.4e-9 dB: the device's sum order differs from the list order by a
few ulp).  Exact counts need every decision to be the restatement's: no evaluated (candidate, format) pair of a case may lie
within 1e-8 relative of its limit, which the child counts on the states it compares (and tests/test_failure_sets_host.py on
the CPU for the same seeds).  A second witness needs no restatement: the E one-link columns equal failure_impact(links=None)
of the same environment."""
import os
import subprocess
import sys

import numpy as np
import pytest

from failure_impact_child import CASES
from optical_networking_gym import _native as nat
from test_gpu_action_impact import DB_ATOL

pytestmark = pytest.mark.gpu
COLS = {k: i for i, k in enumerate(nat.FAILURE_SETS)}


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("failure_sets") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "failure_sets_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "failure sets child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def compare(got, svc, want, act, active, ctx):
    assert got.shape == want.shape and got.shape[1] == 12, ctx
    assert np.array_equal(got[:, 0], want[:, 0]), ctx
    assert np.array_equal(np.isnan(got), np.isnan(want)), ctx
    ok = want[:, 0] == 0
    exact = [1, 2, 3, 4, 5, 6, 7, 8, 10, 11]
    assert np.array_equal(got[ok][:, exact], want[ok][:, exact]), (ctx, got[ok][:, exact], want[ok][:, exact])
    assert np.array_equal(got[ok][:, 1], got[ok][:, 3] + got[ok][:, 5] + got[ok][:, 6]), ctx
    assert np.all(got[ok][:, 10] <= got[ok][:, 5]), ctx
    assert np.all(np.isnan(got[~ok][:, 1:])), ctx
    some = ok & (want[:, 3] > 0)
    np.testing.assert_allclose(got[some][:, 9], want[some][:, 9], rtol=0, atol=DB_ATOL, err_msg=ctx)
    assert np.array_equal(svc[:, :active], act), ctx
    assert np.all(svc[:, active:] == -1), ctx
    return int(ok.sum())


@pytest.mark.parametrize("key", CASES)
def test_failure_sets_equal_the_restatement(res, key):
    """node sets, dual cuts, one-link sets, a duplicate, the empty set and a set with bit E: every column and svc_out"""
    evaluated = victims = 0
    assert int(res[key + "_band"]) == 0                            # a condition of the exact comparison, not a tolerance
    N, F = int(res[key + "_N"]), int(res[key + "_F"])
    for r in range(int(res[key + "_B"])):
        k = f"{key}_r{r}"
        got, want = res[k + "_got"], res[k + "_want"]
        assert len(got) == F
        evaluated += compare(got, res[k + "_svc"], want, res[k + "_act"], int(res[k + "_active"]), f"{key} r{r}")
        victims += int(np.nansum(want[:, 1]))
        assert want[-2:, 0].tolist() == [1, 1] and np.all(want[:-2, 0] == 0)         # the empty set, the set with bit E
        assert np.array_equal(got[-3], got[0], equal_nan=True)                       # the first node set once more
        assert np.array_equal(res[k + "_svc"][-3], res[k + "_svc"][0])
        assert np.all(got[N:-3, COLS["failed_links"]] <= 2) and np.all(got[:-2, COLS["failed_links"]] >= 1)
    print(f"{key}: {evaluated} evaluated scenarios, {victims} victims")
    assert evaluated > 0 and victims > 0
    assert res[key + "_same_without_detail"]


@pytest.mark.parametrize("key", CASES)
def test_one_link_sets_equal_failure_impact(res, key):
    """the second witness: columns 0-9 and svc_out of the E one-link sets are failure_impact(links=None)'s, exactly"""
    assert res[key + "_one_link_same"]


@pytest.mark.parametrize("key", CASES)
def test_a_shared_list_equals_the_tiled_per_replica_list(res, key):
    """per_replica = 0 with the node sets, the same list tiled with per_replica = 1, and the list given as link indices"""
    assert res[key + "_shared_same"] and res[key + "_shared_is_the_node_columns"]


@pytest.mark.parametrize("key", CASES)
def test_no_case_passes_emptily(res, key):
    c = {n: int(res[f"{key}_cond_{n}"]) for n in ("evaluated", "no_victim", "restored", "no_route")}
    print(key, c)
    assert 4 * c["no_victim"] <= c["evaluated"]                     # at most a quarter of the scenarios without a victim
    assert c["restored"] > 0 and c["no_route"] > 0
    if key == "nsfnet":
        assert res[key + "_rec32"]
    if key == "nobeleu":
        assert not res[key + "_rec32"] and int(res[key + "_E"]) > 32


def test_the_cases_together_exercise_every_condition(res):
    """on the RESTATED values of the device's states: a victim lost on QoT, one lost for spectrum with a route left, victims
    that cross two or more failed links, victims restored on a later route because their first route clear of their own
    failed links crosses another failed link"""
    t = {n: sum(int(res[f"{key}_cond_{n}"]) for key in CASES) for n in ("lost_qot", "lost_ns", "no_route", "multi", "skip_restored")}
    print(t)
    assert t["lost_qot"] > 0 and t["lost_ns"] - t["no_route"] > 0 and t["multi"] > 0 and t["skip_restored"] > 0


def test_failure_sets_is_read_only(res):
    assert res["ro_blob_same"] and res["ro_stats_same"] and res["ro_traj_same"]
    assert int(res["ro_victims"]) > 0


def test_fresh_replicas_have_no_victims(res):
    rows, svc = res["fresh_rows"], res["fresh_svc"]
    assert rows.shape[0] >= 8 and rows.shape[2] == 12
    assert np.all(rows[:, :, :9] == 0) and np.all(rows[:, :, 10] == 0) and np.all(np.isnan(rows[:, :, 9]))
    assert np.all(rows[:, :, 11] >= 2)                                  # every NSFNET node has at least two links
    assert np.all(svc == -1)


def test_device_io_on_the_current_stream_equals_the_host_path(res):
    assert res["dev_same"] and res["dev_detail_same"] and res["dev_per_replica_same"] and res["dev_stream_refused"]
    assert np.all(res["dev_refusals"])


def test_single_environment_dict_is_row_0_of_the_batched_call(res):
    assert res["compat_same"] and int(res["compat_victims"]) > 0 and int(res["compat_no_route"]) > 0


def test_library_refusals(res):
    for k in ("zero", "many", "null_sets", "null_out", "window"):
        assert int(res["refuse_rc_" + k]) == -1, k
    assert int(res["refuse_rc_ok"]) == 0 and int(res["refuse_rc_ok_shared"]) == 0
    assert "n_sets" in str(res["refuse_msg_zero"]) and "n_sets" in str(res["refuse_msg_many"])
    assert "null" in str(res["refuse_msg_null_sets"]) and "null" in str(res["refuse_msg_null_out"])
    assert "modulations_to_consider" in str(res["refuse_msg_window"])
