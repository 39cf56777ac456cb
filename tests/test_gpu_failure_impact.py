"""Single-link failures and first-fit restoration (ongym_failure_impact through BatchedQRMSAEnv.failure_impact).  Every GPU
computation runs in ONE fresh child process (tests/failure_impact_child.py); the tests assert on the .npz it writes.

The device is held to the restatement of tests/failure_impact_child.py, computed from the device's own services() and grid()
of each replica: status, every count, the capacity and hop sums and svc_out exactly; lowest_margin at the tolerance
tests/test_gpu_action_impact.py holds its dB columns to (rtol 1e-9 on the linear 1/GSNR, 4.4e-9 dB: the device's sum order
differs from the list order by a few ulp).  Exact counts need every decision to be the restatement's: no evaluated (candidate,
format) pair of a case may lie within 1e-8 relative of its limit, which the child counts on the states it compares (and
tests/test_failure_impact_host.py on the CPU for the same seeds).

The witness through the step itself (gsnr() and is_path_free() of a forked replica for a first victim's restoration) is left
out: a forked state still holds the victims, whose spectrum and interference the restoration no longer sees, and no existing
call takes records out of a replica."""
import os
import subprocess
import sys

import numpy as np
import pytest

from failure_impact_child import CASES
from optical_networking_gym import _native as nat
from test_gpu_action_impact import DB_ATOL

pytestmark = pytest.mark.gpu
COLS = {k: i for i, k in enumerate(nat.FAILURE_IMPACT)}


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("failure_impact") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "failure_impact_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "failure impact child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def compare(got, svc, want, act, active, ctx):
    assert np.array_equal(got[:, 0], want[:, 0]), ctx
    assert np.array_equal(np.isnan(got), np.isnan(want)), ctx
    ok = want[:, 0] == 0
    assert np.array_equal(got[ok][:, 1:9], want[ok][:, 1:9]), (ctx, got[ok][:, 1:9], want[ok][:, 1:9])
    assert np.array_equal(got[ok][:, 1], got[ok][:, 3] + got[ok][:, 5] + got[ok][:, 6]), ctx
    assert np.all(np.isnan(got[~ok][:, 1:])), ctx
    some = ok & (want[:, 3] > 0)
    np.testing.assert_allclose(got[some][:, 9], want[some][:, 9], rtol=0, atol=DB_ATOL, err_msg=ctx)
    assert np.array_equal(svc[:, :active], act), ctx
    assert np.all(svc[:, active:] == -1), ctx
    return int(ok.sum())


@pytest.mark.parametrize("which", ["", "_list"])
@pytest.mark.parametrize("key", CASES)
def test_failure_impact_equals_the_restatement(res, key, which):
    """links = NULL (every link) and the explicit list with a duplicate, a -1 and an index >= E: every column and svc_out"""
    evaluated = victims = 0
    assert int(res[key + "_band"]) == 0                            # a condition of the exact comparison, not a tolerance
    for r in range(int(res[key + "_B"])):
        k = f"{key}_r{r}"
        want = res[k + "_want" + which]
        evaluated += compare(res[k + "_got" + which], res[k + "_svc" + which], want, res[k + "_act" + which],
                             int(res[k + "_active"]), f"{key} r{r}{which}")
        victims += int(np.nansum(want[:, 1]))
        if which:                                                         # explicit_links: ..., the first link again, -1, E + 7
            e = int(res[key + "_E"])
            assert want[-2:, 0].tolist() == [1, 1] and np.all(want[:-2, 0] == 0)
            assert np.array_equal(res[k + "_got_list"][e - 3], res[k + "_got_list"][0], equal_nan=True)
    print(f"{key}{which}: {evaluated} evaluated scenarios, {victims} victims")
    assert evaluated > 0 and victims > 0
    assert res[key + "_same_without_detail"]


@pytest.mark.parametrize("key", CASES)
def test_no_case_passes_emptily(res, key):
    c = {n: int(res[f"{key}_cond_{n}"]) for n in ("evaluated", "no_victim", "restored", "route2", "wide", "wide_seen", "ends_at_S",
                                                         "namesakes")}
    assert c["restored"] > 0
    assert 4 * c["no_victim"] <= c["evaluated"]                     # at most a quarter of the scenarios without a victim
    if key == "ring4":
        assert c["route2"] == 0                                     # K = 2: one eligible route at the most
    if key == "nsfnet":
        assert res[key + "_rec32"] and res[key + "_uniform"]
    if key == "nobeleu":
        assert not res[key + "_rec32"] and int(res[key + "_E"]) > 32
        assert c["wide"] > 0                                        # restorations wider than the pair table ...
        assert c["wide_seen"] > 0                                   # ... met as interferers by later victims' evaluations
    if key == "alpha":
        assert not res[key + "_uniform"]
    if key == "ids":
        assert c["namesakes"] > 0                                   # running records that share a service_id
    if key == "odd":
        assert c["ends_at_S"] > 0                                   # restorations that end at S: no guard slot


def test_the_cases_together_exercise_every_condition(res):
    """on the RESTATED values: a restoration with a lower format and more slots, one on a route index >= 2, a victim lost for
    want of spectrum, one lost on QoT, a scenario whose outcome differs from restoring every victim independently of the
    others (the sequential dependence), a link without a victim"""
    total = {n: sum(int(res[f"{key}_cond_{n}"]) for key in CASES)
             for n in ("down", "route2", "lost_ns", "lost_qot", "sequential", "no_victim")}
    print(total)
    for n, v in total.items():
        assert v > 0, n


def test_failure_impact_is_read_only(res):
    assert res["ro_blob_same"] and res["ro_stats_same"] and res["ro_traj_same"]
    assert int(res["ro_victims"]) > 0 and res["ro_duplicates_same"]


def test_fresh_replicas_have_no_victims(res):
    rows, svc = res["fresh_rows"], res["fresh_svc"]
    assert rows.shape[0] >= 8 and np.all(rows[:, :, :9] == 0) and np.all(np.isnan(rows[:, :, 9]))
    assert np.all(svc == -1)


def test_device_io_on_the_current_stream_equals_the_host_path(res):
    assert res["dev_same"] and res["dev_detail_same"] and res["dev_list_same"] and res["dev_stream_refused"]
    assert np.all(res["dev_refusals"])


def test_single_environment_dict_is_row_0_of_the_batched_call(res):
    assert res["compat_same"] and int(res["compat_victims"]) > 0


def test_library_refusals(res):
    for k in ("zero", "many", "null_links", "null_out", "window"):
        assert int(res["refuse_rc_" + k]) == -1, k
    assert int(res["refuse_rc_ok"]) == 0
    assert "n_fail" in str(res["refuse_zero_msg"]) and "modulations_to_consider" in str(res["refuse_window_msg"])
