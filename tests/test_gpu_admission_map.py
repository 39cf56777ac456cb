"""First-fit admission of every node pair and bit rate (ongym_admission_map through BatchedQRMSAEnv.admission_map).  Every GPU
computation runs in ONE fresh child process (tests/admission_map_child.py); the tests assert on the .npz it writes.

The device is held to the restatement of tests/admission_map_child.py, computed from the device's own services(), grid() and
request() of each replica: the status, the three counts, `detoured` and the map exactly; blocking_probability and
bit_rate_blocking within 1e-12 absolute (at most Q R <= 6 048 terms in [0, 1], each adding at most one rounding of 1.1e-16, in
whatever order the groups of pairs are added); lowest_margin within 4.35e-9 dB (DB_ATOL, the value
tests/test_gpu_failure_impact.py holds the same quantity to); margin_out within that plus one float32 spacing of the value.
Exact counts need every decision to be the restatement's: no evaluated start of a case may lie within 1e-8 relative of its
limit, which the child counts on the states it compares (and tests/test_admission_map_host.py on the CPU for the same seeds)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from admission_map_child import CASES
from optical_networking_gym import _native as nat

pytestmark = pytest.mark.gpu
COLS = {k: i for i, k in enumerate(nat.ADMISSION_MAP)}
SUM_ATOL = 1e-12
DB_ATOL = 10.0 * np.log10(1.0 + 1e-9)     # 4.35e-9 dB (the documents round it up to 4.4e-9): rtol 1e-9 on the linear 1/GSNR
ALL = CASES + ("full",)


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("admission_map") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "admission_map_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "admission map child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def compare(got, gmap, gmar, want, wmap, wmar, ctx):
    print(ctx, "status", got[:, 0].tolist(), "max |sum error|", np.nanmax(np.abs(got[:, 4:6] - want[:, 4:6]), initial=0.0),
          "max |margin error|", np.nanmax(np.abs(got[:, 6] - want[:, 6]), initial=0.0))
    assert np.array_equal(got[:, 0], want[:, 0]), ctx
    assert np.array_equal(np.isnan(got), np.isnan(want)), ctx
    ok = want[:, 0] < 2
    assert np.array_equal(got[ok][:, [1, 2, 3, 7]], want[ok][:, [1, 2, 3, 7]]), (ctx, got[ok], want[ok])
    assert np.all(got[ok][:, 1] + got[ok][:, 2] + got[ok][:, 3] == wmap[0].size), ctx
    assert np.all(np.isnan(got[~ok][:, 1:])), ctx
    np.testing.assert_allclose(got[ok][:, 4:6], want[ok][:, 4:6], rtol=0, atol=SUM_ATOL, err_msg=ctx)
    some = ok & (want[:, 1] > 0)
    np.testing.assert_allclose(got[some][:, 6], want[some][:, 6], rtol=0, atol=DB_ATOL, err_msg=ctx)
    assert np.array_equal(gmap, wmap), ctx
    assert gmar.dtype == np.float32 and np.array_equal(np.isnan(gmar), np.isnan(wmar)), ctx
    adm = ~np.isnan(wmar)
    assert np.all(np.abs(gmar[adm].astype(np.float64) - wmar[adm]) <= DB_ATOL + np.spacing(np.abs(wmar[adm]).astype(np.float32))), ctx
    return int(ok.sum())


@pytest.mark.parametrize("which", ["null", "list"])
@pytest.mark.parametrize("key", ALL)
def test_admission_map_equals_the_restatement(res, key, which):
    """actions = NULL, and the list of five: first fit's choice, the reject action, -1, an occupied action, a valid action on the
    last route at the lowest usable format"""
    assert int(res[key + "_band"]) == 0 and int(res[key + "_evaluated"]) > 0   # a condition of the exact comparison, not a tolerance
    scenarios = 0
    for r in range(int(res[key + "_B"])):
        k = f"{key}_r{r}_{which}"
        scenarios += compare(res[k + "_got"], res[k + "_gmap"], res[k + "_gmar"], res[k + "_want"], res[k + "_wmap"],
                             res[k + "_wmar"], f"{key} r{r} {which}")
        if which == "list":                                                 # the reject action and -1: the baseline of the NULL call
            got, null = res[k + "_got"], res[f"{key}_r{r}_null_got"]
            assert got.shape[0] == 5 and got[1, 0] == got[2, 0] == 1
            assert np.array_equal(got[1, 1:], null[0, 1:], equal_nan=True) and np.array_equal(got[2], got[1], equal_nan=True)
            assert np.array_equal(res[k + "_gmap"][1], res[f"{key}_r{r}_null_gmap"][0])
    assert scenarios > 0
    if key != "full":
        assert res[key + "_same_bytes"] and res[key + "_same_without_detail"]


@pytest.mark.parametrize("key", ALL)
def test_no_case_passes_emptily(res, key):
    c = {n: int(res[f"{key}_cond_{n}"]) for n in ("scenarios", "none_blocked", "status0", "status1", "status3")}
    assert 4 * c["none_blocked"] <= c["scenarios"]                  # at most a quarter of the scenarios without a blocked cell
    if key == "full":
        assert c["status3"] > 0 and np.all(res["full_active"] == 64)
        return
    assert c["status0"] > 0 and c["status1"] > 0
    if key == "nsfnet":
        assert res[key + "_rec32"] and res[key + "_uniform"]
    if key == "nobeleu":
        assert not res[key + "_rec32"] and res[key + "_weights"].shape == (378, 4)
        assert res[key + "_rates"].tolist() == [10.0, 100.0, 400.0, 1000.0]
    else:
        assert res[key + "_traffic_same"] and float(res[key + "_uniform_err"]) <= SUM_ATOL
    if key == "alpha":
        assert not res[key + "_uniform"]


def test_the_cases_together_exercise_every_condition(res):
    """on the RESTATED values: every status, cells blocked for spectrum and on QoT, admissions on a later route and below the top
    format, cells that a candidate changes, newly blocked ones among them, and one that changes on QoT alone (the baseline's
    start evaluated again and refused)"""
    names = ("status0", "status1", "status2", "status3", "ns", "qot", "detoured", "below_top", "changed", "newly_blocked", "qot_alone")
    total = {n: sum(int(res[f"{key}_cond_{n}"]) for key in ALL) for n in names}
    print(total)
    for n, v in total.items():
        assert v > 0, n


@pytest.mark.parametrize("key", ["nsfnet", "nobeleu"])
def test_the_groups_of_pairs_do_not_change_the_answer(res, key):
    """one wavefront per scenario and three groups of pairs against the host rule's split (16 groups at these batch sizes): the
    map, the margins, the counts and lowest_margin exactly, the weighted sums within the bound of their different order"""
    assert res[key + "_groups_same"] and float(res[key + "_groups_err"]) <= SUM_ATOL


def test_witness_through_the_step_itself(res):
    """32 (replica, cell) samples of the nsfnet case: the replica forked, the cell installed as its next request, first fit's
    own decision; both blocked codes are the reject action there"""
    want, got = res["witness_want"], res["witness_got"]
    assert len(want) == 32 and 0 < int(res["witness_blocked"]) < 32
    assert np.array_equal(want, got), (want, got)


def test_admission_map_is_read_only(res):
    assert res["ro_blob_same"] and res["ro_stats_same"] and res["ro_traj_same"]
    assert int(res["ro_cells"]) > 0 and res["ro_baseline_same"] and int(res["ro_applied"]) > 0


def test_fresh_replicas_admit_every_usable_cell_on_the_first_route_at_slot_0(res):
    K, M, S = (int(x) for x in res["fresh_kms"])
    for sfx in ("", "_x"):
        rows, amap, usable = res["fresh_rows" + sfx], res["fresh_map" + sfx], res["fresh_usable" + sfx]
        Q = amap.shape[2]
        assert rows.shape[0] >= 8 and np.all(rows[:, :, 0] == 1)
        cells = amap[:, :, :, usable]
        if sfx:                     # 5 Tb/s: its only usable formats fail on QoT on the long routes; start 0 wherever admitted
            assert np.all((cells == K * M * S + 1) | ((cells < K * M * S) & (cells % S == 0))) and np.any(cells == K * M * S + 1)
        else:                       # the configured rates: k = 0, start 0
            assert np.all(cells < M * S) and np.all(cells % S == 0)
            assert np.all(rows[:, :, 1] == Q * usable.sum()) and np.all(rows[:, :, 3] == 0) and np.all(rows[:, :, 7] == 0)
        assert np.all(amap[:, :, :, ~usable] == K * M * S)                                          # blocked for spectrum
        assert np.all(rows[:, :, 2] == Q * (~usable).sum())
    assert res["fresh_usable"].all() and res["fresh_usable_x"].tolist() == [True, True, False]
    assert np.all(res["fresh_margin"] > 0)


def test_device_io_on_the_current_stream_equals_the_host_path(res):
    assert res["dev_same"] and res["dev_detail_same"] and res["dev_rates_same"] and res["dev_stream_refused"]
    assert np.all(res["dev_refusals"])


def test_single_environment_dict_and_block_lookahead(res):
    assert res["compat_same"] and int(res["compat_blocked"]) > 0
    assert res["look_shape_ok"] and res["look_same"] and res["look_reject_is_baseline"]
    assert float(res["look_spread"]) > 0


def test_library_refusals(res):
    for k in ("zero_actions", "many_actions", "null_actions", "null_summary", "zero_rates", "many_rates", "null_rates_other_count",
              "nan_rate", "inf_rate", "negative_rate", "window", "continuous_null_rates", "asymmetric"):
        assert int(res["refuse_rc_" + k]) == -1, k
    assert int(res["refuse_rc_ok"]) == 0
    assert "n_actions" in str(res["refuse_actions_msg"]) and "rate" in str(res["refuse_rate_msg"])
    assert "modulations_to_consider" in str(res["refuse_window_msg"]) and "(1, 3)" in str(res["refuse_asymmetric_msg"])
