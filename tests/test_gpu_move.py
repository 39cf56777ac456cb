"""Moving running lightpaths on live replicas (ongym_move_services through BatchedQRMSAEnv.move_services and defragment).
Every GPU computation runs in ONE fresh child process (tests/move_child.py); the tests assert on the .npz it writes.

The six configurations are those of tests/failure_impact_child.py.  Replica r's twelve moves are drawn with
default_rng(700 + r) from its pre-call services() and grid() (draw_moves of the child).  The device is held to expected_moves
of the child, computed from the device's own pre-call state: the post-call records and grid and move_out's columns 0-3 and 5
exactly; margin, and under id tracking the Service.OSNR of a moved record, at the tolerance tests/test_gpu_action_impact.py
holds its dB columns to (rtol 1e-9 on the linear 1/GSNR, 4.4e-9 dB: the device's sum order differs from the list order by a
few ulp).  Exact statuses need every decision to be the restatement's: no evaluation of a case may lie within 1e-8 relative of
its limit, which the child counts on the states it compares (and tests/test_move_host.py on the CPU for the same seeds)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from failure_impact_child import CASES
from link_cut_child import FIELDS, OSNR
from move_child import BOTH, COVER, EXACT, LEAN, TRAFFIC
from test_gpu_action_impact import DB_ATOL

pytestmark = pytest.mark.gpu
QOT_ATOL = 1e-8                # dB: move_out's margin against service_qot's, two device paths over the same interferers


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("move") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "move_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "move child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def compare_state(res, k, ctx, got, ids):
    """the device's move_out, records and grid of one replica against the restatement; returns the wanted move_out"""
    want, post, grid, pre = res[k + "_want"], res[k + "_post"], res[k + "_grid"], res.get(k + "_pre")
    assert got.shape == want.shape, ctx
    assert np.array_equal(got[:, EXACT], want[:, EXACT]), (ctx, got, want)
    ok = want[:, 0] == 0
    assert np.all(np.isnan(got[~ok, 4])), ctx
    np.testing.assert_allclose(got[ok, 4], want[ok, 4], rtol=0, atol=DB_ATOL, err_msg=ctx)
    got_post, got_grid = res[k + "_got_post"], res[k + "_got_grid"]
    assert got_post.shape == post.shape, ctx
    rest = [i for i in range(len(FIELDS)) if i != OSNR]
    assert np.array_equal(got_post[:, rest], post[:, rest]), ctx
    moved = np.zeros(len(post), bool)
    moved[want[ok, 1].astype(int)] = True
    assert np.array_equal(got_post[~moved, OSNR], post[~moved, OSNR]), ctx
    if ids:
        np.testing.assert_allclose(got_post[moved, OSNR], post[moved, OSNR], rtol=0, atol=DB_ATOL, err_msg=ctx)
    else:
        assert np.array_equal(got_post[moved, OSNR], post[moved, OSNR]), ctx
    if pre is not None:                                               # indices are stable: what a record owns stays at its index
        own = [FIELDS.index(f) for f in ("reserved", "release_time", "service_id")]
        assert np.array_equal(got_post[:, own], pre[:, own]), ctx
        assert np.array_equal(got_post[~moved], pre[~moved]), ctx
    assert np.array_equal(got_grid, grid), ctx
    return want


@pytest.mark.parametrize("key", CASES)
def test_the_state_after_the_moves_equals_the_restatement(res, key):
    """1: move_out, records and grid of every replica"""
    assert int(res[key + "_band"]) == 0                            # a condition of the exact comparison, not a tolerance
    B, ids = int(res[key + "_B"]), bool(res[key + "_ids"])
    status = np.zeros(5, int)
    for r in range(B):
        want = compare_state(res, f"{key}_r{r}", f"{key} r{r}", res[key + "_got"][r], ids)
        status += np.bincount(want[:, 0].astype(int), minlength=5)
    print(f"{key}: statuses 0-4 {status.tolist()}, kernel {float(res[key + '_kernel_ms']):.3f} ms")
    assert status[0] > 0
    if key == "nsfnet":
        assert res[key + "_rec32"]
    if key == "nobeleu":
        assert not res[key + "_rec32"] and int(res[key + "_E"]) > 32
    # the width limit the restatement applied is the device's: 32 where a lean step kernel runs the case, S elsewhere
    print(f"{key}: lean {bool(res[key + '_lean'])}, width limit {int(res[key + '_limit'])}")
    assert bool(res[key + "_lean"]) == (key in LEAN)               # (tests/test_move_host.py takes LEAN for its band check)
    assert int(res[key + "_limit"]) == (32 if res[key + "_lean"] else int(res[key + "_S"]))


def test_the_cases_together_exercise_every_status_and_condition(res):
    t = {n: sum(int(res[f"{key}_cond_{n}"]) for key in CASES) for n in COVER}
    print(t)
    assert all(t[k] > 0 for k in ("moved", "invalid", "unchanged", "no_spectrum", "qot")), t
    assert all(t[k] > 0 for k in ("other_route", "other_format", "shift_down", "top_skips", "to_S")), t
    assert int(res["odd_cond_ends_at_S"]) > 0 and int(res["ids_cond_namesake"]) > 0


@pytest.mark.parametrize("key", CASES)
def test_the_margin_is_what_service_qot_reports_for_the_record_afterwards(res, key):
    """2: column 4 of EVERY successful move against service_qot()'s margin of that record on the state the move left, less the
    replica's margin: an independent device path that also leaves the service out of its own sum.  The state after a move
    inside a call is not observable, so a twin repeats every move as a call of its own, with the record it resolved to, and
    asks service_qot() after each; the twin's rows and final state are the call's.  The last successful move of each replica is
    also held to service_qot() after the call itself"""
    got, each, ref = res[key + "_got"], res[key + "_each"], res[key + "_each_qot"]
    assert np.array_equal(each, got, equal_nan=True) and res[key + "_each_state_same"]
    ok = got[:, :, 0] == 0
    assert ok.any() and np.array_equal(ok, ~np.isnan(ref))
    np.testing.assert_allclose(got[:, :, 4][ok], ref[ok], rtol=0, atol=QOT_ATOL)
    last = res[key + "_qot_margin"]
    some = ~np.isnan(last)
    assert some.any() and not np.any(np.isnan(got[:, :, 4][some]))
    np.testing.assert_allclose(got[:, :, 4][some], last[some], rtol=0, atol=QOT_ATOL)


@pytest.mark.parametrize("key", CASES)
def test_defragment_is_the_top_to_first_fit_sweep(res, key):
    """3: defragment(n) on a twin equals move_services with n (TOP, FIRST_FIT) rows on the own route byte for byte, and both
    equal the restated sweep"""
    B, ids = int(res[key + "_B"]), bool(res[key + "_ids"])
    assert res[key + "_sweep_same"]
    moved = 0
    for r in range(B):
        want = compare_state(res, f"{key}_r{r}_sweep", f"{key} r{r} sweep", res[key + "_sweep"][r], ids)
        moved += int(np.sum(want[:, 0] == 0))
    assert moved > 0
    if key == "nsfnet":
        assert res[key + "_sweep_anywhere_differs"]                 # own_route=False searches the pair's other routes too


@pytest.mark.parametrize("key", CASES)
def test_statistics_and_untouched_replicas(res, key):
    """4: no statistic moves (total_* included); with ids episode_osnr_sum moves by the sum of new - old Service.OSNR; a replica
    without a successful move keeps its bytes"""
    B, ids = int(res[key + "_B"]), bool(res[key + "_ids"])
    assert res[key + "_stats_same"]
    moved = np.any(res[key + "_got"][:, :, 0] == 0, axis=1)
    assert np.all(res[key + "_blob_same"][~moved]) and not np.all(res[key + "_blob_same"])
    before, after = res[key + "_osnr_sum"]
    if ids:
        assert np.any(res[key + "_osnr_delta"] != 0)
        np.testing.assert_allclose(after, before + res[key + "_osnr_delta"], rtol=1e-9, atol=0)
    else:
        assert np.array_equal(before, after)


def test_failing_moves_and_an_empty_replica_change_no_byte(res):
    """5: byte for byte (save_state blobs)"""
    assert np.all(res["empty_active"] == 0) and res["empty_blob_same"]
    e = res["empty_out"]
    assert np.all(e[:, :, 0] == 1) and np.all(e[:, :, 1:4] == -1) and np.all(np.isnan(e[:, :, 4])) and np.all(e[:, :, 5] == 0)
    f = res["fail_out"]
    assert np.all(res["fail_blob_same"])
    assert np.all(f[:, [0, 2, 3], 0] == 1) and np.all(f[:, [0, 2], 1] == -1)
    has = res["fail_active"] > 0
    assert has.any() and np.all(f[has, 1, 0] == 2) and np.all(f[has, 1, 2] == f[has, 1, 3]) and np.all(f[has, 3, 1] == 0)
    assert np.all(f[~has, 1, 0] == 1)
    assert res["shared_same"] and int(res["shared_moved"]) > 0


@pytest.mark.parametrize("key", TRAFFIC)
def test_traffic_goes_on_after_the_moves(res, key):
    """6: six launches of 50 first-fit steps; the grid stays the union of the records' ranges, so a moved record that departs
    frees its NEW range"""
    assert np.all(res[key + "_run_steps"] == 300)
    assert res[key + "_run_grid_ok"].shape[0] == 6 and np.all(res[key + "_run_grid_ok"])
    left, moved = res[key + "_run_moved_left"], int(res[key + "_run_moved"])
    print(key, "moved records still running after each launch:", left.tolist(), "of", moved)
    assert moved > 0 and left[-1] < moved and np.all(np.diff(left) <= 0)


@pytest.mark.parametrize("key", BOTH)
def test_both_step_kernels_agree_after_the_same_moves(res, key):
    """7: the lean and the generic kernel from the same seed, the same moves after the same launch, five recorded launches of 50
    steps: equal step records, the grid the union of the records' ranges after every launch on both, equal records and grids at
    the end"""
    assert not res[f"{key}_both_lean1"]
    if key == "nsfnet":
        assert res[f"{key}_both_lean0"]
    assert res[key + "_both_same"] and res[key + "_both_moves_same"] and int(res[key + "_both_accepted"]) > 0
    a, b = res[key + "_both_osnr"]
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=0)
    assert res[key + "_both_grid_ok"].shape[0] == 10 and np.all(res[key + "_both_grid_ok"]) and res[key + "_both_end_same"]


def test_no_move_writes_a_record_wider_than_the_lean_kernels_carry(res):
    """7b: on lean NSFNET-320 a 400 Gb/s service of a format above QPSK goes to BPSK, where it would take 33 slots or more: the
    lean environment answers "no spectrum" and keeps its bytes, a forced-generic environment on the same state takes the move
    wherever there is room.  The same service to QPSK (at most 18 slots) moves alike on both, and four launches of 50 steps
    give equal step records on the lean and on the generic kernel, the grid invariant after every launch, equal states at the
    end, with the lean kernel still the one that runs"""
    assert res["wide_lean"] and not res["wide_generic_lean"] and res["wide_start_same"] and int(res["wide_limit"]) == 32
    assert np.all(res["wide_slots"] > 32)
    lean, gen = res["wide_lean_out"][:, 0], res["wide_generic_out"][:, 0]
    assert np.all(lean[:, 0] == 3) and res["wide_lean_untouched"]
    took = gen[:, 0] == 0
    print("forced generic took", int(took.sum()), "of", len(took), "wide moves; slots", res["wide_slots"].tolist())
    room = res["wide_room"]
    assert 2 * took.sum() >= len(took) and np.all(gen[~room, 0] == 3) and np.all(np.isin(gen[room, 0], (0, 4)))
    assert np.array_equal(res["wide_generic_slots"][took], res["wide_slots"][took])
    a, b = res["narrow_lean_out"], res["narrow_generic_out"]
    assert np.array_equal(a[:, :, EXACT], b[:, :, EXACT]) and np.any(a[:, :, 0] == 0)
    assert res["wide_run_same"] and np.all(res["wide_run_grid_ok"]) and res["wide_end_same"] and res["wide_still_lean"]
    x, y = res["wide_run_osnr"]
    np.testing.assert_allclose(x, y, rtol=1e-9, atol=0)


def test_state_calls_after_a_move(res):
    """8: save_state / load_state / fork"""
    assert int(res["state_moved"]) > 0
    assert res["state_records_same"] and res["state_same"] and res["fork_copies"]


def test_a_move_after_a_cut_never_lands_on_a_failed_link(res):
    """9: and failed_links() is unchanged"""
    assert int(res["cut_moved"]) > 0 and res["cut_failed_same"] and int(res["cut_cross"]) == 0
    assert np.all(res["cut_grid_ok"]) and res["cut_restated"]


def test_device_io_on_the_current_stream_equals_the_host_path(res):
    """10"""
    assert res["dev_stream_refused"] and res["dev_same"] and res["dev_state_same"] and int(res["dev_moved"]) > 0
    assert np.all(res["dev_refusals"])


def test_library_refusals(res):
    """11"""
    for k in ("null_moves", "null_out", "zero", "flags", "window", "pairs"):
        assert int(res["refuse_rc_" + k]) == -1, k
    for k in ("ok", "ok_own"):
        assert int(res["refuse_rc_" + k]) == 0, (k, str(res["refuse_msg_" + k]))
    assert "moves" in str(res["refuse_msg_null_moves"]) and "move_out" in str(res["refuse_msg_null_out"])
    assert "n_moves" in str(res["refuse_msg_zero"]) and "flags" in str(res["refuse_msg_flags"])
    assert "modulations_to_consider" in str(res["refuse_msg_window"])
    assert "node pairs" in str(res["refuse_msg_pairs"])
