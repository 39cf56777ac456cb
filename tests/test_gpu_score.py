"""The weighted candidate-scoring policy on device (ongym_score_actions through BatchedQRMSAEnv.score_actions).  Every GPU
computation runs in ONE fresh child process (tests/score_child.py); the tests assert on the .npz it writes.

The five definition states are those of tests/spectrum_map_child.py, driven as its `drive` does (first fit, exact fit, random
valid actions drawn on the device: no oracle follows that), so the restatement of tests/score_child.py is fed by the device's own
available_slots / candidates / gsnr_many queries of every replica; a sixth state is driven by first fit alone, which the oracle
reproduces step for step, and there the restatement is fed by the oracle twins.  The weights are per replica: the four presets
and rows drawn with default_rng(900 + r), and the rows are rotated through the replicas, so every replica meets every row.
Actions, counts, the integer features and `load` are compared exactly; gsnr, margin and the score within 4.4e-9 dB (the score
scaled by the sum of |w|): the bound tests/test_gpu_move.py holds the same evaluation to (rtol 1e-9 on the linear 1/GSNR).  A
replica is left out of the comparison of the winner only where the restatement's best two distinct scores lie within 1e-9 dB x
(|w8| + |w9|), and at most 2 % may be left out."""
import os
import subprocess
import sys

import numpy as np
import pytest

from optical_networking_gym import _native as nat
from test_gpu_action_impact import DB_ATOL

pytestmark = pytest.mark.gpu
DEFINITIONS = ("ring4", "nsfnet100", "nsfnet320", "nobeleu320", "germany100")
COMPARED = tuple("def_" + k for k in DEFINITIONS) + ("twin", "cut")
INTEGER = [1 + nat.SCORE_FEATURES.index(n) for n in ("route", "hops", "format_rank", "slots", "slot_hops", "start", "touch")]
LOAD, GSNR, MARGIN = (1 + nat.SCORE_FEATURES.index(n) for n in ("load", "gsnr", "margin"))


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("score") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "score_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1500)
    assert run.returncode == 0 and "score child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


@pytest.mark.parametrize("k", COMPARED)
def test_device_equals_the_restatement(res, k):
    got = {n: res[f"{k}_{n}"] for n in ("actions", "best", "counts")}
    want = {n: res[f"{k}_want_{n}"] for n in ("actions", "best", "counts", "near")}
    W = res[f"{k}_weights"]
    R, B = got["actions"].shape
    assert R == B and 8 <= B <= 16 and W.shape == (B, 10)
    assert res[f"{k}_margin_gap"] > 1e-8                                   # no QoT decision near its threshold
    assert np.array_equal(got["counts"], want["counts"])                    # candidates with spectrum, feasible ones, flags
    near = want["near"]
    assert near.mean() <= 0.02
    ok = ~near
    assert np.array_equal(got["actions"][ok], want["actions"][ok])
    none = np.isnan(want["best"][..., 0])
    assert np.array_equal(np.isnan(got["best"]), np.isnan(want["best"])) and np.array_equal(none, want["counts"][..., 1] == 0)
    sel = ok & ~none
    g, w = got["best"][sel], want["best"][sel]
    assert np.array_equal(g[:, INTEGER], w[:, INTEGER]) and np.array_equal(g[:, LOAD], w[:, LOAD])
    np.testing.assert_allclose(g[:, [GSNR, MARGIN]], w[:, [GSNR, MARGIN]], rtol=0, atol=DB_ATOL)
    sumw = np.stack([np.abs(np.roll(W, j, axis=0)).sum(axis=1) for j in range(R)])[sel]
    assert np.all(np.abs(g[:, 0] - w[:, 0]) <= DB_ATOL * sumw)
    exact = sel & np.stack([(np.roll(W, j, axis=0)[:, 8:] == 0).all(axis=1) for j in range(R)])
    assert exact.any() and np.array_equal(got["best"][exact][:, 0], want["best"][exact][:, 0])     # w8 = w9 = 0: no rounding to allow for
    # the states are worth the comparison: feasible candidates on most replicas, rows that disagree about the winner
    assert np.count_nonzero(res[f"{k}_feasible"]) >= B // 2
    assert any(len(set(got["actions"][:, r].tolist())) > 1 for r in range(B))


@pytest.mark.parametrize("k", COMPARED)
def test_highest_snr_preset_is_the_fused_policy(res, k):
    assert np.array_equal(res[f"{k}_hs_actions"], res[f"{k}_policy_actions"])
    assert np.array_equal(res[f"{k}_hs_flags"], res[f"{k}_policy_flags"].astype(np.int32))


@pytest.mark.parametrize("k", COMPARED)
def test_a_shared_row_equals_the_row_tiled(res, k):
    assert all(bool(res[f"{k}_shared_{j}"]) and bool(res[f"{k}_plain_{j}"]) for j in range(6))


def test_layouts_covered(res):
    assert [bool(res[f"def_{k}_rec32"]) for k in DEFINITIONS] == [True, True, True, False, False]
    assert bool(res["twin_same_trajectory"])                               # the device followed the oracle to the compared state
    # both ways of finding no placement: no spectrum anywhere (a loaded ring), spectrum but no candidate clears a wide margin
    assert nat.F_BLOCKED_RESOURCES in res["def_ring4_counts"][..., 2] and nat.F_BLOCKED_OSNR in res["twin_counts"][..., 2]


def test_forty_steps_of_score_then_step(res):
    a, reject = res["loop_actions"], int(res["loop_reject"])
    assert a.shape == (40, 16) and np.array_equal(res["loop_rec_action"], a)
    assert np.array_equal(res["loop_rec_accepted"] != 0, a != reject)       # every winner is a placement the step accepts
    assert not np.any(res["loop_rec_flags"] & nat.F_QOT_ERROR) and not np.any(res["loop_rec_retry"])
    assert np.any(a == reject) or np.all(res["loop_rec_accepted"])
    assert len({tuple(a[:, r].tolist()) for r in range(16)}) > 4             # the rows steer their replicas apart
    assert np.all(res["loop_audit"][:, 0] == 0)
    assert bool(res["loop_blob_same"]) and bool(res["loop_stats_same"]) and bool(res["loop_repeatable"])
    assert float(res["loop_last_kernel_ms"]) > 0


def test_no_winner_crosses_a_failed_link(res):
    assert int(res["cut_winners"]) > 100 and not res["cut_crossed"].any()
    assert np.all(res["cut_failed"].view(np.uint64).any(axis=1))


def test_device_buffers(res):
    assert bool(res["dev_is_out"]) and bool(res["dev_shared_is_out"]) and bool(res["dev_stream_refused"])
    for n in ("actions", "best", "counts"):
        assert np.array_equal(res["dev_" + n], res["dev_want_" + n], equal_nan=True), n
    assert np.array_equal(res["dev_shared"], res["dev_want_shared"]) and res["dev_refusals"].all()


def test_refusals(res):
    assert int(res["refuse_null_env"]) == nat.E_ARG
    for name, code, text in (("null_actions", nat.E_ARG, "null actions/weights"), ("null_weights", nat.E_ARG, "null actions/weights"),
                             ("weight_nan", nat.E_ARG, "finite"), ("weight_inf", nat.E_ARG, "finite"),
                             ("weight_minus_inf", nat.E_ARG, "finite"), ("window", nat.E_ARG, "modulations_to_consider"),
                             ("lds", nat.E_LIMIT, "160 KiB")):
        assert int(res["refuse_" + name]) == code and text in str(res[f"refuse_{name}_msg"]), name
    assert bool(res["refuse_actions_untouched"]) and int(res["refuse_ok_after"]) == nat.OK and bool(res["refuse_window_python"])


def test_example_reports_the_blocking_of_its_records(res):
    assert res["ex_blocking"].shape == (2, 16) and np.array_equal(res["ex_blocking"], res["ex_recount"]) and res["ex_blocking"].any()
    assert tuple(res["ex_weights_shape"]) == (16, 10) and int(res["ex_lines"]) == 3
    assert bool(res["ex_same_requests"]) and bool(res["ex_actions_differ"])


def test_single_environment_and_plugin_heuristic(res):
    assert len(res["single_same"]) == 12 and res["single_same"].all() and res["single_named"].all()
