"""Playouts on device (ongym_playout through BatchedQRMSAEnv.playout): candidate actions followed by H policy steps on a private
copy of every replica.  Every GPU computation runs in ONE fresh child process (tests/playout_child.py); the tests assert on the
.npz it writes.

The witness is the step itself (see the child's docstring): save_state, seed(seed + r, replica_base), step(actions),
step_policy with records, on a second environment that runs the generic kernel.  B = 8 replicas, A = 5 actions, R = 2 samples,
H = 32, on states warmed by 300 policy steps.  The comparison is exact: the counts are integers, the bit-rate sums are sums of
small integers in float64."""
import os
import subprocess
import sys

import numpy as np
import pytest

from optical_networking_gym import _native as nat
from playout_child import A, B, CASES, H, LEAN_CASE, R, WARM

pytestmark = pytest.mark.gpu
COL = {k: i for i, k in enumerate(nat.PLAYOUT)}
KEYS = tuple(CASES)


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("playout") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "playout_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "playout child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def compare(got, want, ctx):
    print(ctx, "status", np.unique(want[..., 0]).tolist(), "steps", np.unique(want[..., 2][~np.isnan(want[..., 2])]).tolist())
    assert got.shape == want.shape and got.dtype == np.float64, ctx
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(bad) == 0, (ctx, "first differences (replica, action, sample, column)", bad[:8].tolist(),
                           [(got[tuple(i)], want[tuple(i)]) for i in bad[:8]])
    ok = want[..., 0] < 2
    assert np.all(got[ok][:, 3] + got[ok][:, 4] == got[ok][:, 2]) and np.all(got[ok][:, 2] <= H), ctx
    assert np.all(np.isnan(got[~ok][:, 1:])), ctx


@pytest.mark.parametrize("key", KEYS)
def test_playout_equals_the_step_itself(res, key):
    """the list of five actions per replica: first fit's choice, the reject action, -1, an occupied action, a valid action on
    the last route"""
    got, want = res[key + "_got"], res[key + "_want"]
    own = bool(CASES[key].get("own"))
    assert want.shape == (B, A, 1 if own else R, len(nat.PLAYOUT))
    assert not res[key + "_lean"][1]                              # the witness ran the generic kernel
    compare(got, want, key)


@pytest.mark.parametrize("key", KEYS)
def test_properties(res, key):
    got = res[key + "_got"]
    assert res[key + "_null_is_minus_one"]                        # the -1 row is a NULL-actions call
    assert np.all(got[:, 2, :, 0] == 1) and np.all(got[:, 1, :, 0] == 0)
    if CASES[key].get("policy", nat.POLICY_FIRST_FIT) == nat.POLICY_FIRST_FIT:   # first fit's own choice, applied as an action
        assert np.array_equal(got[:, 0, :, 1:], got[:, 2, :, 1:], equal_nan=True) and np.all(got[:, 0, :, 0] == 0)
    assert res[key + "_same_bytes"] and res[key + "_independent_of_A"] and res[key + "_state_same"]
    if not CASES[key].get("own"):
        assert res[key + "_sample_is_seed"]
        assert not np.array_equal(got[:, :, 0], got[:, :, 1], equal_nan=True)     # two samples, two futures


@pytest.mark.parametrize("key", KEYS)
def test_no_case_passes_emptily(res, key):
    """conditions on the WITNESS values"""
    c = {n: int(res[f"{key}_cond_{n}"]) for n in ("scenarios", "both", "differ", "departed", "status0", "status1", "status2")}
    print(key, c)
    assert c["scenarios"] > 0 and 2 * c["both"] >= c["scenarios"]  # an accepted and a blocked future request in at least half
    assert c["differ"] > 0                                         # two applied candidates of a replica differ in `blocked`
    assert c["departed"] > 0                                       # active_end < active_start + first_accepted + accepted
    assert c["status0"] > 0 and c["status1"] > 0 and c["status2"] > 0
    rec32, uniform = res[key + "_rec32_uniform"]
    assert rec32 == (key != "nobeleu") and uniform == (key != "alpha")


def test_every_status_occurs(res):
    total = {s: sum(int(res[f"{key}_cond_status{s}"]) for key in KEYS) for s in range(4)}
    total[4] = int(np.sum(res["exhausted_want"][..., 0] == 4))
    print(total)
    assert all(v > 0 for v in total.values()), total


def test_the_lean_kernel_is_the_same_witness(res):
    """a difference here would be a k_fast / k_run parity finding, not a playout defect"""
    assert res["lean_is_lean"]
    lean, want = res["lean_want"], res[LEAN_CASE + "_want"]
    bad = np.argwhere(~((lean == want) | (np.isnan(lean) & np.isnan(want))))
    assert len(bad) == 0, ("(replica, action, sample, column)", bad[:8].tolist())


def test_a_trace_that_runs_out_inside_the_horizon(res):
    want, got = res["trace_short_want"], res["trace_short_got"]
    ok = want[..., 0] < 2
    left = CASES["trace_short"]["trace"] - (WARM + 1)              # requests not yet drawn: the first step draws one of them
    assert ok.any() and np.all(want[ok][:, COL["steps"]] == left) and 0 < left < H
    assert np.array_equal(got, want, equal_nan=True)
    assert np.all(res["trace_want"][..., COL["steps"]][res["trace_want"][..., 0] < 2] == H)
    # past the end: no pending request, whatever the action
    assert np.all(res["exhausted_want"][..., 0] == 4) and np.array_equal(res["exhausted_got"], res["exhausted_want"], equal_nan=True)


@pytest.mark.parametrize("key", ["episode_reset", "episode_stop"])
def test_an_episode_that_ends_inside_the_horizon(res, key):
    """`steps` is the witness's index of the terminal record, with auto_reset and without"""
    want, got = res[key + "_want"], res[key + "_got"]
    ok = want[..., 0] < 2
    ends = CASES[key]["episode_length"] - (WARM + 1) - 1           # the first step is one of the episode's, the rest the policy's
    assert ok.any() and 0 < ends < H and np.all(want[ok][:, COL["steps"]] == ends)
    assert np.array_equal(got[..., COL["steps"]], want[..., COL["steps"]], equal_nan=True)
    assert np.array_equal(res["episode_reset_want"], res["episode_stop_want"], equal_nan=True)


def test_a_replica_at_capacity_rejects_in_the_first_step(res):
    want, acts, active0, cap = res["full_want"], res["full_acts"], res["full_active0"], int(res["full_capacity"])
    reject = int(res["full_reject"])
    hit = (active0 == cap) & (acts[:, 0] != reject) & (want[:, 0, 0, 0] == 0)
    assert hit.any(), (active0, acts[:, 0])
    assert np.all(want[hit][:, 0, :, COL["first_accepted"]] == 0)     # first fit found a placement; the table was full
    assert np.array_equal(res["full_got"], want, equal_nan=True)


def test_playout_is_read_only(res):
    assert res["ro_blob_same"] and res["ro_stats_same"] and res["ro_traj_same"]
    assert int(res["ro_ended_early"]) > 0 and int(res["ro_played"]) > 0


def test_device_io_on_the_current_stream_equals_the_host_path(res):
    assert res["dev_stream_refused"] and res["dev_same"] and res["dev_null_same"]
    assert np.all(res["dev_refusals"])


def test_single_environment_dict_and_playout_lookahead(res):
    assert res["compat_same"] and int(res["compat_steps"]) > 0
    assert res["look_shape_ok"] and res["look_same"] and res["look_masked_nan"] and res["look_reject_is_direct"]
    assert float(res["look_spread"]) > 0 and res["look_fresh"]


REFUSED = {"zero_actions": (-1, "n_actions"), "many_actions": (-1, "n_actions"), "zero_samples": (-1, "n_samples"),
           "many_samples": (-1, "n_samples"), "zero_horizon": (-1, "horizon"), "long_horizon": (-1, "horizon"),
           "many_scenarios": (-1, "n_actions * n_samples"), "null_actions": (-1, "actions"), "null_out": (-1, "playout_out"),
           "unknown_flags": (-1, "flags"), "own_stream_samples": (-1, "n_samples"), "window": (-1, "modulations_to_consider"),
           "policy": (-5, "policy"), "track_ids": (-5, "track_service_ids"), "defragmentation": (-5, "defragmentation"),
           "no_source": (-3, "request source"), "trace_seeded": (-3, "ONGYM_PLAYOUT_OWN_STREAM")}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_library_refusals(res, name):
    rc, word = REFUSED[name]
    assert int(res["refuse_rc_" + name]) == rc and word in str(res["refuse_msg_" + name]), str(res["refuse_msg_" + name])
    assert int(res["refuse_rc_ok"]) == 0 and int(res["refuse_rc_trace_own_ok"]) == 0
