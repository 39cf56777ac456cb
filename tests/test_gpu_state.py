"""Save, restore and fork replica states (ongym_state_save / ongym_state_load / ongym_fork through BatchedQRMSAEnv).  Every GPU
computation runs in ONE fresh child process (tests/state_child.py); the tests assert on the .npz it writes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import load_traj
from optical_networking_gym import _native as nat

pytestmark = pytest.mark.gpu

TRAJ = ("traj_nsfnet320", "traj_nobeleu320", "traj_nsfnet320_defrag", "traj_nsfnet320_disr")
GSNR_RTOL = 1e-9
EXACT = ("action", "route", "modulation", "slot", "nslots", "accepted", "terminated", "retry", "flags", "active", "reward")


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("state") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "state_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1200)
    assert run.returncode == 0 and "state child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path))


def assert_golden(rec, d, first=0, ctx=""):
    """rec [n - first] of one replica against the golden st_* arrays from step `first` on (the parity test's fields and bars)"""
    sl = slice(first, first + len(rec))
    for f, g in (("action", "st_action"), ("accepted", "st_accepted"), ("terminated", "st_term"), ("reward", "st_reward"),
                 ("active", "st_active"), ("route", "st_route"), ("slot", "st_slot")):
        assert np.array_equal(rec[f], d[g][sl]), (ctx, f)
    acc = d["st_accepted"][sl] == 1
    assert np.array_equal(rec["modulation"][acc], d["st_mod"][sl][acc]), ctx
    assert np.array_equal(rec["nslots"][acc], d["st_n"][sl][acc]), ctx
    assert np.array_equal((rec["flags"] & nat.F_BLOCKED_RESOURCES) != 0, d["st_bres"][sl] == 1), ctx
    assert np.array_equal((rec["flags"] & nat.F_BLOCKED_OSNR) != 0, d["st_bosnr"][sl] == 1), ctx
    for f, g in (("osnr", "st_osnr"), ("ase", "st_ase"), ("nli", "st_nli")):
        want = d[g][sl]
        known = np.isfinite(want)       # some captures did not record ase / nli (NaN)
        np.testing.assert_allclose(rec[f][known], want[known], rtol=GSNR_RTOL, err_msg=f"{ctx}: {f}")


@pytest.mark.parametrize("tag", TRAJ)
def test_replay_from_a_saved_state_equals_the_reference(res, tag):
    _, d = load_traj(tag)
    for key in ("_recA", "_recB"):
        rec = res[tag + key]
        for r in range(rec.shape[1]):
            assert_golden(rec[:, r], d, ctx=f"{tag}{key} replica {r}")
    assert res[tag + "_bits_same"] and res[tag + "_grids_same"] and res[tag + "_stats_same"], tag
    assert res[tag + "_totals_count"], tag


def test_replay_covers_the_lean_and_generic_kernels(res):
    assert res["traj_nobeleu320_lean"] and res["traj_nsfnet320_lean"]
    assert not res["traj_nsfnet320_defrag_lean"] and not res["traj_nsfnet320_disr_lean"]


def test_fork_is_pinned_to_the_reference(res):
    _, d = load_traj("traj_nsfnet320")
    K = int(res["pin_K"])
    rec = res["pin_rec_fork"]
    for r in range(rec.shape[1]):
        assert_golden(rec[:, r], d, first=K, ctx=f"forked replica {r}")
    nofork = res["pin_rec_nofork"]
    assert_golden(nofork[:, 0], d, first=K, ctx="replica 0 without the fork")
    for r in range(1, nofork.shape[1]):      # without the fork the others are elsewhere
        assert not all(np.array_equal(nofork[f][:, r], rec[f][:, r]) for f in EXACT), r


@pytest.mark.parametrize("name", ["reverse", "cycle3", "mix"])
def test_overlapping_forks_follow_an_unforked_twin(res, name):
    assert res[f"overlap_{name}_rec"] and res[f"overlap_{name}_obs"], name
    assert int(res[f"overlap_{name}_moved"]) > 0


def test_fork_leaves_unchanged_replicas_alone(res):
    assert int(res["overlap_keep_count"]) > 0 and res["overlap_unchanged_grids"]


def test_keep_stream_serves_the_pending_request_then_the_own_stream_at_the_source_counter(res):
    assert res["ks_grid_is_source"] and res["ks_pending_is_source"]
    f, t, D = res["ks_req_fork"], res["ks_req_twin"], int(res["ks_shift"])
    assert D > 0
    assert f[:, 0].tobytes() == t[:, 0].tobytes()                  # the source itself is unchanged
    fd, td = f[:-D, 1:], t[D:, 1:]                                 # destination j at counter c + D + i = twin j at c + (i + D)
    for fld in ("source", "destination", "bit_rate", "holding_time"):
        assert np.array_equal(fd[fld], td[fld]), fld
    df, dt = np.diff(fd["arrival_time"], axis=0).astype(np.float64), np.diff(td["arrival_time"], axis=0).astype(np.float64)
    tol = 4 * np.spacing(np.maximum(np.abs(fd["arrival_time"][1:]), np.abs(td["arrival_time"][1:])).astype(np.float32))
    assert np.all(np.abs(df - dt) <= tol)
    assert not np.array_equal(fd["source"], t[:-D, 1:]["source"])   # not at the destination's own counter
    assert not np.array_equal(f["source"][:, 1:], np.repeat(f["source"][:, :1], f.shape[1] - 1, axis=1))   # own streams


def test_blob_of_an_unreplayable_trace_keeps_the_destination_generic(res):
    assert not res["guard_src_lean"] and int(res["guard_max_nslots"]) > 32
    assert res["guard_lean_before"] and not res["guard_lean_after"]
    assert res["guard_follows_generic"]


def test_fresh_environment_takes_the_generator_from_a_full_load(res):
    assert res["fresh_lean"] and res["fresh_follows"]
    assert int(res["fresh_partial_refused"]) == -3          # ONGYM_E_STATE: no request source


def test_keep_params_follows_the_destination_power(res):
    assert len(res["kp_src_noflag"]) >= 3
    np.testing.assert_array_equal(res["kp_dst_noflag"], res["kp_src_noflag"])
    sh = float(res["kp_shift_db"])
    src, dst = res["kp_src_flag"], res["kp_dst_flag"]
    np.testing.assert_allclose(dst[:, 1], src[:, 1] + sh, rtol=1e-9)            # ASE: +10 log10(Pb/Pa)
    np.testing.assert_allclose(dst[:, 2], src[:, 2] - 2 * sh, rtol=1e-9)        # NLI: -20 log10(Pb/Pa)
    np.testing.assert_array_equal(res["kpl_noflag"], res["kpl_src"])
    np.testing.assert_allclose(res["kpl_flag"][:, 1], res["kpl_src"][:, 1] + sh, rtol=1e-9)
    np.testing.assert_allclose(res["kpl_flag"][:, 2], res["kpl_src"][:, 2] - 2 * sh, rtol=1e-9)


@pytest.mark.parametrize("build", ["narrow", "wide"])
def test_states_load_across_environments(res, build):
    assert res[f"across_{build}_lean"]
    assert res[f"across_{build}_p0"] and res[f"across_{build}_p10"] and res[f"across_{build}_stats"]


def test_bad_loads_and_forks_are_refused(res):
    for k in ("slots", "capacity", "topology", "count", "duplicate", "magic", "fingerprint", "fork_src", "truncated"):
        assert int(res[f"refuse_{k}"]) == -1, k
    assert res["across_after_refusals"] and res["across_nbytes"]
