"""On-device MaskablePPO rollout pieces: GAE over step records (ongym_gae / rl.gae) and the action head on packed masks with any
row count (ongym_masked_categorical_rows / _backward_rows), and tools/bench_rl.py --ppo end to end.  Every GPU computation runs
in ONE fresh child process (tests/rollout_child.py); the tests assert on the .npz it writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("rollout") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rollout_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1500)
    assert run.returncode == 0 and "rollout child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path))


def test_gae_matches_float64_within_the_bound(res):
    bad = [c for c in res["gae_cases"] if not float(res[c + "_excess"]) <= 1.0 or not float(res[c + "_ret_excess"]) <= 1.0]
    assert not bad, [(c, float(res[c + "_excess"]), float(res[c + "_ret_excess"])) for c in bad]


def test_gae_bound_is_met_by_the_sb3_float32_loop(res):
    bad = [c for c in res["gae_cases"] if not float(res[c + "_sb3_excess"]) <= 1.0]
    assert not bad, [(c, float(res[c + "_sb3_excess"])) for c in bad]


def test_gae_nan_pattern_follows_the_recurrence(res):
    for c in res["gae_cases"]:
        assert res[c + "_nan_same"] and res[c + "_ret_nan_same"], c
    assert int(res["gae_nan_nan_count"]) == 101 + 201       # t <= 100 in column 7, t <= 200 in column 3 (across t = 199)


def test_gae_guards_and_inputs_untouched(res):
    for c in res["gae_cases"]:
        assert res[c + "_guards_kept"] and res[c + "_inputs_kept"], c


def test_gae_covers_the_required_shapes(res):
    cases = [str(c) for c in res["gae_cases"]]
    for T in (1, 2, 31, 32, 33, 257, 2048):
        assert any(f"_T{T}_" in c for c in cases), T
    for B in (1, 63, 64, 65, 16384):
        assert any(f"_B{B}_" in c for c in cases), B
    assert "gae_T2048_B16384_random_g0.99_l0.95" in cases
    for gl in ("g1.0_l1.0", "g0.0_l0.95", "g0.99_l0.0"):
        assert any(c.endswith(gl) for c in cases), gl


def test_gae_last_value_ignored_after_a_final_termination(res):
    keys = [k for k in res if k.endswith("_last_ignored")]
    assert keys and all(res[k] for k in keys)


def test_gae_on_environment_records(res):
    """NSFNET-320 with episode_length 40: every replica ends several episodes inside the rollout"""
    assert int(res["gae_env_terminations"]) >= 1024 * 5
    assert float(res["gae_env_excess"]) <= 1.0 and res["gae_env_nan_same"]


@pytest.mark.parametrize("cfg", ("nsf", "mc2"))
def test_mask_bits_out_is_the_packed_mask(res, cfg):
    assert res[f"{cfg}_bits_match_packbits"]


@pytest.mark.parametrize("cfg", ("nsf", "mc2"))
def test_packed_mask_bit_identical_to_bytes(res, cfg):
    assert res[f"{cfg}_bits_equal_bytes_RB"]
    for k in res:
        if k.startswith(f"{cfg}_mb") and k.endswith("_bits_equal_bytes"):
            assert res[k], k


@pytest.mark.parametrize("cfg", ("nsf", "mc2"))
def test_rows_variant_bit_identical_to_the_batch_call(res, cfg):
    assert res[f"{cfg}_rows_equal_legacy"]


@pytest.mark.parametrize("cfg", ("nsf", "mc2"))
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_minibatch_matches_float64(res, cfg, dt):
    B = {"nsf": 64, "mc2": 48}[cfg]
    for R in (4097, 3 * B + 1):
        tag = f"{cfg}_mb{R}_{dt}"
        assert res[tag + "_outside"], tag
        assert float(res[tag + "_lp_err"]) <= 1e-4, tag
        assert float(res[tag + "_H_err"]) <= 1e-4, tag
        # bf16 gradients are rounded to bf16 on output: 2^-8 of the largest entry
        tol = 1e-4 if dt == "f32" else 1e-4 + float(res[tag + "_grad_scale"]) * 2.0 ** -8
        assert float(res[tag + "_grad_err"]) <= tol, tag


def test_ppo_end_to_end(res):
    assert int(res["ppo_rc"]) == 0, str(res["ppo_log"])
    r = json.loads(str(res["ppo_json"]))
    assert r["config"]["ppo"]["n_steps"] == 8 and r["config"]["ppo"]["epochs"] == 1 and r["config"]["ppo"]["gae"] == "ongym_gae"
    for k in ("policy_loss", "value_loss", "entropy", "loss"):
        assert np.isfinite(r["losses"][k]), k
    assert np.isfinite(r["param_delta"]) and r["param_delta"] > 0
    for k in ("rollout", "gae", "update"):
        assert r["phase_ms"][k] > 0, k
