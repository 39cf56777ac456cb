"""Masked categorical action head (ongym_masked_categorical / _backward through optical_networking_gym.rl) against float64
torch on NSFNET-320 (k = 5, six formats: 9601 actions) and a second action space (modulations_to_consider = 2, S = 160).
Every GPU computation runs in ONE fresh child process per module (tests/policy_head_child.py; PyTorch's HIP runtime and this
library's must start together): the tests assert on the .npz it writes."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

pytestmark = pytest.mark.gpu
CONFIGS = ("nsf", "mc2")


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("policy_head") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "policy_head_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "policy head child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path))


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_evaluate_matches_float64(res, cfg, dt):
    lp, H = res[f"{cfg}_eval_{dt}_lp"], res[f"{cfg}_eval_{dt}_H"]
    lp_ref, H_ref = res[f"{cfg}_eval_{dt}_lp_ref"], res[f"{cfg}_eval_{dt}_H_ref"]
    outside = np.isneginf(lp_ref)
    assert outside[::8].all() and outside[3] and (~outside).sum() > len(lp) // 2     # masked, out of range, valid actions
    assert np.array_equal(np.isneginf(lp), outside)
    np.testing.assert_allclose(lp[~outside], lp_ref[~outside], rtol=0, atol=1e-4)
    assert (np.abs(H - H_ref) <= 1e-4 * np.maximum(1.0, H_ref)).all()


@pytest.mark.parametrize("cfg", CONFIGS)
def test_sample_valid_deterministic_and_exact_log_prob(res, cfg):
    mask = res[f"{cfg}_mask"]
    a1, a2, a3 = res[f"{cfg}_sample_a1"], res[f"{cfg}_sample_a2"], res[f"{cfg}_sample_a3"]
    rows = np.arange(len(a1))
    assert mask[rows, a1].all() and mask[rows, a3].all()
    assert np.array_equal(a1, a2) and not np.array_equal(a1, a3)
    np.testing.assert_allclose(res[f"{cfg}_sample_lp"], res[f"{cfg}_sample_lp_ref"], rtol=0, atol=1e-4)
    H, H_ref = res[f"{cfg}_sample_H"], res[f"{cfg}_sample_H_ref"]
    assert (np.abs(H - H_ref) <= 1e-4 * np.maximum(1.0, H_ref)).all()


def test_sample_frequencies_follow_the_softmax(res):
    """rows cut to 11 valid entries (entries 0-2 and the last three among them: the row's unaligned head and tail) with logits
    over -5..5; masked entries hold 50.  Chi-square per row (bins with an expected count < 5 merged) at p < 1e-4."""
    counts, p, D = res["chi_counts"], res["chi_p"], int(res["chi_total"])
    assert res["chi_valid"] and (counts.sum(1) == D).all()
    for r in range(len(counts)):
        exp = p[r] * D
        small = exp < 5
        o = np.append(counts[r][~small], counts[r][small].sum())
        e = np.append(exp[~small], exp[small].sum())
        chi2 = ((o - e) ** 2 / e).sum()
        assert stats.chi2.sf(chi2, len(o) - 1) > 1e-4, (r, counts[r], exp)


def test_mean_log_prob_of_draws_is_minus_entropy(res):
    lp, H = res["mlp_lp"].astype(np.float64), res["mlp_H"].astype(np.float64)
    diff = lp + H[None, :]                     # E[log p(a)] + H = 0 for every row
    se = diff.std() / np.sqrt(diff.size)
    assert abs(diff.mean()) < 5 * se, (diff.mean(), se)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_argmax_is_torch_argmax_with_ties(res, cfg, dt):
    assert np.array_equal(res[f"{cfg}_argmax_{dt}"], res[f"{cfg}_argmax_{dt}_ref"])


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_backward_matches_float64_autograd_after_the_mask_is_overwritten(res, cfg, dt):
    assert res[f"{cfg}_bwd_{dt}_mask_changed"]
    g, ref, mask = res[f"{cfg}_bwd_{dt}_grad"], res[f"{cfg}_bwd_{dt}_grad_ref"], res[f"{cfg}_bwd_{dt}_mask"].astype(bool)
    assert (g[~mask] == 0).all()
    if dt == "f32":
        np.testing.assert_allclose(g, ref, rtol=0, atol=1e-5)
    else:                                      # bf16 gradient: one rounding of the f32 value (8 bits of mantissa)
        np.testing.assert_allclose(g, ref, rtol=2 ** -8, atol=1e-6)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_edge_rows(res, cfg):
    assert res[f"{cfg}_edge_junk_equal"]       # NaN / +inf / -inf in masked entries change nothing, in every mode
    n = res[f"{cfg}_mask"].shape[1]
    a, lp, H, lpe = res[f"{cfg}_edge_a"], res[f"{cfg}_edge_lp"], res[f"{cfg}_edge_H"], res[f"{cfg}_edge_eval_lp"]
    assert (a[0], lp[0], H[0], lpe[0]) == (n - 1, 0.0, 0.0, 0.0)                           # only the reject entry valid
    assert a[1] == n - 1 and np.isnan(lp[1]) and np.isnan(H[1]) and np.isnan(lpe[1])     # nothing valid
    assert np.isfinite(lp[2:]).all()
    mask, a = res[f"{cfg}_after_mask"], res[f"{cfg}_after_a"]                               # the next call works
    assert mask[np.arange(len(a)), a].all()
    np.testing.assert_allclose(res[f"{cfg}_after_lp"], res[f"{cfg}_after_lp_ref"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(res[f"{cfg}_after_H"], res[f"{cfg}_after_H_ref"], rtol=1e-4, atol=1e-4)


def test_sharded_envs_draw_the_same_actions(res):
    assert np.array_equal(res["shard_8"], res["shard_4x2"])
    assert len(np.unique(res["shard_8"][:, 0])) > 1


def test_end_to_end_rollout_with_backward(res):
    from optical_networking_gym import _native as nat
    assert res["e2e_logits_dtype_bf16"] and res["e2e_valid"] and res["e2e_grad_finite"]
    assert not (res["e2e_flags"] & nat.F_QOT_ERROR).any()
