"""Masked categorical action head at its edges, against float64 torch: every residue of n_actions mod 8 at three row sizes
(2..9, ~2000, ~25 000), batch tails, mask patterns on the partial chunks and lane boundaries, the packed mask, guarded
outputs, argmax ties where the lane merge order matters, common offsets and extreme logits, non-finite logits in valid
entries, the backward's optional arguments and the n_actions limit.  Every GPU computation runs in ONE fresh child process
(tests/policy_head_edges_child.py): the tests assert on the .npz it writes."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from policy_head_edges_child import SHAPES  # noqa: E402   (no GPU work at import)

GEO = [s[0] for s in SHAPES]
NONFINITE = ("m2001", "m2036")
TIES = ("m2016", "m2021", "l25401", "l25576")
DT = ("f32", "bf16")


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("policy_head_edges") / "out.npz"
    run = subprocess.run([sys.executable, os.path.join(HERE, "policy_head_edges_child.py"), str(path)], capture_output=True,
                         text=True, timeout=900)
    assert run.returncode == 0 and "policy head edges child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path))


def section(res, name):
    assert res[f"ok_{name}"], str(res.get(f"err_{name}", ""))


def close_H(H, H_ref):
    return np.abs(H - H_ref) <= 1e-4 * np.maximum(1.0, np.abs(H_ref))


def assert_grad(g, ref, dt):
    if dt == "f32":
        np.testing.assert_allclose(g, ref, rtol=0, atol=1e-5)
    else:                                      # one bf16 rounding of the f32 value
        np.testing.assert_allclose(g, ref, rtol=2 ** -8, atol=1e-6)


def test_shapes_cover_every_residue_at_three_sizes(res):
    for size in "tml":
        ns = [int(res[f"{t}_n"]) for t in GEO if t[0] == size and f"{t}_n" in res]
        assert sorted(n % 8 for n in ns) == list(range(8)), (size, ns)
    assert max(int(res[f"{t}_n"]) for t in GEO if f"{t}_n" in res) > 25000
    assert {int(res[f"{t}_B"]) % 4 for t in GEO if f"{t}_B" in res} == {1, 2, 3}


@pytest.mark.parametrize("tag", GEO)
@pytest.mark.parametrize("dt", DT)
def test_geometry_forward_vs_float64(res, tag, dt):
    section(res, f"geo_{tag}")
    k = f"{tag}_{dt}"
    assert (res[k + "_rc"] == 0).all()
    mask = res[f"{tag}_mask"] != 0
    rows = np.arange(mask.shape[0])
    a = res[k + "_sample_a"]
    assert mask[rows, a].all()
    np.testing.assert_allclose(res[k + "_sample_lp"], res[k + "_sample_lp_ref"], rtol=0, atol=1e-4)
    assert np.array_equal(res[k + "_argmax_a"], res[k + "_argmax_ref"])
    lp, lp_ref = res[k + "_eval_lp"], res[k + "_eval_lp_ref"]
    out = np.isneginf(lp_ref)
    assert np.array_equal(np.isneginf(lp), out)
    np.testing.assert_allclose(lp[~out], lp_ref[~out], rtol=0, atol=1e-4)
    for mode in ("sample", "argmax", "eval"):
        assert close_H(res[f"{k}_{mode}_H"], res[k + "_H_ref"]).all(), mode


@pytest.mark.parametrize("tag", GEO)
@pytest.mark.parametrize("dt", DT)
def test_geometry_backward_vs_float64(res, tag, dt):
    section(res, f"geo_{tag}")
    k = f"{tag}_{dt}"
    g, mask = res[k + "_grad"], res[f"{tag}_mask"] != 0
    assert (g[~mask] == 0).all()
    assert_grad(g, res[k + "_grad_ref"], dt)


@pytest.mark.parametrize("tag", GEO)
@pytest.mark.parametrize("dt", DT)
def test_mask_bits_are_the_packed_mask(res, tag, dt):
    section(res, f"geo_{tag}")
    bits, want = res[f"{tag}_{dt}_bits"], res[f"{tag}_{dt}_bits_ref"]
    for b in bits:                             # sample, argmax, evaluate
        assert np.array_equal(b, want)


@pytest.mark.parametrize("tag", GEO)
@pytest.mark.parametrize("dt", DT)
def test_outputs_written_in_range_and_guards_untouched(res, tag, dt):
    section(res, f"geo_{tag}")
    assert res[f"{tag}_{dt}_guard"].all()      # sample, argmax, evaluate, backward
    assert res[f"{tag}_{dt}_written"].all()


@pytest.mark.parametrize("tag", TIES)
@pytest.mark.parametrize("dt", DT)
def test_argmax_ties_where_the_merge_order_matters(res, tag, dt):
    section(res, f"ties_{tag}")
    assert np.array_equal(res[f"{tag}_{dt}_ties_a"], res[f"{tag}_{dt}_ties_ref"])


@pytest.mark.parametrize("case", [("f32", c) for c in ("+1e+02", "-1e+02", "+1e+03", "-1e+03", "+1e+04", "-1e+04")]
                         + [("bf16", "+1e+02"), ("bf16", "-1e+02")])
def test_common_offset_is_shift_invariant(res, case):
    section(res, "vals")
    dt, c = case
    k = f"off_{dt}_{c}"
    np.testing.assert_allclose(res[k + "_lp"], res[k + "_lp_ref"], rtol=0, atol=1e-4)
    assert close_H(res[k + "_H"], res[k + "_H_ref"]).all()
    assert_grad(res[k + "_grad"], res[k + "_grad_ref"], dt)


def test_flat_peaked_and_extreme_rows(res):
    section(res, "vals")
    H, H_ref, nvalid = res["vals_H"], res["vals_H_ref"], res["vals_nvalid"]
    np.testing.assert_allclose(H[2:], np.log(nvalid[2:]), rtol=0, atol=1e-5)      # flat rows: H = log #valid
    assert close_H(H, H_ref).all()                                                 # peaked row 0, +-3e38 row 1
    for lp, ref in ((res["vals_lp"], res["vals_lp_ref"]), (res["vals_sample_lp"], res["vals_sample_lp_ref"])):
        assert not np.isnan(lp).any()
        far = ref < -1e30                      # float64 log p below -1e30 may come out as -inf
        assert (np.isneginf(lp[far]) | (lp[far] < -1e30)).all()
        np.testing.assert_allclose(lp[~far], ref[~far], rtol=0, atol=1e-4)
    assert res["vals_mask"][np.arange(len(H)), res["vals_sample_a"]].all()
    assert not np.isnan(res["vals_grad"]).any()
    np.testing.assert_allclose(res["vals_grad"], res["vals_grad_ref"], rtol=0, atol=1e-5)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("tag", NONFINITE)
@pytest.mark.parametrize("dt", DT)
def test_minus_inf_valid_entry_is_that_entry_masked_bit_for_bit(res, tag, dt):
    section(res, f"nonfinite_{tag}")
    k = f"nf_{tag}_{dt}"
    ninf, mask = res[k + "_ninf"], res[k + "_mask"]
    assert ninf[0, :500].any() and ninf[-1][mask[-1]].all()
    for mode in ("sample", "argmax", "eval"):
        for what in ("a", "lp", "H"):
            assert _same(res[f"{k}_inf_{mode}_{what}"], res[f"{k}_masked_{mode}_{what}"]), (mode, what)
    assert _same(res[k + "_inf_grad"], res[k + "_masked_grad"])
    assert (res[k + "_inf_grad"][ninf | ~mask] == 0).all()
    lp, lp_ref = res[k + "_inf_eval_lp"], res[k + "_eval_lp_ref"]
    assert np.isneginf(lp[1])                  # the evaluated action's logit is -inf
    rows = np.arange(len(lp) - 1)              # the last row has only -inf valid entries
    fin = np.isfinite(lp_ref[rows])
    np.testing.assert_allclose(lp[rows][fin], lp_ref[rows][fin], rtol=0, atol=1e-4)
    assert close_H(res[k + "_inf_eval_H"][rows], res[k + "_H_ref"][rows]).all()
    n = mask.shape[1]
    for mode in ("sample", "argmax"):          # every valid entry -inf: no valid entry (reject, NaN)
        assert res[f"{k}_inf_{mode}_a"][-1] == n - 1
    for mode in ("sample", "argmax", "eval"):
        assert np.isnan(res[f"{k}_inf_{mode}_lp"][-1]) and np.isnan(res[f"{k}_inf_{mode}_H"][-1])


@pytest.mark.parametrize("tag", NONFINITE)
@pytest.mark.parametrize("dt", DT)
def test_nan_or_plus_inf_valid_entry_poisons_only_its_row(res, tag, dt):
    section(res, f"nonfinite_{tag}")
    k = f"nf_{tag}_{dt}"
    bad, mask = res[k + "_poison_rows"], res[k + "_mask"]
    other = np.setdiff1d(np.arange(mask.shape[0]), bad)
    for mode in ("sample", "argmax", "eval"):
        lp, H = res[f"{k}_poison_{mode}_lp"], res[f"{k}_poison_{mode}_H"]
        assert np.isnan(lp[bad]).all() and np.isnan(H[bad]).all(), mode
        for what in ("a", "lp", "H"):
            assert _same(res[f"{k}_poison_{mode}_{what}"][other], res[f"{k}_clean_{mode}_{what}"][other]), (mode, what)
    for mode in ("sample", "argmax"):
        a = res[f"{k}_poison_{mode}_a"]
        assert mask[np.arange(len(a)), a].all(), mode


@pytest.mark.parametrize("tag", NONFINITE)
@pytest.mark.parametrize("dt", DT)
def test_backward_optional_gradients_and_empty_rows(res, tag, dt):
    section(res, f"bwd_{tag}")
    k = f"be_{tag}_{dt}"
    mask = res[k + "_mask"]
    assert res[k + "_sample_a"][0] == mask.shape[1] - 1 and res[k + "_sample_a"][1] == mask.shape[1] - 1
    for name in ("nolp", "noH", "both"):
        assert res[f"{k}_{name}_ok"].all(), name                 # rc 0, guard untouched, every element written
        g = res[f"{k}_{name}_grad"]
        assert not np.isnan(g).any() and (g[~mask] == 0).all() and (g[:2] == 0).all(), name
        assert_grad(g, res[f"{k}_{name}_grad_ref"], dt)


@pytest.mark.parametrize("tag", NONFINITE)
@pytest.mark.parametrize("dt", DT)
def test_autograd_evaluate_with_actions_outside_the_mask(res, tag, dt):
    section(res, f"bwd_{tag}")
    k = f"be_{tag}_{dt}"
    mask, acts = res[k + "_mask"], res[k + "_auto_acts"]
    n = mask.shape[1]
    outside = (acts < 0) | (acts >= n)
    outside[~outside] = ~mask[np.arange(len(acts))[~outside], acts[~outside]]
    assert outside[2:].sum() >= 4 and (acts < 0).any() and (acts >= n).any()
    lp = res[k + "_auto_lp"]
    assert np.isneginf(lp[outside & mask.any(1)]).all() and lp[0] == 0 and np.isnan(lp[1])
    g = res[k + "_auto_grad"]
    assert not np.isnan(g).any() and (g[:2] == 0).all() and (g[~mask] == 0).all()
    assert_grad(g, res[k + "_auto_grad_ref"], dt)


@pytest.mark.parametrize("tag", ("m2016", "m2021"))
def test_sample_frequencies_follow_the_softmax_at_new_shapes(res, tag):
    """~100 valid entries over every lane and both partial chunks, ties on both entries of two counter pairs; masked entries
    hold 60.  Chi-square per row (bins with an expected count < 5 merged) at p < 1e-4."""
    section(res, f"chi_{tag}")
    counts, p, D = res[f"{tag}_chi_counts"], res[f"{tag}_chi_p"], int(res[f"{tag}_chi_total"])
    assert res[f"{tag}_chi_valid"] and (counts.sum(1) == D).all()
    for r in range(len(counts)):
        used = p[r] > 0
        exp = p[r][used] * D
        small = exp < 5
        o = np.append(counts[r][used][~small], counts[r][used][small].sum())
        e = np.append(exp[~small], exp[small].sum())
        if e[-1] == 0:
            o, e = o[:-1], e[:-1]
        chi2 = ((o - e) ** 2 / e).sum()
        assert stats.chi2.sf(chi2, len(o) - 1) > 1e-4, (r, counts[r], exp)


def test_n_actions_limit(res):
    section(res, "limit")
    from optical_networking_gym import _native as nat   # noqa: F401
    assert int(res["lim_ok_n"]) == 128899 and int(res["lim_over_n"]) == 135037
    assert int(res["lim_ok_rc"]) == 0 and res["lim_ok_guard"] and res["lim_ok_written"]
    np.testing.assert_allclose(res["lim_ok_lp"], res["lim_ok_lp_ref"], rtol=0, atol=1e-4)
    assert close_H(res["lim_ok_H"], res["lim_ok_H_ref"]).all()
    assert np.array_equal(res["lim_ok_bits"], res["lim_ok_bits_ref"])
    assert int(res["lim_over_rc"]) == -5 and res["lim_over_untouched"] and res["lim_over_guard"]     # ONGYM_E_LIMIT
