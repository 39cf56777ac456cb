"""Host staging of the four read-only analysis calls (ongym_observe_blocks, ongym_action_impact, ongym_service_qot,
ongym_link_metrics).  With host buffers each call lays its arrays out in a device buffer of its own that grows on demand, copies
the inputs in, and copies the outputs back; with io_device the kernels get the caller's pointers.  Both must give the same values.
Every GPU computation runs in ONE fresh child process (tests/host_staging_child.py); the tests assert on the .npz it writes.

The shapes are the smallest at which the buffers still have to grow: NSFNET, 100 slots, capacity 128, 3 replicas."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, SEED, STEPS = 3, 21, 150
KW = dict(num_spectrum_resources=100, capacity=128, load=60.0, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400),
          auto_reset=True, episode_length=1000, margin=0.5, launch_power_dbm=1.0)
BLOCKS = (1, 16, 4)             # the buffer grows, then serves a smaller call
IMPACT_A = (1, 256, 9)
SUBSETS = tuple(s for s in itertools.product((0, 1), repeat=3) if any(s))     # which of a call's three arrays are passed
SENTINEL = -12345.5            # no output can be this: counts, shares and metrics are >= 0, dB values are small


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("host_staging") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_staging_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "host staging child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_values(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def tag(sub):
    return "".join(map(str, sub))


def test_both_environments_are_in_the_same_state(res):
    assert same_bits(res["h_before_grid"], res["d_before_grid"])
    assert same_bits(res["h_before_services"], res["d_before_services"])
    assert res["h_before_nservices"].min() > 0


@pytest.mark.parametrize("J", BLOCKS)
def test_observe_blocks_host_equals_device(res, J):
    assert same_bits(res[f"h_blk{J}_obs"], res[f"d_blk{J}_obs"])
    assert same_bits(res[f"h_blk{J}_mask"], res[f"d_blk{J}_mask"])
    assert same_bits(res[f"h_blk{J}_map"], res[f"d_blk{J}_map"])
    assert res[f"h_blk{J}_mask"].max() == 1 and not np.any(res[f"d_blk{J}_obs"] == SENTINEL)


@pytest.mark.parametrize("A", IMPACT_A)
def test_action_impact_host_equals_device(res, A):
    assert same_bits(res["h_actions"], res["d_actions"])
    for with_svc in (0, 1):
        h, d = res[f"h_imp{A}_{with_svc}"], res[f"d_imp{A}_{with_svc}"]
        assert h.shape == (B, A, 8) and same_values(h, d), with_svc
        assert not np.any(d == SENTINEL)
    assert np.any(res[f"h_imp{A}_0"][:, :, 0] == 0)               # some candidate is allocable


@pytest.mark.parametrize("sub", SUBSETS, ids=tag)
def test_service_qot_subsets_host_equals_device(res, sub):
    for on, name in zip(sub, ("svc", "rep", "link")):
        h, d = res[f"h_qot{tag(sub)}_{name}"], res[f"d_qot{tag(sub)}_{name}"]
        if on:
            assert same_values(h, d), name
            assert same_values(h, res[f"h_qot111_{name}"]), name  # what is computed does not depend on what else is asked for
            assert not np.any(h == SENTINEL), name
        else:
            assert np.all(h == SENTINEL) and np.all(d == SENTINEL), name
    assert res["h_qot111_rep"][:, 0].min() > 0


@pytest.mark.parametrize("sub", SUBSETS, ids=tag)
def test_link_metrics_subsets_host_equals_device(res, sub):
    for on, name in zip(sub, ("link", "comp", "stats")):
        h, d = res[f"h_lm{tag(sub)}_{name}"], res[f"d_lm{tag(sub)}_{name}"]
        if on:
            assert (same_bits if name == "link" else same_values)(h, d), name
            if name != "stats":
                assert same_bits(h, res[f"h_lm110_{name}"]), name
            assert not np.any(h == SENTINEL), name
        else:
            assert np.all(h == SENTINEL) and np.all(d == SENTINEL), name
    if sub[2]:
        # link_stats accumulates: the second call continued from what the caller handed in, the first call's values with the
        # utilisation halved.  last_update is already the current time, so every average stays what went in, up to rounding
        # (x * t / t: two roundings); a call that started from zeros or from another array's bytes would not give this
        first, second = res[f"h_lm{tag(sub)}_stats_first"], res[f"h_lm{tag(sub)}_stats"]
        assert same_values(first, res[f"d_lm{tag(sub)}_stats_first"])
        assert same_bits(first[:, :, 3], second[:, :, 3]) and first[:, :, 3].min() > 0 and first[:, :, 0].max() > 0
        want = first[:, :, :3] * np.array([0.5, 1.0, 1.0])
        np.testing.assert_allclose(second[:, :, :3], want, rtol=1e-12, equal_nan=True)


def test_the_sequence_is_read_only(res):
    for p in "hd":
        for what in ("grid", "services", "nservices", "stats"):
            assert same_bits(res[f"{p}_before_{what}"], res[f"{p}_after_{what}"]), (p, what)
