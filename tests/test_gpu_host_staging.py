"""Host staging of every entry point that takes host buffers: the four read-only analysis calls (ongym_observe_blocks,
ongym_action_impact, ongym_service_qot, ongym_link_metrics), the step calls, ongym_policy_actions, ongym_observe,
ongym_sample_actions, the two resets and the queries.  With host buffers each call lays its arrays out in the device buffer of
its family, which grows on demand, copies the inputs in, and copies the outputs back; with io_device the kernels get the
caller's pointers (the queries stage under io_device too).  Both must give the same values.
Every GPU computation runs in ONE fresh child process (tests/host_staging_child.py); the tests assert on the .npz it writes.

The shapes are the smallest at which the buffers still have to grow: NSFNET, 100 slots, capacity 128, 3 replicas.  With 100
slots there are 3001 actions, so the rows of an action mask are unaligned inside the staged buffer."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from common import golden_tables, record_bytes

pytestmark = pytest.mark.gpu

B, SEED, STEPS = 3, 21, 150
KW = dict(num_spectrum_resources=100, capacity=128, load=60.0, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400),
          auto_reset=True, episode_length=1000, margin=0.5, launch_power_dbm=1.0)
BLOCKS = (1, 16, 4)             # the buffer grows, then serves a smaller call
IMPACT_A = (1, 256, 9)
SUBSETS = tuple(s for s in itertools.product((0, 1), repeat=3) if any(s))     # which of a call's three arrays are passed
SENTINEL = -12345.5            # no output can be this: counts, shares and metrics are >= 0, dB values are small
NSTEPS = (1, 7, 2)              # ongym_step_policy with records: the buffer grows, then serves a smaller call
RESET_MASK = (1, 0, 1)
QUERY_REPLICA = 1
CAND_ROWS = (1, 63, 64, 65, 1023)
GSNR_COUNTS = (1, 200, 3)


def cand_row(L):
    """the row of length L that ongym_query_candidates gets: about 70 % free"""
    return (np.random.default_rng(SEED + L).random(L) < 0.7).astype(np.int32)


def candidates_np(row, n):
    """_get_candidates by run lengths: start s is feasible when the free run from s, which a virtual free slot after the last
    one extends, holds n slots and the guard slot"""
    free = np.append(np.asarray(row) != 0, True)
    run = np.zeros(len(free) + 1, np.int64)
    for s in range(len(free) - 1, -1, -1):
        run[s] = run[s + 1] + 1 if free[s] else 0
    return [s for s in range(len(row)) if run[s] >= n + 1]


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


def per_replica(res, tag):
    """the snapshot `tag` split by replica: (grid, services, stats) triples"""
    svc = np.split(res[tag + "_services"], np.cumsum(res[tag + "_nservices"])[:-1])
    return [(res[tag + "_grid"][r], svc[r], res[tag + "_stats"][r]) for r in range(B)]


def same_snapshot(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n", NSTEPS)
def test_step_policy_records_host_equals_device(res, n):
    h, d = res[f"h_pol{n}_rec"], res[f"d_pol{n}_rec"]
    assert h.shape == (n, B) and record_bytes(h) == record_bytes(d)
    assert h["accepted"].any() and (h["active"] > 0).all()


def test_policy_actions_and_step_host_equals_device(res):
    for flags in (0, 1):
        assert same_bits(res[f"h_pa{flags}_actions"], res[f"d_pa{flags}_actions"])
        assert same_bits(res[f"h_pa{flags}_actions"], res["h_pa1_actions"]) and res["h_pa1_actions"].min() >= 0
        assert same_bits(res[f"h_pa{flags}_flags"], res[f"d_pa{flags}_flags"])
    assert np.all(res["h_pa0_flags"] == 255) and res["h_pa1_flags"].max() < 255      # NULL flags: nothing written
    assert record_bytes(res["h_step_rec"]) == record_bytes(res["d_step_rec"])
    assert np.array_equal(res["h_step_rec"]["action"], res["h_pa1_actions"])


def test_observe_host_equals_device(res):
    for p in ("", "t"):
        obs, mask = res[p + "h_observe_obs"], res[p + "h_observe_mask"]
        assert same_bits(obs, res[p + "d_observe_obs"]) and same_bits(mask, res[p + "d_observe_mask"])
        assert not np.any(obs == SENTINEL) and set(np.unique(mask)) == {0, 1} and mask.shape[1] == 3001


def test_sample_actions_host_equals_device(res):
    mask, want = res["h_observe_mask"], res["h_sample"]
    assert np.all(mask[np.arange(B), want] == 1) and np.any(want != mask.shape[1] - 1)
    for key in ("d_sample", "th_sample_first", "td_sample_first", "th_sample", "td_sample"):
        assert same_bits(res[key], want), key     # the same mask, seed and draw: before or after the first observation


def test_masked_reset_host_equals_device(res):
    after, h, d = per_replica(res, "h_after"), per_replica(res, "h_reset"), per_replica(res, "d_reset")
    for r, on in enumerate(RESET_MASK):
        assert same_snapshot(h[r], d[r]), r
        if on:
            assert h[r][0].all() and len(h[r][1]) == 0 and h[r][2]["episode_services_accepted"] == 0   # an empty network
        else:
            assert same_snapshot(h[r], after[r]) and len(h[r][1]) > 0


def test_masked_counter_reset_host_equals_device(res):
    before, h, d = per_replica(res, "th_before"), per_replica(res, "th_counters"), per_replica(res, "td_counters")
    assert same_snapshot(before[1], per_replica(res, "td_before")[1])
    for r, on in enumerate(RESET_MASK):
        assert same_snapshot(h[r], d[r]), r
        assert same_bits(h[r][0], before[r][0]) and len(h[r][1]) == len(before[r][1]) > 0     # grid and services stay
        assert before[r][2]["episode_services_processed"] > 0
        if on:
            assert h[r][2]["episode_services_processed"] == 0 and np.all(np.isinf(h[r][1]["release_time"]))
        else:
            assert same_snapshot(h[r], before[r])


def test_services_and_grid_queries(res):
    tb = golden_tables("nsfnet")
    S = KW["num_spectrum_resources"]
    for p in "hd":
        assert res[p + "_fresh_nservices"].tolist() == [0] * B and res[p + "_fresh_grid"].all()
        for grid, svc, _ in per_replica(res, p + "_before"):
            want = np.ones((tb.n_links, S), np.int32)
            for s in svc:                                   # each service holds its slots and, inside the grid, a guard slot
                links = tb.path_links[s["path_id"], :tb.path_hops[s["path_id"]]]
                want[links, s["slot"]:min(s["slot"] + s["nslots"] + 1, S)] = 0
            assert len(svc) > 0 and same_bits(grid, want)
    assert same_bits(res["h_fresh_grid"], res["d_fresh_grid"])


def test_request_and_path_queries(res):
    tb = golden_tables("nsfnet")
    assert same_bits(res["h_q_request"], res["d_q_request"]) and res["h_q_request"]["bit_rate"].min() > 0
    path, avail = int(res["h_q_path"]), res["h_q_avail"]
    assert path == res["d_q_path"] and same_bits(avail, res["d_q_avail"]) and same_bits(res["h_q_free"], res["d_q_free"])
    grid = res["h_before_grid"][QUERY_REPLICA]
    assert np.array_equal(avail, np.logical_and.reduce(grid[tb.path_links[path, :tb.path_hops[path]]], axis=0))
    assert 0 < avail.sum() < len(avail)
    for i, n in enumerate((1, 3)):
        want = np.zeros(len(avail), bool)
        want[candidates_np(avail, n)] = True
        assert np.array_equal(res["h_q_free"][i], want), n


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("L", CAND_ROWS)
def test_candidates_query(res, L, n):
    want = np.array(candidates_np(cand_row(L), n), np.int32)
    assert same_bits(res[f"h_q_cand{L}_{n}"], want) and same_bits(res[f"d_q_cand{L}_{n}"], want)
    assert len(want) > 0 or (L, n) == (1, 3)


def test_gsnr_queries(res):
    cands, alone = res["h_q_cands"], res["h_q_gsnr_alone"]
    assert same_bits(cands, res["d_q_cands"]) and same_bits(alone, res["d_q_gsnr_alone"])
    assert cands.shape == (max(GSNR_COUNTS), 3) and len(np.unique(cands, axis=0)) > 3 and np.isfinite(alone).all()
    for k in GSNR_COUNTS:                                   # each row is the candidate queried alone, bit for bit
        assert same_bits(res[f"h_q_gsnr_many{k}"], alone[:k]) and same_bits(res[f"d_q_gsnr_many{k}"], alone[:k]), k
