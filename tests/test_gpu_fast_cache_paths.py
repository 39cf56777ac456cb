"""The interferer cache of the lean kernels (csrc/ongym_fast.hpp: build_cache, gather, eval_one) in all three regimes of its
narrow instantiation (ENT = 2: two register groups of 64 interferers, the rest read from the LDS list in eval_one): at most 64
interferers on the evaluated route, 65..128, and more than 128.  First fit and load balancing on NSFNET, S = 320, capacity
448, against the CPU oracle (step records, final grids) at three loads.

The test proves its coverage from the oracle's side: every SAMPLE_EVERY steps it counts, from OracleEnv.services() and the
tables' route link lists, the running services that share a link with the first route of the pending request
(OracleEnv.request()), and every replica must have seen each regime at least once over the three runs.  Rejected requests
and first routes without any start (no free run for the narrowest format) must occur too, and the service table must not
overflow.  The loads were chosen with exactly this count on the CPU (first fit, seed 11, 8 replicas, 1500 steps, 150 samples
per replica); shares of the samples per regime, ranges over the replicas:

    load   <= 64        65..128      > 128        largest count   no start   rejected   most services
      60   1.00         0            0            32..48          0          0          73..85
     350   0.61..0.68   0.28..0.36   0.01..0.04   140..181        2..8       11..39     308..356
     480   0.55..0.64   0.30..0.43   0.02..0.10   168..202        5..15      29..63     387..420

Load balancing spreads the services over more routes, so the upper regimes are more frequent: at load 350 the shares are
0.40..0.48 / 0.43..0.52 / 0.05..0.13, at load 480 0.35..0.49 / 0.39..0.52 / 0.08..0.17, at load 60 every sample has at most
59 interferers.  The test prints the shares of every (policy, load, replica) before it asserts.
"""
import numpy as np
import pytest

from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from oracle_lib import OracleEnv

pytestmark = pytest.mark.gpu

GSNR_RTOL = 1e-9
EXACT = ("action", "route", "modulation", "slot", "nslots", "accepted", "terminated", "retry", "flags", "active", "reward")
LOADS = (60.0, 350.0, 480.0)
B, STEPS, SAMPLE_EVERY, SEED = 8, 1500, 10, 11
S, CAPACITY = 320, 448


def assert_records_equal(got, want, ctx=""):
    for f in EXACT:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(got[f] != want[f])[0]
            raise AssertionError(f"{ctx}: field {f} differs first at {tuple(bad)}: {got[f][tuple(bad)]} != {want[f][tuple(bad)]}")
    for f in ("osnr", "ase", "nli"):
        np.testing.assert_allclose(got[f], want[f], rtol=GSNR_RTOL, err_msg=f"{ctx}: {f}")


def config(load):
    return dict(modulations=jocn_modulations(), num_spectrum_resources=S, capacity=CAPACITY, load=load,
                bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), auto_reset=True, episode_length=1000)


def routes_sharing_a_link(tb):
    """share[a, b]: routes a and b have a link in common (from the tables' link lists)."""
    sets = [frozenset(int(l) for l in row[:h]) for row, h in zip(tb.path_links, tb.path_hops)]
    return np.array([[bool(a & b) for b in sets] for a in sets])


def oracle_run(o, tb, share, pid, n_mods):
    """STEPS steps of policy `pid` on the oracle; returns its records, the interferer counts on the first route of the pending
    request at the sampled steps, the number of sampled first routes without any start, and the largest number of services."""
    recs, counts, no_start, most = [], [], 0, 0
    for _ in range(0, STEPS, SAMPLE_EVERY):
        q = o.request()
        p0 = int(tb.pair_paths[int(q["source"]), int(q["destination"]), 0])
        sv = o.services()
        counts.append(int(share[p0, sv["path_id"]].sum()))
        most = max(most, len(sv))
        widths = [o.number_slots(float(q["bit_rate"]), m) for m in range(n_mods)]
        if not o.candidates(o.available(p0), min(n for n in widths if n > 0)):
            no_start += 1
        recs.append(o.run_policy(pid, SAMPLE_EVERY))
    return np.concatenate(recs), np.array(counts), no_start, most


@pytest.mark.parametrize("pid", [nat.POLICY_FIRST_FIT, nat.POLICY_LOAD_BALANCING], ids=["first_fit", "load_balancing"])
def test_cache_regimes_vs_oracle(pid):
    tb = golden_tables("nsfnet")
    share = routes_sharing_a_link(tb)
    n_mods = len(jocn_modulations())
    seen = np.zeros((B, 3), bool)            # per replica: <= 64, 65..128, > 128 interferers on the sampled route
    rejected = no_start = 0
    for load in LOADS:
        kw = config(load)
        holder = nat.ConfigHolder(tb, batch=B, **kw)
        env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
        env.seed(SEED); env.reset()
        occ = env.occupancy(pid)
        assert occ["lean_kernel"]
        got = env.step_policy(STEPS, policy=pid)
        for r in range(B):
            o = OracleEnv(holder, replica=r)
            o.seed(SEED); o.reset()
            want, counts, ns, most = oracle_run(o, tb, share, pid, n_mods)
            print(f"policy {pid} load {load:.0f} replica {r}: <=64 {np.mean(counts <= 64):.2f}  65..128 "
                  f"{np.mean((counts > 64) & (counts <= 128)):.2f}  >128 {np.mean(counts > 128):.2f}  largest {counts.max()}  "
                  f"no start {ns}  rejected {int((want['accepted'] == 0).sum())}  most services {most}")
            assert most < CAPACITY and not (want["flags"] & nat.F_OVERFLOW).any()
            seen[r] |= [(counts <= 64).any(), ((counts > 64) & (counts <= 128)).any(), (counts > 128).any()]
            rejected += int((want["accepted"] == 0).sum())
            no_start += ns
            ctx = f"policy {pid} load {load:.0f} replica {r}"
            assert_records_equal(got[:, r], want, ctx)
            np.testing.assert_array_equal(env.grid(r), o.grid(), err_msg=ctx)
    assert seen.all(), seen
    assert rejected > 0 and no_start > 0, (rejected, no_start)
