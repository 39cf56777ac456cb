"""First fit and load balancing in the lean kernel decide every format of one slot width from one GN evaluation
(csrc/ongym_fast.hpp, eval_one): the formats of the same width that the walk would visit next share the start and the
interferer sum, so their lanes' decisions are read from the same ballots.  These tests hold that to the CPU oracle on loaded
networks, records (OSNR / ASE / NLI included), grids and statistics, with the JOCN table and with a table whose slot counts
are not monotone in the format index (the group must stop at the first feasible format of another width)."""
import numpy as np
import pytest

from common import golden_tables, jocn_modulations, record_bytes
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from optical_networking_gym.topology import Modulation
from oracle_lib import OracleEnv

pytestmark = pytest.mark.gpu

GSNR_RTOL = 1e-9
EXACT = ("action", "route", "modulation", "slot", "nslots", "accepted", "terminated", "retry", "flags", "active", "reward")
STATS = ("services_processed", "services_accepted", "episode_services_processed", "episode_services_accepted",
         "bit_rate_requested", "bit_rate_provisioned", "episode_bit_rate_provisioned", "rejected", "episodes_completed",
         "total_steps", "total_accepted", "total_paths_tried", "total_path_hops", "total_active_sum", "current_time", "active")


def shuffled_modulations():
    """The JOCN formats in another index order: walked from the highest index, the 100G widths are 2, 2, 3, 2, 4, 8 and the
    40G widths 1, 1, 2, 1, 2, 4 — the formats of one width are not contiguous."""
    bpsk, qpsk, qam8, qam16, qam32, qam64 = jocn_modulations()
    return (bpsk, qpsk, qam16, qam8, qam64, qam32)


def assert_records_equal(got, want, ctx=""):
    for f in EXACT:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(got[f] != want[f])[0]
            raise AssertionError(f"{ctx}: field {f} differs first at {tuple(bad)}: {got[f][tuple(bad)]} != {want[f][tuple(bad)]}")
    for f in ("osnr", "ase", "nli"):
        np.testing.assert_allclose(got[f], want[f], rtol=GSNR_RTOL, err_msg=f"{ctx}: {f}")


def run_case(topo, mods, pid, S, load, steps, B, seed, wide, monkeypatch, warm=0):
    rng = np.random.default_rng(seed)
    kw = dict(modulations=mods, num_spectrum_resources=S, capacity=1024, episode_length=1000, auto_reset=True, load=load,
              bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400),
              replica_load=load * rng.uniform(0.6, 1.5, B), replica_launch_power_dbm=rng.uniform(-4.0, 3.0, B),
              replica_margin=rng.choice([0.0, 0.5, 1.0, 2.0], B))
    tb = golden_tables(topo)
    holder = nat.ConfigHolder(tb, batch=B, **kw)
    if wide:
        monkeypatch.setenv("ONGYM_FORCE_WIDE", "1")         # read at ongym_create
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    env.seed(seed); env.reset()
    assert env.occupancy(pid)["lean_kernel"]
    if warm:
        env.step_policy(warm, record=False)
    got = env.step_policy(steps, policy=pid)
    st = env.stats()
    ctx = f"{topo} policy {pid} wide={wide}"
    for r in range(B):
        o = OracleEnv(holder, replica=r)
        o.seed(seed); o.reset()
        if warm:
            o.run_policy(nat.POLICY_FIRST_FIT, warm)
        want = o.run_policy(pid, steps)
        assert_records_equal(got[:, r], want, f"{ctx} replica {r}")
        np.testing.assert_array_equal(env.grid(r), o.grid())
        os_ = o.stats()
        for f in STATS:
            assert st[r][f] == os_[f], (ctx, r, f, st[r][f], os_[f])
        np.testing.assert_array_equal(st[r]["episode_modulation_hist"], os_["episode_modulation_hist"])
        if pid == nat.POLICY_FIRST_FIT:
            # the oracle evaluates every format the bound lets through; the device settles some by the ASE-only bound
            assert st[r]["total_gn_evals"] <= os_["total_gn_evals"] <= st[r]["total_gn_evals"] + st[r]["total_gn_shortcuts"]
            assert st[r]["total_interferer_terms"] <= os_["total_interferer_terms"]
    return got, st


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("table", ["jocn", "shuffled"])
@pytest.mark.parametrize("pid", [nat.POLICY_FIRST_FIT, nat.POLICY_LOAD_BALANCING])
def test_group_decisions_vs_oracle(pid, table, wide, monkeypatch):
    """Loaded NSFNET-320 with per-replica launch power and margin (many formats fail their GN test, so the walk moves on
    to formats of the same width): records, grids and statistics equal to the oracle's."""
    mods = jocn_modulations() if table == "jocn" else shuffled_modulations()
    run_case("nsfnet", mods, pid, 320, 420, 900, 24, 31 + pid, wide, monkeypatch)


@pytest.mark.parametrize("table", ["jocn", "shuffled"])
@pytest.mark.parametrize("pid", [nat.POLICY_FIRST_FIT, nat.POLICY_LOAD_BALANCING])
def test_group_decisions_two_word_link_masks_vs_oracle(pid, table, monkeypatch):
    """nobel-eu (41 links: the M64 instantiations) after a first-fit warm-up."""
    mods = jocn_modulations() if table == "jocn" else shuffled_modulations()
    run_case("nobel-eu", mods, pid, 320, 500, 400, 12, 5 + pid, False, monkeypatch, warm=300)


@pytest.mark.parametrize("pid", [nat.POLICY_FIRST_FIT, nat.POLICY_LOAD_BALANCING])
def test_group_decisions_narrow_and_wide_agree_with_counters(pid, monkeypatch):
    """The shuffled table through both builds: records, every statistic (evaluation and interferer-term counters included)
    and grids bit for bit."""
    tb = golden_tables("nsfnet")
    B = 128
    kw = dict(tables=tb, modulations=shuffled_modulations(), num_spectrum_resources=320, capacity=448, load=360,
              bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), episode_length=1000, batch_size=B,
              replica_margin=np.random.default_rng(3).choice([0.0, 1.0, 2.0], B))
    outs = []
    for wide in (False, True):
        if wide:
            monkeypatch.setenv("ONGYM_FORCE_WIDE", "1")
        e = BatchedQRMSAEnv(**kw); e.seed(19); e.reset()
        assert e.occupancy(pid)["lean_kernel"]
        rec = e.step_policy(1000, policy=pid)
        outs.append((record_bytes(rec), e.stats().tobytes(), [e.grid(r).tobytes() for r in (0, 63, B - 1)]))
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1]
    assert outs[0][2] == outs[1][2]
