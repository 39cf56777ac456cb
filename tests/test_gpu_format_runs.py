"""First fit in the lean kernel takes the formats that one GN evaluation decides from a per-lane launch table
(csrc/ongym_fast.hpp, t_nr): the run of consecutive format indices around a format that need the same slot count.
(Load balancing keeps deriving the group per evaluation: tests/test_gpu_format_groups.py.)
The format loop strips `run & feasible` from the walk and eval_one decides exactly those lanes.  These tests hold the rule to
the CPU oracle where it can go wrong: eight formats and eight bit rates (lanes 6 and 7 of a bit-rate group, a ballot shift of
56), a width that recurs after a format of another width that the bound removes on some routes only, a pass by a lower
member of a run, and two link-mask words.

The GN model's Phi table has six entries (core/osnr.pyx:38-41), and the library refuses a spectral efficiency above 6, so the
two formats added to the six JOCN ones cannot be more efficient than 64QAM: they are 64QAM at higher thresholds (a weaker
FEC), which puts three formats of every bit rate into one run at the top of the walk."""
import json
import os

import numpy as np
import pytest

from common import GOLDEN, golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym._native import REQUEST_DTYPE
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from optical_networking_gym.topology import Modulation
from oracle_lib import OracleEnv
from test_gpu_format_groups import STATS, assert_records_equal, shuffled_modulations

pytestmark = pytest.mark.gpu

RATES8 = (10, 20, 40, 50, 100, 150, 200, 400)        # BPSK needs at most 32 slots; most rates share a width among formats
COUNTERS = ("total_gn_evals", "total_interferer_terms", "total_gn_shortcuts")


def eight_modulations():
    return jocn_modulations() + (Modulation("64QAM-b", 90, 6, 21.5, -31), Modulation("64QAM-c", 60, 6, 24.0, -33))


def case_kw(mods, rates, S, load, B, seed, margins=(0.0, 0.5, 1.0, 2.0)):
    """Per-replica load, launch power and margin as in test_gpu_format_groups.run_case."""
    rng = np.random.default_rng(seed)
    return dict(modulations=mods, num_spectrum_resources=S, capacity=1024, episode_length=1000, auto_reset=True, load=load,
                bit_rate_selection="discrete", bit_rates=rates,
                replica_load=load * rng.uniform(0.6, 1.5, B), replica_launch_power_dbm=rng.uniform(-4.0, 3.0, B),
                replica_margin=rng.choice(list(margins), B))


def assert_state_equal(env, st, r, o, ctx, pid=nat.POLICY_FIRST_FIT):
    np.testing.assert_array_equal(env.grid(r), o.grid())
    os_ = o.stats()
    for f in STATS:
        assert st[r][f] == os_[f], (ctx, r, f, st[r][f], os_[f])
    np.testing.assert_array_equal(st[r]["episode_modulation_hist"], os_["episode_modulation_hist"])
    if pid == nat.POLICY_FIRST_FIT:
        assert st[r]["total_gn_evals"] <= os_["total_gn_evals"] <= st[r]["total_gn_evals"] + st[r]["total_gn_shortcuts"]
        assert st[r]["total_interferer_terms"] <= os_["total_interferer_terms"]


def blocking_flags(bres, bosnr):
    """What the oracle's own run loop adds to a step record from the heuristic's return tuple (orc_run_policy)."""
    return (nat.F_BLOCKED_RESOURCES if bres else 0) | (nat.F_BLOCKED_OSNR if bosnr else 0)


def run_vs_oracle(topo, kw, B, seed, pid, warm, steps, record=True):
    tb = golden_tables(topo)
    holder = nat.ConfigHolder(tb, batch=B, **kw)
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    env.seed(seed); env.reset()
    assert env.occupancy(pid)["lean_kernel"]
    env.step_policy(warm, record=False)
    got = env.step_policy(steps, policy=pid, record=record)
    st = env.stats()
    oracles = []
    for r in range(B):
        o = OracleEnv(holder, replica=r)
        o.seed(seed); o.reset()
        o.run_policy(nat.POLICY_FIRST_FIT, warm)
        want = o.run_policy(pid, steps)
        ctx = f"{topo} policy {pid} replica {r}"
        if record:
            assert_records_equal(got[:, r], want, ctx)
        assert_state_equal(env, st, r, o, ctx, pid)
        oracles.append((o, want))
    return env, st, oracles


@pytest.mark.parametrize("shape", ["narrow", "wide", "narrow_no_records"])
def test_eight_formats_eight_bit_rates_vs_oracle(shape, monkeypatch):
    """Every lane of the per-lane tables is in use: the top three formats of every bit rate form one run, and the runs of the
    eighth bit rate sit in lanes 56..63.  With records (REC), without them, and through the wide build."""
    if shape == "wide":
        monkeypatch.setenv("ONGYM_FORCE_WIDE", "1")         # read at ongym_create
    B = 16
    kw = case_kw(eight_modulations(), RATES8, 320, 420, B, 71)
    run_vs_oracle("nsfnet", kw, B, 71, nat.POLICY_FIRST_FIT, 300, 600, record=shape != "narrow_no_records")


def test_eight_formats_eight_bit_rates_replayed_trace_vs_oracle():
    """The same table through the trace-replaying instantiation (TRACE): per-replica traces written on the host."""
    tb = golden_tables("nsfnet")
    B, n, seed = 16, 900, 73
    kw = case_kw(eight_modulations(), RATES8, 320, 420, B, seed)
    rng = np.random.default_rng(seed + 1)
    reqs = np.zeros((B, n), REQUEST_DTYPE)
    for r in range(B):
        reqs[r]["arrival_time"] = np.cumsum(rng.exponential(10800.0 / kw["replica_load"][r], n)).astype(np.float32)
        reqs[r]["holding_time"] = rng.exponential(10800.0, n).astype(np.float32)
        src = rng.integers(0, tb.n_nodes, n)
        reqs[r]["source"], reqs[r]["destination"] = src, (src + rng.integers(1, tb.n_nodes, n)) % tb.n_nodes
        reqs[r]["bit_rate"] = rng.choice(np.array(RATES8), n)
    holder = nat.ConfigHolder(tb, batch=B, **kw)
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    env.set_requests(reqs); env.reset()
    assert env.occupancy()["lean_kernel"]
    steps = n - 10                                           # stays inside the trace: every step has a request
    got = env.step_policy(steps)
    st = env.stats()
    assert not (got["flags"] & nat.F_NO_REQUEST).any()
    for r in range(B):
        o = OracleEnv(holder, replica=r)
        o.set_trace(reqs[r]); o.reset()
        want = o.run_first_fit(steps)
        assert_records_equal(got[:, r], want, f"trace replica {r}")
        assert_state_equal(env, st, r, o, f"trace replica {r}")


def recurring_width_case():
    B, seed = 24, 83
    # margins from well below to well above what the width-3 format (8QAM at index 3) can carry on the longer routes
    kw = case_kw(shuffled_modulations(), (10, 40, 100, 400), 320, 420, B, seed, margins=(0.0, 1.0, 2.0, 3.0, 4.0))
    return kw, B, seed, 300, 600


def test_width_recurs_after_format_the_bound_removes_vs_oracle_and_parent_counters():
    """Shuffled table: walked from the highest index the 100G widths are 2, 2, 3, 2, 4, 8.  When the bound removes the width-3
    format of a route, the parent's rule put index 2 into the group of indices 5 and 4 while the run table evaluates it as a
    run of its own: same start, same sum, same decisions, and the same counters, which count formats walked.  The counters
    are held to what the parent commit's library gave for this case (tests/golden/format_runs_counters.json, written by
    tools/dump_format_counters.py with that library)."""
    kw, B, seed, warm, steps = recurring_width_case()
    tb = golden_tables("nsfnet")
    holder = nat.ConfigHolder(tb, batch=B, **kw)
    mods = kw["modulations"]
    # host side, oracle only: the bound of the width-3 format on every route the 100G requests of the run walk
    removed = kept = 0
    wants = []
    for r in range(B):
        o = OracleEnv(holder, replica=r)
        o.seed(seed); o.reset()
        o.run_policy(nat.POLICY_FIRST_FIT, warm)
        empty = OracleEnv(holder, replica=r)                # no running service: GN at slot 0 is the bound (ASE + self-channel NLI)
        empty.seed(seed); empty.reset()
        n3 = o.number_slots(100.0, 3)
        assert [o.number_slots(100.0, m) for m in (5, 4, 3, 2, 1, 0)] == [2, 2, 3, 2, 4, 8]
        thr = mods[3].minimum_osnr + float(kw["replica_margin"][r])
        recs = np.zeros(steps, nat.STEP_DTYPE)
        for i in range(steps):
            q = o.request()
            act, bres, bosnr = o.policy_first_fit()
            rc, rec = o.step(act)
            assert rc == 0
            recs[i] = rec
            recs[i]["flags"] |= blocking_flags(bres, bosnr)
            if q["bit_rate"] != 100.0:
                continue
            last = int(rec["route"]) if rec["accepted"] else tb.k_paths - 1
            for k in range(last + 1):
                p = int(tb.pair_paths[int(q["source"]), int(q["destination"]), k])
                if p < 0:
                    break
                if empty.gn(p, 0, n3)[0] >= thr:
                    kept += 1
                else:
                    removed += 1
        wants.append((o, recs))
    assert removed > 50 and kept > 50, f"the case must hold both situations: bound removes width 3 on {removed} routes, keeps it on {kept}"

    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    env.seed(seed); env.reset()
    assert env.occupancy()["lean_kernel"]
    env.step_policy(warm, record=False)
    got = env.step_policy(steps)
    st = env.stats()
    for r in range(B):
        o, want = wants[r]
        assert_records_equal(got[:, r], want, f"recurring width replica {r}")
        assert_state_equal(env, st, r, o, f"recurring width replica {r}")
    with open(os.path.join(GOLDEN, "format_runs_counters.json")) as f:
        parent = json.load(f)
    for c in COUNTERS:
        assert st[c].tolist() == parent["recurring_width"][c], c


def test_pass_is_a_lower_member_of_its_run_vs_oracle():
    """All six formats of a 10G request need one slot: one run, one evaluation.  With margins of several dB the top formats
    fail their GN test at loads where lower ones pass, so the format that passes is a lower member of the run: asserted with
    the oracle (bound and evaluation in dB), then records and the modulation histogram against it."""
    B, seed, warm, steps = 16, 91, 300, 600
    kw = case_kw(jocn_modulations(), (10, 40, 100, 400), 320, 420, B, seed, margins=(1.0, 2.0, 3.0, 4.0))
    tb = golden_tables("nsfnet")
    holder = nat.ConfigHolder(tb, batch=B, **kw)
    mods = kw["modulations"]
    lower = 0
    wants = []
    for r in range(B):
        o = OracleEnv(holder, replica=r)
        o.seed(seed); o.reset()
        o.run_policy(nat.POLICY_FIRST_FIT, warm)
        empty = OracleEnv(holder, replica=r)
        empty.seed(seed); empty.reset()
        assert [o.number_slots(10.0, m) for m in range(6)] == [1] * 6
        margin = float(kw["replica_margin"][r])
        recs = np.zeros(steps, nat.STEP_DTYPE)
        for i in range(steps):
            q = o.request()
            act, bres, bosnr = o.policy_first_fit()
            if q["bit_rate"] == 10.0 and act != o.reject_action:
                k, m, slot = o.decode(act)
                p = int(tb.pair_paths[int(q["source"]), int(q["destination"]), k])
                bound = empty.gn(p, 0, 1)[0]
                # a format above the chosen one that the bound lets through was in the evaluated group and failed there
                lower += any(bound >= mods[mm].minimum_osnr + margin for mm in range(m + 1, 6))
            rc, rec = o.step(act)
            assert rc == 0
            recs[i] = rec
            recs[i]["flags"] |= blocking_flags(bres, bosnr)
        wants.append((o, recs))
    assert lower > 20, f"only {lower} accepted 10G requests took a format below the top of their evaluated run"

    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    env.seed(seed); env.reset()
    assert env.occupancy()["lean_kernel"]
    env.step_policy(warm, record=False)
    got = env.step_policy(steps)
    st = env.stats()
    for r in range(B):
        o, want = wants[r]
        assert_records_equal(got[:, r], want, f"lower member replica {r}")
        assert_state_equal(env, st, r, o, f"lower member replica {r}")


def test_eight_formats_two_word_link_masks_vs_oracle():
    """nobel-eu (41 links: the M64 instantiations, two mask words), first fit after a first-fit warm-up."""
    B = 8
    kw = case_kw(eight_modulations(), RATES8, 320, 500, B, 97)
    run_vs_oracle("nobel-eu", kw, B, 97, nat.POLICY_FIRST_FIT, 300, 300)
