"""Every QoT admission decision on its threshold, in and around the 1e-9 band ("Decision exactness").

tests/threshold_ladder.py builds, per case, 21 replicas whose margins put the threshold on the GSNR g of one candidate of one
request t* (on the equality, 1, 2, 8 ulp off it, 1e-13 .. 2e-9 dB inside the band, 1e-8 and 4.3e-8 dB outside), all on one request
stream; tests/test_threshold_ladder_host.py holds on the oracle that the ladder moves that decision and nothing else.  Here the
kernels run the ladder.

1. Step kernels.  step_policy in launches of uneven length with t* inside a launch, to t* + 40, with records, on the lean narrow
   kernel with the link-weight table and with ONGYM_FAST_NO_LWTAB=1, the lean wide kernel (ONGYM_FORCE_WIDE=1), the lean M64
   kernel (nobel-eu), the lean TRACE kernel, the forced generic kernel (ONGYM_FORCE_GENERIC=1), the generic kernel with per-link
   attenuation, and policies 1 and 2 lean and forced generic.  Each run asserts
     exact set      on every rung with |T_r - g| >= 1e-11 dB the records of the whole run (EXACT fields bit-exact, GSNR/ASE/NLI at
                    1e-9), the final grids, services and stats() equal the rung's own oracle;
     every rung     along T_r the decision at t* changes exactly once, from accepted at format m to fallen through, and that
                    change lies strictly inside |T_r - g| < 1e-11;
     own value      the osnr the kernel wrote at t* is the same bits on all accepting rungs (g_own), and on every rung the kernel
                    accepted m iff g_own >= T_r, except where |g_own - T_r| <= 4 ulp(g_own) (one ulp for the rounding of 1/acc, the
                    rest for -10 log10(acc) as reported against 10 log10(1/acc) as decided);
     evaluations    total_gn_evals <= oracle's <= total_gn_evals + total_gn_shortcuts, as tests/test_gpu_launch_boundaries.py holds
                    it: the upper bound not for the lean kernels of policies 1 and 2, where one device evaluation stands for
                    several of the oracle's by design (UPPER_EXEMPT there).
   A rung inside the zone whose decision at t* agrees with its oracle's is held to the oracle like the exact set (every other
   decision of its run is at least 1e-6 dB from its threshold); one that disagrees runs a different history from t* on and is
   compared with nothing but its own value.
2. The ASE-bound shortcut.  An empty network with uniform attenuation: acc equals the bound up to rounding.  The ladder sits on
   (route 0, top format, slot 0) of a 400 Gb/s demand at the reset state; on both step kernels the assertions of 1 hold, and
   total_gn_shortcuts at the +4.3e-8 rung exceeds its value at the rung nearest delta = 0 (the shortcut's edge was straddled).
3. Read-only and external-action entry points on the pending state (t* steps done, the critical request undecided), every rung
   against its oracle in the same state: policy_actions(0) (and the state byte-identical after it), step(actions) with the explicit
   action (accepted on the low rungs, ONGYM_F_QOT_ERROR and not applied on the high ones), observe() (the whole mask, which the
   margin does not enter while every format is in the window), observe_blocks(4) (a block the ladder refuses is not offered),
   admission_map() (the pending request's cell), playout(horizon=1) (the pending request accepted), and every fused policy 0..11
   lean-eligible and forced generic.

4. Ladders on a state reached under the base margin (replica 0 runs the history, replicas 1..21 take its state by
   fork(keep_params=True); the oracle takes the rung's margin with orc_set_margin): the max_modulation_idx scan of observe() with
   modulations_to_consider = 3 (the generic kernel; the ladder sits on the candidate that decides it), lowest fragmentation on the
   candidate it chooses itself (no first-fit ladder moves its answer), service_qot (the count below minimum_osnr + margin on the
   lowest GSNR - minimum_osnr of the running lightpaths) and action_impact (newly_below_margin on a victim's GSNR after the
   candidate: the pairs tests/test_gpu_action_impact.py leaves out).

The exempt zone.  Rungs closer than 1e-11 dB to g are exempt from oracle parity because the device sums in another order.  Each
case measures e = |env.gsnr(candidate) - oracle.gn(candidate)| in the pending state, prints it and asserts 4 e < 1e-11.
Measured on MI355X (dB): ff_nsfnet_m0 1.8e-15, ff_nsfnet_m1 1.8e-15, ff_nobeleu 0, ff_trace 1.8e-15, ff_alpha 0, lb_nsfnet 1.8e-15,
hsnr_nsfnet 3.6e-15, hsnr_cost239 0, ff_nsfnet_s2 3.6e-15, ff_nsfnet_s13 0, ff_empty 0, max_modulation_idx 0, service_qot 1.8e-15,
action_impact 1.8e-15: one ulp of g at most.  The largest |g_own - T_r| with a decision other than g_own >= T_r was 1 ulp (the
generic kernel and step(actions) accept at T_r = g_own + 1 ulp); the lean kernels showed none.
"""
import numpy as np
import pytest

import threshold_ladder as tl
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv

pytestmark = pytest.mark.gpu

B = tl.B
GSNR_RTOL = 1e-9
OWN_ULP = 4
EXACT = ("action", "route", "modulation", "slot", "nslots", "accepted", "terminated", "retry", "flags", "active", "reward")
STATS = ("services_processed", "services_accepted", "episode_services_processed", "episode_services_accepted",
         "bit_rate_requested", "bit_rate_provisioned", "episode_bit_rate_provisioned", "rejected", "episodes_completed",
         "total_steps", "total_accepted", "total_paths_tried", "total_path_hops", "total_active_sum", "current_time", "active")
UPPER_EXEMPT = {(tl.LB, True), (tl.HSNR, True)}              # (policy, lean kernel), as in tests/test_gpu_launch_boundaries.py
ENV_VARS = ("ONGYM_FORCE_GENERIC", "ONGYM_FORCE_WIDE", "ONGYM_FAST_NO_LWTAB")

# kernel name -> (environment variables read at ongym_create, lean kernel expected, link-weight table expected (None: either))
KERNELS = {
    "lean": ({}, True, None),
    "lean_table": ({}, True, True),
    "lean_loop": ({"ONGYM_FAST_NO_LWTAB": "1"}, True, False),
    "lean_wide": ({"ONGYM_FORCE_WIDE": "1"}, True, None),
    "generic": ({"ONGYM_FORCE_GENERIC": "1"}, False, None),
    "generic_alpha": ({}, False, None),              # per-link attenuation rules the lean kernels out
}
STEP_RUNS = [("ff_nsfnet_m0", "lean_table"), ("ff_nsfnet_m0", "lean_loop"), ("ff_nsfnet_m0", "lean_wide"), ("ff_nsfnet_m0", "generic"),
             ("ff_nsfnet_m1", "lean_table"), ("ff_nsfnet_m1", "generic"),
             ("ff_nobeleu", "lean"), ("ff_nobeleu", "generic"),
             ("ff_trace", "lean"), ("ff_trace", "generic"),
             ("ff_alpha", "generic_alpha"), ("ff_nsfnet_s2", "lean"), ("ff_nsfnet_s13", "generic"),
             ("lb_nsfnet", "lean"), ("lb_nsfnet", "generic"),
             ("hsnr_nsfnet", "lean"), ("hsnr_nsfnet", "generic"), ("hsnr_cost239", "lean"), ("hsnr_cost239", "generic")]
EMPTY_RUNS = [(tl.EMPTY, "lean"), (tl.EMPTY, "generic")]


def make_env(case, kernel, monkeypatch):
    """The device ladder, reset, every rung on replica 0's request stream (fork) or on the one host trace."""
    env_vars, lean, table = KERNELS[kernel]
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, x in env_vars.items():
        monkeypatch.setenv(v, x)                    # read at ongym_create
    env = BatchedQRMSAEnv(tables=case.tables, batch_size=B, **case.kw)
    if case.trace is not None:
        env.set_requests(np.ascontiguousarray(np.broadcast_to(case.trace, (B, len(case.trace)))))
        env.reset()
    else:
        env.seed(case.seed)
        env.reset()
        env.fork(np.zeros(B, np.int32), keep_params=True)
    assert env.occupancy(case.policy)["lean_kernel"] == lean, (case.name, kernel)
    if table is not None:
        assert (env.link_weight_entry(0, 0) is not None) == table, (case.name, kernel)
    if case.tables.n_links > 32:
        assert case.name == "ff_nobeleu"            # the M64 record codec
    return env


def launch_lengths(case):
    """Uneven launches to t* + 41 steps with t* inside one: neither its first nor its last step, where the run allows it."""
    t, n = case.t, case.steps
    cuts = sorted({c for c in (1, 8, t - 5, t + 3, n) if 0 < c <= n and c not in (t, t + 1)})
    assert cuts[-1] == n and t not in cuts and (t + 1) not in cuts
    return np.diff([0] + cuts).tolist()


def assert_records_equal(got, want, ctx):
    for f in EXACT:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(got[f] != want[f])[0]
            raise AssertionError(f"{ctx}: field {f} differs first at {tuple(bad)}: {got[f][tuple(bad)]} != {want[f][tuple(bad)]}")
    for f in ("osnr", "ase", "nli"):
        np.testing.assert_allclose(got[f], want[f], rtol=GSNR_RTOL, err_msg=f"{ctx}: {f}")


def ulps(x, ref):
    return abs(float(x) - float(ref)) / float(np.spacing(abs(float(ref))))


def check_decisions(case, acc, g_own_rungs, ctx):
    """The "every rung" and "own value" assertions on `acc` (the ladder's candidate taken, per rung along T_r) and the value the
    kernel reported on the accepting rungs.  Returns the first rung that fell through."""
    T, g = case.T, case.g
    k = tl.one_change(acc)
    assert k > 0, f"{ctx}: decisions along T_r do not change exactly once: {acc.astype(int)}"
    ex = tl.exact_rungs(case)
    assert np.array_equal(acc[ex], (g >= T)[ex]), f"{ctx}: the change lies outside the zone: {acc.astype(int)} at T - g {T - g}"
    assert abs(T[k - 1] - g) < tl.ZONE_DB and abs(T[k] - g) < tl.ZONE_DB, (ctx, k, T[k - 1] - g, T[k] - g)
    own = np.asarray(g_own_rungs, np.float64)
    assert len(own) == k and len(set(own.tobytes()[i * 8:i * 8 + 8] for i in range(k))) == 1, \
        f"{ctx}: the accepting rungs report different GSNR: {[repr(float(x)) for x in own]}"
    g_own = float(own[0])
    worst = 0.0
    for r in range(B):
        if bool(acc[r]) != (g_own >= T[r]):
            worst = max(worst, ulps(T[r], g_own))
    print(f"{ctx}: g_own {g_own!r} oracle g {g!r} ({ulps(g_own, g):.1f} ulp apart) decision changes between T - g_own = "
          f"{T[k - 1] - g_own:.3e} and {T[k] - g_own:.3e} dB; largest |g_own - T_r| with a decision other than g_own >= T_r: {worst:.1f} ulp")
    assert worst <= OWN_ULP, f"{ctx}: decision differs from g_own >= T_r at {worst:.1f} ulp"
    return k


def run_step_kernels(name, kernel, monkeypatch):
    case = tl.find_case(name)
    env = make_env(case, kernel, monkeypatch)
    got = np.concatenate([env.step_policy(n, record=True, policy=case.policy) for n in launch_lengths(case)])
    ctx = f"{name} {kernel}"
    t = case.t
    acc = tl.accepted_m(case, got[t])
    check_decisions(case, acc, got["osnr"][t][acc], ctx)
    # before t* every rung, inside the zone or not, has the base history
    for r in range(B):
        assert_records_equal(got[:t, r], case.recs[:t, r], f"{ctx} rung {r} before t*")
    st = env.stats()
    held = tl.exact_rungs(case) | (acc == case.accepts)
    assert held.sum() >= B - 13
    for r in np.flatnonzero(held):
        o = case.oracles[r]
        assert_records_equal(got[:, r], case.recs[:, r], f"{ctx} rung {r}")
        np.testing.assert_array_equal(env.grid(r), o.grid(), err_msg=f"{ctx} rung {r}: grid")
        a = np.sort(env.services(r), order=["release_time", "path_id", "slot"])
        b = np.sort(o.services(), order=["release_time", "path_id", "slot"])
        assert a.tobytes() == b.tobytes(), f"{ctx} rung {r}: services"
        so = o.stats()
        for f in STATS:
            assert st[r][f] == so[f], (ctx, r, f, st[r][f], so[f])
        np.testing.assert_array_equal(st[r]["episode_modulation_hist"], so["episode_modulation_hist"])
        work = (ctx, r, int(st[r]["total_gn_evals"]), int(so["total_gn_evals"]), int(st[r]["total_gn_shortcuts"]))
        assert st[r]["total_gn_evals"] <= so["total_gn_evals"], work
        if (case.policy, KERNELS[kernel][1]) not in UPPER_EXEMPT:
            assert so["total_gn_evals"] <= st[r]["total_gn_evals"] + st[r]["total_gn_shortcuts"], work
    return case, env, st


@pytest.mark.parametrize("name,kernel", STEP_RUNS)
def test_step_kernels_on_the_ladder(name, kernel, monkeypatch):
    run_step_kernels(name, kernel, monkeypatch)


@pytest.mark.parametrize("name,kernel", EMPTY_RUNS)
def test_ase_bound_shortcut_on_the_ladder(name, kernel, monkeypatch):
    case, env, st = run_step_kernels(name, kernel, monkeypatch)
    near = int(np.argmin(np.abs(case.T - case.g)))
    print(f"{name} {kernel}: total_gn_shortcuts along T_r {st['total_gn_shortcuts'].tolist()}")
    assert st[B - 1]["total_gn_shortcuts"] > st[near]["total_gn_shortcuts"], (kernel, st["total_gn_shortcuts"].tolist())


# ---- the pending state: t* steps done, the critical request undecided --------------------------------------------------------
def pending_env(case, kernel, monkeypatch):
    env = make_env(case, kernel, monkeypatch)
    if case.t:
        env.step_policy(case.t, record=False, policy=case.policy)
    return env


@pytest.mark.parametrize("name", list(tl.CASES))
def test_summation_order_noise_is_below_the_exempt_zone(name, monkeypatch):
    """e = |device GSNR - oracle GSNR| of the ladder's candidate in the pending state: the zone is 1e-11 dB, four times e must fit."""
    case = tl.find_case(name)
    env = pending_env(case, "generic_alpha" if case.cfg.get("alpha") else "lean", monkeypatch)
    o = tl.pending_oracle(case, 0)
    path, slot, n = case.cand
    want = o.gn(path, slot, n)
    assert want[0] == case.g                     # the oracle's query is the value its step recorded
    got = np.stack([env.gsnr(r, path, slot, n) for r in range(B)])
    assert len(set(got[:, 0].tolist())) == 1     # one state, one arithmetic on every rung
    e = abs(float(got[0, 0]) - float(want[0]))
    print(f"{name}: e = {e:.3e} dB ({tl.ulps_of(got[0, 0], want[0]):.1f} ulp of g)")
    assert 4 * e < tl.ZONE_DB, (name, e)


def ladder_values(case, got, want, ctx):
    """One quantity per rung along T_r, device and oracle: equal outside the zone; where the oracle's answer differs between the
    ladder's ends the device's changes exactly once, inside the zone, from the low rungs' value to the high rungs'; where it
    does not, the device's is one value.  Returns whether it changed."""
    ex = tl.exact_rungs(case)
    for r in np.flatnonzero(ex):
        assert got[r] == want[r], f"{ctx}: rung {r} (T - g = {case.T[r] - case.g:.3e}): {got[r]} != oracle's {want[r]}"
    if want[0] == want[-1]:
        assert all(x == got[0] for x in got), f"{ctx}: {got}"
        return False
    k = tl.one_change([x == got[0] for x in got])
    assert k > 0 and all(x == got[-1] for x in got[k:]), f"{ctx}: not one change along T_r: {got}"
    assert not ex[k - 1] and not ex[k], (ctx, k)
    return True


PENDING_RUNS = [("ff_nsfnet_m0", "lean"), ("ff_nsfnet_m0", "generic"), ("ff_nobeleu", "lean"), ("ff_nsfnet_m1", "generic")]


@pytest.mark.parametrize("name,kernel", PENDING_RUNS)
def test_entry_points_on_the_pending_state(name, kernel, monkeypatch):
    case = tl.find_case(name)
    env = pending_env(case, kernel, monkeypatch)
    oracles = tl.threaded(lambda r: tl.pending_oracle(case, r), B)
    ctx = f"{name} {kernel}"
    holder, c = case.holder, case.holder.struct
    q = oracles[0].request()
    for r in range(B):
        assert env.request(r).tobytes() == q.tobytes(), (ctx, r)
    want_ff = [o.policy_first_fit() for o in oracles]
    takes = [w[0] == case.action for w in want_ff]
    assert takes == (case.g >= case.T).tolist()

    # policy_actions(0): actions and flags, and a state that is byte-identical afterwards
    before = env.save_state().tobytes()
    acts, flags = env.policy_actions(nat.POLICY_FIRST_FIT)
    assert env.save_state().tobytes() == before, f"{ctx}: policy_actions changed the state"
    got = [(int(a), bool(f & nat.F_BLOCKED_RESOURCES), bool(f & nat.F_BLOCKED_OSNR)) for a, f in zip(acts, flags)]
    assert ladder_values(case, got, want_ff, f"{ctx} policy_actions(0)")
    assert got[0][0] == case.action

    # observe(): the whole mask.  With every format in the window (modulations_to_consider = 6) the margin does not enter it: the
    # mask's QoT is calculate_osnr_observation against minimum_osnr alone (envs/qrmsa.pyx:743-763), and max_modulation_idx, the
    # one thing the margin moves, is pinned at 5.  So the mask is the oracle's on every rung, the zone included, and the bit of the
    # critical action is set on all of them; test_max_modulation_idx_scan_on_the_ladder runs the scan that does depend on it.
    pl = np.ctypeslib.as_array(c.path_len_norm, shape=(c.n_paths,))
    _, mask = env.observe()
    for r in range(B):
        np.testing.assert_array_equal(mask[r], oracles[r].observe(pl, c.max_bit_rate)[1], err_msg=f"{ctx} rung {r}: observe() mask")
        assert oracles[r].max_modulation_idx == len(case.thr) - 1
    assert mask[:, case.action].all() and (env.stats()["max_modulation_idx"] == len(case.thr) - 1).all()

    # observe_blocks(4): a block the ladder refuses is not offered
    J = 4
    _, bmask, amap = env.observe_blocks(J)
    offered = [bool(np.any((bmask[r] == 1) & (amap[r] == case.action))) for r in range(B)]
    assert offered[0], f"{ctx}: no block of the lowest rung decodes to the ladder's candidate: {amap[0]}"
    assert ladder_values(case, offered, takes, f"{ctx} observe_blocks")
    e0 = int(np.flatnonzero((bmask[0] == 1) & (amap[0] == case.action))[0])
    assert e0 // J == case.route
    for r in range(B):                       # the entry stays valid or not; where valid on a refusing rung it is another format
        assert amap[r, e0] != case.action or offered[r]
        assert bmask[r, e0] == (amap[r, e0] != env.reject_action), (ctx, r)

    # admission_map() of the state as it is: the cell of the pending request's pair and bit rate
    s, d = sorted((int(q["source"]), int(q["destination"])))
    cell = int(np.flatnonzero((env.admission_pairs == (s, d)).all(1))[0])
    rate = tl._KW["bit_rates"].index(int(q["bit_rate"]))
    _, amap2, margin = env.admission_map(detail=True)
    reject = env.reject_action
    want_cell = [a if a != reject else reject + int(bosnr) for a, bres, bosnr in want_ff]
    assert ladder_values(case, [int(x) for x in amap2[:, 0, cell, rate]], want_cell, f"{ctx} admission_map cell")

    # playout(actions=[first fit's action on the low rungs], horizon=1): applied and accepted (status 0) on the low rungs, "the step
    # would flag a QoT error" (status 3, nothing played) on the high ones
    po = env.playout(actions=np.full(B, case.action, np.int32), horizon=1, policy=nat.POLICY_FIRST_FIT)[:, 0, 0]
    col = nat.PLAYOUT.index("first_accepted")
    got = [(int(x[0]), None if np.isnan(x[col]) else int(x[col])) for x in po]
    assert ladder_values(case, got, [(0, 1) if t else (3, None) for t in takes], f"{ctx} playout")
    assert env.save_state().tobytes() == before, f"{ctx}: a read-only call changed the state"

    # step(actions) with the explicit action: accepted on the low rungs, ONGYM_F_QOT_ERROR and not applied on the high ones
    grids = [env.grid(r) for r in range(B)]
    rec = env.step(np.full(B, case.action, np.int32))
    want_step = [o.step(case.action) for o in oracles]
    got = [(bool(x["accepted"]), bool(x["flags"] & nat.F_QOT_ERROR)) for x in rec]
    assert ladder_values(case, got, [(bool(w["accepted"]), rc != 0) for rc, w in want_step], f"{ctx} step(actions)")
    assert got[0] == (True, False) and got[-1] == (False, True)
    for r in range(B):
        if got[r][1]:
            np.testing.assert_array_equal(env.grid(r), grids[r], err_msg=f"{ctx} rung {r}: a refused action was applied")
        if tl.exact_rungs(case)[r]:
            rc, w = want_step[r]
            np.testing.assert_array_equal(env.grid(r), oracles[r].grid(), err_msg=f"{ctx} rung {r}: grid after step")
            if rc == 0:
                for f in ("action", "accepted", "retry", "route", "slot", "modulation", "nslots", "reward", "terminated", "active"):
                    assert rec[r][f] == w[f], (ctx, r, f)
                np.testing.assert_allclose(rec[r]["osnr"], w["osnr"], rtol=GSNR_RTOL)
    own = rec["osnr"][[g[0] for g in got]]
    check_decisions(case, np.array([g[0] for g in got]), own, f"{ctx} step(actions)")


POLICY_RUNS = [(n, k) for n in tl.POLICY_CASES for k in ("lean", "generic")]


@pytest.mark.parametrize("name,kernel", POLICY_RUNS)
def test_every_fused_policy_on_the_pending_state(name, kernel, monkeypatch):
    """policy_actions(pid), pid 0..11, against oracle.policy(pid) on the ladder; the policies whose answer changes along it are
    the ones tests/test_threshold_ladder_host.py lists for the case."""
    case = tl.find_case(name)
    env = pending_env(case, kernel, monkeypatch)
    oracles = tl.threaded(lambda r: tl.pending_oracle(case, r), B)
    changed = []
    for pid in range(12):
        want = tl.threaded(lambda r: oracles[r].policy(pid), B)
        acts, flags = env.policy_actions(pid)
        got = [(int(a), bool(f & nat.F_BLOCKED_RESOURCES), bool(f & nat.F_BLOCKED_OSNR)) for a, f in zip(acts, flags)]
        if ladder_values(case, got, want, f"{name} {kernel} policy {pid}"):
            changed.append(pid)
    print(f"{name} {kernel}: policies whose answer changes along the ladder: {changed}")
    assert tuple(changed) == tl.changing_policies(name)


# ---- ladders on a state reached under the base margin (tests/threshold_ladder.py, second half) --------------------------------
def state_env(case, monkeypatch, observe_each=False, kernel="lean"):
    """B + 1 replicas: replica 0 runs the history at the base margin, the ladder's replicas 1..B then take its state."""
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, x in KERNELS[kernel][0].items():
        monkeypatch.setenv(v, x)                    # read at ongym_create
    env = BatchedQRMSAEnv(tables=case.tables, batch_size=B + 1, **case.kw)
    env.seed(case.seed)
    env.reset()
    if observe_each:
        for _ in range(case.t):
            env.observe()
            env.step_policy(1, record=False)
    else:
        env.step_policy(case.t, record=False)
    env.fork(np.zeros(B + 1, np.int32), keep_params=True)
    for r in (1, B):
        np.testing.assert_array_equal(env.grid(r), case.oracles[r - 1].grid())
        assert env.request(r).tobytes() == case.oracles[r - 1].request().tobytes()
    return env


def own_value(case, below, g_own, ctx):
    """`below` per rung against the kernel's own value: below iff not g_own >= T_r, except within 4 ulp of g_own."""
    assert len(set(np.asarray(g_own, np.float64).tobytes()[i * 8:i * 8 + 8] for i in range(B))) == 1, (ctx, g_own)
    g = float(g_own[0])
    e = abs(g - case.g)
    worst = max([ulps(case.T[r], g) for r in range(B) if bool(below[r]) == (g >= case.T[r])], default=0.0)
    print(f"{ctx}: g_own {g!r} restated g {case.g!r} e = {e:.3e} dB; largest |g_own - T_r| with a decision other than g_own >= T_r: "
          f"{worst:.1f} ulp")
    assert 4 * e < tl.ZONE_DB, (ctx, e)
    assert worst <= OWN_ULP, (ctx, worst)


def test_max_modulation_idx_scan_on_the_ladder(monkeypatch):
    """modulations_to_consider = 3: the generic kernel, and the scan of the observation that sets max_modulation_idx
    (get_max_modulation_index, envs/qrmsa.pyx:543-581).  The ladder sits on the candidate that decides it."""
    case = tl.mmi_case()
    env = state_env(case, monkeypatch, observe_each=True)
    assert not env.occupancy(nat.POLICY_FIRST_FIT)["lean_kernel"]
    e = abs(float(env.gsnr(1, *case.cand)[0]) - case.g)
    print(f"max_modulation_idx: e = {e:.3e} dB")
    assert 4 * e < tl.ZONE_DB
    want = [tl.oracle_mmi(case, o) for o in case.oracles]
    _, mask = env.observe()
    mmi = env.stats()["max_modulation_idx"]
    acts, flags = env.policy_actions(nat.POLICY_FIRST_FIT)
    assert ladder_values(case, [int(x) for x in mmi[1:]], [w[0] for w in want], "max_modulation_idx")
    assert mmi[1] == case.m and mmi[B] < case.m
    ladder_values(case, [m.tobytes() for m in mask[1:]], [w[1].tobytes() for w in want], "observe() mask, 3 formats")
    got = [(int(a), bool(f & nat.F_BLOCKED_RESOURCES), bool(f & nat.F_BLOCKED_OSNR)) for a, f in zip(acts[1:], flags[1:])]
    ladder_values(case, got, [w[2] for w in want], "policy_actions(0), 3 formats")
    # the step decodes the action under the window the observation left
    rec = env.step(acts)
    ex = tl.exact_rungs(case)
    for r in np.flatnonzero(ex):
        rc, w = case.oracles[r].step(int(acts[r + 1]))
        assert rc == 0 and not (rec[r + 1]["flags"] & nat.F_QOT_ERROR), r
        for f in ("action", "accepted", "retry", "route", "slot", "modulation", "nslots", "reward", "terminated", "active"):
            assert rec[r + 1][f] == w[f], (r, f, rec[r + 1][f], w[f])
        np.testing.assert_allclose(rec[r + 1]["osnr"], w["osnr"], rtol=GSNR_RTOL)


def test_service_qot_on_the_ladder(monkeypatch):
    """below_lane (csrc/ongym_qot.hpp): the count of running lightpaths below minimum_osnr + margin steps from 0 more to 1 more once
    along the ladder on the lowest GSNR - minimum_osnr, and is the restated dB-domain count outside the zone."""
    from test_gpu_service_qot import match
    case = tl.service_case()
    env = state_env(case, monkeypatch)
    svc, rep, _ = env.service_qot()
    dsvc = env.services(1)
    j = match(dsvc, case.svcs)
    idx = int(np.flatnonzero(j == case.y)[0])
    thr_s = case.thr[case.svcs["modulation"]]
    want = [int(np.sum(case.want[:, 0] < thr_s + m)) for m in case.margins]
    got = [int(x) for x in rep[1:, 2]]
    assert ladder_values(case, got, want, "service_qot below_margin")
    assert got[-1] == got[0] + 1
    for col in (0, 1, 3, 4, 5):
        assert len(set(rep[1:, col].tolist())) == 1, (nat.REPLICA_QOT[col], rep[1:, col])
    assert rep[1, 0] == len(case.svcs) and rep[1, 1] == int(np.sum(case.want[:, 0] < thr_s))
    np.testing.assert_allclose(svc[1, :len(dsvc), :3], case.want[j], rtol=GSNR_RTOL)
    own_value(case, [x != got[0] for x in got], svc[1:, idx, 0], "service_qot")


def test_action_impact_on_the_ladder(monkeypatch):
    """The pairs tests/test_gpu_action_impact.py leaves out: a victim whose GSNR after the candidate sits on minimum_osnr + margin.
    newly_below_margin steps once along the ladder; every other column is one value and the restated one."""
    from test_gpu_action_impact import DB_ATOL, rows_from_pairs
    from test_gpu_service_qot import match
    case = tl.impact_case()
    env = state_env(case, monkeypatch)
    dsvc = env.services(1)
    j = match(dsvc, case.svcs)                                  # device record -> oracle index
    record = np.empty(len(j), np.int64)
    record[j] = np.arange(len(j))                               # oracle index -> device record
    out = env.action_impact(np.full(B + 1, case.action, np.int32))[1:, 0]
    want = np.stack([rows_from_pairs(1, case.status, case.pairs, record, m)[0] for m in case.margins])
    col = nat.ACTION_IMPACT.index("newly_below_margin")
    assert ladder_values(case, [int(x) for x in out[:, col]], [int(x) for x in want[:, col]], "action_impact newly_below_margin")
    assert out[-1, col] == out[0, col] + 1
    for c in (0, 1, 2, 3, 7):
        assert np.array_equal(out[:, c], want[:, c]), (nat.ACTION_IMPACT[c], out[:, c], want[:, c])
    for c in (5, 6):
        assert len(set(out[:, c].tolist())) == 1
        np.testing.assert_allclose(out[:, c], want[:, c], rtol=0, atol=DB_ATOL)
    # the kernel's own value of the victim after the candidate: lowest_margin_after + its minimum_osnr (the victim is the lowest)
    assert int(out[0, 7]) == record[int(case.pairs[case.i, 1])]
    e = abs(float(out[0, 5]) + case.pairs[case.i, 4] - case.g)
    print(f"action_impact: lowest margin after {out[0, 5]!r}, restated {case.g - case.pairs[case.i, 4]!r}, e = {e:.3e} dB")
    assert 4 * e < tl.ZONE_DB


@pytest.mark.parametrize("kernel", ["lean", "generic"])
def test_lowest_fragmentation_on_its_own_ladder(kernel, monkeypatch):
    """Policy 10 scores every candidate, so no first-fit ladder moves its answer; this ladder sits on the candidate it chooses
    (tl.policy_state_case).  policy_actions(10) and one step_policy(policy=10) step, which is the lean kernel's own walk."""
    pid = nat.POLICY_LOWEST_FRAGMENTATION
    case = tl.policy_state_case(pid)
    env = state_env(case, monkeypatch, kernel=kernel)
    assert env.occupancy(pid)["lean_kernel"] == KERNELS[kernel][1]
    want = [o.policy(pid) for o in case.oracles]
    acts, flags = env.policy_actions(pid)
    got = [(int(a), bool(f & nat.F_BLOCKED_RESOURCES), bool(f & nat.F_BLOCKED_OSNR)) for a, f in zip(acts[1:], flags[1:])]
    assert ladder_values(case, got, want, f"policy_actions(10) {kernel}")
    rec = env.step_policy(1, record=True, policy=pid)[0, 1:]
    wrec = np.stack([o.run_policy(pid, 1)[0] for o in tl.state_oracles(case.t, case.margins)[1]])
    assert ladder_values(case, [int(x) for x in rec["action"]], [int(x) for x in wrec["action"]], f"step_policy(10) {kernel}")
    assert rec["accepted"].all() and rec["modulation"][0] == case.m and rec["modulation"][-1] != case.m
    for r in np.flatnonzero(tl.exact_rungs(case)):
        assert_records_equal(rec[r:r + 1], wrec[r:r + 1], f"step_policy(10) {kernel} rung {r}")
