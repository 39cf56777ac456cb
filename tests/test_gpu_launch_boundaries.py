"""A replica's state across launch boundaries and across hand-overs between the step kernels (schedules: tests/launch_schedule.py).

1. Partition invariance, same kernel: the chopped schedule (boundaries on the request ring's edge, on terminal steps, on the end of
   a replayed trace) against the same steps in one launch - step records, every byte of stats(), grids, pending requests and
   service tables in order.  k_fast of the four lean policies (narrow and wide build, 32-bit and M64 record codec with the
   path-hash store, the TRACE instantiation) and k_run (per-link attenuation, policy 5, ONGYM_FORCE_GENERIC=1).
2. The mixed schedule against the oracle: the lean kernels of different policies, k_run's four run modes (policy step, action step,
   action-then-policy in step_bundle, policy-only in policy_actions), masked resets and the counters-only reset on one replica.
3. Lean against generic: the two runs of 2. agree at every segment end.
That no launch is idle and that the boundaries sit where they should is asserted from the oracle's records alone
(launch_schedule.check_*; tests/test_launch_schedule_host.py does the same without a GPU).

Stats fields that are NOT held exactly to the oracle in 2. and 3., and why:
  total_gn_evals, total_gn_shortcuts, total_interferer_terms   the device settles evaluations by the ASE + self-channel lower
        bound (`Params.ase_shortcut`, DESIGN.md section 4 "Kernels").  Over EVERY fused policy launch of the mixed schedule (deltas
        of the launch, the first from the reset state) they are held to the inequalities of test_random_traffic_vs_oracle:
            evals <= oracle's evals,  interferer terms <= oracle's terms      every policy, both kernels
            oracle's evals <= evals + shortcuts                               except UPPER_EXEMPT, below
        UPPER_EXEMPT, where one device evaluation or shortcut stands for several evaluations of the oracle by design:
          lowest fragmentation, both kernels: the oracle restates the heuristic literally, every candidate painted and scored
              (DESIGN.md section 2); the device scores a route once and takes its first start that passes (section 4).
          load balancing, lean kernel: routes are examined in ascending (load, index) order and the first that serves wins
              ("ascending (load, index) order"), the oracle walks them in index order; k_run is not exempt.
          highest SNR, lean kernel: the bound at slot 0 settles a whole format (one shortcut for all its starts), and a format
              whose bound cannot beat the best candidate so far is not evaluated (section 4, same paragraph); k_run is not exempt.
  total_paths_tried, total_path_hops   exact over every first-fit, load-balancing and highest-SNR launch, on both kernels.  The
        oracle counts them in these three policies only, and its policy() calls (the mirror of policy_actions and of
        step_bundle's next action) count too, so the cumulative values are not compared; otherwise left to 1.
  episode_osnr_sum, last_mean_gsnr   floating-point sums of GSNR values that agree to GSNR_RTOL: rel = GSNR_RTOL.
In 1. nothing is exempt: stats() is compared as bytes.
"""
import numpy as np
import pytest

import launch_schedule as ls
from common import record_bytes
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import OngymError
from test_gpu_parity import GSNR_RTOL, assert_records_equal

pytestmark = pytest.mark.gpu

B = ls.B
WORK = ("total_gn_evals", "total_gn_shortcuts", "total_interferer_terms", "total_paths_tried", "total_path_hops")
APPROX = ("episode_osnr_sum", "last_mean_gsnr")
EXACT_STATS = tuple(f for f in nat.STATS_DTYPE.names if f not in WORK + APPROX)
UPPER_EXEMPT = {(ls.LF, True), (ls.LF, False), (ls.LB, True), (ls.HSNR, True)}      # (policy, lean kernel): see the module docstring
ORACLE_COUNTS_PATHS = (ls.FF, ls.LB, ls.HSNR)
CHEAP_ORACLE = (ls.FF, ls.LB, ls.GENERIC_ONLY_POLICY)     # policies whose 900 oracle steps take well under a second


def device_snapshot(env) -> ls.Snapshot:
    """stats, grids, pending requests (bytes) and service tables IN TABLE ORDER of every replica."""
    return ls.Snapshot(env.stats(), [env.grid(r) for r in range(B)], [env.request(r).tobytes() for r in range(B)],
                       [env.services(r) for r in range(B)])


def first_difference(a, b) -> str:
    """Where two structured arrays of the same dtype differ: the first field and index."""
    for f in a.dtype.names:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.tobytes() != y.tobytes():
            bad = np.argwhere(x.view(np.uint8).reshape(x.shape + (-1,)) != y.view(np.uint8).reshape(y.shape + (-1,)))[0][:x.ndim]
            return f"field {f} first at {tuple(int(i) for i in bad)}: {x[tuple(bad)]!r} != {y[tuple(bad)]!r}"
    return "equal"


def same_state(a: ls.Snapshot, b: ls.Snapshot, ctx, stats_mask_flags=0):
    """Byte equality of two device snapshots: stats (every field), grids, pending requests, service tables in order."""
    sa, sb = a.stats.copy(), b.stats.copy()
    sa["flags"] &= ~stats_mask_flags
    sb["flags"] &= ~stats_mask_flags
    assert sa.tobytes() == sb.tobytes(), f"{ctx}: stats differ, {first_difference(sa, sb)}"
    for r in range(B):
        np.testing.assert_array_equal(a.grids[r], b.grids[r], err_msg=f"{ctx}: grid of replica {r}")
        assert a.requests[r] == b.requests[r], f"{ctx}: pending request of replica {r}"
        assert len(a.services[r]) == len(b.services[r]), f"{ctx}: replica {r} holds {len(a.services[r])} / {len(b.services[r])} services"
        assert a.services[r].tobytes() == b.services[r].tobytes(), \
            f"{ctx}: service table of replica {r} (in order), {first_difference(a.services[r], b.services[r])}"


# ---- 1. partition invariance ----------------------------------------------------------------------------------------------------
def _case_id(c):
    key, pol, parity, generic, kind = c
    return f"{key}-p{pol}-parity{parity}" + ("-generic" if generic else "") + (f"-{kind}" if kind else "")


@pytest.mark.parametrize("case", ls.PARTITION_CASES, ids=_case_id)
def test_chopped_launches_equal_one_launch(case):
    """Assertion 1.  Launch i of the chopped run is recorded when i + parity is even; the single launch is recorded, and a third
    environment runs it unrecorded (the benchmark's instantiation) and must end in the same state."""
    key, pol, parity, generic, kind = case
    lengths, _, valid, _ = ls.partition_schedule(key, kind)
    total = sum(lengths)
    if pol in CHEAP_ORACLE:
        want, _ = ls.oracle_run(key, pol, ls.TRACE_STEPS if valid is not None else ls.T)
        ls.check_activity(want, lengths, valid, _case_id(case))
    envs = [ls.make_env(key, generic) for _ in range(3)]
    chopped, coarse, coarse_norec = envs
    lean = ls.CONFIGS[key]["lean"] and not generic and pol in ls.LEAN_POLICIES
    for e in envs:
        assert e.occupancy(pol)["lean_kernel"] == lean
    got, snaps = [], []
    for i, n in enumerate(lengths):
        got.append(chopped.step_policy(n, record=ls.recorded(i, parity), policy=pol))
        if valid is not None:
            snaps.append(device_snapshot(chopped))
    whole = coarse.step_policy(total, policy=pol)
    assert coarse_norec.step_policy(total, record=False, policy=pol) is None
    for i, (s, n) in enumerate(zip(ls.starts_of(lengths), lengths)):
        if got[i] is not None:
            assert record_bytes(got[i]) == record_bytes(whole[s:s + n]), \
                f"launch {i} ({n} steps from {s}): records differ from the single launch, {first_difference(got[i], whole[s:s + n])}"
    end = device_snapshot(coarse)
    same_state(device_snapshot(chopped), end, "chopped against one launch")
    same_state(device_snapshot(coarse_norec), end, "one unrecorded launch against one recorded launch")
    if pol in CHEAP_ORACLE:                          # and the single launch is the oracle's trajectory
        for r in range(B):
            v = total if valid is None else int(valid[r])
            assert_records_equal(whole[:v, r], want[:v, r], f"{_case_id(case)} replica {r}")
    if valid is not None:
        # after the trace ran out: every step a flagged no-op, and the no-op launches leave the state as it is
        for r in range(B):
            tail = whole[int(valid[r]):, r]
            assert ((tail["flags"] & nat.F_NO_REQUEST) != 0).all() and (tail["action"] == -1).all() and not tail["accepted"].any()
            assert not (whole[:int(valid[r]), r]["flags"] & nat.F_NO_REQUEST).any()
        st = ls.starts_of(lengths)
        done = [i for i in range(len(lengths)) if st[i] + lengths[i] >= int(valid.max())]
        assert len(done) >= 1 + len(ls.NOOP_TAIL)
        for i in done[1:]:
            same_state(snaps[i], snaps[done[0]], f"no-op launch {i} ({lengths[i]} steps)", stats_mask_flags=nat.F_NO_REQUEST)


# ---- 2. and 3.: the mixed schedule ----------------------------------------------------------------------------------------------
_RUNS = {}          # (key, generic) -> ("ok", result) or ("failed", message): a run that died is not started on the GPU again


def device_mixed_run(key, generic):
    """The mixed plan on the device, once per session (see _mixed_run)."""
    if (key, generic) not in _RUNS:
        try:
            _RUNS[key, generic] = ("ok", _mixed_run(key, generic))
        except BaseException as e:
            _RUNS[key, generic] = ("failed", f"{type(e).__name__}: {e}")
            raise
    state, result = _RUNS[key, generic]
    if state != "ok":
        pytest.fail(f"the mixed run of {key} (generic={generic}) failed before and is not run again: {result}")
    return result


def _mixed_run(key, generic):
    """The plan of launch_schedule.mixed_plan on the device; per segment (records or None, policy_actions' answers, step_bundle's
    answers, snapshot).  Asserts nothing about the results (the tests do), only that a refused call is refused.  The environment
    is closed at the end: only host arrays are kept."""
    env = ls.make_env(key, generic)
    lean = {p: env.occupancy(p)["lean_kernel"] for p in ls.LEAN_POLICIES + (ls.GENERIC_ONLY_POLICY,)}
    out = []
    for seg in ls.mixed_plan(key):
        rec = asked = bundle = None
        if seg.kind == "start":
            pass
        elif seg.kind in ls.KIND_POLICY:
            rec = env.step_policy(seg.n, record=seg.record, policy=seg.policy)
        elif seg.kind == "reset":
            env.reset(seg.mask)
        elif seg.kind == "counters":
            env.reset_episode_counters(seg.mask)
        elif seg.kind == "counters_refused":
            with pytest.raises(OngymError, match="track_service_ids"):
                env.reset_episode_counters(seg.mask)
        else:
            rec = np.zeros((seg.n, B), nat.STEP_DTYPE)
            asked = np.zeros((seg.n, B), np.int32)
            bundle = []
            for j in range(seg.n):
                if seg.kind == "actions_ff":
                    asked[j] = env.policy_actions(ls.FF)[0]
                if seg.kind == "bundle_lb":
                    rec[j], req, st, na, nf = env.step_bundle(seg.actions[j], next_policy=ls.LB)
                    bundle.append((req, st, na))
                else:
                    rec[j] = env.step(seg.actions[j])
        out.append((rec, asked, bundle, device_snapshot(env)))
    env.close()
    return lean, out


def services_for_oracle(svc, ids_tracked):
    """A device service table as the oracle exports it: sorted; with ids tracked, without the id and GSNR columns (the oracle
    fills them under defragmentation only) and without the services a counters-only reset left running for good (release time
    +inf on the device, dropped from the oracle's departure heap; their slots are held to the oracle by the grid)."""
    if ids_tracked:
        svc = svc[np.isfinite(svc["release_time"])].copy()
        svc["service_id"], svc["osnr"] = -1, 0.0
    return ls.sort_services(svc)


def compare_snapshots(got: ls.Snapshot, want: ls.Snapshot, ctx, bad, ids_tracked=False, both_device=False):
    """The field set of assertions 2 and 3; mismatches are appended to `bad`."""
    for r in range(B):
        for f in EXACT_STATS:
            if not np.array_equal(got.stats[r][f], want.stats[r][f]):
                bad.append(f"{ctx} replica {r}: stats {f} {got.stats[r][f]} != {want.stats[r][f]}")
        for f in APPROX:
            if got.stats[r][f] != pytest.approx(want.stats[r][f], rel=GSNR_RTOL):
                bad.append(f"{ctx} replica {r}: stats {f} {got.stats[r][f]!r} != {want.stats[r][f]!r} (rel {GSNR_RTOL})")
        if not np.array_equal(got.grids[r], want.grids[r]):
            bad.append(f"{ctx} replica {r}: grid")
        if got.requests[r] != want.requests[r]:
            bad.append(f"{ctx} replica {r}: pending request")
        if both_device:
            a, b = ls.sort_services(got.services[r]), ls.sort_services(want.services[r])
        else:
            a, b = services_for_oracle(got.services[r], ids_tracked), want.services[r]
        if a.tobytes() != b.tobytes():
            bad.append(f"{ctx} replica {r}: services ({len(a)} / {len(b)}), {first_difference(a, b) if len(a) == len(b) else ''}")


MIXED = [(k, g) for k in ("nsfnet96", "nobeleu128") for g in (False, True)] + [("nsfnet96_ids", False)]


@pytest.mark.parametrize("key,generic", MIXED, ids=[f"{k}-{'generic' if g else 'default'}" for k, g in MIXED])
def test_mixed_schedule_vs_oracle(key, generic):
    """Assertion 2: every recorded segment's records, and after every segment every replica's statistics, grid, pending request and
    services, against the oracle.  policy_actions' and step_bundle's choices must be the oracle's."""
    plan = ls.mixed_plan(key)
    lean, run = device_mixed_run(key, generic)
    ids = bool(ls.config_kw(key).get("track_service_ids"))
    for p in ls.LEAN_POLICIES:
        assert lean[p] == (ls.CONFIGS[key]["lean"] and not generic), p
    assert not lean[ls.GENERIC_ONLY_POLICY]
    bad, worst = [], {}
    prev_dev = prev_orc = None
    for i, (seg, (rec, asked, bundle, snap)) in enumerate(zip(plan, run)):
        ctx = f"segment {i} ({seg.kind}, {seg.n})"
        try:
            if seg.kind in ls.KIND_POLICY:
                if seg.record:
                    assert_records_equal(rec, seg.want, ctx)
                else:
                    assert rec is None
            elif seg.actions is not None:
                ok = seg.rc == 0
                assert_records_equal(rec[ok], seg.want[ok], ctx)
                # the reference raises its QoT ValueError there: flagged, nothing applied (test_random_external_actions_vs_oracle)
                assert ((rec[~ok]["flags"] & nat.F_QOT_ERROR) != 0).all() and not rec[~ok]["accepted"].any(), f"{ctx}: QoT errors"
                assert not (rec[ok]["flags"] & nat.F_QOT_ERROR).any(), f"{ctx}: QoT errors the oracle does not have"
                if seg.kind == "actions_ff":
                    np.testing.assert_array_equal(asked, seg.actions, err_msg=f"{ctx}: policy_actions(first fit)")
                if seg.kind == "bundle_lb":
                    np.testing.assert_array_equal(np.stack([b[2] for b in bundle]), seg.next_actions, err_msg=f"{ctx}: next actions")
                    assert bundle[-1][1].tobytes() == snap.stats.tobytes(), f"{ctx}: the bundle's statistics are not stats()"
                    assert [q.tobytes() for q in bundle[-1][0]] == snap.requests, f"{ctx}: the bundle's requests"
        except AssertionError as e:
            bad.append(str(e)[:600])
        compare_snapshots(snap, seg.after, ctx, bad, ids_tracked=ids)
        if seg.kind == "counters_refused" and prev_dev is not None:
            try:
                same_state(snap, prev_dev, f"{ctx}: the refused call changed the state")
            except AssertionError as e:
                bad.append(str(e)[:600])
        if seg.kind in ls.KIND_POLICY:              # the launch's work counters: deltas over the segment (segment 0: from the reset state)
            for r in range(B):
                d = {f: int(snap.stats[r][f]) - int(prev_dev.stats[r][f]) for f in WORK}
                o = {f: int(seg.after.stats[r][f]) - int(prev_orc.stats[r][f]) for f in WORK}
                worst.setdefault(seg.policy, []).append((d, o))
                ok = d["total_gn_evals"] <= o["total_gn_evals"] and d["total_interferer_terms"] <= o["total_interferer_terms"]
                if (seg.policy, lean[seg.policy]) not in UPPER_EXEMPT:
                    ok = ok and o["total_gn_evals"] <= d["total_gn_evals"] + d["total_gn_shortcuts"]
                if seg.policy in ORACLE_COUNTS_PATHS:
                    ok = ok and d["total_paths_tried"] == o["total_paths_tried"] and d["total_path_hops"] == o["total_path_hops"]
                if not ok:
                    bad.append(f"{ctx} replica {r}: work counters of the launch, device {d}, oracle {o}")
        prev_dev, prev_orc = snap, seg.after
    for pol, rows in sorted(worst.items()):          # printed before the verdict: the figures of every fused policy segment
        tot = lambda side, f: sum(row[side][f] for row in rows)
        print(f"{key} generic={generic} policy {pol}: " + ", ".join(f"{f} {tot(0, f)} / {tot(1, f)}" for f in WORK))
    assert not bad, f"{len(bad)} mismatches, the first:\n" + "\n".join(bad[:25])


@pytest.mark.parametrize("key", ["nsfnet96", "nobeleu128"])
def test_mixed_schedule_lean_equals_generic(key):
    """Assertion 3: the run whose fused launches are k_fast and the run under ONGYM_FORCE_GENERIC=1 agree at every segment end on
    the field set of assertion 2, and on every record both wrote."""
    (_, a), (_, b) = device_mixed_run(key, False), device_mixed_run(key, True)
    bad = []
    for i, (seg, x, y) in enumerate(zip(ls.mixed_plan(key), a, b)):
        ctx = f"segment {i} ({seg.kind}, {seg.n}) lean / generic"
        if x[0] is not None:
            try:
                assert_records_equal(x[0], y[0], ctx)
            except AssertionError as e:
                bad.append(str(e)[:600])
        compare_snapshots(x[3], y[3], ctx, bad, both_device=True)
    assert not bad, f"{len(bad)} mismatches, the first:\n" + "\n".join(bad[:25])
