"""The winner's choice of highest SNR (policy 2) on near-ties between two equal routes ("Decision exactness").

tests/tie_ladder.py builds, per case (S = 64 with 9 requests, S = 160 with 21) and ladder (the noise figure of a link of route 1, or
of route 0, times 1 + eps), 21 environments with eps from 0 to +-1e-6 and three replicas at -3, 0 and +2 dBm; every other
decision meets a state that is symmetric between the routes, whose best candidates then differ by delta of about 1.2 to 2.1 |eps|
dB.  tests/test_tie_ladder_host.py holds on the oracle that the ladders are sound.  Here the kernels run them: the lean narrow
kernel, the lean wide kernel (ONGYM_FORCE_WIDE=1) and the generic kernel (ONGYM_FORCE_GENERIC=1).

1. Step kernels.  step_policy(policy=2) with records, in uneven launches with a laddered decision inside a launch.
     exact rungs    where every laddered decision of a replica has |delta| >= 1e-11 dB, the records of the whole run (EXACT fields
                    bit-exact, GSNR/ASE/NLI at 1e-9), the final grid, services and stats() equal the rung's own oracle;
     exempt rungs   every decision whose own |delta| >= 1e-11 equals the oracle's as long as the histories agree; at a decision
                    inside the zone the device may take either route and must take the oracle's slot, format and width on that
                    route; what follows is compared only if that decision agreed with the oracle's;
     eps = 0        route 0 wins every laddered decision (the first-wins rule, in loaded states);
     lean/generic   on every exact rung the lean and the generic kernels' records are the same bits in the EXACT fields.
2. Measured noise.  Per ladder, e = max |env.gsnr(c) - oracle.gn(c)| over both routes' best candidates at every laddered decision
   of every rung (as long as the device's history is the oracle's) is printed and 4 e < 1e-11 asserted: the condition of
   tests/test_gpu_threshold_ladder.py for the exempt zone, on which the tie band kTieBandDb = 1e-12 dB rests (at least 4 e, and a
   tenth of the zone).
3. Other entry points on the pending state of the last laddered decision: policy_actions(2) is the oracle's action on exact rungs
   and leaves the state byte-identical; the run without step records (the REC == false winner update) reaches the oracle's final
   grids and services; the plugin-API heuristic_highest_snr_plugin (strict `>` over device GSNRs, on the compatibility view of
   the same rung) returns the fused policy's action on exact rungs.

Measured on MI355X: e = 7.1e-15 dB (two ulp of a GSNR near 20 dB) on each of s64 route1 (582 candidates), s64 route0 (582), s160
route1 (1266) and s160 route0 (1266); the band is 140 e.  Every delta comes from the oracle on the CPU
(tests/test_tie_ladder_host.py prints their ranges).  Inside the zone the kernels left the oracle's history only on rungs with
|eps| <= 1e-13 (|delta| below the band); at |eps| = 2e-12 (|delta| 2.4e-12 to 4.2e-12 dB) they took the oracle's route.  With the
bands the kernels had before (1e-9 dB generic, 1e-10 relative lean) this module failed on the rungs |eps| = 3e-11, 1e-10, 2e-10 where
the second route is the better one, the generic kernel and policy_actions also at 4e-10, and lean against generic at 4e-10.
"""
import functools
import os

import numpy as np
import pytest

import tie_ladder as tl
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from test_gpu_threshold_ladder import ENV_VARS, EXACT, STATS, assert_records_equal

pytestmark = pytest.mark.gpu

B = tl.B
# kernel name -> (environment variables read at ongym_create, lean kernel expected)
KERNELS = {"lean": ({}, True), "lean_wide": ({"ONGYM_FORCE_WIDE": "1"}, True), "generic": ({"ONGYM_FORCE_GENERIC": "1"}, False)}
LADDERS = [(c, l) for c in tl.CASES for l in tl.LADDERS]
RUNS = [(c, l, k) for c, l in LADDERS for k in KERNELS]
CUTS = {9: (4, 7, 9), 21: (1, 8, 16, 21)}              # launches end after these many steps


def make_env(rung, kernel):
    """The rung's device environment, reset on the trace; the kernel's environment variables hold while it is created."""
    env_vars, lean = KERNELS[kernel]
    saved = {v: os.environ.pop(v, None) for v in ENV_VARS}
    try:
        os.environ.update(env_vars)                     # read at ongym_create
        env = BatchedQRMSAEnv(tables=rung.tables, batch_size=B, **rung.kw)
    finally:
        for v in ENV_VARS:
            os.environ.pop(v, None)
            if saved[v] is not None:
                os.environ[v] = saved[v]
    env.set_requests(np.ascontiguousarray(np.broadcast_to(rung.trace, (B, len(rung.trace)))))
    env.reset()
    assert env.occupancy(tl.HSNR)["lean_kernel"] == lean, (rung.case, rung.eps, kernel)
    return env


def launch_lengths(n):
    """Uneven launches with a laddered decision that is neither the first nor the last step of its launch."""
    cuts = CUTS[n]
    lengths = np.diff((0,) + cuts).tolist()
    assert cuts[-1] == n and len(set(lengths)) > 1
    assert any(tl.laddered(t) and a < t < b - 1 for a, b in zip((0,) + cuts, cuts) for t in range(a, b))
    return lengths


def sorted_services(svcs):
    return np.sort(svcs, order=["release_time", "path_id", "slot"]).tobytes()


class DeviceRun:
    pass


@functools.lru_cache(maxsize=None)
def device_run(case, ladder, kernel):
    """Per rung: the records of step_policy(policy=2) over the whole trace, and the final grids, services and statistics."""
    runs = []
    for rung in tl.find_ladder(case, ladder):
        env = make_env(rung, kernel)
        d = DeviceRun()
        d.recs = np.concatenate([env.step_policy(k, record=True, policy=tl.HSNR) for k in launch_lengths(rung.n)])
        d.grids = [env.grid(b) for b in range(B)]
        d.services = [sorted_services(env.services(b)) for b in range(B)]
        d.stats = env.stats()
        env.close()
        runs.append(d)
    return runs


def check_final_state(rung, b, grid, services, ctx):
    o = rung.oracles[b]
    np.testing.assert_array_equal(grid, o.grid(), err_msg=f"{ctx}: grid")
    assert services == sorted_services(o.services()), f"{ctx}: services"


def check_replica(rung, d, b, ctx):
    """One replica of one rung against its oracle; returns whether the whole history was the oracle's."""
    got, want = d.recs[:, b], rung.recs[:, b]
    ex = rung.exact()[:, b]
    for t in range(rung.n):
        at = f"{ctx} decision {t} (delta {rung.delta[t, b]:+.3e} dB)"
        if ex[t] or rung.eps == 0.0:
            if tl.laddered(t) and got["route"][t] != want["route"][t]:
                raise AssertionError(f"{at}: route {got['route'][t]}, the oracle's {want['route'][t]}")
            assert_records_equal(got[t:t + 1], want[t:t + 1], at)
            continue
        # inside the zone: either route, and on it the oracle's best candidate
        assert got["accepted"][t] == 1 and got["route"][t] in (0, 1), at
        w = rung.best[t, b, int(got["route"][t])]
        for f in ("modulation", "slot", "nslots"):
            assert got[f][t] == w[f], f"{at}: {f} {got[f][t]} on route {got['route'][t]}, the oracle's best there has {w[f]}"
        np.testing.assert_allclose(got["osnr"][t], w["osnr"], rtol=1e-9, err_msg=at)
        if got["route"][t] != want["route"][t]:
            return False                    # another history from here on
        assert_records_equal(got[t:t + 1], want[t:t + 1], at)
    check_final_state(rung, b, d.grids[b], d.services[b], ctx)
    so = rung.oracles[b].stats()
    for f in STATS:
        assert d.stats[b][f] == so[f], (ctx, f, d.stats[b][f], so[f])
    np.testing.assert_array_equal(d.stats[b]["episode_modulation_hist"], so["episode_modulation_hist"], err_msg=ctx)
    return True


def exact_run(rung, b):
    """Every laddered decision of the replica is exact (the others always are): the whole run is held to the oracle."""
    return bool(rung.exact()[:, b].all())


@pytest.mark.parametrize("case,ladder,kernel", RUNS)
def test_step_kernels_on_the_ladder(case, ladder, kernel):
    rungs, runs = tl.find_ladder(case, ladder), device_run(case, ladder, kernel)
    failures, held, diverged = [], 0, []
    for rung, d in zip(rungs, runs):
        for b in range(B):
            ctx = f"{case} {ladder} {kernel} eps {rung.eps:+.0e} replica {b} ({tl.POWERS_DBM[b]:+.0f} dBm)"
            try:
                whole = check_replica(rung, d, b, ctx)
            except AssertionError as exc:
                failures.append(str(exc).strip().splitlines()[0])
                continue
            if exact_run(rung, b) or rung.eps == 0.0:
                assert whole
                held += 1
            elif not whole:
                diverged.append((rung.eps, b))
        if rung.eps == 0.0:
            lad = [t for t in range(rung.n) if tl.laddered(t)]
            if not (d.recs["route"][lad] == 0).all():
                failures.append(f"{case} {ladder} {kernel} eps 0: a later equal route took the lead: {d.recs['route'][lad].tolist()}")
    print(f"{case} {ladder} {kernel}: {held} of {len(rungs) * B} runs held to the oracle from end to end; inside the zone the device "
          f"left the oracle's history on (eps, replica) {diverged}")
    assert not failures, f"{len(failures)} runs differ from their oracle:\n" + "\n".join(failures)
    assert held >= (len(rungs) - 6) * B


@pytest.mark.parametrize("case,ladder", LADDERS)
def test_lean_against_generic(case, ladder):
    rungs = tl.find_ladder(case, ladder)
    generic = device_run(case, ladder, "generic")
    failures = []
    for kernel in ("lean", "lean_wide"):
        for rung, a, g in zip(rungs, device_run(case, ladder, kernel), generic):
            for b in range(B):
                if not exact_run(rung, b):
                    continue
                for f in EXACT:
                    if not np.array_equal(a.recs[f][:, b], g.recs[f][:, b]):
                        t = int(np.flatnonzero(a.recs[f][:, b] != g.recs[f][:, b])[0])
                        failures.append(f"{case} {ladder} eps {rung.eps:+.0e} replica {b}: {kernel} and generic differ in {f} at "
                                        f"decision {t} (delta {rung.delta[t, b]:+.3e} dB): {a.recs[f][t, b]} != {g.recs[f][t, b]}")
                        break
    assert not failures, f"{len(failures)} runs differ between the kernels:\n" + "\n".join(failures)


@pytest.mark.parametrize("case,ladder", LADDERS)
def test_summation_order_noise_is_below_the_exempt_zone(case, ladder):
    """e = |device GSNR - oracle GSNR| of both routes' best candidates at every laddered decision; the zone is 1e-11 dB and the
    tie band a tenth of it: four times e must fit in the band."""
    e, count = 0.0, 0
    for rung in tl.find_ladder(case, ladder):
        env = make_env(rung, "lean")
        for t in range(0, rung.n, 2):
            assert tl.laddered(t)
            for b in range(B):
                for w in rung.best[t, b]:
                    got = env.gsnr(b, int(w["path"]), int(w["slot"]), int(w["nslots"]))[0]
                    e = max(e, abs(float(got) - float(w["osnr"])))
                    count += 1
            rec = env.step_policy(min(2, rung.n - t), record=True, policy=tl.HSNR)
            if not np.array_equal(rec["action"], rung.recs["action"][t:t + 2]):
                break                       # the device's history is no longer this oracle's
        env.close()
    print(f"{case} {ladder}: e = {e:.3e} dB over {count} candidates")
    assert count >= 21 * B * 2
    assert 4 * e < tl.ZONE_DB, (case, ladder, e)
    assert 4 * e < 1e-12, (case, ladder, e)             # kTieBandDb (csrc/ongym_device.hpp)


@pytest.mark.parametrize("case,ladder,kernel", RUNS)
def test_entry_points_on_the_last_laddered_decision(case, ladder, kernel):
    failures, held = [], 0
    for rung in tl.find_ladder(case, ladder):
        t = rung.n - 1
        assert tl.laddered(t)
        env = make_env(rung, kernel)
        env.step_policy(t, record=False, policy=tl.HSNR)
        before = env.save_state().tobytes()
        acts, flags = env.policy_actions(tl.HSNR)
        assert env.save_state().tobytes() == before, f"{case} {ladder} {kernel} eps {rung.eps}: policy_actions changed the state"
        env.step_policy(1, record=False, policy=tl.HSNR)
        for b in range(B):
            if not (exact_run(rung, b) or rung.eps == 0.0):
                continue
            ctx = f"{case} {ladder} {kernel} eps {rung.eps:+.0e} replica {b} (delta {rung.delta[t, b]:+.3e} dB)"
            held += 1
            try:
                assert (int(acts[b]), int(flags[b])) == (int(rung.recs["action"][t, b]), 0), \
                    f"{ctx}: policy_actions(2) gave {acts[b]}, the oracle {rung.recs['action'][t, b]}"
                check_final_state(rung, b, env.grid(b), sorted_services(env.services(b)), f"{ctx}: run without records")
            except AssertionError as exc:
                failures.append(str(exc).strip().splitlines()[0])
        env.close()
    assert not failures, f"{len(failures)} replicas differ from their oracle:\n" + "\n".join(failures)
    assert held >= (21 - 6) * B


@pytest.mark.parametrize("b", range(B))
@pytest.mark.parametrize("case,ladder", LADDERS)
def test_plugin_heuristic_on_the_last_laddered_decision(case, ladder, b, tmp_path):
    """heuristic_highest_snr_plugin asks the device for every candidate's GSNR and compares with a strict `>`: on an exact rung its
    answer is the fused policy's and the oracle's."""
    from optical_networking_gym.envs.qrmsa import QRMSAEnv
    from optical_networking_gym.heuristics.heuristics import heuristic_highest_snr, heuristic_highest_snr_plugin
    S, held = tl.CASES[case]["S"], 0
    for rung in tl.find_ladder(case, ladder):
        if not exact_run(rung, b):
            continue
        held += 1
        sim = QRMSAEnv(tl.rung_topology(tmp_path, tl.LADDERS[ladder], rung.eps), num_spectrum_resources=S, episode_length=1000, load=10.0,
                       bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), launch_power_dbm=tl.POWERS_DBM[b],
                       bandwidth=S * 12.5e9, margin=0.0, k_paths=2, modulations_to_consider=6, gen_observation=False, capacity=64,
                       sync_views=False, requests=rung.trace)
        ctx = f"{case} {ladder} eps {rung.eps:+.0e} at {tl.POWERS_DBM[b]:+.0f} dBm"
        for t in range(rung.n - 1):
            action, _, _ = heuristic_highest_snr(sim)
            assert action == rung.recs["action"][t, b], (ctx, t)
            sim.step(action)
        fused, plugin = heuristic_highest_snr(sim), heuristic_highest_snr_plugin(sim)
        assert fused == plugin == (int(rung.recs["action"][-1, b]), False, False), (ctx, fused, plugin, rung.delta[-1, b])
        sim.close()
    assert held >= 21 - 7
