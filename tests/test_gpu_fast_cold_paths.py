"""The blocks that first fit's step loop keeps off a request's common path (csrc/ongym_fast.hpp, FF_COLD / FF_HOT; DESIGN.md
section 5, "Branches on a request's path") are still reached and still right: the flush of the GSNR product, a full service
table at both provisioning sites, the refill of the request ring and episode resets at ring positions other than 0, both
rejection passes, routes that take path_and's link loop, the second AND for a narrower width, and the dB-domain test of the
1e-9 band.

Every case runs first fit on 64 replicas, seed 5, in launches of uneven length, in the narrow and the wide build
(ONGYM_FORCE_WIDE=1), with and without step records, against the CPU oracle: the step records where they are written, final
grids, services (sorted) and statistics (episode_osnr_sum at rtol 1e-9).  One run of every case uses the instantiation that sums
link weights in a loop (ONGYM_FAST_NO_LWTAB=1).

The inputs were chosen on the CPU oracle; every case recomputes the counts its assertions rest on from the oracle's records,
prints them and asserts them (all 64 replicas of the run of the test):

    case        topology  S    capacity  load  bit rates        launches               episode  modulations
    flush       nsfnet    320    512     300   10,40,100,400    1,63,250,7,500,129,550   4000    JOCN
    full        nsfnet    320     64     300   10,40,100,400    1,63,250,7,279           4000    JOCN
    ring        nsfnet    320    512     300   10,40,100,400    1,63,64,65,130            150    JOCN
    rejections  nsfnet     80    256     300   100,400          1,63,250,7,279           4000    JOCN
    narrower    nsfnet    160    448     400   10,40,100,400    1,63,250,7,500,179       4000    8QAM and 16QAM swapped

    flush       every replica accepts 1 460 to 1 496 of its 1 500 requests (at least 700 asserted).  Every factor of the product of
                1/GSNR is at most 10^(-3.71/10), BPSK's threshold, so 700 accepted requests carry it below 1e-250 whatever the GSNRs
                are: every replica flushes at least once (twice, in fact).
    full        69.1 % of the steps carry F_OVERFLOW (at least 10 % asserted; 64.8 % on the replica with the fewest); the run without
                records meets it where the format passes (accept in place), the run with records behind the search.  Everything is compared;
                the two fixed differences in how a refused request is booked are asserted as such (compare_full).
    ring        the episodes end at steps 148 and 297 of every replica (a reset draws a request of its own, so the ring positions of
                the resets' draws are 150 % 64 = 22 and 300 % 64 = 44), the ring is refilled five times, and launches of 1, 63, 64, 65 and
                130 steps put launch boundaries at ring positions 1, 0, 0, 2 (after the first reset) and on either side of a refill.
    rejections  41.8 % of the requests are rejected (at least 10 % asserted): 16 034 with F_BLOCKED_RESOURCES, 2 916 with
                F_BLOCKED_OSNR.
    narrower    925 requests are served by a route of five or more hops (path_and's link loop; at least 20 asserted), and 3 076 are
                served at a format above which the walk passed a wider one that the ASE bound had not ruled out on that route
                (at least 20 asserted): the AND of the route's rows is taken a second time for the narrower width.

The JOCN traffic table cannot produce a request of the last kind: its slot counts never fall as the modulation index falls (400
Gb/s: 32, 16, 11, 8, 7, 6 slots for BPSK .. 64QAM), so the walk, which goes from the highest format down, never meets a narrower
width behind a wider one.  The `narrower` case swaps the spectral efficiencies of 8QAM and 16QAM and keeps the thresholds in
place: format 3 (10.84 dB ... 13.24 dB, 3 bit/s/Hz: 11 slots at 400 Gb/s) is wider than format 2 below it (4 bit/s/Hz: 8 slots),
so a request that format 3 refuses and format 2 serves takes the second AND.  "Not ruled out by the bound" is evaluated as the
kernel evaluates it: the GSNR of (route, slot 0, the wider format's width) on the empty network against the format's threshold.

The band is run on tests/threshold_ladder.py's construction (read-only): the first-fit ladders of tests/test_gpu_threshold_ladder.py,
here WITHOUT step records, which is the kernel that provisions in place.  Without records the decision at t* is read off the
final state: all rungs share one request stream and no other decision of a run lies within 1e-6 dB of its threshold, so a rung
ends in the state of the lowest rung's oracle (the candidate accepted) or in the state of the highest rung's (fallen through).
Asserted: every rung ends in one of the two, along T_r the state changes exactly once, every rung with |T_r - g| >= 1e-11 dB ends in
its own oracle's state with its own oracle's statistics, and the change lies inside the zone.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import threshold_ladder as tl
from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv, OngymError
from optical_networking_gym.topology import Modulation
from oracle_lib import OracleEnv

pytestmark = pytest.mark.gpu

GSNR_RTOL = 1e-9
EXACT = ("action", "route", "modulation", "slot", "nslots", "accepted", "terminated", "retry", "flags", "active", "reward")
STATS = ("services_processed", "services_accepted", "episode_services_processed", "episode_services_accepted",
         "bit_rate_requested", "bit_rate_provisioned", "episode_bit_rate_provisioned", "rejected", "episodes_completed",
         "total_steps", "total_accepted", "total_paths_tried", "total_path_hops", "total_active_sum", "current_time", "active")
PID = nat.POLICY_FIRST_FIT
SEED = 5
B = 64
ENV_VARS = ("ONGYM_FORCE_GENERIC", "ONGYM_FORCE_WIDE", "ONGYM_FAST_NO_LWTAB")
RATES = (10, 40, 100, 400)


def swapped_modulations():
    """JOCN's six formats with the spectral efficiencies of 8QAM and 16QAM exchanged (see the module docstring)."""
    m = jocn_modulations()
    return (m[0], m[1], Modulation("16QAM", 500, 4, m[2].minimum_osnr, -20), Modulation("8QAM", 1000, 3, m[3].minimum_osnr, -23),
            m[4], m[5])


CASES = {
    "flush": dict(topo="nsfnet", S=320, capacity=512, load=300.0, bit_rates=RATES, launches=(1, 63, 250, 7, 500, 129, 550),
                  episode_length=4000),
    "full": dict(topo="nsfnet", S=320, capacity=64, load=300.0, bit_rates=RATES, launches=(1, 63, 250, 7, 279), episode_length=4000),
    "ring": dict(topo="nsfnet", S=320, capacity=512, load=300.0, bit_rates=RATES, launches=(1, 63, 64, 65, 130), episode_length=150),
    "rejections": dict(topo="nsfnet", S=80, capacity=256, load=300.0, bit_rates=(100, 400), launches=(1, 63, 250, 7, 279),
                       episode_length=4000),
    "narrower": dict(topo="nsfnet", S=160, capacity=448, load=400.0, bit_rates=RATES, launches=(1, 63, 250, 7, 500, 179),
                     episode_length=4000, modulations=swapped_modulations()),
}


def config(c):
    return dict(modulations=c.get("modulations") or jocn_modulations(), num_spectrum_resources=c["S"], capacity=c["capacity"],
                load=c["load"], bit_rate_selection="discrete", bit_rates=c["bit_rates"], auto_reset=True,
                episode_length=c["episode_length"])


_oracle = {}


def oracle_run(name):
    """Step records [steps, B], the request of every step and the oracles (final state) of one case: computed once, only read
    afterwards."""
    if name not in _oracle:
        c = CASES[name]
        steps = sum(c["launches"])
        holder = nat.ConfigHolder(golden_tables(c["topo"]), batch=B, **config(c))
        recs = np.zeros((steps, B), nat.STEP_DTYPE)
        reqs = np.zeros((steps, B), nat.REQUEST_DTYPE)
        envs = [OracleEnv(holder, replica=r) for r in range(B)]

        def run(r):         # one oracle per replica, no shared state: the C calls run side by side (ctypes drops the GIL)
            o = envs[r]
            o.seed(SEED); o.reset()
            if name == "narrower":      # the request of every step is needed for its counts
                for t in range(steps):
                    reqs[t, r] = o.request()
                    recs[t, r] = o.run_policy(PID, 1)[0]
            else:
                recs[:, r] = o.run_policy(PID, steps)

        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            list(pool.map(run, range(B)))
        _oracle[name] = (holder, recs, reqs, envs)
    return _oracle[name]


def assert_records_equal(got, want, ctx):
    for f in EXACT:
        if not np.array_equal(got[f], want[f]):
            bad = np.argwhere(got[f] != want[f])[0]
            raise AssertionError(f"{ctx}: field {f} differs first at {tuple(bad)}: {got[f][tuple(bad)]} != {want[f][tuple(bad)]}")
    for f in ("osnr", "ase", "nli"):
        np.testing.assert_allclose(got[f], want[f], rtol=GSNR_RTOL, err_msg=f"{ctx}: {f}")


def assert_state_equal(env, st, r, o, ctx):
    np.testing.assert_array_equal(env.grid(r), o.grid(), err_msg=f"{ctx} replica {r}: grid")
    a = np.sort(env.services(r), order=["release_time", "path_id", "slot"])
    b = np.sort(o.services(), order=["release_time", "path_id", "slot"])
    assert a.tobytes() == b.tobytes(), f"{ctx} replica {r}: services"
    so = o.stats()
    for f in STATS:
        assert st[r][f] == so[f], (ctx, r, f, st[r][f], so[f])
    np.testing.assert_array_equal(st[r]["episode_modulation_hist"], so["episode_modulation_hist"])
    np.testing.assert_allclose(st[r]["episode_osnr_sum"], so["episode_osnr_sum"], rtol=GSNR_RTOL, err_msg=f"{ctx} replica {r}")
    # the device settles some evaluations by the ASE bound (see test_gpu_parity.test_random_traffic_vs_oracle)
    assert st[r]["total_gn_evals"] <= so["total_gn_evals"] <= st[r]["total_gn_evals"] + st[r]["total_gn_shortcuts"]


def stats_of(env, full):
    """env.stats(); after a replica has met a full service table the call refuses (ONGYM_E_CAPACITY, "raise capacity") once it has
    filled its output: the refusal is part of the case, and the statistics are read with the same library call."""
    if not full:
        return env.stats()
    with pytest.raises(OngymError, match="overflowed its service table"):
        env.stats()
    out = np.zeros(env.batch_size, nat.STATS_DTYPE)
    assert env.lib.ongym_stats_get(env._h, out.ctypes.data) == -4
    return out


# A full table is an error state (stats() refuses, "raise capacity"), and the oracle and the kernels (the parent's as well) book
# the refused request differently, in a way that is fixed:
#   - the oracle counts the refused request's format in episode_modulation_hist (before it looks for a free record) and not in
#     `rejected`; the kernels count it in `rejected` and not in the histogram;
#   - the oracle's record of such a step keeps the route and the slot of the refused candidate and the reward of an explicit
#     action; the kernels' record has route = slot = -1 and the reward of a rejection, -6.
# Every other record field, every other statistic and the whole state agree, and all of it is asserted: nothing is left open.
def compare_full(env, got, want, oracles, ctx):
    c = CASES["full"]
    S, M = c["S"], len(jocn_modulations())
    ov = (want["flags"] & nat.F_OVERFLOW).astype(bool)
    fmt = M - 1 - (want["action"].astype(np.int64) // S) % M          # format of every step's action (get_action_index)
    if got is not None:
        assert_records_equal(got[~ov], want[~ov], f"{ctx}, steps without overflow")
        for f in EXACT:
            if f not in ("route", "slot", "reward"):
                assert np.array_equal(got[f][ov], want[f][ov]), (ctx, f, "overflow steps")
        for f in ("osnr", "ase", "nli"):
            assert np.array_equal(got[f][ov], want[f][ov]) and not got[f][ov].any(), (ctx, f)
        assert (got["route"][ov] == -1).all() and (got["slot"][ov] == -1).all() and (got["reward"][ov] == -6.0).all(), ctx
        assert (want["route"][ov] >= 0).all() and (want["slot"][ov] >= 0).all()
    st = stats_of(env, full=True)
    for r in range(B):
        o = oracles[r]
        np.testing.assert_array_equal(env.grid(r), o.grid(), err_msg=f"{ctx} replica {r}: grid")
        a = np.sort(env.services(r), order=["release_time", "path_id", "slot"])
        b = np.sort(o.services(), order=["release_time", "path_id", "slot"])
        assert a.tobytes() == b.tobytes(), f"{ctx} replica {r}: services"
        so = o.stats()
        n_ov = int(ov[:, r].sum())
        for f in STATS:
            want_f = so[f] + n_ov if f == "rejected" else so[f]
            assert st[r][f] == want_f, (ctx, r, f, st[r][f], so[f], n_ov)
        hist = np.asarray(so["episode_modulation_hist"]).copy()
        hist[:M] -= np.bincount(fmt[ov[:, r], r], minlength=M)
        np.testing.assert_array_equal(st[r]["episode_modulation_hist"], hist, err_msg=f"{ctx} replica {r}")
        np.testing.assert_allclose(st[r]["episode_osnr_sum"], so["episode_osnr_sum"], rtol=GSNR_RTOL, err_msg=f"{ctx} replica {r}")
        assert st[r]["total_gn_evals"] <= so["total_gn_evals"] <= st[r]["total_gn_evals"] + st[r]["total_gn_shortcuts"]
        assert bool(st[r]["flags"] & nat.F_OVERFLOW) == (n_ov > 0), (ctx, r)


def set_kernel(monkeypatch, wide, table):
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    if wide:
        monkeypatch.setenv("ONGYM_FORCE_WIDE", "1")       # read at ongym_create
    if not table:
        monkeypatch.setenv("ONGYM_FAST_NO_LWTAB", "1")    # read at ongym_create


def run_and_compare(name, wide, record, table, monkeypatch):
    c = CASES[name]
    set_kernel(monkeypatch, wide, table)
    holder, want, reqs, oracles = oracle_run(name)
    env = BatchedQRMSAEnv(tables=golden_tables(c["topo"]), batch_size=B, **config(c))
    env.seed(SEED); env.reset()
    assert env.occupancy(PID)["lean_kernel"]
    assert (env.link_weight_entry(0, 0) is not None) == table
    got = [env.step_policy(n, record=record, policy=PID) for n in c["launches"]]
    ctx = f"{name} wide {wide} record {record} table {table}"
    if name == "full":
        compare_full(env, np.concatenate(got) if record else None, want, oracles, ctx)
        return want, reqs
    if record:
        assert_records_equal(np.concatenate(got), want, ctx)
    st = stats_of(env, full=False)
    for r in range(B):
        assert_state_equal(env, st, r, oracles[r], ctx)
    return want, reqs


# (wide, record, table): narrow and wide, with and without records, and the link-loop instantiation
KERNELS = [(False, False, True), (False, True, True), (True, False, True), (True, True, True), (False, False, False)]
KERNEL_IDS = ["narrow-norecord", "narrow-record", "wide-norecord", "wide-record", "linkloop-norecord"]


@pytest.mark.parametrize("wide,record,table", KERNELS, ids=KERNEL_IDS)
def test_flush_of_the_gsnr_product_vs_oracle(wide, record, table, monkeypatch):
    want, _ = run_and_compare("flush", wide, record, table, monkeypatch)
    acc = want["accepted"].astype(bool).sum(0)
    worst = float(want["osnr"][want["accepted"].astype(bool)].min())
    print(f"flush: accepted per replica {int(acc.min())} .. {int(acc.max())} of {want.shape[0]}; lowest GSNR accepted {worst:.3f} dB")
    assert acc.min() >= 700
    # every factor 1/GSNR is at most 10^(-3.71/10): 700 of them are below 1e-250
    assert worst >= 3.71 and 700 * 3.71 / 10.0 > 250.0


@pytest.mark.parametrize("wide,record,table", KERNELS, ids=KERNEL_IDS)
def test_full_service_table_at_both_provisioning_sites_vs_oracle(wide, record, table, monkeypatch):
    want, _ = run_and_compare("full", wide, record, table, monkeypatch)
    ov = (want["flags"] & nat.F_OVERFLOW).astype(bool)
    print(f"full: steps with F_OVERFLOW {ov.mean():.3f} (fewest on one replica {ov.mean(0).min():.3f}) accepted "
          f"{want['accepted'].mean():.3f} most services {int(want['active'].max())}")
    assert 10 * int(ov.sum()) >= ov.size
    assert ov.any(0).all() and int(want["active"].max()) == CASES["full"]["capacity"]
    assert not (ov & want["accepted"].astype(bool)).any()


@pytest.mark.parametrize("wide,record,table", KERNELS, ids=KERNEL_IDS)
def test_ring_refills_and_resets_off_the_grid_vs_oracle(wide, record, table, monkeypatch):
    want, _ = run_and_compare("ring", wide, record, table, monkeypatch)
    c = CASES["ring"]
    term = want["terminated"].astype(bool)
    at = np.unique(np.argwhere(term)[:, 0])
    # requests drawn before the reset at step t: the one of the start, one per step, one per earlier reset
    pos = [(int(t) + 2 + i) % 64 for i, t in enumerate(at)]
    print(f"ring: episodes end at steps {at.tolist()} of every replica; ring positions of the resets' draws {pos}; launches "
          f"{c['launches']}")
    assert (term.sum(0) == 2).all() and at.size == 2
    assert all(p != 0 for p in pos)
    assert sum(c["launches"]) + 1 + at.size > 5 * 64              # five refills
    assert c["launches"] == (1, 63, 64, 65, 130)


@pytest.mark.parametrize("wide,record,table", KERNELS, ids=KERNEL_IDS)
def test_rejection_passes_vs_oracle(wide, record, table, monkeypatch):
    want, _ = run_and_compare("rejections", wide, record, table, monkeypatch)
    acc = want["accepted"].astype(bool)
    fl = want["flags"][~acc]
    n_res, n_osnr = int((fl & nat.F_BLOCKED_RESOURCES).astype(bool).sum()), int((fl & nat.F_BLOCKED_OSNR).astype(bool).sum())
    print(f"rejections: rejected {1 - acc.mean():.3f} with F_BLOCKED_RESOURCES {n_res} with F_BLOCKED_OSNR {n_osnr} overflow "
          f"{int((want['flags'] & nat.F_OVERFLOW).astype(bool).sum())}")
    assert 10 * int((~acc).sum()) >= acc.size
    assert n_res >= 20 and n_osnr >= 20
    assert not (want["flags"] & nat.F_OVERFLOW).any()


def narrower_counts(holder, want, reqs):
    """(requests served by a route of >= 5 hops, requests served at a format behind a wider one the bound had not ruled out)."""
    c = CASES["narrower"]
    tb = golden_tables(c["topo"])
    thr = np.array([m.minimum_osnr for m in c["modulations"]], np.float64)
    empty = OracleEnv(holder, replica=0)
    empty.seed(SEED); empty.reset()
    n_of = {(br, m): empty.number_slots(float(br), m) for br in c["bit_rates"] for m in range(len(thr))}
    acc = want["accepted"].astype(bool)
    pp = np.asarray(tb.pair_paths).reshape(tb.n_nodes, tb.n_nodes, tb.k_paths)
    path = pp[reqs["source"].astype(int), reqs["destination"].astype(int), np.clip(want["route"].astype(int), 0, tb.k_paths - 1)]
    long5 = int((acc & (np.asarray(tb.path_hops)[path] >= 5)).sum())
    open_ = {}

    def not_ruled_out(p, br, m):            # the ASE bound of (route, format): the GSNR at slot 0 of the empty network
        if (p, br, m) not in open_:
            open_[(p, br, m)] = float(empty.gn(p, 0, n_of[(br, m)])[0]) >= thr[m]
        return open_[(p, br, m)]

    again = 0
    for t, r in np.argwhere(acc):
        m, br, p = int(want["modulation"][t, r]), int(reqs["bit_rate"][t, r]), int(path[t, r])
        again += any(n_of[(br, m2)] > n_of[(br, m)] and not_ruled_out(p, br, m2) for m2 in range(m + 1, len(thr)))
    return long5, again, {br: [n_of[(br, m)] for m in range(len(thr))] for br in c["bit_rates"]}


@pytest.mark.parametrize("wide,record,table", KERNELS, ids=KERNEL_IDS)
def test_long_routes_and_a_narrower_width_vs_oracle(wide, record, table, monkeypatch):
    want, reqs = run_and_compare("narrower", wide, record, table, monkeypatch)
    if "counts" not in CASES["narrower"]:
        CASES["narrower"]["counts"] = narrower_counts(oracle_run("narrower")[0], want, reqs)
    long5, again, slots = CASES["narrower"]["counts"]
    print(f"narrower: slots per (bit rate, format) {slots}; accepted {want['accepted'].mean():.3f}; served by a route of >= 5 hops "
          f"{long5}; served at a format behind a wider one that the bound had not ruled out {again}")
    assert slots[400][3] > slots[400][2] and slots[100][3] > slots[100][2]
    assert long5 >= 20 and again >= 20
    assert not (want["flags"] & nat.F_OVERFLOW).any()


# ---- the band: tests/threshold_ladder.py's first-fit ladders without step records ----------------------------------------------
# (case, environment variables read at ongym_create, link-weight table expected (None: either))
BAND_RUNS = [("ff_nsfnet_m0", {}, True), ("ff_nsfnet_m0", {"ONGYM_FAST_NO_LWTAB": "1"}, False),
             ("ff_nsfnet_m0", {"ONGYM_FORCE_WIDE": "1"}, None), ("ff_nsfnet_m1", {}, True), ("ff_nobeleu", {}, None),
             ("ff_nsfnet_s2", {}, True), ("ff_trace", {}, None)]
BAND_IDS = ["m0-table", "m0-linkloop", "m0-wide", "m1-table", "nobeleu-two-words", "s2-table", "trace"]


def state_bytes(grid, services):
    s = np.sort(services, order=["release_time", "path_id", "slot"])
    return np.ascontiguousarray(grid).tobytes() + s.tobytes()


@pytest.mark.parametrize("name,env_vars,table", BAND_RUNS, ids=BAND_IDS)
def test_band_decisions_without_records_on_the_ladder(name, env_vars, table, monkeypatch):
    case = tl.find_case(name)
    assert case.policy == PID
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for v, x in env_vars.items():
        monkeypatch.setenv(v, x)                    # read at ongym_create
    nb = tl.B
    env = BatchedQRMSAEnv(tables=case.tables, batch_size=nb, **case.kw)
    if case.trace is not None:
        env.set_requests(np.ascontiguousarray(np.broadcast_to(case.trace, (nb, len(case.trace)))))
        env.reset()
    else:
        env.seed(case.seed)
        env.reset()
        env.fork(np.zeros(nb, np.int32), keep_params=True)
    assert env.occupancy(PID)["lean_kernel"]
    if table is not None:
        assert (env.link_weight_entry(0, 0) is not None) == table
    # uneven launches to t* + 41 steps with t* inside one (as tests/test_gpu_threshold_ladder.py cuts them)
    t, n = case.t, case.steps
    cuts = sorted({x for x in (1, 8, t - 5, t + 3, n) if 0 < x <= n and x not in (t, t + 1)})
    assert cuts[-1] == n
    for k in np.diff([0] + cuts).tolist():
        env.step_policy(k, record=False, policy=PID)
    st = env.stats()
    want = [state_bytes(o.grid(), o.services()) for o in case.oracles]
    assert want[0] != want[-1] and case.accepts[0] and not case.accepts[-1]
    got = [state_bytes(env.grid(r), env.services(r)) for r in range(nb)]
    took = np.array([g == want[0] for g in got])
    fell = np.array([g == want[-1] for g in got])
    assert (took ^ fell).all(), f"{name}: a rung ends in neither history: took {took.astype(int)} fell {fell.astype(int)}"
    k = tl.one_change(took)
    ex = tl.exact_rungs(case)
    print(f"{name} {env_vars}: t* {t} g {case.g!r} format {case.m}; accepted along T_r {took.astype(int).tolist()}; change between "
          f"T - g = {case.T[k - 1] - case.g:.3e} and {case.T[k] - case.g:.3e} dB; rungs held to their own oracle {int(ex.sum())}")
    assert k > 0, f"{name}: decisions along T_r do not change exactly once: {took.astype(int)}"
    assert np.array_equal(took[ex], case.accepts[ex])
    assert abs(case.T[k - 1] - case.g) < tl.ZONE_DB and abs(case.T[k] - case.g) < tl.ZONE_DB
    for r in np.flatnonzero(ex | (took == case.accepts)):
        assert_state_equal(env, st, r, case.oracles[r], f"{name} rung {r}")
