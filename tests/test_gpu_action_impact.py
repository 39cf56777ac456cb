"""Effect of candidate actions on the running lightpaths (ongym_action_impact through BatchedQRMSAEnv.action_impact).  Every GPU
computation runs in ONE fresh child process (tests/action_impact_child.py); the tests assert on the .npz it writes.

The restatement lives here.  For a state, an action and a victim y: the per-link interferer lists of
test_gpu_service_qot.interferer_lists, with the candidate's (slot, n, se) appended LAST on every link of y's path that the
candidate's route uses (the reference appends to a link's running list when it provisions), evaluated by the oracle's literal
GN (OracleEnv.gn_lists).  tests/test_action_impact_host.py pins it to the oracle's own step and counts, for the seeds used
here, the (action, victim) pairs the restatement alone puts within 1e-8 relative of a limit: 0 of 45 305 pairs over the seven
cases that need no device records (ids_nsfnet_320 takes its service ids from the device), so the 0.1 % cap on pairs left out
of the count comparison is far away.

Tolerances (none of them comes from the code under test): columns 5 and 6 are compared at rtol = 1e-9 on the linear 1/GSNR
(GN_RTOL of the project: the device's sum order differs from the reference's list order by a few ulp), which is
10 log10(1 + 1e-9) = 4.4e-9 dB absolute on a margin and on a drop; columns 0, 1, 7 exactly; columns 2-4 exactly except for
actions that hold a pair inside the band, at most 0.1 % of the pairs of a case."""
import os
import subprocess
import sys

import numpy as np
import pytest

from optical_networking_gym import _native as nat
from test_gpu_blocks import fitting_blocks, route_row
from test_gpu_service_qot import GN_RTOL, insertion_order, interferer_lists

pytestmark = pytest.mark.gpu

# "<traffic>_<topology>_<S>" (service_qot_child.case_config builds them)
CASES = ("ff_nsfnet_320", "disr_nsfnet_320", "lb_cost239_160", "wide_nobeleu_320", "alpha_nsfnet_320", "trace_nsfnet_160",
         "ids_nsfnet_320", "ff_germany50_100")
REPLICAS = {"disr_nsfnet_320": 16}          # the others: 3
SEED = 11
J = 8
DB_ATOL = 10.0 * np.log10(1.0 + GN_RTOL)    # 4.4e-9 dB: rtol 1e-9 on the linear 1/GSNR
BAND = 1e-8                                 # relative distance of 1/GSNR to a limit inside which a count may differ
BAND_CAP = 1e-3                             # ... for at most this fraction of the compared pairs of a case
COLS = {k: i for i, k in enumerate(nat.ACTION_IMPACT)}


# ---- the restatement ----------------------------------------------------------------------------------------------------
def drive(key, B, seed, env=None):
    """(tables, kwargs, holder, oracles) of a case after its traffic; `env`, a device environment of the same
    configuration, is driven in lock step (service_qot_child.oracle_case, the traffic kinds of CASES)"""
    from oracle_lib import OracleEnv
    from service_qot_child import case_config
    tb, kw, how, steps = case_config(key)
    holder = nat.ConfigHolder(tb, batch=B, **kw)
    oracles = [OracleEnv(holder, replica=r) for r in range(B)]
    rng = np.random.default_rng(seed)
    if how == "trace":                  # bit rates beyond the configured table: slot counts above the pair table's range
        n = steps + 40
        reqs = np.zeros((B, n), nat.REQUEST_DTYPE)
        for r in range(B):
            reqs[r]["arrival_time"] = np.cumsum(rng.exponential(10800.0 / kw["load"], n)).astype(np.float32)
            reqs[r]["holding_time"] = rng.exponential(10800.0, n).astype(np.float32)
            src = rng.integers(0, tb.n_nodes, n)
            reqs[r]["source"], reqs[r]["destination"] = src, (src + rng.integers(1, tb.n_nodes, n)) % tb.n_nodes
            reqs[r]["bit_rate"] = rng.choice(np.array([10, 100, 400, 1000]), n)
        if env is not None:
            env.set_requests(reqs)
        for r, o in enumerate(oracles):
            o.set_trace(reqs[r])
    else:
        if env is not None:
            env.seed(seed)
        for o in oracles:
            o.seed(seed)
    if env is not None:
        env.reset()
    for o in oracles:
        o.reset()
    if how == "ids":                    # counters-only reset in the middle: ids restart under services that keep running
        half = steps // 2
        if env is not None:
            env.step_policy(half, record=False)
            env.reset_episode_counters()
            env.step_policy(steps - half, record=False)
        for o in oracles:
            o.run_first_fit(half)
            o.reset_counters()
            o.run_first_fit(steps - half)
    elif how == "lb":
        if env is not None:
            env.step_policy(steps, record=False, policy=nat.POLICY_LOAD_BALANCING)
        for o in oracles:
            o.run_policy(nat.POLICY_LOAD_BALANCING, steps)
    else:
        if env is not None:
            env.step_policy(steps, record=False)
        for o in oracles:
            o.run_first_fit(steps)
    return tb, kw, holder, oracles


def oracle_block_row(o, tb, holder, blocks=J):
    """the action_map row of observe_blocks(blocks) for the oracle's current request (the definition of test_gpu_blocks.restate)"""
    c = holder.struct
    K, M = c.k_paths, c.n_mods
    reject = o.reject_action
    row = np.full(K * blocks + 1, reject, np.int32)
    q = o.request()
    src, dst = int(q["source"]), int(q["destination"])
    grid = o.grid() != 0
    n = [o.number_slots(float(q["bit_rate"]), m) for m in range(M)]
    for k in range(K):
        path = int(tb.pair_paths[src, dst, k])
        if path < 0:
            continue
        free = route_row(grid, tb.path_links, tb.path_hops, path)
        fit = [fitting_blocks(free, n[m])[:blocks] if 0 < n[m] <= c.n_slots else [] for m in range(M)]
        for j in range(blocks):
            for m in range(M - 1, -1, -1):
                if len(fit[m]) <= j:
                    continue
                a = fit[m][j][0]
                if o.gn(path, a, n[m])[0] >= holder.mod_thr[m] + c.margin:
                    row[k * blocks + j] = o.encode(k, m, a)
                    break
    return row


def decode(o, tb, holder, action):
    """(status, path, slot, n, modulation) of a step action on the oracle's current request: 1 no placement, 2 not free"""
    c = holder.struct
    if action < 0 or action >= o.reject_action:
        return 1, -1, 0, 0, 0
    route, m, slot = o.decode(int(action))
    q = o.request()
    if m < 0 or m >= c.n_mods:
        return 2, -1, 0, 0, 0
    path = int(tb.pair_paths[int(q["source"]), int(q["destination"]), route])
    n = o.number_slots(float(q["bit_rate"]), m)
    if path < 0 or n <= 0 or not o.is_path_free(path, slot, n):
        return 2, path, slot, n, m
    return 0, path, slot, n, m


def candidate_actions(o, tb, holder, block_row):
    """the list of a replica: its block row, the first-fit action, the reject action, -1 and one action on occupied spectrum"""
    ff = o.policy_first_fit()[0]
    q = o.request()
    occupied = o.reject_action
    m = o.max_modulation_idx
    path = int(tb.pair_paths[int(q["source"]), int(q["destination"]), 0])
    n = o.number_slots(float(q["bit_rate"]), m)
    if path >= 0 and n > 0:
        for s in range(holder.struct.n_slots - n):
            if not o.is_path_free(path, s, n):
                occupied = o.encode(0, m, s)
                break
    return np.concatenate([np.asarray(block_row, np.int32), np.array([ff, o.reject_action, -1, occupied], np.int32)])


class Restater:
    """GSNR (dB) of the running services `svcs` (the oracle's order) before and after a candidate, by the literal GN"""

    def __init__(self, o, tb, mod_se, svcs, ids=None):
        self.o, self.tb, self.se, self.svcs, self.ids = o, tb, np.asarray(mod_se), svcs, ids
        self.paths = svcs["path_id"].astype(np.int64)
        self.on_link = np.zeros((len(svcs), tb.n_links), bool)
        for y, p in enumerate(self.paths):
            self.on_link[y, tb.path_links[p, :tb.path_hops[p]]] = True
        self._lists, self._before = {}, {}

    def lists(self, y):
        if y not in self._lists:
            counts, intf = interferer_lists(self.tb, self.se, self.svcs, y, self.ids)
            self._lists[y] = np.split(intf.reshape(-1, 3), np.cumsum(counts)[:-1])
        return self._lists[y]

    def _gn(self, y, segs):
        s = self.svcs
        return self.o.gn_lists(int(s["path_id"][y]), int(s["slot"][y]), int(s["nslots"][y]),
                               np.array([len(x) for x in segs], np.int32), np.concatenate(segs))[0]

    def before(self, y):
        if y not in self._before:
            self._before[y] = self._gn(y, self.lists(y))
        return self._before[y]

    def victims(self, path, cur_id=None):
        links = self.tb.path_links[path, :self.tb.path_hops[path]]
        v = np.any(self.on_link[:, links], axis=1)
        if self.ids is not None and cur_id is not None:
            v &= self.ids != cur_id                                 # the request's namesakes never see it (quirk Q12)
        return np.flatnonzero(v)

    def after(self, y, path, slot, n, m):
        cl = set(self.tb.path_links[path, :self.tb.path_hops[path]].tolist())
        mine = self.tb.path_links[self.paths[y], :self.tb.path_hops[self.paths[y]]].tolist()
        cand = np.array([[slot, n, self.se[m]]], np.int16)
        segs = [np.concatenate([seg, cand]) if l in cl else seg for l, seg in zip(mine, self.lists(y))]
        return self._gn(y, segs)


def restate_replica(o, tb, holder, svcs, actions, ids=None, cur_id=None):
    """(status [A], pairs [n, 5]: action index, index into svcs, GSNR before, GSNR after, minimum_osnr of the victim)"""
    rs = Restater(o, tb, holder.mod_se, svcs, ids)
    status, pairs = np.zeros(len(actions), np.int64), []
    for a, action in enumerate(actions):
        st, path, slot, n, m = decode(o, tb, holder, int(action))
        status[a] = st
        if st:
            continue
        for y in rs.victims(path, cur_id):
            pairs.append((a, y, rs.before(y), rs.after(y, path, slot, n, m), holder.mod_thr[svcs["modulation"][y]]))
    return status, np.array(pairs, np.float64).reshape(-1, 5)


def in_band(pairs, margin):
    """pairs whose restated 1/GSNR, before or after, lies within BAND relative of minimum_osnr or minimum_osnr + margin"""
    out = np.zeros(len(pairs), bool)
    for g in (pairs[:, 2], pairs[:, 3]):
        for lim in (pairs[:, 4], pairs[:, 4] + margin):
            out |= np.abs(10.0 ** ((lim - g) / 10.0) - 1.0) < BAND
    return out


def rows_from_pairs(n_actions, status, pairs, record, margin):
    """the impact_out rows of one replica from the restated pairs; record[y] = device record index of svcs[y]"""
    rows = np.full((n_actions, len(nat.ACTION_IMPACT)), np.nan)
    rows[:, 0] = status
    for a in np.flatnonzero(status == 0):
        p = pairs[pairs[:, 0] == a]
        rows[a, 1:5] = 0
        rows[a, 7] = -1
        if not len(p):
            continue
        before, after, thr = p[:, 2], p[:, 3], p[:, 4]
        rec = record[p[:, 1].astype(np.int64)]
        mg = after - thr
        lo = np.flatnonzero(mg == mg.min())
        rows[a, 1] = len(p)
        rows[a, 2] = np.sum(after < thr)
        rows[a, 3] = np.sum((after < thr) & ~(before < thr))
        rows[a, 4] = np.sum((after < thr + margin) & ~(before < thr + margin))
        rows[a, 5], rows[a, 6], rows[a, 7] = mg.min(), np.max(before - after), rec[lo].min()
    return rows


def compare_rows(got, want, skip_counts=(), ctx=""):
    """impact rows against restated rows under the module's rules; the count columns of the actions in skip_counts are left out"""
    assert np.array_equal(got[:, 0], want[:, 0]), ctx
    assert np.array_equal(np.isnan(got), np.isnan(want)), ctx
    ok = want[:, 0] == 0
    assert np.array_equal(got[ok][:, [1, 7]], want[ok][:, [1, 7]]), ctx
    counted = ok & ~np.isin(np.arange(len(got)), list(skip_counts))
    assert np.array_equal(got[counted][:, 2:5], want[counted][:, 2:5]), (ctx, got[counted][:, 2:5], want[counted][:, 2:5])
    some = ok & (want[:, 1] > 0)
    np.testing.assert_allclose(got[some][:, 5:7], want[some][:, 5:7], rtol=0, atol=DB_ATOL, err_msg=ctx)
    return int(ok.sum())


# ---- the child's results ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("action_impact") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "action_impact_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "action impact child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def case_rows(res, key, which="impact"):
    """per replica: (device rows, restated rows, actions whose counts are left out, pairs, pairs in the band)"""
    out = []
    for r in range(int(res[key + "_B"])):
        k = f"{key}_r{r}"
        pairs, margin = res[k + "_pairs"], float(res[key + "_margin"])
        want = rows_from_pairs(len(res[k + "_actions"]), res[k + "_status"], pairs, res[k + "_record"], margin)
        band = in_band(pairs, margin)
        out.append((res[f"{k}_{which}"], want, set(pairs[band, 0].astype(int).tolist()), pairs, int(band.sum())))
    return out


@pytest.mark.parametrize("which", ["impact", "impact_svc"])
@pytest.mark.parametrize("key", CASES)
def test_impact_equals_the_restatement(res, key, which):
    """the NULL path and the svc_in path, every column, every replica and action of the case"""
    n_pairs = n_band = evaluated = 0
    for r, (got, want, skip, pairs, band) in enumerate(case_rows(res, key, which)):
        evaluated += compare_rows(got, want, skip, f"{key} r{r} {which}")
        n_pairs += len(pairs)
        n_band += band
    print(f"{key} {which}: {evaluated} evaluated actions, {n_pairs} pairs, {n_band} in the band")
    assert evaluated > 0 and n_pairs > 0
    assert n_band <= BAND_CAP * n_pairs, (key, n_band, n_pairs)


@pytest.mark.parametrize("key", CASES)
def test_every_status_occurs_and_the_block_row_is_the_restated_one(res, key):
    seen = set()
    for r in range(int(res[key + "_B"])):
        k = f"{key}_r{r}"
        seen |= set(res[k + "_impact"][:, 0].astype(int).tolist())
        assert np.array_equal(res[k + "_actions"][:len(res[k + "_oracle_row"])], res[k + "_oracle_row"]), k
    assert seen == {0, 1, 2}, (key, seen)


def test_the_disruption_case_is_not_trivial(res):
    key = "disr_nsfnet_320"
    assert int(res[key + "_B"]) >= 16
    newly = np.concatenate([g[w[:, 0] == 0][:, COLS["newly_below_minimum"]] for g, w, _, _, _ in case_rows(res, key)])
    below = np.concatenate([g[w[:, 0] == 0][:, COLS["below_minimum_after"]] for g, w, _, _, _ in case_rows(res, key)])
    print(f"disr: {len(newly)} evaluated actions, {int(np.sum(newly > 0))} with newly_below_minimum > 0, "
          f"{int(np.sum(below > newly))} where below_minimum_after exceeds it")
    assert np.any(newly > 0) and np.any(newly == 0)
    assert np.any(below > newly)                                  # victims already below before: column 3 is not column 2


def test_the_cases_exercise_what_they_claim(res):
    assert res["trace_nsfnet_160_wide_candidates"] > 0            # candidates wider than the pair table (the asinh path)
    assert res["ids_nsfnet_320_namesakes"] > 0                    # running records with the request's id, left out
    assert not res["alpha_nsfnet_320_uniform"]
    assert res["ff_germany50_100_links"] > 64                     # the generic record codec, two mask words


def test_forked_steps_agree_with_the_reported_impact(res):
    """existing device code as the witness: fork every source replica over its block row, step, service_qot().  Where the step
    accepted and released nothing, every old record's new margin is the After of the call: its aggregates are recomputed
    from the stepped replica's service_qot margins (matched by path and slot) and compared under the module's rules"""
    accepted, qualified = int(res["fork_accepted"]), int(res["fork_qualified"])
    print(f"forks: {accepted} accepted, {qualified} released nothing, {int(res['fork_pairs'])} old records compared")
    assert accepted > 0 and 4 * qualified >= accepted
    got, want, skip = res["fork_got"], res["fork_want"], res["fork_band"] != 0
    assert len(got) == qualified
    assert np.array_equal(got[:, [0, 1, 7]], want[:, [0, 1, 7]])
    assert np.array_equal(got[~skip][:, 2:5], want[~skip][:, 2:5])
    assert skip.sum() <= BAND_CAP * int(res["fork_pairs"])
    some = want[:, 1] > 0
    np.testing.assert_allclose(got[some][:, 5:7], want[some][:, 5:7], rtol=0, atol=DB_ATOL)


def test_action_impact_is_read_only(res):
    assert res["ro_blob_same"] and res["ro_stats_same"] and res["ro_traj_same"]


def test_fresh_replicas_have_no_victims(res):
    rows = res["fresh_rows"]
    assert len(rows) >= 8 and np.all(rows[:, 0] == 0) and np.all(rows[:, 1:5] == 0)
    assert np.all(np.isnan(rows[:, 5:7])) and np.all(rows[:, 7] == -1)


def test_device_io_on_the_current_stream_equals_the_host_path(res):
    assert res["dev_same"] and res["dev_svc_same"] and res["dev_one_column_same"] and res["dev_stream_refused"]


def test_compat_environment_reports_the_first_fit_action(res):
    assert res["compat_same"]


def test_library_refuses_bad_counts(res):
    assert int(res["refuse_zero_rc"]) == -1 and int(res["refuse_257_rc"]) == -1 and int(res["refuse_null_rc"]) == -1
    assert "n_actions" in str(res["refuse_zero_msg"])


def test_protect_running_masks_and_rollout(res):
    assert res["protect_off_masks_same"]                          # default: the masks of observe_blocks, bit for bit
    assert res["protect_cleared"] > 0 and res["protect_cleared_all_disrupt"] and res["protect_reject_allowed"]
    assert res["protect_infos_ok"]
    off, on = int(res["protect_disrupted_off"]), int(res["protect_disrupted_on"])
    print(f"masked-random rollout, disrupted services: {off} unprotected, {on} with protect_running")
    assert off > 0 and on <= off
