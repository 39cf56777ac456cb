"""Child process of tests/test_gpu_admission_map.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP
runtime and this library's must start together), saved to an .npz that the tests assert on.

    python tests/admission_map_child.py OUT.npz

It also holds the restatement of ongym_admission_map (include/ongym.h) in plain numpy, which shares nothing with the device
code and is built from the pieces of tests/failure_impact_child.py that tests/test_failure_impact_host.py pins to the CPU
oracle's own first fit: a scenario starts from a replica's running records and slot grid (the device's services() and grid()
on the GPU, an oracle's on the CPU), optionally provisions the decoded candidate and appends it to the running records, and
then calls `search` for every (node pair, rate) cell with all routes of the pair, the slot counts of the header's formula and
`gn_running` with nobody left out.  The summary is summed over the cells in pair-major order.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402,F401  (before the library is loaded: the two HIP runtimes must start together)

from common import golden_tables, jocn_modulations  # noqa: E402,F401
from failure_impact_child import (BAND, BASE, SEED, case_config, free_row, gn_running, oracle_records,  # noqa: E402,F401
                                  path_links_of, provision, replica_margin, ring_tables, search)
from optical_networking_gym import _native as nat  # noqa: E402

CASES = ("ring4", "nsfnet", "nobeleu", "alpha", "ids", "odd")
RATES = {"nobeleu": (10.0, 100.0, 400.0, 1000.0)}       # explicit rates over the case's 100 Gb/s table; the others: configured
NCOL = len(nat.ADMISSION_MAP)
# the load of a case where its own leaves more than a quarter of the scenarios without a blocked cell
LOAD = {"ring4": dict(load=40.0, replica_load=np.linspace(25.0, 70.0, 8))}


def case_cfg(key):
    """case_config of tests/failure_impact_child.py, with the load of LOAD"""
    tb, kw, B, steps, how = case_config(key)
    return tb, dict(kw, **LOAD.get(key, {})), B, steps, how


def drive(key, env=None, oracles=True):
    """(tables, kwargs, holder, oracles) of a case after its traffic, as failure_impact_child.drive drives it; `env`, a device
    environment of the same configuration, is driven in lock step"""
    from oracle_lib import OracleEnv
    tb, kw, B, steps, how = case_cfg(key)
    holder = nat.ConfigHolder(tb, batch=B, **kw)
    ors = [OracleEnv(holder, replica=r) for r in range(B)]
    runs = [steps // 2, steps - steps // 2] if how == "ids" else [steps]
    reqs = None
    if how == "trace":                  # bit rates beyond the configured table; one arrival rate per replica
        rng = np.random.default_rng(SEED)
        n = steps + 8
        reqs = np.zeros((B, n), nat.REQUEST_DTYPE)
        for r in range(B):
            reqs[r]["arrival_time"] = np.cumsum(rng.exponential(10800.0 / (kw["load"] * (0.6 + 0.1 * r)), n)).astype(np.float32)
            reqs[r]["holding_time"] = rng.exponential(10800.0, n).astype(np.float32)
            src = rng.integers(0, tb.n_nodes, n)
            reqs[r]["source"], reqs[r]["destination"] = src, (src + rng.integers(1, tb.n_nodes, n)) % tb.n_nodes
            reqs[r]["bit_rate"] = rng.choice(np.array([100, 400, 1000]), n)
    if env is not None:
        if reqs is not None:
            env.set_requests(reqs)
        else:
            env.seed(SEED)
        env.reset()
        for i, n in enumerate(runs):
            if i:
                env.reset_episode_counters()
            env.step_policy(n, record=False)
    if oracles:
        for r, o in enumerate(ors):
            if reqs is not None:
                o.set_trace(reqs[r])
            else:
                o.seed(SEED)
            o.reset()
            o.kept = np.zeros(0, nat.SERVICE_DTYPE)
            for i, n in enumerate(runs):
                if i:                   # the counters-only reset drops the departure heap: what runs now runs for good
                    o.kept = oracle_records(o)
                    o.kept["release_time"] = np.inf
                    o.reset_counters()
                o.run_first_fit(n)
    return tb, kw, holder, ors


# ---- the restatement ----------------------------------------------------------------------------------------------------
def pairs_of(N):
    return [(s, d) for s in range(N) for d in range(s + 1, N)]


def slot_counts(holder, rates):
    """[R][M] slots of every rate under every format, the header's formula; 0: unusable (n < 1 or n > S)"""
    c = holder.struct
    width = c.nslots_channel_width if c.nslots_channel_width > 0 else c.channel_width
    out = np.zeros((len(rates), c.n_mods), np.int64)
    for r, rate in enumerate(rates):
        for m, se in enumerate(holder.mod_se):
            n = int(np.ceil(float(np.float32(rate)) / (float(se) * width)))
            out[r, m] = n if 1 <= n <= c.n_slots else 0
    return out


def traffic_weights(holder):
    """[Q][R] by direct enumeration of the two-stage draw (_get_node_pair, qrmsa.pyx:1134-1148): the source by its node
    probability, the destination among the other nodes by theirs renormalised; then the rate"""
    N = holder.struct.n_nodes
    p = np.diff(holder._keep["node_cum"], prepend=0.0)
    p = p / p.sum()
    pr = np.diff(holder._keep["bit_rate_cum"], prepend=0.0)
    pr = pr / pr.sum()
    w = {pair: 0.0 for pair in pairs_of(N)}
    for s in range(N):
        rest = sum(p[d] for d in range(N) if d != s)
        for d in range(N):
            if d != s:
                w[(min(s, d), max(s, d))] += p[s] * p[d] / rest
    return np.array([[w[pair] * x for x in pr] for pair in pairs_of(N)])


def decode(tb, holder, nreq, req, action):
    """(status, path, slot, n, m) of a step action for the current request, as ongym_action_impact decodes it (the format
    window covers every format: max_modulation_idx = M - 1)"""
    c = holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    if action is None or req is None or action < 0 or action >= K * M * S:
        return 1, -1, 0, 0, 0
    slot, t = action % S, action // S
    m, route = M - 1 - t % M, t // M
    path = int(tb.pair_paths[int(req["source"]), int(req["destination"]), route])
    n = int(nreq[m])
    if path < 0 or n <= 0:
        return 2, -1, 0, 0, 0
    return 0, path, slot, n, m


def is_free(grid, tb, path, slot, n):
    """is_path_free (qrmsa.pyx:1248-1264): n slots and the guard slot, the guard waived iff the allocation ends at S"""
    S = grid.shape[1]
    row = free_row(grid, tb, path)
    return slot + n <= S and bool(np.all(row[slot:slot + n])) and (slot + n == S or bool(row[slot + n]))


def restate_map(o, tb, holder, margin, running, grid, nslots, rates, weights, log=None):
    """(summary row, map [Q][R], margins [Q][R], per cell the evaluated (path, start, n, gsnr)) of one state"""
    c = holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    se, thr = np.asarray(holder.mod_se), np.asarray(holder.mod_thr)
    pairs = pairs_of(c.n_nodes)
    Q, R = len(pairs), len(rates)
    amap, mar = np.zeros((Q, R), np.int32), np.full((Q, R), np.nan)
    evals = {}
    adm = ns = qt = det = 0
    bp = num = den = 0.0
    low = np.inf
    for q, (s, d) in enumerate(pairs):
        routes = []
        for k in range(K):
            p = int(tb.pair_paths[s, d, k])
            if p < 0:
                break
            routes.append((k, p))
        for r in range(R):
            seen = evals[(q, r)] = []

            def gn(p, a, n):
                g = gn_running(o, tb, se, running, p, a, n, skip_id=None)[0]
                seen.append((p, a, n, g))
                return g

            hit, evaluated = search(o, tb, thr, margin, nslots[r], routes, grid, gn, log)
            w = float(weights[q, r])
            wr = w * float(np.float32(rates[r]))
            den += wr
            if hit is None:
                amap[q, r] = K * M * S + (1 if evaluated else 0)
                qt += evaluated
                ns += not evaluated
                bp += w
                num += wr
                continue
            k, m, a, g = hit
            amap[q, r] = k * M * S + (M - 1 - m) * S + a
            mar[q, r] = g - thr[m] - margin
            adm += 1
            det += k > 0
            low = min(low, mar[q, r])
    row = np.array([0, adm, ns, qt, bp, num / den, low if adm else np.nan, det], np.float64)
    return row, amap, mar, evals


def restate_replica(o, tb, holder, margin, svcs, grid, req, actions, rates, weights, log=None):
    """(summary [A][8], map [A][Q][R], margins [A][Q][R], evaluations per scenario) of a replica's action list (None: the
    state as it is, A = 1).  req: the current request, or None"""
    c = holder.struct
    Q, R = len(pairs_of(c.n_nodes)), len(rates)
    nslots = slot_counts(holder, rates)
    recs = [(int(s["path_id"]), int(s["slot"]), int(s["nslots"]), int(s["modulation"]), int(s["service_id"])) for s in svcs]
    nreq = slot_counts(holder, [float(req["bit_rate"])])[0] if req is not None else None
    base = None
    rows, maps, mars, evs = [], [], [], []
    for action in ([None] if actions is None else [int(a) for a in actions]):
        status, path, slot, n, m = decode(tb, holder, nreq, req, action)
        if status == 0 and not is_free(grid, tb, path, slot, n):
            status = 2
        if status == 0 and len(recs) >= c.capacity:
            status = 3
        if status >= 2:
            rows.append(np.array([status] + [np.nan] * (NCOL - 1)))
            maps.append(np.full((Q, R), -1, np.int32))
            mars.append(np.full((Q, R), np.nan))
            evs.append({})
            continue
        if status == 1:
            if base is None:                    # every status-1 scenario of a replica is the same state: restated once
                base = restate_map(o, tb, holder, margin, recs, grid, nslots, rates, weights, log)
            row, amap, mar, ev = base
        else:
            g2 = grid.copy()
            provision(g2, tb, path, slot, n)
            sid = int(req["service_id"]) if "service_id" in (req.dtype.names or ()) else -1
            row, amap, mar, ev = restate_map(o, tb, holder, margin, recs + [(path, slot, n, m, sid)], g2, nslots, rates, weights, log)
        row = row.copy()
        row[0] = status
        rows.append(row)
        maps.append(amap)
        mars.append(mar)
        evs.append(ev)
    return np.stack(rows), np.stack(maps), np.stack(mars), evs


def action_list(o, tb, holder, grid, req, choice):
    """the five actions of a replica: first fit's choice, the reject action, -1, an action whose slots are occupied, and a valid
    action on the last route at the lowest usable format"""
    c = holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    reject = K * M * S
    nreq = slot_counts(holder, [float(req["bit_rate"])])[0]
    routes = [int(p) for p in tb.pair_paths[int(req["source"]), int(req["destination"])] if p >= 0]
    usable = [m for m in range(M) if nreq[m] > 0]
    occupied = valid = reject
    for k, p in enumerate(routes):
        busy = np.flatnonzero(free_row(grid, tb, p) == 0)
        if len(busy) and usable:
            occupied = k * M * S + (M - 1 - usable[-1]) * S + int(busy[0])
            break
    for k in range(len(routes) - 1, -1, -1):
        for m in usable:
            starts = o.candidates(free_row(grid, tb, routes[k]), int(nreq[m]))
            if starts:
                valid = k * M * S + (M - 1 - m) * S + int(starts[-1])
                break
        if valid != reject:
            break
    return np.array([int(choice), reject, -1, occupied, valid], np.int32)


def conditions(holder, rows, maps, evs):
    """what a replica's restated scenarios exercise (the tests assert the sums over the cases)"""
    c = holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    thr = np.asarray(holder.mod_thr)
    reject = K * M * S
    out = dict(scenarios=0, none_blocked=0, ns=0, qot=0, detoured=0, below_top=0, changed=0, newly_blocked=0, qot_alone=0)
    for s in range(4):
        out[f"status{s}"] = int(np.sum(rows[:, 0] == s))
    ok = rows[:, 0] < 2
    out["scenarios"] = int(ok.sum())
    out["none_blocked"] = int(np.sum(rows[ok, 2] + rows[ok, 3] == 0))
    out["ns"], out["qot"], out["detoured"] = (int(np.sum(rows[ok, i])) for i in (2, 3, 7))
    for a in np.flatnonzero(ok):
        adm = maps[a][maps[a] < reject]
        out["below_top"] += int(np.sum((adm // S) % M > 0))
    base = np.flatnonzero(rows[:, 0] == 1)
    if len(base):
        b = int(base[0])
        for a in np.flatnonzero(rows[:, 0] == 0):
            diff = maps[a] != maps[b]
            out["changed"] += int(diff.sum())
            out["newly_blocked"] += int(np.sum(diff & (maps[a] >= reject) & (maps[b] < reject)))
            for q, r in zip(*np.nonzero(diff)):                 # the baseline's placement evaluated again at the same start and refused
                if maps[b][q, r] >= reject:
                    continue
                won = evs[b][(q, r)][-1]
                m = M - 1 - (int(maps[b][q, r]) // S) % M
                out["qot_alone"] += any(e[:3] == won[:3] and e[3] < thr[m] + evs[b]["margin"] <= won[3] for e in evs[a][(q, r)])
    return out


# ---- one case on any source of states -----------------------------------------------------------------------------------
def case_rates(key, holder):
    return tuple(RATES.get(key, tuple(float(x) for x in holder.bit_rates)))


def case_weights(key, holder, rates):
    """the traffic weights with the configured rates; with explicit rates a fixed non-uniform array"""
    if key not in RATES:
        return traffic_weights(holder)
    Q = len(pairs_of(holder.struct.n_nodes))
    w = 1.0 + (np.arange(Q * len(rates)).reshape(Q, len(rates)) % 7)
    return w / w.sum()


def restate_case(key, tb, kw, holder, ors, state_of, choice_of):
    """per replica: the action list, the restated rows of the NULL call and of the list, the conditions and the band count.
    state_of(r) -> (records, grid, request); choice_of(r) -> first fit's action"""
    rates = case_rates(key, holder)
    weights = case_weights(key, holder, rates)
    reps, log = [], []
    for r, o in enumerate(ors):
        svcs, grid, req = state_of(r)
        margin = replica_margin(kw, r)
        acts = action_list(o, tb, holder, grid, req, choice_of(r))
        null = restate_replica(o, tb, holder, margin, svcs, grid, req, None, rates, weights, log)
        lst = restate_replica(o, tb, holder, margin, svcs, grid, req, acts, rates, weights, log)
        for ev in lst[3]:
            ev["margin"] = margin
        reps.append(dict(actions=acts, null=null, list=lst, cond=conditions(holder, lst[0], lst[1], lst[3]), active=len(svcs)))
    return rates, weights, reps, int(np.sum(np.array(log) < BAND)), len(log)


FULL_B = 2


def full_table():
    """ring4 with C = 64 filled to 64 records: a trace of 10 Gb/s requests between neighbours that never leave, 20 on each of
    two links (which are full then: every cell of the pair between them is blocked), 12 on each of the other two"""
    tb = ring_tables()
    kw = dict(BASE, num_spectrum_resources=40, capacity=64, load=10.0)
    n = 72
    reqs = np.zeros((FULL_B, n), nat.REQUEST_DTYPE)
    for r in range(FULL_B):
        reqs[r]["arrival_time"] = np.arange(1, n + 1, dtype=np.float32)
        reqs[r]["holding_time"] = 1e9
        src = (np.repeat(np.arange(4), (20, 20, 12, 12))[np.minimum(np.arange(n), 63)] + r) % 4   # the current request: a 12-record link
        reqs[r]["source"], reqs[r]["destination"] = src, (src + 1) % 4
        reqs[r]["bit_rate"] = 10
    return tb, kw, reqs


def drive_full(env=None, oracles=True):
    from oracle_lib import OracleEnv
    tb, kw, reqs = full_table()
    holder = nat.ConfigHolder(tb, batch=FULL_B, **kw)
    ors = [OracleEnv(holder, replica=r) for r in range(FULL_B)]
    if env is not None:
        env.set_requests(reqs)
        env.reset()
        env.step_policy(64, record=False)
    if oracles:
        for r, o in enumerate(ors):
            o.set_trace(reqs[r])
            o.reset()
            o.run_first_fit(64)
    return tb, kw, holder, ors


# ---- the GPU computations -----------------------------------------------------------------------------------------------
def store(out, key, rates, weights, reps, band, evaluated, got_null, got_list):
    tot = {}
    for r, rep in enumerate(reps):
        k = f"{key}_r{r}"
        out[k + "_actions"] = rep["actions"]
        for name, want, got in (("null", rep["null"], got_null), ("list", rep["list"], got_list)):
            out[f"{k}_{name}_want"], out[f"{k}_{name}_wmap"], out[f"{k}_{name}_wmar"] = want[:3]
            out[f"{k}_{name}_got"], out[f"{k}_{name}_gmap"], out[f"{k}_{name}_gmar"] = got[0][r], got[1][r], got[2][r]
        for name, v in rep["cond"].items():
            tot[name] = tot.get(name, 0) + int(v)
    for name, v in tot.items():
        out[f"{key}_cond_{name}"] = v
    out[key + "_B"], out[key + "_band"], out[key + "_evaluated"] = len(reps), band, evaluated
    out[key + "_rates"], out[key + "_weights"] = np.array(rates), weights


def gpu_case(out, key):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb, kw, B, _, how = case_cfg(key)
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    tb, kw, holder, ors = drive(key, env, oracles=False)      # the oracles only lend `candidates` and `gn_lists`
    choice = env.policy_actions()[0]
    rates, weights, reps, band, evaluated = restate_case(
        key, tb, kw, holder, ors, lambda r: (env.services(r), env.grid(r), env.request(r)), lambda r: choice[r])
    explicit = key in RATES
    args = dict(rates=rates, weights=weights) if explicit else dict(weights="traffic")
    acts = np.stack([rep["actions"] for rep in reps])
    got_null = env.admission_map(detail=True, **args)
    got_list = env.admission_map(acts, detail=True, **args)
    again = env.admission_map(acts, detail=True, **args)
    out[key + "_same_bytes"] = all(a.tobytes() == b.tobytes() for a, b in zip(got_list, again))
    out[key + "_same_without_detail"] = np.array_equal(env.admission_map(acts, **args), got_list[0], equal_nan=True)
    if not explicit:                                           # "traffic" is admission_weights() passed as an array; uniform ones
        out[key + "_traffic_same"] = np.array_equal(env.admission_map(acts, weights=env.admission_weights()), got_list[0], equal_nan=True)
        uni = env.admission_map(acts, weights=None)
        cells = weights.size
        out[key + "_uniform_err"] = float(np.nanmax(np.abs(uni[:, :, 4] - (uni[:, :, 2] + uni[:, :, 3]) / cells)))
    if key in ("nsfnet", "nobeleu"):                           # one wavefront per scenario, and three groups of pairs: the same answer
        same, err = True, 0.0
        for g in ("1", "3"):                                   # the knob is read at create: a twin environment, driven alike
            os.environ["ONGYM_ADMISSION_GROUPS"] = g
            try:
                twin = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
            finally:
                del os.environ["ONGYM_ADMISSION_GROUPS"]
            drive(key, twin, oracles=False)
            alt = twin.admission_map(acts, detail=True, **args)
            twin.close()
            same &= bool(np.array_equal(alt[0][:, :, [0, 1, 2, 3, 7]], got_list[0][:, :, [0, 1, 2, 3, 7]], equal_nan=True)
                         and np.array_equal(alt[1], got_list[1]) and np.array_equal(alt[2], got_list[2], equal_nan=True)
                         and np.array_equal(alt[0][:, :, 6], got_list[0][:, :, 6], equal_nan=True))
            err = max(err, float(np.nanmax(np.abs(alt[0][:, :, 4:6] - got_list[0][:, :, 4:6]))))
        out[key + "_groups_same"], out[key + "_groups_err"] = same, err
    store(out, key, rates, weights, reps, band, evaluated, got_null, got_list)
    out[key + "_uniform"] = bool(np.all(tb.link_alpha == tb.link_alpha[0]))
    out[key + "_rec32"] = bool(tb.n_links <= 32 and len(tb.path_hops) <= 512)
    if key == "nsfnet":
        witness(out, env, holder, rates, got_null[1][:, 0])
    env.close()


def witness(out, env, holder, rates, amap):
    """32 (replica, cell) samples through the step itself: the replica forked, the cell installed as its next request, the
    current one rejected, then first fit's own decision.  Blocked cells among them"""
    c = holder.struct
    B, reject = env.batch_size, c.k_paths * c.n_mods * c.n_slots
    pairs = pairs_of(c.n_nodes)
    rng = np.random.default_rng(SEED)
    blob = env.save_state()
    want, got, blocked = [], [], 0
    for rnd in range(2):
        src = np.roll(np.arange(B), rnd + 1).astype(np.int32)           # replica j takes the state of replica src[j]
        cells = []
        for j in range(B):
            flat = np.flatnonzero(amap[src[j]] >= reject) if (j + rnd) % 2 else np.arange(amap[src[j]].size)
            if not len(flat):
                flat = np.arange(amap[src[j]].size)
            cells.append(np.unravel_index(int(rng.choice(flat)), amap[src[j]].shape))
        env.fork(src)
        reqs = np.zeros((B, 4), nat.REQUEST_DTYPE)
        for j, (q, r) in enumerate(cells):
            s, d = pairs[q] if j % 2 else pairs[q][::-1]                # both directions of a pair
            reqs[j]["source"], reqs[j]["destination"], reqs[j]["bit_rate"] = s, d, rates[r]
            reqs[j]["holding_time"] = 1.0                               # arrival_time 0: no running service has left by then
        env.set_requests(reqs)
        env.step(np.full(B, reject, np.int32))
        a = env.policy_actions()[0]
        for j, (q, r) in enumerate(cells):
            want.append(min(int(amap[src[j], q, r]), reject))
            got.append(int(a[j]))
            blocked += int(amap[src[j], q, r]) >= reject
        env.load_state(blob)
    out["witness_want"], out["witness_got"], out["witness_blocked"] = np.array(want), np.array(got), blocked


def gpu_full(out):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb, kw, _ = full_table()
    env = BatchedQRMSAEnv(tables=tb, batch_size=FULL_B, **kw)
    tb, kw, holder, ors = drive_full(env, oracles=False)
    choice = env.policy_actions()[0]
    out["full_active"] = env.stats()["active"]
    rates, weights, reps, band, evaluated = restate_case(
        "full", tb, kw, holder, ors, lambda r: (env.services(r), env.grid(r), env.request(r)), lambda r: choice[r])
    acts = np.stack([rep["actions"] for rep in reps])
    store(out, "full", rates, weights, reps, band, evaluated, env.admission_map(detail=True), env.admission_map(acts, detail=True))
    env.close()


def read_only(out, B=32):
    from common import record_bytes
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    kw = dict(BASE, num_spectrum_resources=128, capacity=192, load=120.0, measure_disruptions=True)
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    twin = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    for e in (env, twin):
        e.seed(4)
        e.reset()
        e.step_policy(200, record=False)
    blob0, st0 = env.save_state(), env.stats()
    a = env.admission_map()
    acts = np.stack([env.policy_actions()[0], np.full(B, -1, np.int32)], axis=1).astype(np.int32)
    b = env.admission_map(acts, detail=True)
    blob1, st1 = env.save_state(), env.stats()
    out["ro_blob_same"] = blob0.tobytes() == blob1.tobytes()
    out["ro_stats_same"] = st0.tobytes() == st1.tobytes()
    out["ro_traj_same"] = record_bytes(env.step_policy(60)) == record_bytes(twin.step_policy(60))
    out["ro_cells"] = int(np.sum(a[:, :, 1:4]))
    out["ro_baseline_same"] = bool(np.array_equal(b[0][:, 1, 1:], a[:, 0, 1:], equal_nan=True))
    out["ro_applied"] = int(np.sum(b[0][:, 0, 0] == 0))
    env.close()
    twin.close()


def fresh(out, B=8):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **dict(BASE, num_spectrum_resources=128, capacity=128, load=100.0))
    env.seed(3)
    env.reset()
    out["fresh_rows"], out["fresh_map"], out["fresh_margin"] = env.admission_map(detail=True)
    out["fresh_usable"] = np.any(slot_counts(env.holder, env.holder.bit_rates) > 0, axis=1)
    rates = (10.0, 5000.0, 1e6)                                 # the last has no usable format at S = 128
    out["fresh_rows_x"], out["fresh_map_x"], _ = env.admission_map(rates=rates, weights=None, detail=True)
    out["fresh_usable_x"] = np.any(slot_counts(env.holder, rates) > 0, axis=1)
    c = env.holder.struct
    out["fresh_kms"] = np.array([c.k_paths, c.n_mods, c.n_slots])
    env.close()


def device_io(out, B=32):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    kw = dict(BASE, num_spectrum_resources=128, capacity=192, load=120.0)
    host = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    dev = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, io_device=True, **kw)
    c = host.holder.struct
    Q, R = len(pairs_of(c.n_nodes)), c.n_bit_rates
    t = torch.full((B, 1, NCOL), 7.0, dtype=torch.float64, device="cuda")
    try:
        dev.admission_map(out=t)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    host.seed(5)
    host.reset()
    host.step_policy(220, record=False)
    acts = np.stack([host.policy_actions()[0], np.full(B, -1, np.int32), np.zeros(B, np.int32)], axis=1).astype(np.int32)
    want = host.admission_map()
    want_l = host.admission_map(acts, detail=True)
    want_x = host.admission_map(acts, rates=(40.0, 250.0), weights=None)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        dev.seed(5)
        dev.reset()
        dev.step_policy(220, record=False)
        r = dev.admission_map(out=t)
        t2 = torch.full((B, 3, NCOL), 7.0, dtype=torch.float64, device="cuda")
        m2 = torch.full((B, 3, Q, R), 7, dtype=torch.int32, device="cuda")
        g2 = torch.full((B, 3, Q, R), 7.0, dtype=torch.float32, device="cuda")
        acts_t = torch.from_numpy(acts).cuda()
        dev.admission_map(acts_t, out=(t2, m2, g2), detail=True)
        t3 = torch.full((B, 3, NCOL), 7.0, dtype=torch.float64, device="cuda")
        dev.admission_map(acts_t, rates=(40.0, 250.0), weights=None, out=t3)
        stream.synchronize()
        out["dev_same"] = r is t and np.array_equal(t.cpu().numpy(), want, equal_nan=True)
        out["dev_detail_same"] = (np.array_equal(t2.cpu().numpy(), want_l[0], equal_nan=True) and np.array_equal(m2.cpu().numpy(), want_l[1])
                                  and np.array_equal(g2.cpu().numpy(), want_l[2], equal_nan=True))
        out["dev_rates_same"] = np.array_equal(t3.cpu().numpy(), want_x, equal_nan=True)
        bad = []
        for args, kws in (((acts_t.long(),), dict(out=t2)), ((torch.from_numpy(acts),), dict(out=t2)), ((acts,), dict(out=t2)),
                          ((acts_t,), dict(out=t)), ((acts_t,), dict(out=t2, detail=True)),
                          ((acts_t,), dict(out=(t2, m2.long(), g2), detail=True)),
                          ((acts_t,), dict(out=t2, weights=torch.ones((Q, R), dtype=torch.float64)))):
            try:
                dev.admission_map(*args, **kws)
                bad.append(False)
            except ValueError:
                bad.append(True)
        out["dev_refusals"] = np.array(bad)
        dev.set_stream(None)
    host.close()
    dev.close()


def compat(out):
    from optical_networking_gym.envs.block_vec_env import QRMSABlockVecEnv
    from optical_networking_gym.envs.qrmsa import QRMSAEnv
    from optical_networking_gym.topology import bundled_topology_path, get_topology
    topology = get_topology(bundled_topology_path("nsfnet_chen.txt"), None, jocn_modulations(), 80, 0.2, 4.5, 5)
    single = QRMSAEnv(topology=topology, seed=9, load=400, episode_length=1000, num_spectrum_resources=112, bandwidth=112 * 12.5e9, launch_power_dbm=2.0,
                      margin=0.5, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), gen_observation=False)
    single.reset()
    for _ in range(200):
        single.step(single.first_fit_action()[0])
    c = single._dev.holder.struct
    reject = c.k_paths * c.n_mods * c.n_slots
    same, blocked = True, 0
    for action in (None, single.first_fit_action()[0], reject, 0):
        d = single.admission_map(action)
        acts = None if action is None else np.array([[action]], np.int32)
        row, amap, _ = single._dev.admission_map(acts, detail=True)
        same &= list(d)[:NCOL] == list(nat.ADMISSION_MAP) and set(d) == set(nat.ADMISSION_MAP) | {"blocked"}
        same &= all((np.isnan(row[0, 0, i]) and np.isnan(d[k])) or float(d[k]) == row[0, 0, i] for i, k in enumerate(nat.ADMISSION_MAP))
        if d["status"] < 2:
            same &= isinstance(d["admitted"], int) and len(d["blocked"]) == d["blocked_no_spectrum"] + d["blocked_qot"]
            same &= sum(b[3] == "qot" for b in d["blocked"]) == d["blocked_qot"]
            same &= all(b[0] in topology.nodes and b[1] in topology.nodes and b[2] in (10, 40, 100, 400) for b in d["blocked"])
            blocked += len(d["blocked"])
        else:
            same &= d["blocked"] == []
    out["compat_same"], out["compat_blocked"] = bool(same), blocked
    single.close()
    vec = QRMSABlockVecEnv(tables=golden_tables("nsfnet"), num_envs=8, blocks_to_consider=4, seed=2,
                           **dict(BASE, num_spectrum_resources=112, capacity=128, load=150.0, launch_power_dbm=1.0))
    vec.reset()
    for _ in range(120):
        vec.step(np.argmax(vec.action_masks(), axis=1))
    la = vec.action_lookahead()
    ref = vec.env.admission_map(np.ascontiguousarray(vec._map, np.int32))[:, :, 4]
    mask = vec.action_masks()
    out["look_shape_ok"] = la.shape == (8, vec.n_actions) and la.dtype == np.float64
    out["look_same"] = bool(np.array_equal(la[mask], ref[mask]) and np.all(np.isnan(la[~mask])) and not np.any(np.isnan(la[mask])))
    out["look_reject_is_baseline"] = bool(np.array_equal(la[:, -1], vec.env.admission_map()[:, 0, 4]))
    out["look_spread"] = float(np.nanmax(la) - np.nanmin(la))
    vec.close()


def refusals(out):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, **dict(BASE, num_spectrum_resources=128, capacity=128, load=100.0))
    env.seed(1)
    env.reset()
    f, h = env.lib.ongym_admission_map, env._h
    acts, res = np.zeros((4, 257), np.int32), np.zeros((4, 257, NCOL))
    rates = lambda *x: np.array(x, np.float32).ctypes.data      # noqa: E731
    rc = {}
    rc["zero_actions"] = f(h, 0, acts.ctypes.data, 4, None, None, res.ctypes.data, None, None)
    out["refuse_actions_msg"] = env.lib.ongym_last_error(h).decode()
    rc["many_actions"] = f(h, 257, acts.ctypes.data, 4, None, None, res.ctypes.data, None, None)
    rc["null_actions"] = f(h, 2, None, 4, None, None, res.ctypes.data, None, None)
    rc["null_summary"] = f(h, 1, None, 4, None, None, None, None, None)
    rc["zero_rates"] = f(h, 1, None, 0, rates(10.0), None, res.ctypes.data, None, None)
    rc["many_rates"] = f(h, 1, None, 17, np.ones(17, np.float32).ctypes.data, None, res.ctypes.data, None, None)
    rc["null_rates_other_count"] = f(h, 1, None, 3, None, None, res.ctypes.data, None, None)
    rc["nan_rate"] = f(h, 1, None, 2, rates(10.0, np.nan), None, res.ctypes.data, None, None)
    rc["inf_rate"] = f(h, 1, None, 2, rates(10.0, np.inf), None, res.ctypes.data, None, None)
    rc["negative_rate"] = f(h, 1, None, 2, rates(10.0, -1.0), None, res.ctypes.data, None, None)
    out["refuse_rate_msg"] = env.lib.ongym_last_error(h).decode()
    rc["ok"] = f(h, 1, None, 4, None, None, res.ctypes.data, None, None)
    env.close()
    kw = dict(BASE, num_spectrum_resources=128, capacity=128, load=100.0)
    narrow = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, modulations_to_consider=3, **kw)
    rc["window"] = narrow.lib.ongym_admission_map(narrow._h, 1, None, 4, None, None, res.ctypes.data, None, None)
    out["refuse_window_msg"] = narrow.lib.ongym_last_error(narrow._h).decode()
    narrow.close()
    cont = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, **dict(kw, bit_rate_selection="continuous"))
    rc["continuous_null_rates"] = cont.lib.ongym_admission_map(cont._h, 1, None, 1, None, None, res.ctypes.data, None, None)
    cont.close()
    from dataclasses import replace
    tb = golden_tables("nsfnet")
    pp = tb.pair_paths.copy()
    pp[3, 1, :2] = pp[3, 1, :2][::-1].copy()                    # one direction of pair (1, 3) lists its routes in another order
    skew = BatchedQRMSAEnv(tables=replace(tb, pair_paths=pp), batch_size=4, **kw)
    rc["asymmetric"] = skew.lib.ongym_admission_map(skew._h, 1, None, 4, None, None, res.ctypes.data, None, None)
    out["refuse_asymmetric_msg"] = skew.lib.ongym_last_error(skew._h).decode()
    skew.close()
    for k, v in rc.items():
        out["refuse_rc_" + k] = v


def main():
    out = {}
    refusals(out)
    fresh(out)
    read_only(out)
    device_io(out)
    compat(out)
    gpu_full(out)
    for key in CASES:
        gpu_case(out, key)
        print(key, "done", flush=True)
    np.savez(sys.argv[1], **out)
    print("admission map child ok")


if __name__ == "__main__":
    main()
