"""Child process of tests/test_gpu_failure_impact.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP
runtime and this library's must start together), saved to an .npz that the tests assert on.

    python tests/failure_impact_child.py OUT.npz

It also holds the restatement of ongym_failure_impact (include/ongym.h) in plain numpy, which shares nothing with the device
code: a scenario is restated from a replica's running records and slot grid alone (the device's services() and grid() on the
GPU, an oracle's on the CPU), the valid starts come from the oracle's `candidates` (_get_candidates) and every GN value from
the oracle's literal GN on explicit per-link interferer lists (`gn_lists`): the survivors in record order, then the victims
restored so far in the order of their restoration.  tests/test_failure_impact_host.py pins `search` to the oracle's own
first-fit decision.
"""
import copy
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402,F401  (before the library is loaded: the two HIP runtimes must start together)

from common import golden_tables, jocn_modulations  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402

BAND = 1e-8          # relative distance of 1/GSNR to its limit inside which a decision could differ: no evaluation may lie there
SEED = 23
BASE = dict(modulations=jocn_modulations(), bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), auto_reset=True,
            episode_length=10 ** 6, margin=0.0, launch_power_dbm=0.0)


def case_config(key):
    """(tables, keyword arguments with one value of load, launch power or margin per replica, batch, steps, how)"""
    B, steps, how = 8, 250, "ff"
    if key == "ring4":          # two routes per pair, one of them through any failed link: exactly one eligible route
        tb = ring_tables()
        kw = dict(BASE, num_spectrum_resources=40, capacity=64, load=18.0, replica_load=np.linspace(8.0, 30.0, B))
        steps = 150
    elif key == "nsfnet":       # R32 codec, uniform attenuation
        B = 16
        tb = golden_tables("nsfnet")
        kw = dict(BASE, num_spectrum_resources=112, capacity=128, load=110.0, replica_load=np.linspace(60.0, 150.0, B),
                  replica_launch_power_dbm=np.linspace(-1.0, 4.0, B))
    elif key == "nobeleu":      # generic codec, link masks beyond 32 bits; a trace with 400 Gb/s and 1 Tb/s requests over a
        tb = golden_tables("nobel-eu")   # 100 Gb/s table: restorations (and records) wider than the pair table's 8 slots
        kw = dict(BASE, num_spectrum_resources=160, capacity=192, bit_rates=(10, 40, 100), load=60.0,
                  replica_margin=np.linspace(0.0, 3.0, B))
        steps, how = 200, "trace"
    elif key == "alpha":        # per-link attenuation: the non-uniform template path
        tb = copy.deepcopy(golden_tables("nsfnet"))
        tb.link_alpha = tb.link_alpha * np.linspace(0.85, 1.2, tb.n_links)
        kw = dict(BASE, num_spectrum_resources=96, capacity=128, load=90.0, replica_load=np.linspace(50.0, 120.0, B),
                  replica_margin=np.linspace(0.0, 1.5, B))
    elif key == "ids":          # service ids with a counters-only reset in the middle: running namesakes (quirk Q12)
        tb = golden_tables("nsfnet")
        kw = dict(BASE, num_spectrum_resources=128, capacity=128, load=100.0, replica_load=np.linspace(60.0, 130.0, B),
                  track_service_ids=True)
        how = "ids"
    elif key == "odd":          # S no multiple of 64, services that end at S: no guard slot at the row's end
        tb = golden_tables("nsfnet")
        kw = dict(BASE, num_spectrum_resources=100, capacity=128, load=140.0, replica_load=np.linspace(100.0, 180.0, B),
                  replica_launch_power_dbm=np.linspace(0.0, 3.0, B))
    else:
        raise KeyError(key)
    return tb, kw, B, steps, how


def ring_tables():
    """A ring of four nodes with both routes of every node pair.  The bundled ring_4 is a line (its file loses the first edge,
    optical_networking_gym/topology.py), where a cut leaves no route at all: the golden tables' three links, closed by a fourth
    of the same fibre"""
    from dataclasses import replace
    t = golden_tables("ring4")
    ends = [tuple(sorted(x)) for x in t.link_nodes.tolist()] + [(0, 1)]
    link = {e: i for i, e in enumerate(ends)}
    assert len(link) == 4 and all(((a + 1) % 4 == b or (b + 1) % 4 == a) for a, b in ends)
    pair_paths = np.full((4, 4, 2), -1, np.int32)
    hops, links, nodes = [], [], []
    for a in range(4):
        for b in range(a + 1, 4):
            ways = []
            for step in (1, -1):
                seq = [a]
                while seq[-1] != b:
                    seq.append((seq[-1] + step) % 4)
                ways.append(seq)
            for k, seq in enumerate(sorted(ways, key=len)):
                pair_paths[a, b, k] = pair_paths[b, a, k] = len(hops)
                hops.append(len(seq) - 1)
                links.append([link[tuple(sorted(x))] for x in zip(seq, seq[1:])])
                nodes.append(tuple(seq))
    path_links = np.full((len(hops), 3), -1, np.int32)
    for p, l in enumerate(links):
        path_links[p, :len(l)] = l
    rep = lambda x: np.concatenate([x, x[:1]])      # noqa: E731
    return replace(t, n_links=4, n_paths=len(hops), k_paths=2, max_hops=3, pair_paths=pair_paths,
                   path_hops=np.array(hops, np.int32), path_links=path_links,
                   path_length=np.array([h * float(t.link_length[0]) for h in hops]), path_nodes=nodes,
                   link_nodes=np.array(ends, np.int32), link_length=rep(t.link_length), link_nspans=rep(t.link_nspans),
                   link_span_km=rep(t.link_span_km), link_alpha=rep(t.link_alpha), link_nf=rep(t.link_nf))


CASES = ("ring4", "nsfnet", "nobeleu", "alpha", "ids", "odd")


def replica_margin(kw, r):
    return float(kw["replica_margin"][r]) if kw.get("replica_margin") is not None else float(kw["margin"])


def explicit_links(E, B):
    """the explicit list of the cases, F = E entries per replica: E - 3 different links (rotated by the replica), the first of
    them once more, a -1 and an index >= E"""
    return np.stack([np.concatenate([np.roll(np.arange(E), -r)[:E - 3], [r % E, -1, E + 7]]) for r in range(B)]).astype(np.int32)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def path_links_of(tb, path):
    return tb.path_links[path, :tb.path_hops[path]]


def route_of(tb):
    """path -> (pair index, k): the pair with the lowest src * n_nodes + dst whose list holds the path"""
    N, K = tb.n_nodes, tb.pair_paths.shape[2]
    out = {}
    for s in range(N):
        for d in range(N):
            for k in range(K):
                p = int(tb.pair_paths[s, d, k])
                if p >= 0 and p not in out:
                    out[p] = (s, d, k)
    return out


def free_row(grid, tb, path):
    return np.all(grid[path_links_of(tb, path)] != 0, axis=0).astype(np.int32)


def gn_running(o, tb, se, running, path, slot, n, skip_id=None):
    """GSNR, ASE, NLI (dB) of (path, slot, n) against `running`, a list of (path, slot, n, modulation, id) in list order; records
    with id == skip_id are no interferers"""
    counts, intf = [], []
    on = [set(path_links_of(tb, r[0]).tolist()) for r in running]
    for l in path_links_of(tb, path):
        z = [(r[1], r[2], se[r[3]]) for r, links in zip(running, on)
             if l in links and not (skip_id is not None and r[4] == skip_id)]
        counts.append(len(z))
        intf += z
    return o.gn_lists(int(path), int(slot), int(n), np.array(counts, np.int32), np.array(intf, np.int16).reshape(-1, 3))


def search(o, tb, thr, margin, nslots, routes, grid, gn, log=None):
    """first fit's search (heuristics.py:923-966): `routes` is the list of (k, path) to try in order, nslots[m] the slot count
    under format m (<= 0 or > S: unusable), gn(path, start, n) the GSNR in dB.  Returns ((k, m, start, gsnr) or None, whether
    any start was evaluated); log collects the relative distance to the limit of every evaluation"""
    S = grid.shape[1]
    evaluated = False
    for k, path in routes:
        row = free_row(grid, tb, path)
        for m in range(len(nslots) - 1, -1, -1):
            n = int(nslots[m])
            if n <= 0 or n > S:
                continue
            starts = o.candidates(row, n)
            if not starts:
                continue
            g = gn(path, starts[0], n)
            evaluated = True
            if log is not None:
                log.append(abs(10.0 ** ((thr[m] + margin - g) / 10.0) - 1.0))
            if g >= thr[m] + margin:
                return (k, m, starts[0], g), evaluated
    return None, evaluated


def release(grid, tb, path, slot, n):
    """_release_path (qrmsa.pyx:1332-1350): n + 1 slots, clamped at S"""
    grid[path_links_of(tb, path), slot:min(slot + n + 1, grid.shape[1])] = 1


def provision(grid, tb, path, slot, n):
    """_provision_path (qrmsa.pyx:1292-1296): n slots plus the guard slot unless the allocation ends at S"""
    end = slot + n
    grid[path_links_of(tb, path), slot:(end + 1 if end < grid.shape[1] else end)] = 0


def fail_link(tb, svcs, grid, link):
    """steps 1 and 2: (records, victim indices, the survivors, the grid with every victim released)"""
    recs = [(int(s["path_id"]), int(s["slot"]), int(s["nslots"]), int(s["modulation"]), int(s["service_id"])) for s in svcs]
    victims = [i for i, r in enumerate(recs) if link in path_links_of(tb, r[0])]
    running = [r for i, r in enumerate(recs) if i not in set(victims)]
    grid = grid.copy()
    for i in victims:
        release(grid, tb, *recs[i][:3])
    return recs, victims, running, grid


def restate_scenario(o, tb, holder, margin, svcs, grid, link, ids=False, sequential=True, log=None):
    """(link_out row, svc_out row of len(svcs), (restorations wider than the pair table, evaluations that had such a restored
    record among their interferers)) of one failed link on the state (svcs in record order, grid)"""
    c = holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    se, thr = np.asarray(holder.mod_se), np.asarray(holder.mod_thr)
    row, act = np.full(len(nat.FAILURE_IMPACT), np.nan), np.full(len(svcs), -1, np.int32)
    if link < 0 or link >= tb.n_links:
        row[0] = 1
        return row, act, (0, 0)
    routes = route_of(tb)
    recs, victims, running, grid = fail_link(tb, svcs, grid, link)
    base_grid, base_running, survivors = grid, running, len(running)
    row[:9] = 0
    low, wide, wide_seen, nmax = np.inf, 0, 0, tab_nmax(holder)
    for i in victims:
        path, _, n, m, sid = recs[i]
        if not sequential:
            grid, running = base_grid.copy(), list(base_running)
        cap = n * int(se[m])
        nslots = [-(-cap // int(s)) for s in se]
        row[1] += 1
        row[2] += cap
        eligible = []
        if path in routes:
            s, d, _ = routes[path]
            for k in range(K):
                p = int(tb.pair_paths[s, d, k])
                if p < 0:
                    break
                if link not in path_links_of(tb, p):
                    eligible.append((k, p))
        def gn(p, a, nn):
            nonlocal wide_seen
            mine = set(path_links_of(tb, p).tolist())       # a restored record beyond the pair table among the interferers
            wide_seen += any(r[2] > nmax and not (ids and r[4] == sid) and mine & set(path_links_of(tb, r[0]).tolist())
                             for r in running[survivors:])
            return gn_running(o, tb, se, running, p, a, nn, sid if ids else None)[0]

        hit, evaluated = search(o, tb, thr, margin, nslots, eligible, grid, gn, log)
        if hit is None:
            row[6 if evaluated else 5] += 1
            act[i] = K * M * S
            continue
        k, mm, a, g = hit
        p, nn = dict(eligible)[k], nslots[mm]
        provision(grid, tb, p, a, nn)
        running.append((p, a, nn, mm, sid))
        act[i] = k * M * S + (M - 1 - mm) * S + a
        row[3] += 1
        row[4] += cap
        row[7] += int(tb.path_hops[p]) - int(tb.path_hops[path])
        row[8] += nn * int(tb.path_hops[p]) - n * int(tb.path_hops[path])
        low = min(low, g - thr[mm] - margin)
        wide += nn > nmax
    row[9] = low if row[3] else np.nan
    return row, act, (wide, wide_seen)


def tab_nmax(holder):
    """rows of the device's pair table: the widest slot count of the configured traffic table, ceil(max bit rate / (lowest
    spectral efficiency x the slot-count width)) clamped to [1, S].  This is P.tab_nmax as build() computes it
    (csrc/ongym_hip.hip, "int nmax = ..."): keep the two together.  Interferers beyond it take gn_eval's asinh path"""
    c = holder.struct
    width = c.nslots_channel_width if c.nslots_channel_width > 0 else c.channel_width
    return max(1, min(int(np.ceil(max(holder.bit_rates) / (min(holder.mod_se) * width))), c.n_slots))


def restate_replica(o, tb, holder, margin, svcs, grid, links, ids=False, sequential=True, log=None):
    out = [restate_scenario(o, tb, holder, margin, svcs, grid, int(l), ids, sequential, log) for l in links]
    return np.stack([r for r, _, _ in out]), np.stack([a for _, a, _ in out]), tuple(sum(w[i] for _, _, w in out) for i in (0, 1))


def conditions(tb, holder, svcs, want, act, indep_act):
    """what a replica's restated scenarios exercise (tests/test_gpu_failure_impact.py asserts one of each across the cases)"""
    c = holder.struct
    M, S, K = c.n_mods, c.n_slots, c.k_paths
    se = np.asarray(holder.mod_se)
    down = route2 = ends_at_S = 0
    for f in range(len(act)):
        for i in np.flatnonzero((act[f] >= 0) & (act[f] < K * M * S)):
            a = int(act[f, i])
            mm, k, start = M - 1 - (a // S) % M, a // (M * S), a % S
            n, m = int(svcs["nslots"][i]), int(svcs["modulation"][i])
            nn = -(-n * int(se[m]) // int(se[mm]))
            down += mm < m and nn > n
            route2 += k >= 2
            ends_at_S += start + nn == S
    ok = want[:, 0] == 0
    return dict(down=down, route2=route2, ends_at_S=ends_at_S, lost_ns=int(np.nansum(want[ok, 5])), lost_qot=int(np.nansum(want[ok, 6])),
                sequential=int(np.sum(np.any(act != indep_act, axis=1))), no_victim=int(np.sum(want[ok, 1] == 0)),
                evaluated=int(ok.sum()), restored=int(np.nansum(want[ok, 3])))


def oracle_records(o):
    """an oracle's running services in the order of the links' lists (by release time: one holding-time law for every
    request), behind the ones a counters-only reset made permanent (drive)"""
    svcs = o.services()
    return np.concatenate([getattr(o, "kept", svcs[:0]), svcs[np.argsort(svcs["release_time"], kind="stable")]])


def drive(key, env=None, oracles=True):
    """(tables, kwargs, holder, oracles) of a case after its traffic; `env`, a device environment of the same configuration,
    is driven in lock step"""
    from oracle_lib import OracleEnv
    tb, kw, B, steps, how = case_config(key)
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
                if i:                   # the counters-only reset drops the departure heap: what runs now runs for good, and
                    o.kept = oracle_records(o)      # the oracle no longer lists it
                    o.kept["release_time"] = np.inf
                    o.reset_counters()
                o.run_first_fit(n)
    return tb, kw, holder, ors


# ---- the GPU computations -----------------------------------------------------------------------------------------------
def gpu_case(out, key):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb, kw, B, _, how = case_config(key)
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    tb, kw, holder, ors = drive(key, env, oracles=False)      # the oracles only lend `candidates` and `gn_lists`
    E = tb.n_links
    links = explicit_links(E, B)
    got_all, svc_all = env.failure_impact(detail=True)
    got_list, svc_list = env.failure_impact(links, detail=True)
    only = env.failure_impact()
    out[key + "_same_without_detail"] = np.array_equal(only, got_all, equal_nan=True)
    tot = dict()
    near = 0
    for r, o in enumerate(ors):
        svcs, grid = env.services(r), env.grid(r)
        margin, log = replica_margin(kw, r), []
        want, act, wide = restate_replica(o, tb, holder, margin, svcs, grid, np.arange(E), how == "ids", True, log)
        _, indep, _ = restate_replica(o, tb, holder, margin, svcs, grid, np.arange(E), how == "ids", False)
        want_l, act_l, _ = restate_replica(o, tb, holder, margin, svcs, grid, links[r], how == "ids", True, log)
        near += int(np.sum(np.array(log) < BAND))
        k = f"{key}_r{r}"
        out[k + "_got"], out[k + "_svc"], out[k + "_want"], out[k + "_act"] = got_all[r], svc_all[r], want, act
        out[k + "_got_list"], out[k + "_svc_list"], out[k + "_want_list"], out[k + "_act_list"] = got_list[r], svc_list[r], want_l, act_l
        out[k + "_active"] = len(svcs)
        cond = conditions(tb, holder, svcs, want, act, indep)
        cond["wide"], cond["wide_seen"] = wide
        cond["namesakes"] = len(svcs) - len(np.unique(svcs["service_id"])) if how == "ids" else 0
        for name, v in cond.items():
            tot[name] = tot.get(name, 0) + int(v)
    for name, v in tot.items():
        out[f"{key}_cond_{name}"] = v
    out[key + "_B"], out[key + "_E"], out[key + "_band"] = B, E, near
    out[key + "_uniform"] = bool(np.all(tb.link_alpha == tb.link_alpha[0]))
    out[key + "_rec32"] = bool(tb.n_links <= 32 and len(tb.path_hops) <= 512)
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
    a = env.failure_impact()
    b, _ = env.failure_impact(np.zeros((B, 3), np.int32), detail=True)
    blob1, st1 = env.save_state(), env.stats()
    out["ro_blob_same"] = blob0.tobytes() == blob1.tobytes()
    out["ro_stats_same"] = st0.tobytes() == st1.tobytes()
    out["ro_traj_same"] = record_bytes(env.step_policy(60)) == record_bytes(twin.step_policy(60))
    out["ro_victims"] = int(np.sum(a[:, :, 1]))
    out["ro_duplicates_same"] = bool(np.array_equal(b[:, 0], a[:, 0], equal_nan=True) and np.array_equal(b[:, 1], b[:, 2], equal_nan=True))
    env.close()
    twin.close()


def fresh(out, B=8):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **dict(BASE, num_spectrum_resources=128, capacity=128, load=100.0))
    env.seed(3)
    env.reset()
    out["fresh_rows"], out["fresh_svc"] = env.failure_impact(detail=True)
    env.close()


def device_io(out, B=32):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    kw = dict(BASE, num_spectrum_resources=128, capacity=192, load=120.0)
    host = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    dev = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, io_device=True, **kw)
    c = host.holder.struct
    E, Cp = c.n_links, c.capacity
    t = torch.full((B, E, 10), 7.0, dtype=torch.float64, device="cuda")
    try:
        dev.failure_impact(out=t)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    host.seed(5)
    host.reset()
    host.step_policy(220, record=False)
    links = explicit_links(E, B)[:, :5].copy()
    want, want_svc = host.failure_impact(detail=True)
    want_l = host.failure_impact(links)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        dev.seed(5)
        dev.reset()
        dev.step_policy(220, record=False)
        r = dev.failure_impact(out=t)
        t2 = torch.full((B, E, 10), 7.0, dtype=torch.float64, device="cuda")
        s2 = torch.full((B, E, Cp), 7, dtype=torch.int32, device="cuda")
        dev.failure_impact(out=(t2, s2), detail=True)
        t3 = torch.full((B, 5, 10), 7.0, dtype=torch.float64, device="cuda")
        dev.failure_impact(torch.from_numpy(links).cuda(), out=t3)
        stream.synchronize()
        out["dev_same"] = r is t and np.array_equal(t.cpu().numpy(), want, equal_nan=True)
        out["dev_detail_same"] = (np.array_equal(t2.cpu().numpy(), want, equal_nan=True)
                                  and np.array_equal(s2.cpu().numpy(), want_svc))
        out["dev_list_same"] = np.array_equal(t3.cpu().numpy(), want_l, equal_nan=True)
        bad = []
        for args, kws in (((torch.zeros((B, 5), dtype=torch.int64, device="cuda"),), dict(out=t3)),
                          ((torch.zeros((B, 5), dtype=torch.int32),), dict(out=t3)),
                          ((links,), dict(out=t3)),
                          ((), dict(out=t3)),
                          ((), dict(out=t, detail=True)),
                          ((), dict(out=(t, s2.long()), detail=True))):
            try:
                dev.failure_impact(*args, **kws)
                bad.append(False)
            except ValueError:
                bad.append(True)
        out["dev_refusals"] = np.array(bad)
        dev.set_stream(None)
    host.close()
    dev.close()


def compat(out):
    from optical_networking_gym.envs.qrmsa import QRMSAEnv
    from optical_networking_gym.topology import bundled_topology_path, get_topology
    topology = get_topology(bundled_topology_path("nsfnet_chen.txt"), None, jocn_modulations(), 80, 0.2, 4.5, 5)
    single = QRMSAEnv(topology=topology, seed=9, load=300, episode_length=1000, num_spectrum_resources=320, launch_power_dbm=1.0,
                      margin=0.5, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), gen_observation=False)
    single.reset()
    for _ in range(150):
        single.step(single.first_fit_action()[0])
    c = single._dev.holder.struct
    M, S = c.n_mods, c.n_slots
    same, victims = True, 0
    u, v = next(iter(topology.edges()))
    for link in (topology[u][v]["index"], (u, v), 3, -1):
        d = single.failure_impact(link)
        idx = topology[u][v]["index"] if isinstance(link, tuple) else link
        row, svc = single._dev.failure_impact(np.array([[idx]], np.int32), detail=True)
        same &= list(d)[:10] == list(nat.FAILURE_IMPACT) and set(d) == set(nat.FAILURE_IMPACT) | {"restorations", "lost"}
        same &= all((np.isnan(row[0, 0, i]) and np.isnan(d[k])) or float(d[k]) == row[0, 0, i] for i, k in enumerate(nat.FAILURE_IMPACT))
        same &= all(svc[0, 0, i] == k * M * S + (M - 1 - m) * S + a for i, k, m, a in d["restorations"])
        same &= all(svc[0, 0, i] == c.k_paths * M * S for i in d["lost"])
        if idx >= 0:
            same &= len(d["restorations"]) == d["restored"] and len(d["lost"]) == d["lost_no_spectrum"] + d["lost_qot"]
            same &= isinstance(d["victims"], int)
            victims += d["victims"]
        else:
            same &= d["status"] == 1 and d["restorations"] == [] and d["lost"] == []
    out["compat_same"], out["compat_victims"] = bool(same), victims
    single.close()


def refusals(out):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, **dict(BASE, num_spectrum_resources=128, capacity=128, load=100.0))
    E = env.holder.struct.n_links
    links, res = np.zeros((4, E + 1), np.int32), np.zeros((4, E + 1, 10))
    rc = {}
    rc["zero"] = env.lib.ongym_failure_impact(env._h, 0, links.ctypes.data, res.ctypes.data, None)
    out["refuse_zero_msg"] = env.lib.ongym_last_error(env._h).decode()
    rc["many"] = env.lib.ongym_failure_impact(env._h, E + 1, links.ctypes.data, res.ctypes.data, None)
    rc["null_links"] = env.lib.ongym_failure_impact(env._h, 3, None, res.ctypes.data, None)
    rc["null_out"] = env.lib.ongym_failure_impact(env._h, 3, links.ctypes.data, None, None)
    rc["ok"] = env.lib.ongym_failure_impact(env._h, E, None, res.ctypes.data, None)
    env.close()
    narrow = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, modulations_to_consider=3,
                             **dict(BASE, num_spectrum_resources=128, capacity=128, load=100.0))
    rc["window"] = narrow.lib.ongym_failure_impact(narrow._h, E, None, res.ctypes.data, None)
    out["refuse_window_msg"] = narrow.lib.ongym_last_error(narrow._h).decode()
    narrow.close()
    for k, v in rc.items():
        out["refuse_rc_" + k] = v


def main():
    out = {}
    refusals(out)
    fresh(out)
    read_only(out)
    device_io(out)
    compat(out)
    for key in CASES:
        gpu_case(out, key)
        print(key, "done", flush=True)
    np.savez(sys.argv[1], **out)
    print("failure impact child ok")


if __name__ == "__main__":
    main()
