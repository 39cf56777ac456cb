"""Child process of tests/test_gpu_link_cut.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP
runtime and this library's must start together), saved to an .npz that the tests assert on.

    python tests/link_cut_child.py OUT.npz

It also holds the restatement of ongym_cut_links (include/ongym.h) in plain numpy, `expected_cut`: the row and the placements
come from restate_set of tests/failure_sets_child.py on the pre-cut records and grid; from them follow the post-cut records
(the survivors in order, then the restored victims with their own release time, id and disrupted flag), the post-cut grid
(victims released, restorations provisioned, failed rows without a free slot) and the index of every pre-cut record.
`first_fit_restated` is first fit's decision for the pending request on a state, with `search` and `gn_running` of
tests/failure_impact_child.py.  tests/test_link_cut_host.py runs both on the CPU oracles of the same cases and seeds.

Replica r's set: r % 4 == 0 a node's links, 1 a dual cut drawn with default_rng(300 + r), 2 the link most records cross,
3 the empty set.
"""
import os
import sys
from itertools import combinations

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402,F401  (before the library is loaded: the two HIP runtimes must start together)

from common import golden_tables, record_bytes  # noqa: E402
from failure_impact_child import (BAND, BASE, CASES, SEED, case_config, drive, gn_running, path_links_of, provision, release,  # noqa: E402
                                  replica_margin, ring_tables, route_of, search)
from failure_sets_child import as_words, node_lists, restate_set  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402

SET_SEED = 300                                   # replica r draws its dual cut with default_rng(SET_SEED + r)
TRAFFIC = ("nsfnet", "nobeleu", "odd", "ring4")  # the cases that go on with traffic after the cut
BOTH = ("nsfnet", "nobeleu")                     # the cases run on both step kernels
FIELDS = ("path_id", "slot", "nslots", "modulation", "reserved", "release_time", "service_id", "osnr")
OSNR = FIELDS.index("osnr")
COVER = ("multi", "skip_restored")


# ---- the sets -------------------------------------------------------------------------------------------------------------
def replica_links(tb, svcs, r):
    """the link list of replica r on the state `svcs`"""
    E = tb.n_links
    if r % 4 == 0:
        return node_lists(tb)[(r // 4) % tb.n_nodes]
    if r % 4 == 1:
        pairs = list(combinations(range(E), 2))
        return list(pairs[int(np.random.default_rng(SET_SEED + r).integers(len(pairs)))])
    if r % 4 == 2:
        count = np.zeros(E, np.int64)
        for s in svcs:
            count[path_links_of(tb, int(s["path_id"]))] += 1
        return [int(np.argmax(count))]
    return []


def links_of(w):
    bits = int(w[0]) | (int(w[1]) << 64)
    return [e for e in range(128) if (bits >> e) & 1]


# ---- the restatement ------------------------------------------------------------------------------------------------------
def svc_rows(svcs):
    """float64 [n, 8], columns FIELDS: every value is exact in a double"""
    return np.stack([svcs[f].astype(np.float64) for f in FIELDS], axis=1).reshape(-1, len(FIELDS))


def running_of(rows):
    return [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[6])) for r in rows]


def expected_cut(o, tb, holder, margin, svcs, grid, w, ids=False, restore=True, log=None, cover=None):
    """(cut_out row [13], svc_out [n], index_out [n], post-cut records [n', 8] in the columns FIELDS, post-cut grid) of the set
    `w` (two uint64 words) on the state (svcs in record order, grid).  With ids the osnr column of a restored record is the
    restoration's GSNR from the oracle's literal GN; without, a record's osnr column stays what it was"""
    c = holder.struct
    K, M, S, n = c.k_paths, c.n_mods, c.n_slots, len(svcs)
    se = np.asarray(holder.mod_se)
    rows = svc_rows(svcs)
    failed = links_of(w)
    row = np.full(len(nat.CUT_LINKS), np.nan)
    if not failed or max(failed) >= tb.n_links:
        row[0] = 1
        return row, np.full(n, -1, np.int32), np.full(n, -1, np.int32), rows, grid.copy()
    if restore:
        row[:12], act = restate_set(o, tb, holder, margin, svcs, grid, w, ids, log, cover)
        row[12] = 0
    else:
        hit = [bool(set(path_links_of(tb, int(s["path_id"])).tolist()) & set(failed)) for s in svcs]
        act = np.where(hit, K * M * S, -1).astype(np.int32)
        cap = sum(int(s["nslots"]) * int(se[int(s["modulation"])]) for s, h in zip(svcs, hit) if h)
        row[:] = [0, sum(hit), cap, 0, 0, 0, 0, 0, 0, np.nan, 0, len(failed), sum(hit)]
    victims, survivors = np.flatnonzero(act >= 0), np.flatnonzero(act < 0)
    index = np.full(n, -1, np.int32)
    index[survivors] = np.arange(len(survivors))
    post = [rows[i] for i in survivors]
    grid = grid.copy()
    for i in victims:
        release(grid, tb, int(rows[i, 0]), int(rows[i, 1]), int(rows[i, 2]))
    routes = route_of(tb)
    for i in victims:
        a = int(act[i])
        if a >= K * M * S:
            continue
        k, mm, start = a // (M * S), M - 1 - (a // S) % M, a % S
        old, nold, mold, sid = int(rows[i, 0]), int(rows[i, 2]), int(rows[i, 3]), int(rows[i, 6])
        s, d, _ = routes[old]
        p = int(tb.pair_paths[s, d, k])
        nn = -(-nold * int(se[mold]) // int(se[mm]))
        new = rows[i].copy()
        new[:4] = p, start, nn, mm
        if ids:
            new[OSNR] = gn_running(o, tb, se, running_of(post), p, start, nn, sid)[0]
        provision(grid, tb, p, start, nn)
        index[i] = len(post)
        post.append(new)
    grid[failed, :] = 0
    return row, act, index, np.array(post, np.float64).reshape(-1, len(FIELDS)), grid


def first_fit_restated(o, tb, holder, margin, rows, grid, req, cur_id=None, log=None):
    """first fit's action for the pending request `req` on the state (records `rows` in the columns FIELDS, grid); cur_id: the
    request's service id under id tracking (its running namesakes are no interferers)"""
    c = holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    se, thr = np.asarray(holder.mod_se), np.asarray(holder.mod_thr)
    running = running_of(rows)
    nslots = [o.number_slots(float(req["bit_rate"]), m) for m in range(M)]
    routes = []
    for k in range(K):
        p = int(tb.pair_paths[int(req["source"]), int(req["destination"]), k])
        if p < 0:
            break
        routes.append((k, p))
    hit, _ = search(o, tb, thr, margin, nslots, routes, grid,
                    lambda p, a, nn: gn_running(o, tb, se, running, p, a, nn, cur_id)[0], log)
    return K * M * S if hit is None else hit[0] * M * S + (M - 1 - hit[1]) * S + hit[2]


def grid_of_records(tb, E, S, rows, failed=()):
    """the grid that provisioning `rows` on an empty network gives, with the rows of `failed` full"""
    g = np.ones((E, S), np.int32)
    for r in rows:
        provision(g, tb, int(r[0]), int(r[1]), int(r[2]))
    g[list(failed), :] = 0
    return g


def crossing(tb, rows, links):
    """records of `rows` whose route contains a link of `links`"""
    links = set(links)
    return sum(bool(set(path_links_of(tb, int(r[0])).tolist()) & links) for r in rows)


def coverage(row, cover):
    """what a replica's restated cut exercises"""
    if row[0] != 0:
        return dict(evaluated=0, no_victim=0, restored=0, lost_qot=0, lost_ns_route=0, no_route=0, multi=0)
    return dict(evaluated=1, no_victim=int(row[1] == 0), restored=int(row[3]), lost_qot=int(row[6]),
                lost_ns_route=int(row[5] - row[10]), no_route=int(row[10]), multi=int(cover["multi"]))


# ---- the GPU computations -------------------------------------------------------------------------------------------------
def make_env(key, generic=False, **more):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb, kw, B, _, _ = case_config(key)
    if generic:
        os.environ["ONGYM_FORCE_GENERIC"] = "1"          # read at create
    # twice the case's record table: it is sized for the steps of `drive`, and the traffic after the cut goes on for 400 more
    # (the table's size changes no decision short of an overflow, which the library reports as an error)
    more.setdefault("capacity", 2 * kw["capacity"])
    try:
        return BatchedQRMSAEnv(tables=tb, batch_size=B, **dict(kw, **more))
    finally:
        os.environ.pop("ONGYM_FORCE_GENERIC", None)


def extend_trace(env, tb, kw, B, n=480):
    """the trace of a `trace` case ends with its drive: a continuation by the same law from each replica's clock (the pending
    request stays; the new trace starts at its first entry)"""
    rng = np.random.default_rng(SEED + 1)
    now = env.stats()["current_time"]
    reqs = np.zeros((B, n), nat.REQUEST_DTYPE)
    for r in range(B):
        reqs[r]["arrival_time"] = (now[r] + np.cumsum(rng.exponential(10800.0 / (kw["load"] * (0.6 + 0.1 * r)), n))).astype(np.float32)
        reqs[r]["holding_time"] = rng.exponential(10800.0, n).astype(np.float32)
        src = rng.integers(0, tb.n_nodes, n)
        reqs[r]["source"], reqs[r]["destination"] = src, (src + rng.integers(1, tb.n_nodes, n)) % tb.n_nodes
        reqs[r]["bit_rate"] = rng.choice(np.array([100, 400, 1000]), n)
    env.set_requests(reqs)


def state_of(env, B):
    return [env.services(r) for r in range(B)], [env.grid(r) for r in range(B)]


def stats_same(a, b, skip):
    return all(np.array_equal(a[f], b[f]) for f in a.dtype.names if f not in skip)


def gpu_case(out, key):
    tb, kw, B, _, how = case_config(key)
    ids = how == "ids"
    env, twin = make_env(key), make_env(key)
    tb, kw, holder, ors = drive(key, env, oracles=False)          # the oracles only lend `candidates` and `gn_lists`
    drive(key, twin, oracles=False)
    if how == "trace":
        extend_trace(env, tb, kw, B)
    c = holder.struct
    E, S, K, M = tb.n_links, c.n_slots, c.k_paths, c.n_mods
    svcs0, grid0 = state_of(env, B)
    lists = [replica_links(tb, svcs0[r], r) for r in range(B)]
    W = as_words(lists)
    blob0, st0 = env.save_state(), env.stats()
    blobs0 = [env.save_state([r]).tobytes() for r in range(B)]
    twin.load_state(blob0)                                           # the twin: the pre-cut state in a second environment
    fs, fs_svc = twin.failure_sets(np.ascontiguousarray(W[:, None, :]), detail=True)
    out[key + "_fs"], out[key + "_fs_svc"] = fs[:, 0], fs_svc[:, 0]

    cut, (svc, index) = env.cut_links(W, detail=True)
    st1, failed = env.stats(), env.failed_links()
    svcs1, grid1 = state_of(env, B)
    ff, _ = env.policy_actions(nat.POLICY_FIRST_FIT)
    reqs = [env.request(r) for r in range(B)]
    blobs1 = [env.save_state([r]).tobytes() for r in range(B)]
    out[key + "_cut"], out[key + "_svc"], out[key + "_index"], out[key + "_failed"], out[key + "_W"] = cut, svc, index, failed, W
    out[key + "_ff"] = ff
    out[key + "_noop_blob_same"] = np.array([blobs0[r] == blobs1[r] for r in range(B)])
    out[key + "_stats_same"] = stats_same(st0, st1, ("active", "episode_osnr_sum") if ids else ("active",))
    out[key + "_active_after"], out[key + "_osnr_sum"] = st1["active"], np.stack([st0["episode_osnr_sum"], st1["episode_osnr_sum"]])

    # the restatement of the cut and of the first decision after it, from the device's own pre- and post-cut state
    near, tot, delta = 0, {}, np.zeros(B)
    want_ff = np.zeros(B, np.int32)
    for r, o in enumerate(ors):
        log, cover = [], dict.fromkeys(COVER, 0)
        margin = replica_margin(kw, r)
        row, act, idx, post, grid = expected_cut(o, tb, holder, margin, svcs0[r], grid0[r], W[r], ids, True, log, cover)
        k = f"{key}_r{r}"
        out[k + "_row"], out[k + "_act"], out[k + "_idx"], out[k + "_post"], out[k + "_grid"] = row, act, idx, post, grid
        out[k + "_got_post"], out[k + "_got_grid"], out[k + "_active0"] = svc_rows(svcs1[r]), grid1[r], len(svcs0[r])
        cur_id = int(st1[r]["episode_services_processed"]) - 1 if ids else None
        want_ff[r] = first_fit_restated(o, tb, holder, margin, svc_rows(svcs1[r]), grid1[r], reqs[r], cur_id, log)
        near += int(np.sum(np.array(log) < BAND))
        moved = np.flatnonzero((index[r, :len(svcs0[r])] >= 0) & (svc[r, :len(svcs0[r])] >= 0))      # the restored
        if ids and len(svcs1[r]) == len(post):
            delta[r] = float(np.sum(svcs1[r]["osnr"][index[r, moved]] - svcs0[r]["osnr"][moved]))
        for name, v in coverage(row, cover).items():
            tot[name] = tot.get(name, 0) + v
    out[key + "_want_ff"], out[key + "_band"], out[key + "_osnr_delta"] = want_ff, near, delta
    for name, v in tot.items():
        out[f"{key}_cond_{name}"] = v
    out[key + "_B"], out[key + "_E"], out[key + "_S"], out[key + "_ids"] = B, E, S, ids
    out[key + "_rec32"] = bool(tb.n_links <= 32 and len(tb.path_hops) <= 512)

    # restore=False on the twin, which still holds the pre-cut state
    cut_n, (svc_n, index_n) = twin.cut_links(lists, restore=False, detail=True)
    out[key + "_nr_cut"], out[key + "_nr_svc"], out[key + "_nr_index"], out[key + "_nr_failed"] = cut_n, svc_n, index_n, twin.failed_links()
    for r, o in enumerate(ors):
        row, act, idx, post, grid = expected_cut(o, tb, holder, replica_margin(kw, r), svcs0[r], grid0[r], W[r], ids, False)
        k = f"{key}_r{r}_nr"
        out[k + "_row"], out[k + "_act"], out[k + "_idx"], out[k + "_post"], out[k + "_grid"] = row, act, idx, post, grid
        out[k + "_got_post"], out[k + "_got_grid"] = svc_rows(twin.services(r)), twin.grid(r)
    twin.close()

    if key in TRAFFIC:                                               # traffic continues on the degraded network
        fl = [links_of(failed[r]) for r in range(B)]
        grid_ok, cross, failed_same = [], [], []
        for _ in range(6):
            env.step_policy(50, record=False)
            s, g = state_of(env, B)
            grid_ok.append([np.array_equal(g[r], grid_of_records(tb, E, S, svc_rows(s[r]), fl[r])) for r in range(B)])
            cross.append([crossing(tb, svc_rows(s[r]), fl[r]) for r in range(B)])
            failed_same.append(np.array_equal(env.failed_links(), failed))
        out[key + "_run_grid_ok"], out[key + "_run_cross"], out[key + "_run_failed_same"] = np.array(grid_ok), np.array(cross), np.array(failed_same)
        out[key + "_run_steps"] = env.stats()["total_steps"] - st1["total_steps"]
        out[key + "_repaired"], out[key + "_set_size"] = env.repair_links(W), np.array([len(l) for l in lists])
        g = [env.grid(r) for r in range(B)]
        out[key + "_rows_free"] = all(np.all(g[r][lists[r], :] == 1) for r in range(B))
        out[key + "_failed_after_repair"] = env.failed_links()
        env.step_policy(100, record=False)
        s, g = state_of(env, B)
        out[key + "_later_grid_ok"] = np.array([np.array_equal(g[r], grid_of_records(tb, E, S, svc_rows(s[r]))) for r in range(B)])
        out[key + "_later_cross"] = sum(crossing(tb, svc_rows(s[r]), lists[r]) for r in range(B))
    env.close()


def both_kernels(out, key):
    """the same cut after the same launch on the lean and on the generic step kernel, then 250 recorded steps"""
    tb, kw, B, _, how = case_config(key)
    recs, fails = [], []
    for generic in (False, True):
        env = make_env(key, generic=generic)
        drive(key, env, oracles=False)
        if how == "trace":
            extend_trace(env, tb, kw, B)
        lists = [replica_links(tb, env.services(r), r) for r in range(B)]
        env.cut_links(lists)
        recs.append(env.step_policy(250))
        fails.append(env.failed_links())
        out[f"{key}_both_lean{int(generic)}"] = env.occupancy()["lean_kernel"]
        env.close()
    a, b = recs
    out[key + "_both_same"] = all(np.array_equal(a[f], b[f]) for f in ("action", "accepted", "flags", "active"))
    out[key + "_both_osnr"] = np.stack([a["osnr"], b["osnr"]])
    out[key + "_both_accepted"] = int(a["accepted"].sum())
    out[key + "_both_failed_same"] = np.array_equal(fails[0], fails[1]) and bool(np.any(fails[0]))


LOW = dict(BASE, num_spectrum_resources=128, capacity=128, load=3.0)      # a few records: most links carry none


def noops(out, B=8):
    """a cut without victims and its repair give the starting state back; one shared set equals the set tiled per replica"""
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb = golden_tables("nsfnet")
    envs = [BatchedQRMSAEnv(tables=tb, batch_size=B, **LOW) for _ in range(2)]
    for e in envs:
        e.seed(11)
        e.reset()
        e.step_policy(40, record=False)
    env, other = envs
    idle = []
    for r in range(B):
        used = set()
        for s in env.services(r):
            used |= set(path_links_of(tb, int(s["path_id"])).tolist())
        idle.append([min(set(range(tb.n_links)) - used)])
    start = [env.save_state([r]).tobytes() for r in range(B)]
    cut = env.cut_links(idle)
    out["noop_victims"], out["noop_status"] = cut[:, 1], cut[:, 0]
    out["noop_failed"] = np.array_equal(env.failed_links(), as_words(idle))
    out["noop_changed"] = np.array([env.save_state([r]).tobytes() != start[r] for r in range(B)])
    again = env.cut_links(idle)                                      # an already failed link: no victim, nothing changes
    mid = [env.save_state([r]).tobytes() for r in range(B)]
    out["noop_again_victims"] = again[:, 1]
    out["noop_repaired"] = env.repair_links(idle)
    out["noop_back"] = np.array([env.save_state([r]).tobytes() == start[r] for r in range(B)])
    out["noop_repaired_twice"] = env.repair_links(idle)              # healthy links are ignored
    out["noop_still_back"] = np.array([env.save_state([r]).tobytes() == start[r] for r in range(B)])
    env.cut_links(idle)
    out["noop_recut_same"] = np.array([env.save_state([r]).tobytes() == mid[r] for r in range(B)])
    env.repair_links(idle)
    shared = as_words([[5, 9]])[0]
    a = env.cut_links(shared, detail=True)
    b = other.cut_links(np.ascontiguousarray(np.tile(shared[None], (B, 1))), detail=True)
    out["shared_same"] = (np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1][0], b[1][0])
                          and np.array_equal(a[1][1], b[1][1]) and env.save_state().tobytes() == other.save_state().tobytes())
    out["shared_victims"] = int(np.sum(a[0][:, 1]))
    for e in envs:
        e.close()


def state_calls(out, key="nsfnet"):
    """save / load / fork carry failures, a reset returns every fibre"""
    tb, kw, B, _, _ = case_config(key)
    env, second = make_env(key), make_env(key)
    drive(key, env, oracles=False)
    second.seed(SEED)
    second.reset()
    lists = [replica_links(tb, env.services(r), r) for r in range(B)]
    env.cut_links(lists)
    failed = env.failed_links()
    blob = env.save_state()
    want = env.step_policy(100)
    second.load_state(blob)
    out["state_failed_same"] = np.array_equal(second.failed_links(), failed) and bool(np.all(np.any(failed[np.arange(B) % 4 != 3] != 0, axis=1)))
    out["state_records_same"] = record_bytes(second.step_policy(100)) == record_bytes(want)
    out["state_failed_kept"] = np.array_equal(env.failed_links(), failed)
    src = np.arange(B, dtype=np.int32)
    src[3] = 0                                                       # a cut replica into a healthy one
    out["fork_healthy_before"] = not np.any(failed[3])
    env.fork(src)
    after = env.failed_links()
    out["fork_copies"] = np.array_equal(after[3], failed[0]) and np.array_equal(np.delete(after, 3, 0), np.delete(failed, 3, 0))
    mask = (np.arange(B) % 4 == 0).astype(np.uint8)
    env.reset(mask)
    reset = env.failed_links()
    out["reset_clears"] = not np.any(reset[mask == 1]) and np.array_equal(reset[mask == 0], after[mask == 0])
    env.close()
    second.close()


NSF = dict(BASE, num_spectrum_resources=128, capacity=192, load=120.0)


def device_io(out, B=32):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb = golden_tables("nsfnet")
    host = BatchedQRMSAEnv(tables=tb, batch_size=B, **NSF)
    dev = BatchedQRMSAEnv(tables=tb, batch_size=B, io_device=True, **NSF)
    Cp = host.holder.struct.capacity
    host.seed(5)
    host.reset()
    host.step_policy(220, record=False)
    W = as_words([replica_links(tb, host.services(r), r) for r in range(B)])
    W_t = torch.from_numpy(W.view(np.int64)).cuda()
    t = torch.full((B, 13), 7.0, dtype=torch.float64, device="cuda")
    try:
        dev.cut_links(W_t, out=t)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    want, (want_svc, want_idx) = host.cut_links(W, detail=True)
    want_failed = host.failed_links()
    want_blob = host.save_state()
    want_rep = host.repair_links(W)
    want_after = host.save_state()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        dev.seed(5)
        dev.reset()
        dev.step_policy(220, record=False)
        s2 = torch.full((B, Cp), 7, dtype=torch.int32, device="cuda")
        i2 = torch.full((B, Cp), 7, dtype=torch.int32, device="cuda")
        r = dev.cut_links(W_t.view(torch.uint64) if hasattr(torch, "uint64") else W_t, out=(t, s2, i2), detail=True)
        f = torch.full((B, 2), 7, dtype=torch.int64, device="cuda")
        dev.failed_links(out=f)
        blob = dev.save_state()
        n = torch.full((B,), 7, dtype=torch.int32, device="cuda")
        dev.repair_links(W_t, out=n)
        after = dev.save_state()
        stream.synchronize()
        out["dev_same"] = (r[0] is t and np.array_equal(t.cpu().numpy(), want, equal_nan=True)
                           and np.array_equal(s2.cpu().numpy(), want_svc) and np.array_equal(i2.cpu().numpy(), want_idx))
        out["dev_failed_same"] = np.array_equal(f.cpu().numpy().view(np.uint64), want_failed) and bool(np.any(want_failed))
        out["dev_state_same"] = blob.cpu().numpy().tobytes() == want_blob.tobytes()
        out["dev_repair_same"] = (np.array_equal(n.cpu().numpy(), want_rep) and int(want_rep.sum()) > 0
                                  and after.cpu().numpy().tobytes() == want_after.tobytes())
        bad = []
        for call in (lambda: dev.cut_links(W_t.int(), out=t),                   # dtype
                     lambda: dev.cut_links(torch.from_numpy(W.view(np.int64)), out=t),   # a host tensor
                     lambda: dev.cut_links(W, out=t),                           # not a tensor
                     lambda: dev.cut_links(W_t),                                # no out
                     lambda: dev.cut_links(W_t[:B - 1], out=t),                 # a set per replica for B - 1 replicas
                     lambda: dev.cut_links(W_t, out=t, detail=True),            # detail without the triple
                     lambda: dev.cut_links(W_t, out=(t, s2.long(), i2), detail=True),
                     lambda: dev.repair_links(W_t),
                     lambda: dev.repair_links(W_t, out=n.long()),
                     lambda: dev.failed_links(),
                     lambda: dev.failed_links(out=f.int())):
            try:
                call()
                bad.append(False)
            except ValueError:
                bad.append(True)
        out["dev_refusals"] = np.array(bad)
        dev.set_stream(None)
    host.close()
    dev.close()


def refusals(out):
    from dataclasses import replace
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    small = dict(NSF, capacity=128)
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, **small)
    env.seed(1)
    env.reset()
    sets, res, failed = np.ones((4, 2), np.uint64), np.zeros((4, 13)), np.zeros((4, 2), np.uint64)
    sets[:, 1] = 0
    rc, msg = {}, {}

    def call(name, e, fn, *a):
        rc[name] = getattr(e.lib, fn)(e._h, *a)
        msg[name] = e.lib.ongym_last_error(e._h).decode() if rc[name] else ""

    call("null_sets", env, "ongym_cut_links", None, 1, 0, res.ctypes.data, None, None)
    call("null_out", env, "ongym_cut_links", sets.ctypes.data, 1, 0, None, None, None)
    call("flags", env, "ongym_cut_links", sets.ctypes.data, 1, 2, res.ctypes.data, None, None)
    call("repair_null_sets", env, "ongym_repair_links", None, 1, None)
    call("null_failed", env, "ongym_failed_links", None)
    call("ok", env, "ongym_cut_links", sets.ctypes.data, 1, 0, res.ctypes.data, None, None)
    call("ok_shared", env, "ongym_cut_links", sets.ctypes.data, 0, nat.CUT_NO_RESTORE, res.ctypes.data, None, None)
    call("ok_failed", env, "ongym_failed_links", failed.ctypes.data)
    call("ok_repair", env, "ongym_repair_links", sets.ctypes.data, 1, None)
    out["refuse_failed_between"] = failed
    env.close()
    narrow = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, modulations_to_consider=3, **small)
    call("window", narrow, "ongym_cut_links", sets.ctypes.data, 1, 0, res.ctypes.data, None, None)
    narrow.close()
    tb = ring_tables()                                               # one pair lists its two routes in the other order
    pp = tb.pair_paths.copy()
    pp[1, 0] = pp[1, 0][::-1]
    odd = BatchedQRMSAEnv(tables=replace(tb, pair_paths=pp), batch_size=4, **dict(BASE, num_spectrum_resources=40, capacity=64, load=10.0))
    call("pairs", odd, "ongym_cut_links", sets.ctypes.data, 1, 0, res.ctypes.data, None, None)
    odd.close()
    for k, v in rc.items():
        out["refuse_rc_" + k], out["refuse_msg_" + k] = v, msg[k]


def main():
    out = {}
    refusals(out)
    noops(out)
    state_calls(out)
    device_io(out)
    for key in BOTH:
        both_kernels(out, key)
    for key in CASES:
        gpu_case(out, key)
        print(key, "done", flush=True)
    np.savez(sys.argv[1], **out)
    print("link cut child ok")


if __name__ == "__main__":
    main()
