"""Child process of tests/test_gpu_failure_sets.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP
runtime and this library's must start together), saved to an .npz that the tests assert on.

    python tests/failure_sets_child.py OUT.npz

It also holds `restate_set`, the restatement of a link-set scenario of ongym_failure_sets (include/ongym.h) in plain numpy.  It
is restate_scenario of tests/failure_impact_child.py with the membership tests `link in ...` replaced by set intersection and
lost_no_route counted when the eligible list is empty; it uses that module's helpers (search, release, provision, gn_running,
route_of) as they are.  tests/test_failure_sets_host.py pins it to restate_scenario on one-element sets.
"""
import os
import sys
from itertools import combinations

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402,F401  (before the library is loaded: the two HIP runtimes must start together)

from common import golden_tables, jocn_modulations  # noqa: E402
from failure_impact_child import (BAND, BASE, CASES, case_config, drive, gn_running, path_links_of, provision, release,  # noqa: E402
                                  replica_margin, route_of, search)
from optical_networking_gym import _native as nat  # noqa: E402

PAIRS = 12           # dual cuts per replica
PAIR_SEED = 100      # replica r draws its dual cuts with default_rng(PAIR_SEED + r)
COVER = ("multi", "skip_restored")


# ---- the scenario lists, constructed directly from link_nodes -------------------------------------------------------------
def words(links):
    """[word 0, word 1] of a set of link indices: bit e & 63 of word e >> 6"""
    bits = 0
    for e in links:
        bits |= 1 << int(e)
    return [bits & (2 ** 64 - 1), bits >> 64]


def node_lists(tb):
    """per node the links that end there"""
    return [[e for e, (a, b) in enumerate(tb.link_nodes.tolist()) if v in (a, b)] for v in range(tb.n_nodes)]


def pair_lists(tb, r):
    """up to PAIRS dual cuts of replica r"""
    pairs = list(combinations(range(tb.n_links), 2))
    pick = np.random.default_rng(PAIR_SEED + r).choice(len(pairs), min(len(pairs), PAIRS), replace=False)
    return [list(pairs[i]) for i in pick]


def scenario_lists(tb, r):
    """the list of replica r: every node's links, its dual cuts, the E one-link sets, the first node once more, the empty
    set, a set with bit E"""
    E, nodes = tb.n_links, node_lists(tb)
    return nodes + pair_lists(tb, r) + [[e] for e in range(E)] + [nodes[0], [], [E]]


def as_words(lists):
    return np.array([words(l) for l in lists], np.uint64).reshape(-1, 2)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def restate_set(o, tb, holder, margin, svcs, grid, w, ids=False, log=None, cover=None, routes=None):
    """(set_out row, svc_out row of len(svcs)) of one failed link set `w` (two uint64 words) on the state (svcs in record
    order, grid).  cover counts the victims that cross two or more failed links (multi) and the restored victims whose first
    route clear of their OWN failed links crosses another failed link (skip_restored: they were restored on a later route)"""
    c = holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    se, thr = np.asarray(holder.mod_se), np.asarray(holder.mod_thr)
    row, act = np.full(len(nat.FAILURE_SETS), np.nan), np.full(len(svcs), -1, np.int32)
    bits = int(w[0]) | (int(w[1]) << 64)
    failed = {e for e in range(128) if (bits >> e) & 1}
    if not failed or max(failed) >= tb.n_links:
        row[0] = 1
        return row, act
    routes = route_of(tb) if routes is None else routes
    recs = [(int(s["path_id"]), int(s["slot"]), int(s["nslots"]), int(s["modulation"]), int(s["service_id"])) for s in svcs]
    on = [set(path_links_of(tb, r[0]).tolist()) for r in recs]
    victims = [i for i, links in enumerate(on) if links & failed]
    running = [r for r, links in zip(recs, on) if not links & failed]
    grid = grid.copy()
    for i in victims:
        release(grid, tb, *recs[i][:3])
    row[:9] = 0
    row[10], row[11] = 0, len(failed)
    low = np.inf
    for i in victims:
        path, _, n, m, sid = recs[i]
        cap = n * int(se[m])
        nslots = [-(-cap // int(s)) for s in se]
        row[1] += 1
        row[2] += cap
        own = on[i] & failed
        eligible, first_clear_blocked = [], None
        if path in routes:
            s, d, _ = routes[path]
            for k in range(K):
                p = int(tb.pair_paths[s, d, k])
                if p < 0:
                    break
                links = set(path_links_of(tb, p).tolist())
                if first_clear_blocked is None and not links & own:
                    first_clear_blocked = bool(links & failed)
                if not links & failed:
                    eligible.append((k, p))
        if cover is not None:
            cover["multi"] += len(own) >= 2
        hit, evaluated = search(o, tb, thr, margin, nslots, eligible, grid,
                                lambda p, a, nn: gn_running(o, tb, se, running, p, a, nn, sid if ids else None)[0], log)
        if hit is None:
            row[6 if evaluated else 5] += 1
            row[10] += not eligible
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
        if cover is not None:
            cover["skip_restored"] += bool(first_clear_blocked)
    row[9] = low if row[3] else np.nan
    return row, act


def restate_sets(o, tb, holder, margin, svcs, grid, ws, ids=False, log=None, cover=None):
    routes = route_of(tb)
    out = [restate_set(o, tb, holder, margin, svcs, grid, w, ids, log, cover, routes) for w in ws]
    return np.stack([r for r, _ in out]), np.stack([a for _, a in out])


def coverage(want, cover):
    """what a replica's restated scenarios exercise"""
    ok = want[:, 0] == 0
    return dict(evaluated=int(ok.sum()), no_victim=int(np.sum(want[ok, 1] == 0)), restored=int(np.sum(want[ok, 3])),
                lost_ns=int(np.sum(want[ok, 5])), lost_qot=int(np.sum(want[ok, 6])), no_route=int(np.sum(want[ok, 10])),
                **{k: int(cover[k]) for k in COVER})


# ---- the GPU computations -----------------------------------------------------------------------------------------------
def gpu_case(out, key):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb, kw, B, _, how = case_config(key)
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    tb, kw, holder, ors = drive(key, env, oracles=False)      # the oracles only lend `candidates` and `gn_lists`
    E, N = tb.n_links, tb.n_nodes
    W = np.stack([as_words(scenario_lists(tb, r)) for r in range(B)])
    got, svc = env.failure_sets(W, detail=True)
    out[key + "_same_without_detail"] = np.array_equal(env.failure_sets(W), got, equal_nan=True)
    one, one_svc = env.failure_impact(detail=True)
    first = N + len(pair_lists(tb, 0))                               # the E one-link columns
    out[key + "_one_link_same"] = (np.array_equal(got[:, first:first + E, :10], one, equal_nan=True)
                                   and np.array_equal(svc[:, first:first + E], one_svc))
    nodes = as_words(node_lists(tb))
    shared = env.failure_sets(nodes, detail=True)
    tiled = env.failure_sets(np.ascontiguousarray(np.tile(nodes[None], (B, 1, 1))), detail=True)
    lists = env.failure_sets(node_lists(tb), detail=True)
    out[key + "_shared_same"] = all(np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
                                    for a, b, c in zip(shared, tiled, lists))
    out[key + "_shared_is_the_node_columns"] = np.array_equal(shared[0], got[:, :N], equal_nan=True)
    tot, near = {}, 0
    for r, o in enumerate(ors):
        svcs, grid = env.services(r), env.grid(r)
        log, cover = [], dict.fromkeys(COVER, 0)
        want, act = restate_sets(o, tb, holder, replica_margin(kw, r), svcs, grid, W[r], how == "ids", log, cover)
        near += int(np.sum(np.array(log) < BAND))
        k = f"{key}_r{r}"
        out[k + "_got"], out[k + "_svc"], out[k + "_want"], out[k + "_act"], out[k + "_active"] = got[r], svc[r], want, act, len(svcs)
        for name, v in coverage(want, cover).items():
            tot[name] = tot.get(name, 0) + v
    for name, v in tot.items():
        out[f"{key}_cond_{name}"] = v
    out[key + "_B"], out[key + "_E"], out[key + "_N"], out[key + "_F"], out[key + "_band"] = B, E, N, W.shape[1], near
    out[key + "_rec32"] = bool(tb.n_links <= 32 and len(tb.path_hops) <= 512)
    env.close()


NSF = dict(BASE, num_spectrum_resources=128, capacity=192, load=120.0)


def read_only(out, B=32):
    from common import record_bytes
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    kw = dict(NSF, measure_disruptions=True)
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    twin = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    for e in (env, twin):
        e.seed(4)
        e.reset()
        e.step_policy(200, record=False)
    blob0, st0 = env.save_state(), env.stats()
    a = env.failure_sets(env.node_link_sets())
    env.failure_sets(env.link_pair_sets()[:40], detail=True)
    blob1, st1 = env.save_state(), env.stats()
    out["ro_blob_same"] = blob0.tobytes() == blob1.tobytes()
    out["ro_stats_same"] = st0.tobytes() == st1.tobytes()
    out["ro_traj_same"] = record_bytes(env.step_policy(60)) == record_bytes(twin.step_policy(60))
    out["ro_victims"] = int(np.sum(a[:, :, 1]))
    env.close()
    twin.close()


def fresh(out, B=8):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **dict(NSF, capacity=128))
    env.seed(3)
    env.reset()
    out["fresh_rows"], out["fresh_svc"] = env.failure_sets(env.node_link_sets(), detail=True)
    env.close()


def device_io(out, B=32):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    host = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **NSF)
    dev = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, io_device=True, **NSF)
    Cp = host.holder.struct.capacity
    nodes = host.node_link_sets()
    per = np.ascontiguousarray(np.stack([np.roll(host.link_pair_sets()[:9], r, axis=0) for r in range(B)]))
    N = len(nodes)
    nodes_t = torch.from_numpy(nodes.view(np.int64)).cuda()
    t = torch.full((B, N, 12), 7.0, dtype=torch.float64, device="cuda")
    try:
        dev.failure_sets(nodes_t, out=t)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    host.seed(5)
    host.reset()
    host.step_policy(220, record=False)
    want, want_svc = host.failure_sets(nodes, detail=True)
    want_p = host.failure_sets(per)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        dev.seed(5)
        dev.reset()
        dev.step_policy(220, record=False)
        r = dev.failure_sets(nodes_t, out=t)
        t2 = torch.full((B, N, 12), 7.0, dtype=torch.float64, device="cuda")
        s2 = torch.full((B, N, Cp), 7, dtype=torch.int32, device="cuda")
        dev.failure_sets(nodes_t, out=(t2, s2), detail=True)
        t3 = torch.full((B, 9, 12), 7.0, dtype=torch.float64, device="cuda")
        per_t = torch.from_numpy(per.view(np.int64)).cuda()
        dev.failure_sets(per_t.view(torch.uint64) if hasattr(torch, "uint64") else per_t, out=t3)
        stream.synchronize()
        out["dev_same"] = r is t and np.array_equal(t.cpu().numpy(), want, equal_nan=True)
        out["dev_detail_same"] = (np.array_equal(t2.cpu().numpy(), want, equal_nan=True)
                                  and np.array_equal(s2.cpu().numpy(), want_svc))
        out["dev_per_replica_same"] = np.array_equal(t3.cpu().numpy(), want_p, equal_nan=True)
        bad = []
        for args, kws in (((nodes_t.int(),), dict(out=t)),                          # dtype
                          ((torch.from_numpy(nodes.view(np.int64)),), dict(out=t)),     # a host tensor
                          ((nodes,), dict(out=t)),                                      # not a tensor
                          ((nodes_t,), dict()),                                         # no out
                          ((nodes_t,), dict(out=t3)),                                   # out of another F
                          ((per_t[:B - 1],), dict(out=t3)),                             # a list per replica for B - 1 replicas
                          ((nodes_t,), dict(out=t, detail=True)),                       # detail without the pair
                          ((nodes_t,), dict(out=(t, s2.long()), detail=True))):
            try:
                dev.failure_sets(*args, **kws)
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
    same, victims, no_route = True, 0, 0
    edges = list(topology.edges())
    node = edges[0][0]
    index = lambda e: topology[e[0]][e[1]]["index"]      # noqa: E731
    for kws, idx in ((dict(links=[edges[0], edges[3]]), [index(edges[0]), index(edges[3])]),
                     (dict(links=[index(edges[1]), edges[2]]), [index(edges[1]), index(edges[2])]),
                     (dict(node=node), [index((node, v)) for v in topology[node]])):
        d = single.failure_sets_impact(**kws)
        row, svc = single._dev.failure_sets([idx], detail=True)
        same &= list(d)[:12] == list(nat.FAILURE_SETS) and set(d) == set(nat.FAILURE_SETS) | {"restorations", "lost"}
        same &= all((np.isnan(row[0, 0, i]) and np.isnan(d[k])) or float(d[k]) == row[0, 0, i] for i, k in enumerate(nat.FAILURE_SETS))
        same &= all(svc[0, 0, i] == k * M * S + (M - 1 - m) * S + a for i, k, m, a in d["restorations"])
        same &= all(svc[0, 0, i] == c.k_paths * M * S for i in d["lost"])
        same &= d["status"] == 0 and d["failed_links"] == len(set(idx)) and isinstance(d["victims"], int)
        same &= len(d["restorations"]) == d["restored"] and len(d["lost"]) == d["lost_no_spectrum"] + d["lost_qot"]
        victims += d["victims"]
        no_route += d["lost_no_route"]
    for kws in (dict(), dict(links=[0], node=node)):
        try:
            single.failure_sets_impact(**kws)
            same = False
        except ValueError:
            pass
    out["compat_same"], out["compat_victims"], out["compat_no_route"] = bool(same), victims, no_route
    single.close()


def refusals(out):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, **dict(NSF, capacity=128))
    sets, res = np.ones((4, 3, 2), np.uint64), np.zeros((4, 3, 12))
    rc, msg = {}, {}
    call = lambda e, *a: e.lib.ongym_failure_sets(e._h, *a)      # noqa: E731
    for name, args in (("zero", (0, sets.ctypes.data, 1, res.ctypes.data, None)),
                       ("many", (65536, sets.ctypes.data, 1, res.ctypes.data, None)),
                       ("null_sets", (3, None, 1, res.ctypes.data, None)),
                       ("null_out", (3, sets.ctypes.data, 1, None, None)),
                       ("ok", (3, sets.ctypes.data, 1, res.ctypes.data, None)),
                       ("ok_shared", (3, sets.ctypes.data, 0, res.ctypes.data, None))):
        rc[name] = call(env, *args)
        msg[name] = env.lib.ongym_last_error(env._h).decode() if rc[name] else ""
    env.close()
    narrow = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, modulations_to_consider=3, **dict(NSF, capacity=128))
    rc["window"] = call(narrow, 3, sets.ctypes.data, 1, res.ctypes.data, None)
    msg["window"] = narrow.lib.ongym_last_error(narrow._h).decode()
    narrow.close()
    for k, v in rc.items():
        out["refuse_rc_" + k], out["refuse_msg_" + k] = v, msg[k]


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
    print("failure sets child ok")


if __name__ == "__main__":
    main()
