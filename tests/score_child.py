"""Child process of tests/test_gpu_score.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP runtime
and this library's must start together), saved to an .npz that the tests assert on.

    python tests/score_child.py OUT.npz

It also holds the restatement of ongym_score_actions (include/ongym_score.h) in plain numpy, which shares nothing with the device
code: `candidate_table` walks the routes, formats and starts of one pending request from `available` rows, `_get_candidates` and
the GSNR of every candidate (an oracle's on the CPU, the device's own queries on the GPU) and builds the ten features by their
definitions; `expected_scores` scores the table with one weight vector and walks it for the winner.  tests/test_score_host.py
pins the restatement to the oracle's own highest-SNR and first-fit decisions."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402,F401  (before the library is loaded: the two HIP runtimes must start together)

from optical_networking_gym import _native as nat  # noqa: E402

F = len(nat.SCORE_FEATURES)
TIE_BAND = 1e-12               # dB per unit of |w8| + |w9|: the device's band (kTieBandDb, csrc/ongym_device.hpp)
NEAR = 1e-9                    # ... and the distance of the best two distinct scores inside which a winner is not compared
PRESETS = ("first_feasible", "highest_snr", "lowest_margin", "least_slot_hops")


# ---- the restatement ------------------------------------------------------------------------------------------------------
def slot_counts(holder, bit_rate):
    """slots of a request of `bit_rate` under every format (envs/qrmsa.pyx get_number_slots)"""
    c = holder.struct
    width = c.nslots_channel_width if c.nslots_channel_width > 0 else c.channel_width
    return [int(np.ceil(float(bit_rate) / (float(se) * width))) for se in holder.mod_se]


def touch_of(row, s, n):
    """0..2: the cell left of the block is the row's edge or not free, the cell behind the guard slot is the edge or not free"""
    S = len(row)
    e = min(s + n + 1, S)
    return int(s == 0 or row[s - 1] == 0) + int(e == S or row[e] == 0)


def load_of(row, hops):
    return (len(row) - int(np.sum(row))) / hops


def candidate_table(tb, holder, margin, src, dst, nslots, available, candidates, gsnr_many):
    """The candidates of one pending request in walk order (route ascending, format best first, start ascending).
    available(path) -> the route row (1 = free); candidates(row, n) -> the starts of _get_candidates; gsnr_many([(path, s, n)])
    -> GSNR in dB.  Returns dict(x float64 [N, 10] the features, feasible bool [N], path int [N], empty_group: a (route,
    format) with a positive slot count had no start)"""
    c = holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    thr = np.asarray(holder.mod_thr, np.float64)
    rows, keys, empty = [], [], False
    for k in range(K):
        path = int(tb.pair_paths[src, dst, k])
        if path < 0:
            break
        hops = int(tb.path_hops[path])
        row = np.asarray(available(path))
        load = load_of(row, hops)
        for m in range(M - 1, -1, -1):
            n = int(nslots[m])
            if n <= 0:
                continue
            starts = list(candidates(row, n)) if n <= S else []
            empty |= not starts
            for s in starts:
                rows.append([k, hops, M - 1 - m, n, n * hops, s, load, touch_of(row, s, n), np.nan, np.nan])
                keys.append((path, int(s), n, m))
    x = np.array(rows, np.float64).reshape(-1, F)
    feasible = np.zeros(len(keys), bool)
    if keys:
        g = np.asarray(gsnr_many([(p, s, n) for p, s, n, _ in keys]), np.float64).reshape(len(keys))
        need = thr[[m for _, _, _, m in keys]] + float(margin)
        x[:, 8], x[:, 9] = g, g - need
        feasible = g >= need
    return dict(x=x, feasible=feasible, path=np.array([k[0] for k in keys], np.int64), empty_group=bool(empty), K=K, M=M, S=S)


def scores_of(x, w):
    """t = w0 x0, then t = t + wf xf: every product and every sum a float64 operation of its own"""
    t = w[0] * x[:, 0]
    for f in range(1, F):
        t = t + w[f] * x[:, f]
    return t


def expected_scores(table, w):
    """dict(action, best float64 [11], counts int32 [3], index of the winner in the table or -1, near: the best two distinct
    feasible scores lie within NEAR (|w8| + |w9|), where the device's GSNR, a few ulp from the restatement's, may order them
    the other way)"""
    w = np.asarray(w, np.float64)
    x, ok = table["x"], table["feasible"]
    K, M, S = table["K"], table["M"], table["S"]
    t = scores_of(x, w)
    band = TIE_BAND * (abs(w[8]) + abs(w[9]))
    win = -1
    for i in np.flatnonzero(ok):
        if not np.isnan(t[i]) and (win < 0 or t[i] < t[win] - band):
            win = int(i)
    best, flags = np.full(1 + F, np.nan), 0
    if win >= 0:
        action = int(x[win, 0]) * M * S + int(x[win, 2]) * S + int(x[win, 5])
        best[0], best[1:] = t[win], x[win]
    else:
        action = K * M * S
        osnr = bool(np.any(~ok))
        flags = (nat.F_BLOCKED_OSNR if osnr else 0) | (nat.F_BLOCKED_RESOURCES if table["empty_group"] and not osnr else 0)
    u = np.unique(t[ok & ~np.isnan(t)])
    near = bool(len(u) > 1 and u[1] - u[0] <= NEAR * (abs(w[8]) + abs(w[9])))
    return dict(action=action, best=best, counts=np.array([len(x), int(ok.sum()), flags], np.int32), index=win, near=near)


def oracle_table(o, tb, holder, margin):
    """candidate_table of an OracleEnv's pending request"""
    q = o.request()
    return candidate_table(tb, holder, margin, int(q["source"]), int(q["destination"]), slot_counts(holder, q["bit_rate"]),
                           o.available, o.candidates, lambda cands: o.gn_many(cands)[:, 0])


def device_table(env, r, margin):
    """candidate_table of replica r's pending request from the device's own queries"""
    q = env.request(r)
    return candidate_table(env.tables, env.holder, margin, int(q["source"]), int(q["destination"]),
                           slot_counts(env.holder, q["bit_rate"]), lambda p: env.available_slots(r, p), env.candidates,
                           lambda cands: env.gsnr_many(r, cands)[:, 0])


def weight_rows(holder, B):
    """B weight vectors: the four presets, then rows drawn with default_rng(900 + r): odd r small integers with w8 = w9 = 0
    (every score exact, ties frequent), even r normal deviates on all ten features"""
    c = holder.struct
    rows = [nat.score_preset(n, c.n_mods, c.n_slots) for n in PRESETS]
    for r in range(len(rows), B):
        rng = np.random.default_rng(900 + r)
        if r % 2:
            w = rng.integers(-3, 4, F).astype(np.float64)
            w[8] = w[9] = 0.0
        else:
            w = rng.normal(size=F)
        rows.append(w)
    return np.array(rows[:B], np.float64)


# ---- the GPU child --------------------------------------------------------------------------------------------------------
def margins_of(env):
    kw = env.holder._keep
    return np.asarray(kw["rmargin"], np.float64) if "rmargin" in kw else np.full(env.batch_size, env.holder.struct.margin)


def compare(out, k, env, tables=None):
    """score_actions with every rotation of the weight rows (each replica meets each row) against the restatement of every
    replica (tables: from an oracle twin; None: from the device's own queries); the highest-SNR preset against the fused
    policy; a shared row against the same row tiled"""
    B = env.batch_size
    mg = margins_of(env)
    if tables is None:
        tables = [device_table(env, r, mg[r]) for r in range(B)]
    W = weight_rows(env.holder, B)
    keys = ("actions", "best", "counts")
    got, want = {n: [] for n in keys}, {n: [] for n in keys + ("near",)}
    for j in range(B):
        Wj = np.roll(W, j, axis=0)
        a, b, c = env.score_actions(Wj, detail=True)
        for n, v in zip(keys, (a, b, c)):
            got[n].append(v)
        e = [expected_scores(tables[r], Wj[r]) for r in range(B)]
        want["actions"].append(np.array([x["action"] for x in e], np.int32))
        want["best"].append(np.stack([x["best"] for x in e]))
        want["counts"].append(np.stack([x["counts"] for x in e]))
        want["near"].append(np.array([x["near"] for x in e]))
    for n in keys:
        out[f"{k}_{n}"] = np.stack(got[n])
    for n in want:
        out[f"{k}_want_{n}"] = np.stack(want[n])
    out[f"{k}_weights"] = W
    out[f"{k}_feasible"] = np.array([int(t["feasible"].sum()) for t in tables])
    out[f"{k}_margin_gap"] = min([float(np.min(np.abs(t["x"][:, 9]))) for t in tables if len(t["x"])] + [np.inf])
    pa, pf = env.policy_actions(nat.POLICY_HIGHEST_SNR)
    hs = env.score_preset("highest_snr")
    a, _, c = env.score_actions(hs, detail=True)
    out[f"{k}_policy_actions"], out[f"{k}_policy_flags"], out[f"{k}_hs_actions"], out[f"{k}_hs_flags"] = pa, pf, a, c[:, 2]
    for j, w in enumerate(W[:6]):
        s, t = env.score_actions(w, detail=True), env.score_actions(np.tile(w, (B, 1)), detail=True)
        out[f"{k}_shared_{j}"] = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(s, t))
        out[f"{k}_plain_{j}"] = np.array_equal(env.score_actions(w), s[0])
    return tables


def definition_case(out, key, B):
    from spectrum_map_child import DEFINITIONS, drive, make
    tb, kw = DEFINITIONS[key]
    env = make(tb, batch_size=B, **kw)
    drive(env, 31)
    out[f"def_{key}_rec32"] = bool(env.tables.n_links <= 32 and env.tables.n_paths <= 512)
    compare(out, f"def_{key}", env)
    env.close()


def oracle_twin(out, B=8):
    """first fit only, which the oracle reproduces step for step: the restatement fed by the oracle twins, with a margin per
    replica, the largest of which no candidate clears (the replica blocks on QoT)"""
    from common import golden_tables
    from oracle_lib import OracleEnv
    from spectrum_map_child import make
    kw = dict(num_spectrum_resources=320, capacity=448, load=300.0, replica_margin=np.linspace(0.0, 20.0, B))
    env = make("nsfnet", batch_size=B, **kw)
    env.seed(41)
    env.reset()
    rec = env.step_policy(260)
    tables, same = [], True
    for r in range(B):
        o = OracleEnv(env.holder, replica=r)
        o.seed(41)
        o.reset()
        want = o.run_first_fit(260)
        same &= all(np.array_equal(rec[f][:, r], want[f]) for f in ("action", "slot", "modulation", "accepted", "active"))
        tables.append(oracle_table(o, golden_tables("nsfnet"), env.holder, margins_of(env)[r]))
    out["twin_same_trajectory"] = same
    compare(out, "twin", env, tables)
    env.close()


def step_loop(out, B=16, steps=40):
    from spectrum_map_child import make
    env = make("nsfnet", batch_size=B, num_spectrum_resources=320, capacity=448, load=300.0, replica_margin=np.linspace(0.0, 1.5, B))
    env.seed(13)
    env.reset()
    env.step_policy(220, record=False)
    W = weight_rows(env.holder, B)
    blob = env.save_state()
    st0 = env.stats()
    a0 = env.score_actions(W, detail=True)
    out["loop_last_kernel_ms"] = env.last_kernel_ms()
    out["loop_blob_same"] = env.save_state().tobytes() == blob.tobytes()
    st1 = env.stats()
    out["loop_stats_same"] = all(np.array_equal(st0[f], st1[f], equal_nan=True) for f in st0.dtype.names)
    a1 = env.score_actions(W, detail=True)
    out["loop_repeatable"] = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a0, a1))
    acts, recs = [], []
    for _ in range(steps):
        a = env.score_actions(W)
        acts.append(a)
        recs.append(env.step(a))
    rec = np.stack(recs)
    out["loop_actions"], out["loop_reject"] = np.stack(acts), env.reject_action
    for f in ("action", "accepted", "retry", "flags"):
        out["loop_rec_" + f] = rec[f]
    out["loop_audit"] = env.check_state()
    env.close()


def after_cut(out, B=16):
    from spectrum_map_child import make
    env = make("nsfnet", batch_size=B, num_spectrum_resources=320, capacity=448, load=300.0)
    env.seed(17)
    env.reset()
    env.step_policy(250, record=False)
    E = env.holder.struct.n_links
    sets = [[r % E, (5 * r + 3) % E, (7 * r + 1) % E] for r in range(B)]
    env.cut_links(sets)
    compare(out, "cut", env)
    tb, c = env.tables, env.holder.struct
    crossed = []
    for j in range(B):
        for r in range(B):
            a = int(out["cut_actions"][j, r])
            if a == env.reject_action:
                continue
            q = env.request(r)
            path = int(tb.pair_paths[int(q["source"]), int(q["destination"]), a // (c.n_mods * c.n_slots)])
            crossed.append(bool(set(tb.path_links[path, :tb.path_hops[path]].tolist()) & set(sets[r])))
    out["cut_crossed"], out["cut_winners"] = np.array(crossed), len(crossed)
    out["cut_failed"] = env.failed_links()
    env.close()


def device_io(out, B=8):
    from spectrum_map_child import make, on_device
    kw = dict(num_spectrum_resources=100, capacity=256, load=140.0)
    host = make("nsfnet", batch_size=B, **kw)
    host.seed(29)
    host.reset()
    host.step_policy(240, record=False)
    W = weight_rows(host.holder, B)
    want = host.score_actions(W, detail=True)
    want_shared = host.score_actions(W[3])
    blob = host.save_state()
    dev = make("nsfnet", io_device=True, batch_size=B, **kw)

    def run():
        dev.load_state(torch.from_numpy(blob).cuda())
        t = (torch.full((B,), 7, dtype=torch.int32, device="cuda"), torch.full((B, 1 + F), 7.0, dtype=torch.float64, device="cuda"),
             torch.full((B, 3), 7, dtype=torch.int32, device="cuda"))
        ret = dev.score_actions(torch.from_numpy(W).cuda(), out=t, detail=True)
        a = torch.full((B,), 7, dtype=torch.int32, device="cuda")
        ret1 = dev.score_actions(torch.from_numpy(W[3].copy()).cuda(), out=a)
        bad = []
        for call in (lambda: dev.score_actions(torch.from_numpy(W).cuda()),                                  # no out
                     lambda: dev.score_actions(W, out=a),                                                      # numpy weights
                     lambda: dev.score_actions(torch.from_numpy(W).cuda().float(), out=a),                     # dtype
                     lambda: dev.score_actions(torch.from_numpy(W), out=a),                                    # a host tensor
                     lambda: dev.score_actions(torch.from_numpy(W[:, :9].copy()).cuda(), out=a),               # shape
                     lambda: dev.score_actions(torch.from_numpy(W).cuda(), out=a.long()),                      # out dtype
                     lambda: dev.score_actions(torch.from_numpy(W).cuda(), out=a, detail=True),                # detail wants a triple
                     lambda: dev.score_actions(torch.from_numpy(W).cuda(), out=t[:2], detail=True)):           # too short
            try:
                call()
                bad.append(False)
            except ValueError:
                bad.append(True)
        return [x.cpu().numpy() for x in t], all(x is y for x, y in zip(ret, t)), a.cpu().numpy(), ret1 is a, np.array(bad)
    got, is_out, got_shared, is_out1, bad = on_device(dev, run)
    for n, g, w in zip(("actions", "best", "counts"), got, want):
        out[f"dev_{n}"], out[f"dev_want_{n}"] = g, w
    out["dev_is_out"], out["dev_shared"], out["dev_want_shared"], out["dev_shared_is_out"], out["dev_refusals"] = \
        is_out, got_shared, want_shared, is_out1, bad
    try:
        dev.score_actions(torch.from_numpy(W).cuda(), out=torch.zeros(B, dtype=torch.int32, device="cuda"))
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    host.close()
    dev.close()


def refusals(out, B=2):
    from spectrum_map_child import make
    env = make("nsfnet", batch_size=B, num_spectrum_resources=320, capacity=448, load=300.0)
    env.seed(3)
    env.reset()
    lib, h = env.lib, env._h
    w = env.score_preset("highest_snr")
    a = np.full(B, 7, np.int32)
    codes, texts = [], []

    def raw(name, *args):
        codes.append(lib.ongym_score_actions(*args))
        texts.append(lib.ongym_last_error(args[0]).decode() if args[0] else "")
        out["refuse_" + name] = codes[-1]
        out["refuse_" + name + "_msg"] = texts[-1]
    raw("null_env", None, w.ctypes.data, 0, a.ctypes.data, None, None)
    raw("null_actions", h, w.ctypes.data, 0, None, None, None)
    raw("null_weights", h, None, 0, a.ctypes.data, None, None)
    for name, v in (("nan", np.nan), ("inf", np.inf), ("minus_inf", -np.inf)):
        bad = np.tile(w, (B, 1))
        bad[B - 1, 4] = v
        raw("weight_" + name, h, bad.ctypes.data, 1, a.ctypes.data, None, None)
    out["refuse_actions_untouched"] = bool(np.all(a == 7))
    out["refuse_ok_after"] = lib.ongym_score_actions(h, w.ctypes.data, 0, a.ctypes.data, None, None)
    env.close()
    window = make("nsfnet", batch_size=B, num_spectrum_resources=320, capacity=448, load=300.0, modulations_to_consider=3)
    window.seed(3)
    window.reset()
    raw("window", window._h, w.ctypes.data, 0, a.ctypes.data, None, None)
    try:
        window.score_actions(w)
        out["refuse_window_python"] = False
    except ValueError:
        out["refuse_window_python"] = True
    window.close()
    # 14 bytes per record: the state block of 11 200 records fits the 160 KiB of a compute unit, the field behind it does not
    big = make("nsfnet", batch_size=B, num_spectrum_resources=320, capacity=11200, load=300.0)
    big.seed(3)
    big.reset()
    raw("lds", big._h, w.ctypes.data, 0, a.ctypes.data, None, None)
    big.close()


def example(out, B=16):
    sys.path.insert(0, os.path.join(REPO, "examples"))
    import weighted_policy_search as ex
    lines = []
    res = ex.search(batch=B, generations=2, steps=40, load=1500.0, warmup=400, seed=5, log=lines.append, keep_records=True)
    out["ex_blocking"] = np.array(res["blocking"])
    out["ex_recount"] = np.array([[np.sum(rec["accepted"][:, r] == 0) / len(rec) for r in range(B)] for rec in res["records"]])
    out["ex_actions_differ"] = bool(np.any(res["records"][0]["action"] != res["records"][0]["action"][:, :1]))
    out["ex_weights_shape"], out["ex_lines"] = np.array(res["weights"][-1].shape), len(lines)
    # the population's premise: after the fork every replica holds the same pending request, whatever its row decided before
    env = ex.make_env(B, warmup=150, seed=5)
    W = weight_rows(env.holder, B)
    same = True
    for _ in range(6):
        env.step(env.score_actions(W))
        q = [env.request(r) for r in range(B)]
        same &= all(x == q[0] for x in q)
    out["ex_same_requests"] = bool(same)
    env.close()


def single(out):
    """QRMSAEnv.score_action and heuristics.heuristic_weighted on the single environment"""
    from common import jocn_modulations
    from optical_networking_gym.envs.qrmsa import QRMSAEnv
    from optical_networking_gym.heuristics import heuristics
    from optical_networking_gym.topology import bundled_topology_path, get_topology
    topology = get_topology(bundled_topology_path("nsfnet_chen.txt"), None, jocn_modulations(), 80, 0.2, 4.5, 5)
    env = QRMSAEnv(topology=topology, seed=9, load=300, episode_length=1000, num_spectrum_resources=320, launch_power_dbm=1.0,
                   margin=0.5, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), gen_observation=False)
    env.reset()
    same, named = [], []
    for i in range(120):
        if i % 10 == 0:
            d = env.score_action("highest_snr")
            p = env.policy_action(nat.POLICY_HIGHEST_SNR)
            same.append((d["action"], d["blocked_resources"], d["blocked_osnr"]) == tuple(p)
                        and heuristics.heuristic_weighted(env, "highest_snr") == tuple(p)
                        and heuristics.heuristic_weighted(env, nat.score_preset("highest_snr", 6, 320)) == tuple(p))
            d = env.score_action(nat.score_weights(start=1, touch=-50))
            named.append(set(d) == {"action", "blocked_resources", "blocked_osnr", "candidates", "feasible", "score", *nat.SCORE_FEATURES}
                         and (d["score"] is None or (isinstance(d["start"], int) and d["score"] == d["start"] - 50 * d["touch"]
                                                     and d["feasible"] <= d["candidates"])))
        env.step(env.first_fit_action()[0])
    out["single_same"], out["single_named"] = np.array(same), np.array(named)
    env.close()


def main():
    out = {}
    for key, B in (("ring4", 8), ("nsfnet100", 16), ("nsfnet320", 16), ("nobeleu320", 8), ("germany100", 8)):
        definition_case(out, key, B)
        print(key, "done", flush=True)
    oracle_twin(out)
    step_loop(out)
    after_cut(out)
    device_io(out)
    refusals(out)
    example(out)
    single(out)
    np.savez(sys.argv[1], **out)
    print("score child ok")


if __name__ == "__main__":
    main()
