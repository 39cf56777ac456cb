"""Child process of tests/test_gpu_playout.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP runtime
and this library's must start together), saved to an .npz that the tests assert on.

    python tests/playout_child.py OUT.npz

The witness of ongym_playout (include/ongym.h) is the step itself, nothing is restated: a second environment of the same
configuration, created with ONGYM_FORCE_GENERIC=1 (k_run: the device functions the playout kernel reuses), takes the state of
the environment under test with load_state and then, for one (action column a, sample r) at a time and all replicas at once,
    seed(seed + r, replica_base)            (not with own_stream)
    step(actions[:, a])                     (step_policy(1) for the column of -1)
    H x step_policy(1, policy), with stats() and every replica's pending request after each step.
Columns 0-4 and 7 come from the records.  Columns 5 and 6 are sums of the per-step differences of stats()'s
bit_rate_provisioned and bit_rate_requested; bit_rate_requested counts a request when it is drawn, so each difference is
corrected by the pending request's bit rate before and after the step (nothing is pending once stats()'s flags carry
F_NO_REQUEST).  The sums telescope to "after the last step minus after the first step".  The one exception: a terminal step with
auto_reset wipes both counters in the same launch, so that step adds the bit rate of the request it decided (the one pending
before it) directly.  All these are sums of small integers in float64: the comparison is exact.
"""
import copy
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402,F401  (before the library is loaded: the two HIP runtimes must start together)

from admission_map_child import slot_counts  # noqa: E402
from common import golden_tables, jocn_modulations, record_bytes  # noqa: E402
from failure_impact_child import free_row  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402

B, A, R, H = 8, 5, 2, 32
WARM = 300
SEED, PSEED = 31, 1000          # the environments' stream, the playouts' first sample
TRACE_SEED = 46                 # ... and the traces': one for which, on the CPU oracle, rejecting the pending request instead of
                                # placing it changes the number of blocked requests behind it in some replica, at both lengths
NCOL = len(nat.PLAYOUT)
FF, LB = nat.POLICY_FIRST_FIT, nat.POLICY_LOAD_BALANCING
BASE = dict(modulations=jocn_modulations(), bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), auto_reset=True,
            episode_length=10 ** 6, margin=0.0, launch_power_dbm=0.0, num_spectrum_resources=64, capacity=256)
# Loads and slot counts chosen on the CPU with tests/oracle_lib.py: after WARM first-fit steps the blocking rate of the next 64
# requests lies between 0.3 and 0.6 in every replica (S = 64: nsfnet 300 Erlang, nobel-eu 400 Erlang), so that H = 32 sees
# several blocked and several accepted requests; capacity 64 at S = 128 and 400 Erlang keeps most replicas at active == capacity.
CASES = {
    "nsfnet": dict(topo="nsfnet", load=300.0),                                   # R32 records, uniform attenuation
    "nobeleu": dict(topo="nobel-eu", load=400.0),                                # 41 links: the non-R32 codec
    "alpha": dict(topo="alpha", load=300.0),                                     # per-link attenuation: UA = false
    "lb": dict(topo="nsfnet", load=300.0, policy=LB),
    "disrupt": dict(topo="nsfnet", load=300.0, measure_disruptions=True),
    "trace": dict(topo="nsfnet", load=300.0, trace=WARM + 1 + H + 8, own=True),
    "trace_short": dict(topo="nsfnet", load=300.0, trace=WARM + 1 + 20, own=True),   # 20 requests left after the first step
    "own_rng": dict(topo="nsfnet", load=300.0, own=True),
    "episode_reset": dict(topo="nsfnet", load=300.0, episode_length=WARM + 1 + 14, auto_reset=True),
    "episode_stop": dict(topo="nsfnet", load=300.0, episode_length=WARM + 1 + 14, auto_reset=False),
    "full": dict(topo="nsfnet", load=400.0, num_spectrum_resources=128, capacity=64),
    "base": dict(topo="nsfnet", load=300.0, replica_base=5),
}
LEAN_CASE = "nsfnet"            # ... whose witness also runs on the default (lean) kernel


def tables_of(topo):
    if topo == "alpha":
        tb = copy.deepcopy(golden_tables("nsfnet"))
        tb.link_alpha = tb.link_alpha * np.linspace(0.85, 1.2, tb.n_links)
        return tb
    return golden_tables(topo)


def case_kw(cfg):
    kw = dict(BASE)
    for k in ("load", "measure_disruptions", "episode_length", "auto_reset", "num_spectrum_resources", "capacity"):
        if k in cfg:
            kw[k] = cfg[k]
    return kw


def make_trace(tb, kw, n):
    rng = np.random.default_rng(TRACE_SEED)
    reqs = np.zeros((B, n), nat.REQUEST_DTYPE)
    for r in range(B):
        reqs[r]["arrival_time"] = np.cumsum(rng.exponential(10800.0 / kw["load"], n)).astype(np.float32)
        reqs[r]["holding_time"] = rng.exponential(10800.0, n).astype(np.float32)
        src = rng.integers(0, tb.n_nodes, n)
        reqs[r]["source"], reqs[r]["destination"] = src, (src + rng.integers(1, tb.n_nodes, n)) % tb.n_nodes
        reqs[r]["bit_rate"] = rng.choice(np.array(kw["bit_rates"]), n)
    return reqs


def make_env(cfg, generic=False, **over):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb, kw = tables_of(cfg["topo"]), case_kw(cfg)
    if generic:
        os.environ["ONGYM_FORCE_GENERIC"] = "1"       # read at create
    try:
        env = BatchedQRMSAEnv(tables=tb, batch_size=B, **dict(kw, **over))
    finally:
        os.environ.pop("ONGYM_FORCE_GENERIC", None)
    if "trace" in cfg:
        env.set_requests(make_trace(tb, kw, cfg["trace"]))
    else:
        env.seed(SEED, cfg.get("replica_base", 0))
    return env


def warm(env, cfg):
    env.reset()
    env.step_policy(WARM, record=False, policy=cfg.get("policy", FF))


def action_list(env, tb, r):
    """the five actions of a replica: first fit's choice, the reject action, -1, an action whose slots are occupied, and a valid
    action (slots free) on the last route - at the lowest format in even replicas, at the highest usable one in odd replicas,
    where a long route fails on QoT"""
    c = env.holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    reject = K * M * S
    grid, req = env.grid(r), env.request(r)
    nreq = slot_counts(env.holder, [float(req["bit_rate"])])[0]
    routes = [int(p) for p in tb.pair_paths[int(req["source"]), int(req["destination"])] if p >= 0]
    usable = [m for m in range(M) if nreq[m] > 0]
    occupied = valid = reject
    for k, p in enumerate(routes):
        busy = np.flatnonzero(free_row(grid, tb, p) == 0)
        if len(busy) and usable:
            occupied = k * M * S + (M - 1 - usable[-1]) * S + int(busy[0])
            break
    for k in range(len(routes) - 1, -1, -1):
        row = free_row(grid, tb, routes[k])
        for m in (usable if r % 2 == 0 else usable[::-1]):
            n = int(nreq[m])
            starts = [s for s in range(S - n) if row[s:s + n + 1].all()]      # n slots and the guard slot free
            if starts:
                valid = k * M * S + (M - 1 - m) * S + starts[-1]
                break
        if valid != reject:
            break
    return [-2, reject, -1, occupied, valid]            # -2: first fit's choice, filled in by the caller


def stats_of(env):
    """stats() that also answers after a replica has overflowed its service table (the flag is sticky and the call then returns
    ONGYM_E_CAPACITY with the statistics filled in)"""
    st = np.zeros(B, nat.STATS_DTYPE)
    rc = env.lib.ongym_stats_get(env._h, st.ctypes.data)
    assert rc in (0, -4), rc
    return st


def pending(env, st):
    """bit rate of every replica's pending request, 0 where the source has run out"""
    br = np.array([float(env.request(b)["bit_rate"]) for b in range(B)])
    br[(st["flags"] & nat.F_NO_REQUEST) != 0] = 0.0
    return br


def witness(wit, blob, acts, horizon, policy, seeds, base, own, auto_reset):
    """float64 [B, A, len(seeds), 8] through the step itself, and the replicas' `active` at the start"""
    nA = acts.shape[1]
    out = np.full((B, nA, len(seeds), NCOL), np.nan)
    active0 = None
    for r, sd in enumerate(seeds):
        for a in range(nA):
            wit.load_state(blob)
            if active0 is None:
                active0 = stats_of(wit)["active"].copy()
            if not own:
                wit.seed(sd, base)
            col = np.ascontiguousarray(acts[:, a])
            by_policy = bool(np.all(col < 0))
            assert by_policy or np.all(col >= 0)
            rec = wit.step_policy(1, policy=policy)[0] if by_policy else wit.step(col)
            status = np.where(rec["retry"] != 0, 2, np.where(rec["flags"] & nat.F_QOT_ERROR, 3,
                              np.where(rec["flags"] & nat.F_NO_REQUEST, 4, 1 if by_policy else 0)))
            st = stats_of(wit)
            pend = pending(wit, st)
            alive = (status < 2) & (rec["terminated"] == 0)
            first = rec["accepted"].astype(np.float64)
            steps, acc, br_acc, br_req = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
            active_end = rec["active"].astype(np.float64)
            for _ in range(horizon):
                if not alive.any():
                    break
                rec = wit.step_policy(1, policy=policy)[0]
                st1 = stats_of(wit)
                pend1 = pending(wit, st1)
                ran = alive & ((rec["flags"] & nat.F_NO_REQUEST) == 0)
                ok = ran & (rec["accepted"] != 0)
                term = ran & (rec["terminated"] != 0)
                wiped = term & bool(auto_reset)       # the reset of the same launch zeroed both counters
                d_acc = np.where(wiped, np.where(ok, pend, 0.0), st1["bit_rate_provisioned"] - st["bit_rate_provisioned"])
                d_req = np.where(wiped, pend, st1["bit_rate_requested"] - st["bit_rate_requested"] - pend1 + pend)
                steps += ran
                acc += ok
                br_acc += np.where(ran, d_acc, 0.0)
                br_req += np.where(ran, d_req, 0.0)
                active_end = np.where(ran, rec["active"], active_end)
                alive = ran & ~term
                st, pend = st1, pend1
            good = status < 2
            out[:, a, r, 0] = status
            for i, v in enumerate((first, steps, acc, steps - acc, br_acc, br_req, active_end), start=1):
                out[good, a, r, i] = v[good]
    wit.load_state(blob)
    return out, active0


def conditions(want, active0):
    """what a case's witness values exercise (tests/test_gpu_playout.py asserts them)"""
    ok = want[..., 0] < 2
    both = ok & (want[..., 3] > 0) & (want[..., 4] > 0)
    differ = 0
    for b in range(want.shape[0]):
        for r in range(want.shape[2]):
            blocked = want[b, want[b, :, r, 0] == 0, r, 4]
            differ += len(np.unique(blocked)) > 1
    departed = ok & (want[..., 7] < active0[:, None, None] + want[..., 1] + want[..., 3])
    return dict(scenarios=int(ok.sum()), both=int(both.sum()), differ=int(differ), departed=int(departed.sum()),
                **{f"status{s}": int((want[..., 0] == s).sum()) for s in range(5)})


def gpu_case(out, key):
    cfg = CASES[key]
    tb = tables_of(cfg["topo"])
    policy, own, base = cfg.get("policy", FF), bool(cfg.get("own")), cfg.get("replica_base", 0)
    nR = 1 if own else R
    env, wit = make_env(cfg), make_env(cfg, generic=True)
    warm(env, cfg)
    c = env.holder.struct
    out[key + "_rec32_uniform"] = np.array([c.n_links <= 32, not np.any(np.diff(tb.link_alpha))])
    out[key + "_lean"] = np.array([env.occupancy(policy)["lean_kernel"], wit.occupancy(policy)["lean_kernel"]])
    choice = env.policy_actions(FF)[0]
    acts = np.array([action_list(env, tb, r) for r in range(B)], np.int32)
    acts[:, 0] = choice
    blob = env.save_state()
    seeds = [PSEED + r for r in range(nR)]
    kw = dict(horizon=H, policy=policy, samples=nR, seed=PSEED, own_stream=own)
    got = env.playout(acts, **kw)
    want, active0 = witness(wit, blob, acts, H, policy, seeds, base, own, case_kw(cfg)["auto_reset"])
    out[key + "_got"], out[key + "_want"], out[key + "_acts"], out[key + "_active0"] = got, want, acts, active0
    out[key + "_capacity"], out[key + "_reject"] = c.capacity, env.reject_action
    for n, v in conditions(want, active0).items():
        out[f"{key}_cond_{n}"] = v
    # properties
    null = env.playout(None, **kw)
    out[key + "_null_is_minus_one"] = np.array_equal(null[:, 0], got[:, 2], equal_nan=True)
    out[key + "_same_bytes"] = env.playout(acts, **kw).tobytes() == got.tobytes()
    one = np.stack([env.playout(np.ascontiguousarray(acts[:, a:a + 1]), **kw)[:, 0] for a in range(A)], axis=1)
    out[key + "_independent_of_A"] = np.array_equal(one, got, equal_nan=True)
    if not own:
        alone = env.playout(acts, **dict(kw, samples=1, seed=PSEED + 1))
        out[key + "_sample_is_seed"] = np.array_equal(alone[:, :, 0], got[:, :, 1], equal_nan=True)
    out[key + "_state_same"] = env.save_state().tobytes() == blob.tobytes()
    if key == LEAN_CASE:        # the same witness on the default kernel: a k_fast / k_run parity statement
        lean = make_env(cfg)
        out["lean_is_lean"] = lean.occupancy(policy)["lean_kernel"]
        out["lean_want"], _ = witness(lean, blob, acts, H, policy, seeds, base, own, True)
        lean.close()
    if key == "trace_short":    # past the end of the trace: no replica has a pending request
        env.step_policy(40, record=False)
        blob = env.save_state()
        out["exhausted_got"] = env.playout(acts, **kw)
        out["exhausted_want"], _ = witness(wit, blob, acts, H, policy, seeds, base, own, True)
    env.close()
    wit.close()


def read_only(out):
    """an episode that ends inside H, with disruptions measured: the terminal step is the one that writes to memory in k_run"""
    cfg = dict(topo="nsfnet", load=300.0, measure_disruptions=True, episode_length=WARM + 1 + 10, auto_reset=True)
    env, twin = make_env(cfg), make_env(cfg)
    for e in (env, twin):
        warm(e, cfg)
    blob0, st0 = env.save_state(), env.stats()
    acts = np.stack([env.policy_actions()[0], np.full(B, -1, np.int32)], axis=1).astype(np.int32)
    a = env.playout(acts, horizon=H, samples=R, seed=3)
    b = env.playout(None, horizon=H, policy=LB, own_stream=True)
    blob1, st1 = env.save_state(), env.stats()
    out["ro_blob_same"] = blob0.tobytes() == blob1.tobytes()
    out["ro_stats_same"] = st0.tobytes() == st1.tobytes()
    out["ro_traj_same"] = record_bytes(env.step_policy(50)) == record_bytes(twin.step_policy(50))
    out["ro_ended_early"] = int(np.sum(a[..., 2] < H)) + int(np.sum(b[..., 2] < H))
    out["ro_played"] = int(np.nansum(a[..., 2]))
    env.close()
    twin.close()


def device_io(out):
    cfg = CASES["nsfnet"]
    host, dev = make_env(cfg), make_env(cfg, io_device=True)
    warm(host, cfg)
    acts = np.stack([host.policy_actions()[0], np.full(B, -1, np.int32), np.full(B, host.reject_action, np.int32)], axis=1).astype(np.int32)
    want = host.playout(acts, horizon=H, samples=R, seed=9)
    want_null = host.playout(None, horizon=8, policy=LB, own_stream=True)
    t = torch.full((B, 3, R, NCOL), 7.0, dtype=torch.float64, device="cuda")
    try:
        dev.playout(torch.from_numpy(acts).cuda(), horizon=H, samples=R, seed=9, out=t)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        warm(dev, cfg)
        acts_t = torch.from_numpy(acts).cuda()
        r = dev.playout(acts_t, horizon=H, samples=R, seed=9, out=t)
        t1 = torch.full((B, 1, 1, NCOL), 7.0, dtype=torch.float64, device="cuda")
        dev.playout(None, horizon=8, policy=LB, own_stream=True, out=t1)
        stream.synchronize()
        out["dev_same"] = r is t and np.array_equal(t.cpu().numpy(), want, equal_nan=True)
        out["dev_null_same"] = np.array_equal(t1.cpu().numpy(), want_null, equal_nan=True)
        bad = []
        for args, kws in (((acts_t.long(),), dict(out=t)), ((torch.from_numpy(acts),), dict(out=t)), ((acts,), dict(out=t)),
                          ((acts_t,), dict(out=t1)), ((acts_t,), dict(out=t.float())), ((acts_t,), dict(out=None))):
            try:
                dev.playout(*args, horizon=H, samples=R, seed=9, **kws)
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
    single = QRMSAEnv(topology=topology, seed=9, load=600, episode_length=1000, num_spectrum_resources=64, bandwidth=64 * 12.5e9,
                      launch_power_dbm=0.0, margin=0.0, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), gen_observation=False,
                      track_service_ids=False)      # the library refuses playouts where the step tracks service ids
    single.reset()
    for _ in range(200):
        single.step(single.first_fit_action()[0])
    c = single._dev.holder.struct
    reject = c.k_paths * c.n_mods * c.n_slots
    cand = [single.first_fit_action()[0], reject, -1, 0]
    d = single.playout(cand, horizon=H, samples=R, seed=4)
    raw = single._dev.playout(np.array([cand], np.int32), horizon=H, samples=R, seed=4)[0]
    same = isinstance(d, list) and len(d) == len(cand) and all(list(x) == list(nat.PLAYOUT) for x in d)
    for x, rows in zip(d, raw):
        same &= isinstance(x["status"], int) and x["status"] == int(rows[0, 0])
        for i, k in enumerate(nat.PLAYOUT[1:], start=1):
            m = rows[:, i].mean()
            same &= (np.isnan(m) and np.isnan(x[k])) or x[k] == m
    out["compat_same"], out["compat_steps"] = bool(same), int(sum(x["steps"] for x in d if x["status"] < 2))
    single.close()
    vec = QRMSABlockVecEnv(tables=golden_tables("nsfnet"), num_envs=B, blocks_to_consider=4, seed=2, **dict(BASE, load=300.0))
    vec.reset()
    for _ in range(150):
        vec.step(np.argmax(vec.action_masks(), axis=1))
    la = vec.playout_lookahead(horizon=H, samples=4, seed=11)
    mask = vec.action_masks()
    ref = vec.env.playout(np.ascontiguousarray(vec._map, np.int32), horizon=H, samples=4, seed=11)
    val = ((1.0 - ref[..., 1]) + ref[..., 4]).mean(axis=2)
    direct = vec.env.playout(np.full((B, 1), vec.env.reject_action, np.int32), horizon=H, samples=4, seed=11)
    out["look_shape_ok"] = la.shape == (B, vec.n_actions) and la.dtype == np.float64
    out["look_same"] = bool(np.array_equal(la[mask], val[mask]) and not np.any(np.isnan(la[mask])))
    out["look_masked_nan"] = bool(np.all(np.isnan(la[~mask])) and np.any(~mask))
    out["look_reject_is_direct"] = bool(np.array_equal(la[:, -1], (1.0 + direct[:, 0, :, 4]).mean(axis=1)) and np.all(direct[:, 0, :, 0] == 0))
    out["look_spread"] = float(np.nanmax(la) - np.nanmin(la))
    a, b = vec.playout_lookahead(horizon=8, samples=2), vec.playout_lookahead(horizon=8, samples=2)      # seed=None: fresh futures
    out["look_fresh"] = bool(not np.array_equal(a, b, equal_nan=True))
    vec.close()


def refusals(out):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb = golden_tables("nsfnet")
    kw = dict(BASE, load=100.0, capacity=128)
    env = BatchedQRMSAEnv(tables=tb, batch_size=4, **kw)
    res, acts = np.zeros((4, 4096, NCOL)), np.zeros((4, 257), np.int32)
    rc, msg = {}, {}

    def call(name, e, nA, a, hor, pol, nR, flags, o=res):
        rc[name] = e.lib.ongym_playout(e._h, nA, a.ctypes.data if a is not None else None, hor, pol, nR, 0, flags,
                                       o.ctypes.data if o is not None else None)
        msg[name] = e.lib.ongym_last_error(e._h).decode()

    call("no_source", env, 1, None, 8, FF, 1, 0)
    env.seed(1)
    env.reset()
    call("zero_actions", env, 0, acts, 8, FF, 1, 0)
    call("many_actions", env, 257, acts, 8, FF, 1, 0)
    call("zero_samples", env, 1, None, 8, FF, 0, 0)
    call("many_samples", env, 1, None, 8, FF, 65, 0)
    call("zero_horizon", env, 1, None, 0, FF, 1, 0)
    call("long_horizon", env, 1, None, 4097, FF, 1, 0)
    call("many_scenarios", env, 256, acts, 8, FF, 17, 0)
    call("null_actions", env, 2, None, 8, FF, 1, 0)
    call("null_out", env, 1, None, 8, FF, 1, 0, None)
    call("unknown_flags", env, 1, None, 8, FF, 1, 2)
    call("own_stream_samples", env, 1, None, 8, FF, 2, nat.PLAYOUT_OWN_STREAM)
    call("policy", env, 1, None, 8, nat.POLICY_HIGHEST_SNR, 1, 0)
    call("ok", env, 256, acts, 8, FF, 16, 0)
    env.close()
    narrow = BatchedQRMSAEnv(tables=tb, batch_size=4, modulations_to_consider=3, **kw)
    narrow.seed(1)
    narrow.reset()
    call("window", narrow, 1, None, 8, FF, 1, 0)
    narrow.close()
    ids = BatchedQRMSAEnv(tables=tb, batch_size=4, track_service_ids=True, **kw)
    ids.seed(1)
    ids.reset()
    call("track_ids", ids, 1, None, 8, FF, 1, 0)
    ids.close()
    defrag = BatchedQRMSAEnv(tables=tb, batch_size=4, defragmentation=True, n_defrag_services=2, **kw)
    defrag.seed(1)
    defrag.reset()
    call("defragmentation", defrag, 1, None, 8, FF, 1, 0)
    defrag.close()
    trace = BatchedQRMSAEnv(tables=tb, batch_size=4, **kw)
    trace.set_requests(make_trace(tb, kw, 64)[:4])
    trace.reset()
    call("trace_seeded", trace, 1, None, 8, FF, 1, 0)
    call("trace_own_ok", trace, 1, None, 8, FF, 1, nat.PLAYOUT_OWN_STREAM)
    trace.close()
    for k in rc:
        out["refuse_rc_" + k], out["refuse_msg_" + k] = rc[k], msg[k]


def main():
    out = {}
    refusals(out)
    read_only(out)
    device_io(out)
    compat(out)
    for key in CASES:
        gpu_case(out, key)
        print(key, "done", flush=True)
    np.savez(sys.argv[1], **out)
    print("playout child ok")


if __name__ == "__main__":
    main()
