"""Child process of tests/test_gpu_state.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP runtime and
this library's must start together), saved to an .npz that the tests assert on.

    python tests/state_child.py OUT.npz

Covers ongym_state_save / ongym_state_load / ongym_fork (BatchedQRMSAEnv.save_state / load_state / fork): replays from a saved
state against the reference's golden trajectories, a fork pinned to them, overlapping forks on the device stream against an
unforked twin, the two flags, and loads across environments (with the refusals).
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402

from common import golden_tables, jocn_modulations, load_traj, record_bytes, traj_requests  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv  # noqa: E402

TRAJ = ("traj_nsfnet320", "traj_nobeleu320", "traj_nsfnet320_defrag", "traj_nsfnet320_disr")
TOTALS = ("total_steps", "total_accepted", "total_gn_evals", "total_interferer_terms", "total_paths_tried", "total_path_hops",
          "total_gn_shortcuts", "total_active_sum")
RNG_KW = dict(num_spectrum_resources=320, capacity=512, load=300, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400),
              episode_length=1000)


def make_env(meta, batch=1, **over):
    """the environment of a golden trajectory, as the reference's run was configured"""
    kw = dict(tables=golden_tables(meta["topology"]), modulations=jocn_modulations(), batch_size=batch,
              num_spectrum_resources=meta["S"], episode_length=meta["episode_length"], load=meta["load"],
              mean_service_holding_time=meta["mean_holding"], bit_rate_selection=meta["bit_rate_selection"],
              bit_rates=tuple(meta["bit_rates"]), bit_rate_lower_bound=25, bit_rate_higher_bound=100,
              launch_power_dbm=meta["launch_power_dbm"], frequency_start=meta["frequency_start"],
              frequency_slot_bandwidth=meta["slot_bw"], margin=meta["margin"], capacity=1024,
              nslots_channel_width=meta.get("nslots_channel_width", 0.0))
    if meta.get("defragmentation"):
        kw.update(defragmentation=True, n_defrag_services=meta["n_defrag_services"])
    if meta.get("measure_disruptions"):
        kw.update(measure_disruptions=True)
    kw.update(over)
    return BatchedQRMSAEnv(**kw)


def traj_env(meta, rows, batch):
    """rows: REQUEST_DTYPE [batch, n] trace; the setup of the reference's run (resets before the first step)"""
    env = make_env(meta, batch=batch, auto_reset=True)
    env.set_requests(rows)
    for _ in range(meta["initial_resets"]):
        env.reset()
    return env


def stats_wo_totals(st):
    return [st[f].copy() for f in st.dtype.names if f not in TOTALS]


def same_stats(a, b):
    return all(np.array_equal(x, y) for x, y in zip(stats_wo_totals(a), stats_wo_totals(b)))


def grids(env, replicas):
    return np.stack([env.grid(r) for r in replicas])


def replay(out):
    """step K, save, step to the end, load, step to the end again: both continuations (and the first K steps) vs golden"""
    for tag in TRAJ:
        meta, d = load_traj(tag)
        n, B = meta["n_steps"], 3
        K = n // 3
        env = traj_env(meta, np.tile(traj_requests(d), (B, 1)), B)
        out[tag + "_lean"] = env.occupancy()["lean_kernel"]
        r1 = env.step_policy(K)
        blob = env.save_state()
        rA = env.step_policy(n - K)
        gA, sA = grids(env, range(B)), env.stats()
        env.load_state(blob)
        rB = env.step_policy(n - K)
        gB, sB = grids(env, range(B)), env.stats()
        out[tag + "_recA"] = np.concatenate([r1, rA])
        out[tag + "_recB"] = np.concatenate([r1, rB])
        out[tag + "_bits_same"] = record_bytes(rA) == record_bytes(rB)
        out[tag + "_grids_same"] = np.array_equal(gA, gB)
        out[tag + "_stats_same"] = same_stats(sA, sB)
        out[tag + "_totals_count"] = bool(np.all(sB["total_steps"] == sA["total_steps"] + (n - K)) and
                                          np.all(sB["total_accepted"] >= sA["total_accepted"]))
        out[tag + "_K"] = K
        env.close()


def fork_pinned(out):
    """replica 0 carries the golden trace, the others other requests for their first K rows: fork(0) puts them all on it"""
    tag = "traj_nsfnet320"
    meta, d = load_traj(tag)
    n, B, K = meta["n_steps"], 4, 400
    gold = traj_requests(d)
    rows = np.tile(gold, (B, 1))
    for j in range(1, B):
        rows[j, :K]["source"], rows[j, :K]["destination"] = gold[:K]["destination"], gold[:K]["source"]
        rows[j, :K]["bit_rate"] = np.roll(gold[:K]["bit_rate"], j)
    recs = {}
    for forked in (False, True):
        env = traj_env(meta, rows, B)
        env.step_policy(K)
        if forked:
            env.fork(np.zeros(B, np.int32))
        recs[forked] = env.step_policy(n - K)
        env.close()
    out["pin_K"] = K
    out["pin_rec_fork"] = recs[True]
    out["pin_rec_nofork"] = recs[False]


def io_env(batch, seed=11, **over):
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=batch, io_device=True,
                          **dict(RNG_KW, **over))
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    env.seed(seed)
    env.reset()
    return env


def io_step(env, n):
    recs = torch.empty((n, env.batch_size, nat.STEP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    env.step_policy(n, out_device_ptr=recs.data_ptr())
    return recs.cpu().numpy().view(nat.STEP_DTYPE)[..., 0]


def io_observe(env):
    c = env.holder.struct
    obs = torch.empty((env.batch_size, 3 + c.k_paths + c.k_paths * c.n_mods_consider * 12), dtype=torch.float32, device="cuda")
    mask = torch.empty((env.batch_size, env.num_actions), dtype=torch.uint8, device="cuda")
    env._check(env.lib.ongym_observe(env._h, obs.data_ptr(), mask.data_ptr()), "observe")
    return obs.cpu().numpy(), mask.cpu().numpy()


def overlap(out):
    """forks with every kind of overlap on the device stream; F[j] follows twin T[m[j]] (m composed over the forks)"""
    B, N = 64, 40
    F, T = io_env(B), io_env(B)
    io_step(F, 150), io_step(T, 150)
    m = np.arange(B)
    cyc = np.arange(B)
    cyc[[0, 1, 2]] = [1, 2, 0]
    mix = np.arange(B)
    mix[::3] = -1
    mix[1::7] = B + 5
    mix[2::5] = np.arange(B)[::-1][2::5]
    ok = []
    for name, src in (("reverse", np.arange(B)[::-1].copy()), ("cycle3", cyc), ("mix", mix)):
        F.fork(torch.tensor(src, dtype=torch.int32, device="cuda"))
        eff = np.where((src < 0) | (src >= B), np.arange(B), src)
        m = m[eff]
        rf, rt = io_step(F, N), io_step(T, N)
        of, mf = io_observe(F)
        ot, mt = io_observe(T)
        rec_ok = all(record_bytes(rf[:, j]) == record_bytes(rt[:, m[j]]) for j in range(B))
        obs_ok = np.array_equal(of, ot[m]) and np.array_equal(mf, mt[m])
        moved = int(np.sum(m != np.arange(B)))
        ok.append((name, rec_ok, obs_ok, moved))
        out[f"overlap_{name}_rec"] = rec_ok
        out[f"overlap_{name}_obs"] = obs_ok
        out[f"overlap_{name}_moved"] = moved
    # unchanged replicas of the last fork: their records and grids before and after it are the same bytes
    keep = np.where((mix < 0) | (mix >= B))[0]
    before = np.stack([F.grid(int(j)) for j in keep])
    F.fork(torch.tensor(mix, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    after = np.stack([F.grid(int(j)) for j in keep])
    out["overlap_unchanged_grids"] = np.array_equal(before, after)
    out["overlap_keep_count"] = len(keep)
    F.close(), T.close()


def keep_stream(out):
    """keep_stream: the fork serves the source's pending request, then draws from the destination's own stream at the SOURCE's
    counter.  The source (replica 0) is reset KS_SHIFT more times than the others first, so its counter is ahead by that much:
    destination j's requests are then twin j's requests KS_SHIFT steps later."""
    B, K, N, D = 6, 200, 25, 3
    mk = lambda: BatchedQRMSAEnv(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=B, **RNG_KW)
    F, T = mk(), mk()
    only0 = np.zeros(B, np.uint8)
    only0[0] = 1
    for e in (F, T):
        e.seed(5)
        e.reset()
        for _ in range(D):           # each reset draws one request
            e.reset(only0)
        e.step_policy(K, record=False)
    F.fork(np.zeros(B, np.int32), keep_stream=True)
    out["ks_grid_is_source"] = all(np.array_equal(F.grid(j), T.grid(0)) for j in range(B))
    out["ks_pending_is_source"] = all(F.request(j).tobytes() == T.request(0).tobytes() for j in range(B))
    rf, rt = [], []
    for _ in range(N):
        F.step_policy(1, record=False), T.step_policy(1, record=False)
        rf.append([F.request(j) for j in range(B)])
        rt.append([T.request(j) for j in range(B)])
    rf, rt = np.array(rf, nat.REQUEST_DTYPE), np.array(rt, nat.REQUEST_DTYPE)
    out["ks_req_fork"], out["ks_req_twin"], out["ks_shift"] = rf, rt, D
    F.close(), T.close()


def lean_guard(out):
    """a blob saved from a trace the lean kernels cannot replay (bit rates outside the table, services wider than the lean
    tables) keeps the destination on the generic kernels: it then follows a generic-only twin that loaded the same blob"""
    mk = lambda: BatchedQRMSAEnv(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=2, **RNG_KW)
    A = mk()
    rng = np.random.default_rng(4)
    n, nn = 700, A.holder.struct.n_nodes
    reqs = np.zeros((2, n), nat.REQUEST_DTYPE)
    reqs["arrival_time"] = np.cumsum(rng.exponential(36.0, (2, n)), axis=1).astype(np.float32)
    reqs["holding_time"] = rng.exponential(10800.0, (2, n)).astype(np.float32)
    reqs["bit_rate"] = rng.choice([100.0, 200.0, 400.0, 3200.0], (2, n))
    src = rng.integers(0, nn, (2, n))
    reqs["source"], reqs["destination"] = src, (src + rng.integers(1, nn, (2, n))) % nn
    A.set_requests(reqs)
    A.reset()
    A.step_policy(400, record=False)
    blob = A.save_state()
    out["guard_src_lean"] = A.occupancy()["lean_kernel"]
    out["guard_max_nslots"] = max(int(A.services(r)["nslots"].max()) for r in range(2))
    Bv = mk()
    Bv.seed(3)
    Bv.reset()
    out["guard_lean_before"] = Bv.occupancy()["lean_kernel"]
    Bv.load_state(blob)
    out["guard_lean_after"] = Bv.occupancy()["lean_kernel"]
    os.environ["ONGYM_FORCE_GENERIC"] = "1"
    G = mk()
    del os.environ["ONGYM_FORCE_GENERIC"]
    G.seed(3)
    G.reset()
    G.load_state(blob)
    ok = True
    for policy, steps in ((nat.POLICY_FIRST_FIT, 150), (nat.POLICY_LOWEST_FRAGMENTATION, 40), (nat.POLICY_LOAD_BALANCING, 40)):
        ok &= record_bytes(Bv.step_policy(steps, policy=policy)) == record_bytes(G.step_policy(steps, policy=policy))
    out["guard_follows_generic"] = ok
    A.close(), Bv.close(), G.close()


def gsnr_cands(env, replica, n=4, want=6):
    """free candidates (path, slot, nslots) of a replica"""
    cands = []
    for p in range(0, env.holder.struct.n_paths, 7):
        row = env.available_slots(replica, p)
        for s in range(0, len(row) - n):
            if row[s:s + n].all():
                cands.append((p, s, n))
                break
        if len(cands) >= want:
            break
    return cands


def keep_params(out):
    """keep_params: after a fork the destination's GSNR follows the source's launch power, or with the flag its own"""
    B, K, Pa, Pb = 4, 300, 0.0, 3.0
    lps = [Pa, Pb, Pa, Pb]
    res = {}
    for flag in (False, True):
        env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=B,
                              replica_launch_power_dbm=lps, **RNG_KW)
        env.seed(9)
        env.reset()
        env.step_policy(K, record=False)
        env.fork(np.array([0, 0, -1, -1], np.int32), keep_params=flag)
        cands = gsnr_cands(env, 0)
        res[flag] = (np.array([env.gsnr(0, *c) for c in cands]), np.array([env.gsnr(1, *c) for c in cands]))
        env.close()
    out["kp_src_noflag"], out["kp_dst_noflag"] = res[False]
    out["kp_src_flag"], out["kp_dst_flag"] = res[True]
    out["kp_shift_db"] = 10 * np.log10(10 ** ((Pb - 30) / 10) / 10 ** ((Pa - 30) / 10))
    # the same through load_state into a second environment with another scalar launch power
    A = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=2, launch_power_dbm=Pa,
                        **RNG_KW)
    A.seed(3)
    A.reset()
    A.step_policy(K, record=False)
    blob = A.save_state([0])
    cands = gsnr_cands(A, 0)
    src = np.array([A.gsnr(0, *c) for c in cands])
    got = {}
    for flag in (False, True):
        Bv = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=3,
                             launch_power_dbm=Pb, **RNG_KW)
        Bv.seed(4)
        Bv.reset()
        Bv.load_state(blob, [2], keep_params=flag)
        got[flag] = np.array([Bv.gsnr(2, *c) for c in cands])
        Bv.close()
    A.close()
    out["kpl_src"], out["kpl_noflag"], out["kpl_flag"] = src, got[False], got[True]


def raw_load(env, blob, count, replicas, flags=0):
    r = None if replicas is None else np.ascontiguousarray(replicas, np.int32)
    return env.lib.ongym_state_load(env._h, count, None if r is None else r.ctypes.data, blob.ctypes.data, flags)


def across(out):
    """save a subset of B = 64, load it into chosen replicas of B = 128; refusals; the lean paths after a load"""
    save_idx, load_idx = [5, 17, 40, 63], [100, 3, 64, 127]
    for wide in (False, True):
        if wide:
            os.environ["ONGYM_FORCE_WIDE"] = "1"
        mk = lambda B, seed: BatchedQRMSAEnv(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=B,
                                             **RNG_KW)
        A, Bv = mk(64, 0), mk(128, 0)
        A.seed(21), Bv.seed(22)
        A.reset(), Bv.reset()
        A.step_policy(250, record=False), Bv.step_policy(100, record=False)
        blob = A.save_state(save_idx)
        Bv.load_state(blob, load_idx)
        tag = "wide" if wide else "narrow"
        out[f"across_{tag}_lean"] = A.occupancy()["lean_kernel"] and Bv.occupancy()["lean_kernel"]
        ra, rb = A.step_policy(120), Bv.step_policy(120)
        ok = all(record_bytes(ra[:, i]) == record_bytes(rb[:, j]) for i, j in zip(save_idx, load_idx))
        ra, rb = A.step_policy(60, policy=nat.POLICY_LOWEST_FRAGMENTATION), Bv.step_policy(60, policy=nat.POLICY_LOWEST_FRAGMENTATION)
        ok10 = all(record_bytes(ra[:, i]) == record_bytes(rb[:, j]) for i, j in zip(save_idx, load_idx))
        sa, sb = A.stats(), Bv.stats()
        out[f"across_{tag}_p0"] = ok
        out[f"across_{tag}_p10"] = ok10
        out[f"across_{tag}_stats"] = all(same_stats(sa[i:i + 1], sb[j:j + 1]) for i, j in zip(save_idx, load_idx))
        if wide:
            del os.environ["ONGYM_FORCE_WIDE"]
            A.close(), Bv.close()
            continue
        # refusals (the raw entry point, so that the library's own checks are reached)
        refusals = {}
        for name, kw in (("slots", dict(num_spectrum_resources=160)), ("capacity", dict(capacity=576)),
                         ("topology", dict(tables=golden_tables("nobel-eu")))):
            other = BatchedQRMSAEnv(**dict(dict(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=8,
                                                **RNG_KW), **kw))
            refusals[name] = raw_load(other, blob, 4, [0, 1, 2, 3])
            other.close()
        refusals["count"] = raw_load(Bv, blob, 3, [0, 1, 2])
        refusals["duplicate"] = raw_load(Bv, blob, 4, [0, 1, 1, 2])
        bad = blob.copy()
        bad[0] ^= 0xFF
        refusals["magic"] = raw_load(Bv, bad, 4, [0, 1, 2, 3])
        bad = blob.copy()
        bad[16] ^= 0x01     # the fingerprint
        refusals["fingerprint"] = raw_load(Bv, bad, 4, [0, 1, 2, 3])
        src = np.arange(128, dtype=np.int32)
        src[7] = 128
        refusals["fork_src"] = Bv.lib.ongym_fork(Bv._h, src.ctypes.data, 0)
        try:
            Bv.load_state(blob[:200], [0, 1, 2, 3])
            refusals["truncated"] = 0
        except ValueError:
            refusals["truncated"] = -1
        for k, v in refusals.items():
            out[f"refuse_{k}"] = v
        # a refused call changed nothing: the loaded replicas still follow A
        ra, rb = A.step_policy(30), Bv.step_policy(30)
        out["across_after_refusals"] = all(record_bytes(ra[:, i]) == record_bytes(rb[:, j]) for i, j in zip(save_idx, load_idx))
        # a fresh environment (no request source) takes the device generator from a load of all replicas, and follows A;
        # a partial load into one is refused
        fresh = mk(64, 0)
        refusals_state = raw_load(fresh, blob, 4, [0, 1, 2, 3])
        fresh.load_state(A.save_state())
        out["fresh_lean"] = fresh.occupancy()["lean_kernel"]
        out["fresh_follows"] = record_bytes(A.step_policy(60)) == record_bytes(fresh.step_policy(60))
        out["fresh_partial_refused"] = refusals_state
        fresh.close()
        out["across_nbytes"] = A.state_nbytes(4) == blob.size
        A.close(), Bv.close()


def main():
    out = {}
    replay(out)
    print("replay done", flush=True)
    fork_pinned(out)
    overlap(out)
    print("fork done", flush=True)
    keep_stream(out)
    lean_guard(out)
    keep_params(out)
    across(out)
    np.savez(sys.argv[1], **out)
    print("state child ok", flush=True)


if __name__ == "__main__":
    main()
