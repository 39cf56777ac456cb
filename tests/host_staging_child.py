"""Child process of tests/test_gpu_host_staging.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP
runtime and this library's must start together), saved to an .npz that the tests assert on.

    python tests/host_staging_child.py OUT.npz

Two environments on the same state, one with host buffers and one with io_device, go through the same calls: first the step
calls in lockstep (step_side), then a read-only sequence of the four analysis calls (ongym_observe_blocks, ongym_action_impact,
ongym_service_qot, ongym_link_metrics), ongym_observe, ongym_sample_actions and the queries, then a masked reset.  A second pair
that tracks service ids samples before its first observation and has its episode counters reset.  The sequences make each
call's host staging buffer grow, be reused while larger than needed, lay its arrays out with optional ones missing, and carry
inputs in and outputs out.  Every output starts as SENTINEL or another value no call writes; results are saved as "h_<name>"
(host) and "d_<name>" (device), "th_" / "td_" for the pair that tracks ids.  A device environment only ever gets device
tensors where the library takes the caller's pointers; the queries take host buffers on both.
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402

from common import golden_tables, jocn_modulations  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv  # noqa: E402
from test_gpu_host_staging import (B, BLOCKS, CAND_ROWS, GSNR_COUNTS, IMPACT_A, KW, NSTEPS, QUERY_REPLICA, RESET_MASK, SEED,  # noqa: E402
                                   SENTINEL, STEPS, SUBSETS, cand_row, candidates_np)

TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
         np.dtype(np.uint8): torch.uint8}


def ptr(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a.ctypes.data


def filled(env, shape, dtype, value=SENTINEL):
    """an output array of the environment's kind (numpy, or a tensor on the device), filled"""
    if env.holder.struct.io_device:
        return torch.full(shape, value, dtype=TORCH[np.dtype(dtype)], device="cuda")
    return np.full(shape, value, dtype)


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def snapshot(out, tag, env):
    out[tag + "_grid"] = np.stack([env.grid(r) for r in range(B)])
    services = [env.services(r) for r in range(B)]
    out[tag + "_services"], out[tag + "_nservices"] = np.concatenate(services), np.array([len(s) for s in services])
    out[tag + "_stats"] = env.stats()


def dev_records(t, shape):
    """step records a device environment wrote into a uint8 tensor"""
    return t.cpu().numpy().view(nat.STEP_DTYPE).reshape(shape)


def record_tensor(n):
    return torch.zeros(n * nat.STEP_DTYPE.itemsize, dtype=torch.uint8, device="cuda")


def step_side(out, h, d):
    """the calls that step, on both environments in lockstep: policy steps with records (the record buffer grows, then serves a
    smaller call) and without, the policy's actions with and without flags, and a step with those actions"""
    for n in NSTEPS:
        out[f"h_pol{n}_rec"] = h.step_policy(n)
        t = record_tensor(n * B)
        d.step_policy(n, out_device_ptr=t.data_ptr())
        out[f"d_pol{n}_rec"] = dev_records(t, (n, B))
        for env in (h, d):
            env.step_policy(3, record=False)
    for p, env in (("h", h), ("d", d)):
        for flags in (True, False):                            # flags = NULL only through the raw library
            a, f = filled(env, (B,), np.int32, -9), filled(env, (B,), np.uint8, 255)
            env._check(env.lib.ongym_policy_actions(env._h, nat.POLICY_FIRST_FIT, ptr(a), ptr(f) if flags else None),
                       "ongym_policy_actions")
            out[f"{p}_pa{int(flags)}_actions"], out[f"{p}_pa{int(flags)}_flags"] = host(a), host(f)
    out["h_step_rec"] = h.step(out["h_pa1_actions"])
    t = record_tensor(B)
    a = torch.from_numpy(out["d_pa1_actions"]).cuda()
    d._check(d.lib.ongym_step_actions(d._h, ptr(a), ptr(t)), "ongym_step_actions")
    out["d_step_rec"] = dev_records(t, (B,))


def observe(out, key, env):
    c = env.holder.struct
    obs = filled(env, (B, 3 + c.k_paths + c.k_paths * c.n_mods_consider * 12), np.float32)
    mask = filled(env, (B, env.num_actions), np.uint8, 255)
    env._check(env.lib.ongym_observe(env._h, ptr(obs), ptr(mask)), "ongym_observe")
    out[key + "_obs"], out[key + "_mask"] = host(obs), host(mask)


def sample(env, mask):
    """ongym_sample_actions on a host mask (copied to the device for a device environment), seed SEED, draw 5"""
    m = torch.from_numpy(mask).cuda() if env.holder.struct.io_device else mask
    a = filled(env, (B,), np.int32, -9)
    env._check(env.lib.ongym_sample_actions(env._h, ptr(m), SEED, 5, ptr(a)), "ongym_sample_actions")
    return host(a)


def queries(out, p, env, tables):
    """the plugin-API queries on one replica; host buffers on both environments"""
    r, S = QUERY_REPLICA, env.holder.struct.n_slots
    out[p + "_q_request"] = np.stack([env.request(k) for k in range(B)])
    req = env.request(r)
    path = int(tables.pair_paths[req["source"], req["destination"], 0])
    out[p + "_q_path"] = np.array(path)
    out[p + "_q_avail"] = env.available_slots(r, path)
    out[p + "_q_free"] = np.array([[env.is_path_free(r, path, s, n) for s in range(S)] for n in (1, 3)])
    for L in CAND_ROWS:
        for n in (1, 3):
            out[f"{p}_q_cand{L}_{n}"] = np.array(env.candidates(cand_row(L), n), np.int32)
    cands = []                                                  # free candidates of the replica, a few per path
    for q in range(tables.n_paths):
        avail = env.available_slots(r, q)
        cands += [(q, s, n) for n in (2, 3) for s in candidates_np(avail, n)[:4]]
        if len(cands) >= max(GSNR_COUNTS):
            break
    cands = np.array((cands * max(GSNR_COUNTS))[:max(GSNR_COUNTS)], np.int32)
    out[p + "_q_cands"] = cands
    for k in GSNR_COUNTS:                                       # the buffer grows, then serves a smaller call
        out[f"{p}_q_gsnr_many{k}"] = env.gsnr_many(r, cands[:k])
    out[p + "_q_gsnr_alone"] = np.stack([env.gsnr(r, *map(int, c)) for c in cands])


def masked(env, call, mask):
    """ongym_reset / ongym_reset_episode_counters with a mask; neither synchronises, the snapshot that follows does"""
    m = torch.from_numpy(mask).cuda() if env.holder.struct.io_device else mask
    env._check(call(env._h, ptr(m)), "masked reset")
    return m                                                    # alive until the caller has synchronised


def sequence(out, p, env):
    """the whole sequence on one environment, results under prefix p"""
    c = env.holder.struct
    dev = bool(c.io_device)
    for J in BLOCKS:                                            # grow (1 -> 16), then a larger buffer than needed (4)
        n = c.k_paths * J + 1
        if dev:
            t = (torch.full((B, env.block_obs_dim(J)), SENTINEL, dtype=torch.float32, device="cuda"),
                 torch.full((B, n), 255, dtype=torch.uint8, device="cuda"), torch.full((B, n), -7, dtype=torch.int32, device="cuda"))
            env.observe_blocks(J, out=t)
        else:
            t = env.observe_blocks(J)
        out[f"{p}_blk{J}_obs"], out[f"{p}_blk{J}_mask"], out[f"{p}_blk{J}_map"] = (host(x) for x in t)
    # candidate actions: the 16-block action map, then random indices (most of them not allocable)
    rnd = np.random.default_rng(SEED).integers(0, env.num_actions, (B, nat.MAX_IMPACT_ACTIONS))
    actions = np.concatenate([out[f"{p}_blk{nat.MAX_BLOCKS}_map"], rnd], axis=1)[:, :nat.MAX_IMPACT_ACTIONS].astype(np.int32)
    out[p + "_actions"] = actions
    svc_full = filled(env, (B, c.capacity, 4), np.float64)
    env._check(env.lib.ongym_service_qot(env._h, ptr(svc_full), None, None), "ongym_service_qot")
    for A in IMPACT_A:
        a = np.ascontiguousarray(actions[:, :A])
        for with_svc in (False, True):
            if dev:
                res = torch.full((B, A, 8), SENTINEL, dtype=torch.float64, device="cuda")
                env.action_impact(torch.from_numpy(a).cuda(), svc=svc_full if with_svc else None, out=res)
            else:
                res = env.action_impact(a, svc=svc_full if with_svc else None)
            out[f"{p}_imp{A}_{int(with_svc)}"] = host(res)
    E = c.n_links
    for sub in SUBSETS:                                         # ongym_service_qot: (svc_out, replica_out, link_out)
        arrs = (filled(env, (B, c.capacity, 4), np.float64), filled(env, (B, 6), np.float64), filled(env, (B, E, 3), np.float32))
        env._check(env.lib.ongym_service_qot(env._h, *(ptr(x) if on else None for x, on in zip(arrs, sub))), "ongym_service_qot")
        for x, name in zip(arrs, ("svc", "rep", "link")):
            out[f"{p}_qot{''.join(map(str, sub))}_{name}"] = host(x)
    for sub in SUBSETS:                                         # ongym_link_metrics: (link_out, compactness, link_stats)
        arrs = (filled(env, (B, E, 8), np.float32), filled(env, (B,), np.float64),
                filled(env, (B, E, 4), np.float64, 0.0 if sub[2] else SENTINEL))
        key = f"{p}_lm{''.join(map(str, sub))}"
        env._check(env.lib.ongym_link_metrics(env._h, *(ptr(x) if on else None for x, on in zip(arrs, sub))), "ongym_link_metrics")
        if sub[2]:
            # link_stats goes in and comes out: a second call continues from the caller's values, here the first call's with
            # the utilisation halved.  The call in between puts another array where link_stats was staged.
            out[key + "_stats_first"] = host(arrs[2]).copy()
            arrs[2][:, :, 0] *= 0.5
            other = filled(env, (B, E, 8), np.float32)
            env._check(env.lib.ongym_link_metrics(env._h, ptr(other), None, None), "ongym_link_metrics")
            env._check(env.lib.ongym_link_metrics(env._h, *(ptr(x) if on else None for x, on in zip(arrs, sub))), "ongym_link_metrics")
        for x, name in zip(arrs, ("link", "comp", "stats")):
            out[f"{key}_{name}"] = host(x)


def main():
    out = {}
    tables = golden_tables("nsfnet")
    mk = lambda **kw: [BatchedQRMSAEnv(tables=tables, modulations=jocn_modulations(), batch_size=B, io_device=d, **KW, **kw)
                       for d in (False, True)]
    envs, tracked = mk(), mk(track_service_ids=True)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for pair in (envs, tracked):
            pair[1].set_stream(torch.cuda.current_stream().cuda_stream)
            for env in pair:
                env.seed(SEED)
                env.reset()
        for p, env in zip("hd", envs):
            snapshot(out, p + "_fresh", env)                    # the queries right after reset(): no service runs
            env.step_policy(STEPS, record=False)
        step_side(out, *envs)
        for p, env in zip("hd", envs):
            snapshot(out, p + "_before", env)
            sequence(out, p, env)
            observe(out, p + "_observe", env)
            out[p + "_sample"] = sample(env, out["h_observe_mask"])
            queries(out, p, env, tables)
            stream.synchronize()
            snapshot(out, p + "_after", env)
        mask = np.array(RESET_MASK, np.uint8)
        for p, env in zip("hd", envs):
            keep = masked(env, env.lib.ongym_reset, mask)
            snapshot(out, p + "_reset", env)
        for p, env in zip(("th", "td"), tracked):
            out[p + "_sample_first"] = sample(env, out["h_observe_mask"])     # the mask buffer's first use is the sampler's
            env.step_policy(STEPS, record=False)
            observe(out, p + "_observe", env)
            out[p + "_sample"] = sample(env, out["h_observe_mask"])
            snapshot(out, p + "_before", env)
            keep = masked(env, env.lib.ongym_reset_episode_counters, mask)
            snapshot(out, p + "_counters", env)
        del keep
        for pair in (envs, tracked):
            pair[1].set_stream(None)
    for env in envs + tracked:
        env.close()
    np.savez(sys.argv[1], **out)
    print("host staging child ok")


if __name__ == "__main__":
    main()
