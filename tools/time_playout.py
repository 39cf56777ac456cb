#!/usr/bin/env python3
"""Device time of ongym_playout for the A = 41 block actions of observe_blocks(8): NSFNET-320 (capacity 448) after 600 first-fit
steps, device buffers, torch events on the environment's stream, the calls alternated round by round.

    python tools/time_playout.py [B ...]                 (default 16384)
    python tools/time_playout.py --fork [B H ...]        (default 2048 8 32 128)
    python tools/time_playout.py --quality [B STEPS]     (default 256 800)

The default mode times H = 8, 32, 128 at R = 1 and R = 4 at H = 32, both grid orders of the kernel (ONGYM_PLAYOUT_ORDER, read at
create: 0 = a replica's scenarios adjacent, 1 = replicas fastest), load balancing at H = 32, and beside them one step of
step_policy on the lean kernel and on the generic one (ONGYM_FORCE_GENERIC), the device functions the playout kernel reuses.
--fork times the route that exists without the call: a second environment of B A replicas, save_state, A times load_state
into it (one per action column), seed, step(actions), step_policy(H, record=False), stats - host buffers, copies included - beside
playout() on host buffers for the same B, and says how many bytes the second environment's state takes.
--quality runs the block environment choosing argmin playout_lookahead(32, 4), against argmin action_lookahead() and against
first fit on twins with the same seed, and reports the three blocking rates.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv  # noqa: E402

ROUNDS = 5
J = 8


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def config():
    wl = bench.WORKLOADS["nsfnet320"]
    return bench.build_tables(wl["topology"]), dict(
        modulations=bench.jocn_modulations(), num_spectrum_resources=wl["S"], capacity=wl["capacity"], episode_length=10 ** 6,
        auto_reset=True, load=wl["load"], bit_rate_selection="discrete", bit_rates=wl["bit_rates"])


def make_env(B, io_device=True, warm=600, **environ):
    """environ: variables the library reads at create (ONGYM_PLAYOUT_ORDER, ONGYM_FORCE_GENERIC)"""
    tb, kw = config()
    os.environ.update({k: str(v) for k, v in environ.items()})
    try:
        env = BatchedQRMSAEnv(tables=tb, batch_size=B, io_device=io_device, **kw)
    finally:
        for k in environ:
            os.environ.pop(k, None)
    if io_device:
        env.set_stream(torch.cuda.current_stream().cuda_stream)
    env.seed(1)
    env.reset()
    if warm:
        env.step_policy(warm, record=False)
    return env


def spread(v):
    return f"{np.median(v):9.3f} ms (median of {len(v)}, {min(v):.3f} to {max(v):.3f})"


def kernel_times(B):
    envs = {0: make_env(B, ONGYM_PLAYOUT_ORDER=0), 1: make_env(B, ONGYM_PLAYOUT_ORDER=1)}
    generic = make_env(B, ONGYM_FORCE_GENERIC=1)
    env = envs[0]
    c = env.holder.struct
    dev = torch.device("cuda", c.device)
    A = c.k_paths * J + 1
    blocks = (torch.empty((B, env.block_obs_dim(J)), dtype=torch.float32, device=dev),
              torch.empty((B, A), dtype=torch.uint8, device=dev), torch.empty((B, A), dtype=torch.int32, device=dev))
    env.observe_blocks(J, out=blocks)
    out = {R: torch.empty((B, A, R, 8), dtype=torch.float64, device=dev) for R in (1, 4)}
    FF, LB = nat.POLICY_FIRST_FIT, nat.POLICY_LOAD_BALANCING
    calls = {}
    for order, e in envs.items():
        for H, R, pol in ((8, 1, FF), (32, 1, FF), (128, 1, FF), (32, 4, FF), (32, 1, LB)):
            calls[(order, H, R, pol)] = lambda e=e, H=H, R=R, pol=pol: e.playout(blocks[2], horizon=H, policy=pol, samples=R, seed=5, out=out[R])
    steps = {("lean", FF): lambda: env.step_policy(32, record=False), ("lean", LB): lambda: env.step_policy(32, record=False, policy=LB),
             ("generic", FF): lambda: generic.step_policy(32, record=False),
             ("generic", LB): lambda: generic.step_policy(32, record=False, policy=LB)}
    played = {}
    for k, f in calls.items():                                  # warm-up: code objects, LDS limits; and the work done
        f()
        torch.cuda.synchronize()
        o = out[k[2]]
        ok = o[..., 0] < 2
        played[k] = float(ok.sum() + torch.nan_to_num(o[..., 2]).sum())
        if k == (0, 32, 4, FF):
            res_quality = {"applied": float((o[..., 0] == 0).float().mean()), "refused": float((o[..., 0] >= 2).float().mean()),
                           "blocked_per_scenario": float(o[..., 4][ok].mean()), "steps_per_scenario": float(o[..., 2][ok].mean())}
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, f in calls.items():
            ms[k].append(timed(f))
    step_ms = {k: [] for k in steps}
    for _ in range(ROUNDS + 1):                                 # these advance the replicas: after the playouts
        for k, f in steps.items():
            step_ms[k].append(timed(f))
    step_ns = {k: float(np.median(v[1:])) * 1e6 / (32 * B) for k, v in step_ms.items()}
    print(f"B={B}, A={A}: {100 * res_quality['applied']:.1f} % of the block actions applied, {100 * res_quality['refused']:.1f} % "
          f"refused (status 2/3); H=32: {res_quality['blocked_per_scenario']:.3f} of {res_quality['steps_per_scenario']:.1f} "
          f"requests blocked per scenario")
    res = {"B": B, "A": A, **res_quality}
    for k, v in ms.items():
        order, H, R, pol = k
        ns = float(np.median(v)) * 1e6 / played[k]
        name = f"order={order} H={H} R={R} policy={pol}"
        print(f"B={B}: playout {name:32s} {spread(v)}  {played[k] / 1e6:8.2f} M played steps, {ns:6.2f} ns per played step "
              f"(k_run {step_ns[('generic', pol)]:.2f}, k_fast {step_ns[('lean', pol)]:.2f} ns per step)")
        res[f"playout_{order}_{H}_{R}_{pol}_ms"] = float(np.median(v))
        res[f"playout_{order}_{H}_{R}_{pol}_ns_per_step"] = ns
    for k, v in step_ns.items():
        res[f"step_{k[0]}_{k[1]}_ns"] = v
    print(json.dumps(res))
    for e in (*envs.values(), generic):
        e.set_stream(None)
        e.close()


def fork_route(B, horizons):
    tb, kw = config()
    env = make_env(B, io_device=False)
    c = env.holder.struct
    A = c.k_paths * J + 1
    amap = np.ascontiguousarray(env.observe_blocks(J)[2], np.int32)
    big = BatchedQRMSAEnv(tables=tb, batch_size=B * A, **kw)
    big.seed(1)
    big.reset()
    into = [np.arange(B, dtype=np.int32) * A + a for a in range(A)]       # replica b * A + a of the second environment: (b, a)
    state_bytes = big.state_nbytes()
    print(f"fork route, B={B}, A={A}: the second environment holds {B * A} replicas, {state_bytes / 2 ** 20:.0f} MiB of state "
          f"({state_bytes / (B * A):.0f} B per scenario); the playout holds none (its output: {B * A * 64} B per sample)")
    res = {"B": B, "A": A, "fork_state_bytes": int(state_bytes)}
    for H in horizons:
        fork_s, kern_ms, play_s, play_ms = [], [], [], []
        for i in range(4):
            t0 = time.perf_counter()
            blob = env.save_state()
            for idx in into:
                big.load_state(blob, idx)
            big.seed(5)
            big.step(amap.reshape(-1))
            big.step_policy(H, record=False)
            k = big.last_kernel_ms()
            big.stats()
            fork_s.append(time.perf_counter() - t0)
            kern_ms.append(k)
            t0 = time.perf_counter()
            env.playout(amap, horizon=H, seed=5)
            play_s.append(time.perf_counter() - t0)
            play_ms.append(env.last_kernel_ms())
        fs, ps = float(np.median(fork_s[1:])), float(np.median(play_s[1:]))
        print(f"fork route, B={B}, H={H}: save + load + seed + step + step_policy + stats {fs * 1e3:9.2f} ms wall "
              f"(step_policy kernel alone {np.median(kern_ms[1:]):.2f} ms); playout(host buffers) {ps * 1e3:9.2f} ms wall "
              f"(kernel {np.median(play_ms[1:]):.2f} ms): {fs / ps:.2f}x")
        res[f"fork_H{H}_ms"], res[f"fork_H{H}_kernel_ms"] = fs * 1e3, float(np.median(kern_ms[1:]))
        res[f"playout_H{H}_ms"], res[f"playout_H{H}_kernel_ms"] = ps * 1e3, float(np.median(play_ms[1:]))
    print(json.dumps(res))
    env.close()
    big.close()


def quality(B, steps):
    from optical_networking_gym.envs.block_vec_env import QRMSABlockVecEnv
    tb, kw = config()
    kw = dict(kw, episode_length=1000)
    rates = {}
    for name in ("playout_lookahead", "action_lookahead"):
        vec = QRMSABlockVecEnv(tables=tb, num_envs=B, blocks_to_consider=J, seed=1, **kw)
        vec.reset()
        accepted, t0 = 0.0, time.perf_counter()
        for _ in range(steps):
            la = vec.playout_lookahead(horizon=32, samples=4) if name == "playout_lookahead" else vec.action_lookahead()
            la[:, -1] = np.inf                                  # reject only when no block is valid
            a = np.where(np.all(np.isnan(la[:, :-1]), axis=1), la.shape[1] - 1, np.argmin(np.nan_to_num(la, nan=np.inf), axis=1))
            _, rew, _, _ = vec.step(a)
            accepted += float(np.sum(rew == 0))                 # an accepted request has reward 0 (quirk Q1)
        rates[name] = 1.0 - accepted / (B * steps)
        rates[name + "_env_steps_per_s"] = B * steps / (time.perf_counter() - t0)
        vec.close()
    twin = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    twin.seed(1)
    twin.reset()
    rates["first_fit"] = 1.0 - float(np.mean(twin.step_policy(steps)["accepted"]))
    twin.close()
    print(f"quality, B={B}, {steps} steps ({B * steps} requests): blocking {rates['playout_lookahead']:.4f} choosing argmin "
          f"playout_lookahead(32, 4) ({rates['playout_lookahead_env_steps_per_s']:.0f} env-steps/s), {rates['action_lookahead']:.4f} "
          f"choosing argmin action_lookahead() ({rates['action_lookahead_env_steps_per_s']:.0f} env-steps/s), "
          f"{rates['first_fit']:.4f} with first fit")
    print(json.dumps({"B": B, "steps": steps, **rates}))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--fork":
        v = [int(a) for a in args[1:]]
        return fork_route(v[0] if v else 2048, v[1:] or [8, 32, 128])
    if args and args[0] == "--quality":
        return quality(int(args[1]) if len(args) > 1 else 256, int(args[2]) if len(args) > 2 else 800)
    for B in [int(a) for a in args] or [16384]:
        kernel_times(B)


if __name__ == "__main__":
    main()
