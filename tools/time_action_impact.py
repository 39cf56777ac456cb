#!/usr/bin/env python3
"""Device time of ongym_action_impact for A = 1 (the first-fit action), 9 (route 0's eight blocks and reject) and 41 (the whole
J = 8 block row), with and without svc_in, beside service_qot() and observe_blocks(8) on the same states: NSFNET-320
(capacity 448) after 600 first-fit steps, device buffers, torch events on the environment's stream, the calls alternated round
by round.

    python tools/time_action_impact.py [B ...]              (default 16384 65536)
    python tools/time_action_impact.py --fork-loop [B]      (default 16384)

--fork-loop times the only way to the same answer without the call: fork every source state over its 41 block actions, step
the forks, service_qot().  It uses nothing of this feature, so ONGYM_HIP_LIB may point it at an older build of the library.
An environment of B replicas holds floor(B / 42) source states and 41 forks of each; the time of one fork + step + service_qot
of that environment is scaled by B / floor(B / 42) to B source states.
"""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv  # noqa: E402

ROUNDS = 9
J = 8


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make_env(B):
    wl = bench.WORKLOADS["nsfnet320"]
    env = BatchedQRMSAEnv(tables=bench.build_tables(wl["topology"]), modulations=bench.jocn_modulations(), batch_size=B,
                          num_spectrum_resources=wl["S"], capacity=wl["capacity"], episode_length=1000, auto_reset=True,
                          load=wl["load"], bit_rate_selection="discrete", bit_rates=wl["bit_rates"], io_device=True)
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    env.seed(1)
    env.reset()
    env.step_policy(600, record=False)
    return env


def block_buffers(env, B, dev):
    K = env.holder.struct.k_paths
    return (torch.empty((B, env.block_obs_dim(J)), dtype=torch.float32, device=dev),
            torch.empty((B, K * J + 1), dtype=torch.uint8, device=dev), torch.empty((B, K * J + 1), dtype=torch.int32, device=dev))


def fork_loop(B):
    env = make_env(B)
    c = env.holder.struct
    dev = torch.device("cuda", c.device)
    A = c.k_paths * J + 1
    nsrc = B // (A + 1)
    blocks = block_buffers(env, B, dev)
    env.observe_blocks(J, out=blocks)
    src = torch.full((B,), -1, dtype=torch.int32, device=dev)
    acts = torch.full((B,), env.reject_action, dtype=torch.int32, device=dev)
    src[nsrc:nsrc + nsrc * A] = torch.arange(nsrc, dtype=torch.int32, device=dev).repeat_interleave(A)
    acts[nsrc:nsrc + nsrc * A] = blocks[2][:nsrc].reshape(-1)
    svc = torch.empty((B, c.capacity, 4), dtype=torch.float64, device=dev)
    rep = torch.empty((B, 6), dtype=torch.float64, device=dev)

    def loop():
        env.fork(src)
        env._check(env.lib.ongym_step_actions(env._h, C.c_void_p(acts.data_ptr()), None), "ongym_step_actions")
        env.service_qot(out=(svc, rep, None))

    loop()
    ms = float(np.median([timed(loop) for _ in range(ROUNDS)]))
    scale = B / nsrc
    res = {"B": B, "source_states": nsrc, "forks_per_state": A, "fork_step_qot_ms": ms, "scaled_to_B_source_states_ms": ms * scale}
    print(f"B={B}: {nsrc} source states x {A} forks: fork + step + service_qot {ms:.3f} ms (median of {ROUNDS}); "
          f"x {scale:.2f} = {ms * scale:.1f} ms for {B} source states")
    print(json.dumps(res))
    env.set_stream(None)
    env.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--fork-loop":
        for B in [int(a) for a in args[1:]] or [16384]:
            fork_loop(B)
        return
    for B in [int(a) for a in args] or [16384, 65536]:
        env = make_env(B)
        c = env.holder.struct
        K, dev = c.k_paths, torch.device("cuda", c.device)
        blocks = block_buffers(env, B, dev)
        env.observe_blocks(J, out=blocks)
        amap = blocks[2]
        ff = torch.empty((B,), dtype=torch.int32, device=dev)
        flags = torch.empty((B,), dtype=torch.uint8, device=dev)
        env._check(env.lib.ongym_policy_actions(env._h, 0, C.c_void_p(ff.data_ptr()), C.c_void_p(flags.data_ptr())), "policy_actions")
        lists = {1: ff.reshape(B, 1).contiguous(), 9: torch.cat([amap[:, :J], amap[:, -1:]], dim=1).contiguous(), K * J + 1: amap}
        outs = {A: torch.empty((B, A, 8), dtype=torch.float64, device=dev) for A in lists}
        svc = torch.empty((B, c.capacity, 4), dtype=torch.float64, device=dev)
        rep = torch.empty((B, 6), dtype=torch.float64, device=dev)
        active = float(np.mean(env.stats()["active"]))
        calls = {"service_qot": lambda: env.service_qot(out=(svc, rep, None)),
                 f"observe_blocks({J})": lambda: env.observe_blocks(J, out=blocks)}
        for A in lists:
            calls[f"action_impact A={A}"] = lambda A=A: env.action_impact(lists[A], out=outs[A])
            calls[f"action_impact A={A} svc_in"] = lambda A=A: env.action_impact(lists[A], svc=svc, out=outs[A])
        for f in calls.values():                                   # warm-up: code objects, LDS limits (and svc for svc_in)
            f()
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, f in calls.items():
                ms[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        full = outs[K * J + 1]
        ok = full[:, :, 0] == 0
        res = {"B": B, "active": active, **{f"{k}_ms": v for k, v in med.items()},
               "evaluated_actions_per_replica": float(ok.float().sum(dim=1).mean()),
               "victims_per_evaluated_action": float(full[:, :, 1][ok].mean())}
        print(f"B={B}: {active:.0f} running services per replica, {res['evaluated_actions_per_replica']:.1f} evaluated actions "
              f"of {K * J + 1} per replica, {res['victims_per_evaluated_action']:.1f} victims per evaluated action")
        for k in calls:
            print(f"B={B}: {k:30s} {med[k]:.3f} ms (median of {ROUNDS})")
        print(json.dumps(res))
        env.set_stream(None)
        env.close()
        del svc, outs


if __name__ == "__main__":
    main()
