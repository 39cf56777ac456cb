#!/usr/bin/env python3
"""Device time of ongym_failure_impact for F = 1 (one link per replica) and F = E (every link), beside service_qot() and
observe_blocks(8) on the same states: NSFNET-320 (capacity 448) after 600 first-fit steps, device buffers, torch events on the
environment's stream, the calls alternated round by round.

    python tools/time_failure_impact.py [B ...]              (default 16384 65536)
    python tools/time_failure_impact.py --host-loop [N]      (default 4 replicas)

--host-loop times the only way to the same answer without the call, the loop an application would write: services() and
grid() of a replica, then the numpy restatement of tests/failure_impact_child.py with the CPU oracle's GN, for every link of
N sample replicas; it also counts the GN evaluations per scenario and compares its rows with the device's.
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

ROUNDS = 9
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
        modulations=bench.jocn_modulations(), num_spectrum_resources=wl["S"], capacity=wl["capacity"], episode_length=1000,
        auto_reset=True, load=wl["load"], bit_rate_selection="discrete", bit_rates=wl["bit_rates"])


def make_env(B):
    tb, kw = config()
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, io_device=True, **kw)
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    env.seed(1)
    env.reset()
    env.step_policy(600, record=False)
    return env


def host_loop(N):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from failure_impact_child import restate_replica
    from oracle_lib import OracleEnv
    tb, kw = config()
    env = make_env(max(N, 64))
    E = tb.n_links
    out = torch.empty((env.batch_size, E, 10), dtype=torch.float64, device="cuda")
    env.failure_impact(out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    holder = nat.ConfigHolder(tb, batch=env.batch_size, **kw)
    secs, evals, same = [], 0, True
    for r in range(N):
        o = OracleEnv(holder, replica=r)
        t0 = time.perf_counter()
        svcs, grid = env.services(r), env.grid(r)
        log = []
        want, _, _ = restate_replica(o, tb, holder, float(kw.get("margin", 0.0)), svcs, grid, np.arange(E), log=log)
        secs.append(time.perf_counter() - t0)
        evals += len(log)
        same &= bool(np.array_equal(got[r][:, :9], want[:, :9]))
    per = float(np.mean(secs))
    res = {"replicas": N, "links": E, "host_seconds_per_replica": per, "gn_evaluations_per_scenario": evals / (N * E),
           "rows_equal_device": same}
    print(f"host loop: {per:.3f} s per replica ({E} scenarios), {evals / (N * E):.1f} GN evaluations per scenario (the device "
          f"answers some of them with the ASE bound), rows equal the device's: {same}")
    for B in (16384, 65536):
        print(f"  scaled to B = {B}: {per * B:.0f} s")
    print(json.dumps(res))
    env.set_stream(None)
    env.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--host-loop":
        host_loop(int(args[1]) if len(args) > 1 else 4)
        return
    for B in [int(a) for a in args] or [16384, 65536]:
        env = make_env(B)
        c = env.holder.struct
        K, E, dev = c.k_paths, c.n_links, torch.device("cuda", c.device)
        blocks = (torch.empty((B, env.block_obs_dim(J)), dtype=torch.float32, device=dev),
                  torch.empty((B, K * J + 1), dtype=torch.uint8, device=dev), torch.empty((B, K * J + 1), dtype=torch.int32, device=dev))
        svc = torch.empty((B, c.capacity, 4), dtype=torch.float64, device=dev)
        rep = torch.empty((B, 6), dtype=torch.float64, device=dev)
        one = (torch.arange(B, dtype=torch.int32, device=dev) % E).reshape(B, 1).contiguous()
        out1 = torch.empty((B, 1, 10), dtype=torch.float64, device=dev)
        outE = torch.empty((B, E, 10), dtype=torch.float64, device=dev)
        active = float(np.mean(env.stats()["active"]))
        calls = {"service_qot": lambda: env.service_qot(out=(svc, rep, None)),
                 f"observe_blocks({J})": lambda: env.observe_blocks(J, out=blocks),
                 "failure_impact F=1": lambda: env.failure_impact(one, out=out1),
                 f"failure_impact F={E}": lambda: env.failure_impact(out=outE)}
        for f in calls.values():                                   # warm-up: code objects, LDS limits
            f()
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, f in calls.items():
                ms[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res = {"B": B, "active": active, **{f"{k}_ms": v for k, v in med.items()},
               "victims_per_scenario": float(outE[:, :, 1].mean()), "restored_per_scenario": float(outE[:, :, 3].mean()),
               "lost_no_spectrum_per_scenario": float(outE[:, :, 5].mean()), "lost_qot_per_scenario": float(outE[:, :, 6].mean())}
        print(f"B={B}: {active:.0f} running services per replica; per scenario {res['victims_per_scenario']:.1f} victims, "
              f"{res['restored_per_scenario']:.1f} restored, {res['lost_no_spectrum_per_scenario']:.2f} lost for spectrum, "
              f"{res['lost_qot_per_scenario']:.2f} lost on QoT")
        for k in calls:
            print(f"B={B}: {k:30s} {med[k]:.3f} ms (median of {ROUNDS})")
        print(json.dumps(res))
        env.set_stream(None)
        env.close()
        del svc, outE


if __name__ == "__main__":
    main()
