#!/usr/bin/env python3
"""Device time of ongym_service_qot (every output, and the replica / link aggregates alone) beside ongym_observe and
link_metrics() on the same states: NSFNET-320 (capacity 448) after 600 first-fit steps, device buffers, torch events on the
environment's stream, the calls alternated round by round.

    python tools/time_service_qot.py [B ...]          (default 16384 65536)
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    batches = [int(a) for a in sys.argv[1:]] or [16384, 65536]
    wl = bench.WORKLOADS["nsfnet320"]
    for B in batches:
        env = BatchedQRMSAEnv(tables=bench.build_tables(wl["topology"]), modulations=bench.jocn_modulations(), batch_size=B,
                              num_spectrum_resources=wl["S"], capacity=wl["capacity"], episode_length=1000, auto_reset=True,
                              load=wl["load"], bit_rate_selection="discrete", bit_rates=wl["bit_rates"], io_device=True)
        env.set_stream(torch.cuda.current_stream().cuda_stream)
        env.seed(1)
        env.reset()
        env.step_policy(600, record=False)
        c = env.holder.struct
        E, dev = c.n_links, torch.device("cuda", c.device)
        obs = torch.empty((B, 3 + c.k_paths + c.k_paths * c.n_mods_consider * 12), dtype=torch.float32, device=dev)
        mask = torch.empty((B, env.num_actions), dtype=torch.uint8, device=dev)
        svc = torch.empty((B, c.capacity, 4), dtype=torch.float64, device=dev)
        rep = torch.empty((B, 6), dtype=torch.float64, device=dev)
        link = torch.empty((B, E, 3), dtype=torch.float32, device=dev)
        lm = (torch.empty((B, E, 8), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float64, device=dev))
        active = float(np.mean(env.stats()["active"]))

        def observe():
            env._check(env.lib.ongym_observe(env._h, C.c_void_p(obs.data_ptr()), C.c_void_p(mask.data_ptr())), "observe")

        calls = {"service_qot": lambda: env.service_qot(out=(svc, rep, link)),
                 "service_qot aggregates": lambda: env.service_qot(out=(None, rep, link)),
                 "observe": observe,
                 "link_metrics": lambda: env.link_metrics(out=lm)}
        for f in calls.values():                                   # warm-up: code objects, LDS limits
            f()
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, f in calls.items():
                ms[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        kernel = []
        for _ in range(ROUNDS):
            env.service_qot(out=(svc, rep, link))
            kernel.append(env.last_kernel_ms())
        res = {"B": B, "active": active, **{f"{k}_ms": v for k, v in med.items()},
               "service_qot_event_ms": float(np.median(kernel))}
        print(f"B={B}: {active:.0f} running services per replica, svc_out {svc.numel() * 8 / 1e6:.1f} MB")
        for k in calls:
            print(f"B={B}: {k:24s} {med[k]:.3f} ms (median of {ROUNDS})")
        print(f"B={B}: service_qot by the library's ev0/ev1 events {res['service_qot_event_ms']:.3f} ms, "
              f"{med['service_qot'] * 1e6 / (B * active):.3f} ns per running service")
        print(json.dumps(res))
        env.set_stream(None)
        env.close()
        del svc


if __name__ == "__main__":
    main()
