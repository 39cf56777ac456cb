#!/usr/bin/env python3
"""Device time of ongym_observe_blocks (block observation, mask and action map) for J in {1, 4, 8, 16}, beside ongym_observe on
the same states: NSFNET-320 after 600 first-fit steps, device buffers, torch events on the environment's stream, the calls
alternated round by round.

    python tools/time_blocks.py [B ...]          (default 16384 65536)
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

BLOCKS = (1, 4, 8, 16)
ROUNDS = 7


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
        K, dev = c.k_paths, torch.device("cuda", c.device)
        obs = torch.empty((B, 3 + K + K * c.n_mods_consider * 12), dtype=torch.float32, device=dev)
        mask = torch.empty((B, env.num_actions), dtype=torch.uint8, device=dev)
        outs = {J: (torch.empty((B, env.block_obs_dim(J)), dtype=torch.float32, device=dev),
                    torch.empty((B, K * J + 1), dtype=torch.uint8, device=dev),
                    torch.empty((B, K * J + 1), dtype=torch.int32, device=dev)) for J in BLOCKS}

        def observe():
            env._check(env.lib.ongym_observe(env._h, C.c_void_p(obs.data_ptr()), C.c_void_p(mask.data_ptr())), "observe")

        observe()
        for J in BLOCKS:                                          # warm-up: code objects, LDS limits
            env.observe_blocks(J, out=outs[J])
        ms = {"observe": []}
        ms.update({J: [] for J in BLOCKS})
        for _ in range(ROUNDS):
            ms["observe"].append(timed(observe))
            for J in BLOCKS:
                ms[J].append(timed(lambda: env.observe_blocks(J, out=outs[J])))
        base = float(np.median(ms["observe"]))
        res = {"B": B, "observe_ms": base}
        print(f"B={B}: ongym_observe {base:.3f} ms (median of {ROUNDS})")
        for J in BLOCKS:
            t = float(np.median(ms[J]))
            valid = float(outs[J][1][:, :-1].float().sum(dim=1).mean())
            res[f"blocks_{J}_ms"] = t
            print(f"B={B}: observe_blocks J={J:2d} {t:.3f} ms ({t / base:.2f}x ongym_observe), "
                  f"{B / t * 1e3:.3e} observations/s, {valid:.1f} valid block actions per replica")
        print(json.dumps(res))
        env.set_stream(None)
        env.close()


if __name__ == "__main__":
    main()
