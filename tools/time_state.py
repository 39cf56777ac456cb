#!/usr/bin/env python3
"""Device time of saving, loading and forking replica states (ongym_state_save / ongym_state_load / ongym_fork through
BatchedQRMSAEnv) beside torch.Tensor.copy_ of a buffer of the same size, in the same process, at NSFNET-320, capacity 448,
B = 65 536 replicas (first-fit traffic stepped for --warmup steps first, so the blocks hold a loaded network).

    python tools/time_state.py [--batch B] [--capacity C] [--warmup W] [--iters N] [--reps R]

Device events around N back-to-back calls on torch's current stream after one untimed call; the five operations alternate over
R rounds (min / max of the per-call time reported).  GB/s counts the state bytes once read and once written.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests"), REPO]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--capacity", type=int, default=448)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from common import golden_tables, jocn_modulations
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv

    B = args.batch
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=B, io_device=True,
                          num_spectrum_resources=320, capacity=args.capacity, load=300, bit_rate_selection="discrete",
                          bit_rates=(10, 40, 100, 400), episode_length=1000)
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    env.seed(1)
    env.reset()
    env.step_policy(args.warmup, record=False)
    nbytes = env.state_nbytes()
    per = (nbytes - 256) // B
    blob = env.save_state()
    zeros = torch.zeros(B, dtype=torch.int32, device="cuda")
    perm = torch.randperm(B, device="cuda").to(torch.int32)
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ops = {
        "save (device blob)": lambda: env.save_state(out=blob),
        "load (device blob)": lambda: env.load_state(blob),
        "fork src = 0 (broadcast)": lambda: env.fork(zeros),
        "fork random permutation": lambda: env.fork(perm),
        "torch copy_ (same bytes)": lambda: b.copy_(a),
    }
    times = {k: [] for k in ops}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        for name, fn in ops.items():
            fn()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    dev = torch.cuda.get_device_name()
    print(f"# tools/time_state.py on {dev}: NSFNET-320, capacity {args.capacity}, B = {B}, {args.warmup} first-fit steps first")
    print(f"# state: {per} bytes per replica block, {nbytes / 1e9:.3f} GB blob; {args.iters} calls x {args.reps} rounds")
    ref = min(times["torch copy_ (same bytes)"])
    print(f"{'operation':28s} {'min ms':>9s} {'max ms':>9s} {'GB/s':>8s} {'x copy_':>8s}")
    for name, t in times.items():
        print(f"{name:28s} {min(t):9.4f} {max(t):9.4f} {2 * nbytes / min(t) / 1e6:8.0f} {min(t) / ref:8.2f}")
    env.close()


if __name__ == "__main__":
    main()
