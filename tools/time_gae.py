#!/usr/bin/env python3
"""Device time of GAE over a rollout (ongym_gae through optical_networking_gym.rl.gae) beside the sequential torch loop it
replaces (one step at a time over [B] vectors, reward and terminated cut out of the 56-byte step records each step), at
B = 16384 replicas and T in {16, 128, 2048} steps.  Records are synthetic (the kernel reads every byte of them whatever they
hold): normal rewards, 5 % terminations.

    python tools/time_gae.py [--batch B] [--steps 16 128 2048] [--iters N] [--reps R]

Device events around N back-to-back calls after warm-up; the two implementations alternate over R rounds (min / max reported).
Algorithmic bytes: T B (56 + 4 + 4 + 4) + 4 B (whole records, values, advantages, returns; last values).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), REPO]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--steps", type=int, nargs="*", default=[16, 128, 2048])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hip-only", action="store_true", help="skip the torch loop (profiler passes)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from optical_networking_gym import _native as nat
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    from optical_networking_gym.rl import gae
    import __graft_entry__ as entry
    entry.build()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    B = args.batch
    wl = bench.WORKLOADS["nsfnet320"]
    env = BatchedQRMSAEnv(tables=bench.build_tables(wl["topology"]), modulations=bench.jocn_modulations(), batch_size=B,
                          num_spectrum_resources=wl["S"], capacity=wl["capacity"], episode_length=1000, auto_reset=True,
                          load=wl["load"], bit_rate_selection="discrete", bit_rates=wl["bit_rates"], io_device=True)
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = torch.device("cuda", 0)
    REC = nat.STEP_DTYPE.itemsize
    r_off, t_off = nat.STEP_DTYPE.fields["reward"][1], nat.STEP_DTYPE.fields["terminated"][1]
    gamma, lam = 0.99, 0.95

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    rows = []
    rng = np.random.default_rng(0)
    for T in args.steps:
        rec = np.zeros((T, B), nat.STEP_DTYPE)
        rec["reward"] = rng.normal(0.0, 1.0, (T, B))
        rec["terminated"] = rng.random((T, B)) < 0.05
        recs = torch.from_numpy(rec.view(np.uint8).reshape(T, B, REC)).to(dev)
        del rec
        values = torch.randn((T, B), device=dev)
        last = torch.randn(B, device=dev)
        adv, ret = torch.empty((T, B), device=dev), torch.empty((T, B), device=dev)
        adv_t, ret_t = torch.empty((T, B), device=dev), torch.empty((T, B), device=dev)

        def hip():
            gae(env, recs, values, last, gamma, lam, out=(adv, ret))

        def loop():
            a = torch.zeros(B, device=dev)
            for t in reversed(range(T)):
                rew = recs[t][:, r_off:r_off + 8].contiguous().view(torch.float64).squeeze(1).float()
                nnt = 1.0 - recs[t][:, t_off].float()
                vnext = last if t == T - 1 else values[t + 1]
                a = (rew + gamma * vnext * nnt - values[t]) + gamma * lam * nnt * a
                adv_t[t].copy_(a)
            torch.add(adv_t, values, out=ret_t)

        nbytes = T * B * (REC + 4 + 4 + 4) + 4 * B
        impls = (("ongym_gae", hip),) if args.hip_only else (("ongym_gae", hip), ("torch loop", loop))
        ms = {k: [] for k, _ in impls}
        for _ in range(args.reps):
            for k, fn in impls:
                ms[k].append(timed(fn))
        agree = None
        if not args.hip_only:
            torch.cuda.synchronize()
            agree = float((adv - adv_t).abs().max() / (1 + adv_t.abs().max()))
        for k, _ in impls:
            rows.append(dict(T=T, B=B, impl=k, ms_min=min(ms[k]), ms_max=max(ms[k]), gbytes=nbytes / 1e9,
                             tb_s=nbytes / min(ms[k]) / 1e9, max_rel_diff=agree))
        del recs, values, adv, ret, adv_t, ret_t
        torch.cuda.empty_cache()
    print(f"GAE (gamma {gamma}, lambda {lam}) over ongym_step_rec rollouts, B = {B}; device events, {args.reps} alternated rounds "
          f"of {args.iters} calls")
    print(f"{'T':>5} {'impl':11} {'ms min':>9} {'ms max':>9} {'GB (alg.)':>10} {'TB/s':>6} {'loop/hip':>8}")
    for r in rows:
        hip_ms = next(q["ms_min"] for q in rows if q["T"] == r["T"] and q["impl"] == "ongym_gae")
        ratio = f"{r['ms_min'] / hip_ms:8.1f}" if r["impl"] != "ongym_gae" else ""
        print(f"{r['T']:5d} {r['impl']:11} {r['ms_min']:9.4f} {r['ms_max']:9.4f} {r['gbytes']:10.3f} {r['tb_s']:6.2f} {ratio}")
    print(json.dumps(dict(batch=B, gamma=gamma, gae_lambda=lam, rows=rows)))


if __name__ == "__main__":
    main()
