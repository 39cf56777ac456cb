#!/usr/bin/env python3
"""Device time of the masked categorical head (ongym_masked_categorical / _backward) beside the torch formulation it
replaces (masked_fill(mask == 0, -1e8) + torch.distributions.Categorical, what sb3-contrib's MaskableCategorical does), at
B = 16384 on the NSFNET-320 action mask of a loaded network (9601 actions), f32 and bf16 logits.

    python tools/time_policy_head.py [--batch B] [--iters N] [--head-only]
    python tools/time_policy_head.py --packed [--rows R ...]     # bf16 evaluate + backward, packed bits vs bytes

`--packed`: the PPO-update form (ongym_masked_categorical_rows / _backward_rows) at R = B and at the given row counts (default
B and 262144: minibatch rows tiled from the B observed rows), byte mask vs packed bits, alternated over --reps rounds.

Times are device events around N back-to-back calls after warm-up.  Bytes are algorithmic, from shapes: forward = logits +
mask read + mask bits written; backward = logits + mask bits read + gradient written (per-row vectors not counted).
"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), REPO]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--head-only", action="store_true", help="skip the torch formulation (profiler passes)")
    ap.add_argument("--packed", action="store_true", help="bf16 evaluate + backward with packed bits vs bytes (only)")
    ap.add_argument("--rows", type=int, nargs="*", default=None, help="--packed: row counts (default: B and 262144)")
    ap.add_argument("--reps", type=int, default=3, help="--packed: alternated rounds")
    args = ap.parse_args()
    import torch
    import bench
    from optical_networking_gym import _native as nat
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    import __graft_entry__ as entry
    entry.build()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    B = args.batch
    wl = bench.WORKLOADS["nsfnet320"]
    env = BatchedQRMSAEnv(tables=bench.build_tables(wl["topology"]), modulations=bench.jocn_modulations(), batch_size=B,
                          num_spectrum_resources=wl["S"], capacity=wl["capacity"], episode_length=1000, auto_reset=True,
                          load=wl["load"], bit_rate_selection="discrete", bit_rates=wl["bit_rates"], io_device=True)
    dev = torch.device("cuda", 0)
    c = env.holder.struct
    n = env.num_actions
    obs = torch.empty((B, 3 + c.k_paths + c.k_paths * c.n_mods_consider * 12), device=dev)
    mask = torch.empty((B, n), dtype=torch.uint8, device=dev)
    env.seed(1)
    env.reset()
    env.step_policy(300, record=False)
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    env._check(env.lib.ongym_observe(env._h, obs.data_ptr(), mask.data_ptr()), "observe")
    torch.cuda.synchronize()
    valid_frac = float(mask.float().mean())
    W = (n + 31) // 32
    acts = torch.empty(B, dtype=torch.int32, device=dev)
    lp, H = (torch.empty(B, device=dev) for _ in range(2))
    stats = torch.empty((B, 2), device=dev)      # row stats: max valid logit, log sum
    bits = torch.empty((B, W), dtype=torch.int32, device=dev)
    g_lp, g_H = torch.randn(B, device=dev), torch.randn(B, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731

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

    if args.packed:
        return packed_vs_bytes(env, mask, args, timed, p)
    rows = []
    for dt, code in ((torch.bfloat16, nat.DTYPE_BF16), (torch.float32, nat.DTYPE_F32)):
        logits = (torch.randn((B, n), device=dev) * 2).to(dt)
        grad = torch.empty_like(logits)
        es = logits.element_size()
        fwd_bytes = B * n * es + B * n + B * W * 4
        bwd_bytes = 2 * B * n * es + B * W * 4
        draw = [0]

        def head(mode):
            def f():
                env._check(env.lib.ongym_masked_categorical(env._h, p(logits), code, p(mask), mode, 0, draw[0], p(acts), p(lp), p(H),
                                                             p(stats), p(bits)), "head")
                draw[0] += 1
            return f

        def head_bwd():
            env._check(env.lib.ongym_masked_categorical_backward(env._h, p(logits), code, p(bits), p(acts), p(stats), p(H), p(g_lp),
                                                                 p(g_H), p(grad)), "head bwd")

        def torch_fwd(sample):
            def f():
                x = logits.float().masked_fill(mask == 0, -1e8)
                d = torch.distributions.Categorical(logits=x)
                a = d.sample() if sample else acts.long()
                return d.log_prob(a), d.entropy()
            return f

        x_req = logits.detach().clone().requires_grad_(True)

        def torch_bwd():
            x = x_req.float().masked_fill(mask == 0, -1e8)
            d = torch.distributions.Categorical(logits=x)
            l, h = d.log_prob(acts.long()), d.entropy()
            (l * g_lp + h * g_H).sum().backward()
            x_req.grad = None

        name = "bf16" if dt == torch.bfloat16 else "f32"
        head(nat.HEAD_SAMPLE)()        # actions / row stats / entropy / bits for the evaluate and backward timings
        for what, fn, nbytes in (("sample", head(nat.HEAD_SAMPLE), fwd_bytes), ("argmax", head(nat.HEAD_ARGMAX), fwd_bytes),
                                 ("evaluate", head(nat.HEAD_EVALUATE), fwd_bytes), ("backward", head_bwd, bwd_bytes)):
            ms = timed(fn)
            rows.append(dict(dtype=name, op=what, impl="hip head", ms=ms, gbytes=nbytes / 1e9, tb_s=nbytes / ms / 1e9))
        for what, fn in () if args.head_only else (("sample", torch_fwd(True)), ("evaluate", torch_fwd(False)), ("backward", torch_bwd)):
            rows.append(dict(dtype=name, op=what, impl="torch Categorical", ms=timed(fn)))
        del logits, grad, x_req
        torch.cuda.empty_cache()

    print(f"masked categorical head, B = {B}, n_actions = {n} (NSFNET-320 after 300 first-fit steps: {valid_frac:.3f} of the "
          f"entries valid), device events over {args.iters} calls after warm-up")
    print(f"{'dtype':5} {'op':9} {'impl':18} {'ms':>8} {'GB (alg.)':>10} {'TB/s':>6} {'torch/hip':>9}")
    for r in rows:
        ref = next((q for q in rows if q["dtype"] == r["dtype"] and q["op"] == r["op"] and q["impl"] == "hip head"), None)
        extra = (f"{r['gbytes']:10.3f} {r['tb_s']:6.2f}" if "gbytes" in r else f"{'':10} {'':6}")
        ratio = f"{r['ms'] / ref['ms']:9.1f}" if ref and r is not ref else ""
        print(f"{r['dtype']:5} {r['op']:9} {r['impl']:18} {r['ms']:8.3f} {extra} {ratio}")
    print(json.dumps(dict(batch=B, n_actions=n, valid_fraction=valid_frac, rows=rows)))


def packed_vs_bytes(env, mask, args, timed, p):
    """bf16 evaluate + backward through the _rows pair at R rows, the mask as bytes or packed bits, alternated"""
    import torch
    from optical_networking_gym import _native as nat
    B, n = mask.shape
    W = (n + 31) // 32
    dev = mask.device
    bits_b = torch.empty((B, W), dtype=torch.int32, device=dev)
    lg = torch.randn((B, n), device=dev).to(torch.bfloat16)
    a, lp, H, st = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev),
                    torch.empty((B, 2), device=dev))
    env._check(env.lib.ongym_masked_categorical(env._h, p(lg), nat.DTYPE_BF16, p(mask), nat.HEAD_SAMPLE, 0, 0, p(a), p(lp), p(H),
                                                p(st), p(bits_b)), "head")
    res = []
    for R in args.rows or (B, 262144):
        reps = -(-R // B)
        m_r, b_r = mask.repeat(reps, 1)[:R].contiguous(), bits_b.repeat(reps, 1)[:R].contiguous()
        a_r = a.repeat(reps)[:R].contiguous()
        logits = (torch.randn((R, n), device=dev) * 2).to(torch.bfloat16)
        grad = torch.empty_like(logits)
        lp, H, st = torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty((R, 2), device=dev)
        g_lp, g_H = torch.randn(R, device=dev), torch.randn(R, device=dev)
        keep = torch.empty((R, W), dtype=torch.int32, device=dev)       # bits the byte forward writes for its backward

        def run(fmt):
            m, bits_out = (m_r, keep) if fmt == nat.MASK_BYTES else (b_r, None)
            saved = keep if fmt == nat.MASK_BYTES else b_r

            def f():
                env._check(env.lib.ongym_masked_categorical_rows(env._h, R, p(logits), nat.DTYPE_BF16, p(m), fmt, nat.HEAD_EVALUATE,
                                                                 0, 0, p(a_r), p(lp), p(H), p(st),
                                                                 None if bits_out is None else p(bits_out)), "rows")
                env._check(env.lib.ongym_masked_categorical_backward_rows(env._h, R, p(logits), nat.DTYPE_BF16, p(saved), p(a_r),
                                                                          p(st), p(H), p(g_lp), p(g_H), p(grad)), "bwd rows")
            return f
        ms = {nat.MASK_BYTES: [], nat.MASK_BITS: []}
        for _ in range(args.reps):
            for fmt in (nat.MASK_BYTES, nat.MASK_BITS):
                ms[fmt].append(timed(run(fmt)))
        for fmt, name in ((nat.MASK_BYTES, "bytes"), (nat.MASK_BITS, "bits")):
            # evaluate reads logits + mask (+ writes bits for bytes); backward reads logits + bits, writes the gradient
            mbytes = R * n if fmt == nat.MASK_BYTES else R * W * 4
            nbytes = R * n * 2 + mbytes + (R * W * 4 if fmt == nat.MASK_BYTES else 0) + 2 * R * n * 2 + R * W * 4
            res.append(dict(rows=R, mask=name, ms_min=min(ms[fmt]), ms_max=max(ms[fmt]), gbytes=nbytes / 1e9,
                            tb_s=nbytes / min(ms[fmt]) / 1e9, mask_bytes_per_row=mbytes // R))
        del logits, grad, m_r, b_r
        torch.cuda.empty_cache()
    print(f"bf16 evaluate + backward (ongym_masked_categorical_rows / _backward_rows), n_actions = {n}, byte mask vs packed bits, "
          f"{args.reps} alternated rounds of {args.iters} calls (device events)")
    print(f"{'rows':>7} {'mask':5} {'ms min':>8} {'ms max':>8} {'GB (alg.)':>10} {'TB/s':>6} {'mask B/row':>10}")
    for r in res:
        print(f"{r['rows']:7d} {r['mask']:5} {r['ms_min']:8.3f} {r['ms_max']:8.3f} {r['gbytes']:10.3f} {r['tb_s']:6.2f} "
              f"{r['mask_bytes_per_row']:10d}")
    print(json.dumps(dict(batch=B, n_actions=n, packed=res)))


if __name__ == "__main__":
    main()
