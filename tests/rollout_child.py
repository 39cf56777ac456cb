"""Child process of tests/test_gpu_rollout.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP runtime
and this library's must start together), saved to an .npz that the tests assert on.

    python tests/rollout_child.py OUT.npz

GAE (ongym_gae through optical_networking_gym.rl.gae) is checked against `gae_reference`, the sequential recurrence in float64,
and, to show the bound is attainable, SB3's float32 loop (`gae_sb3_f32`).  The head with packed masks and any row count
(ongym_masked_categorical_rows / _backward_rows) is checked against the byte-mask calls bit for bit and against float64 torch.
The end-to-end check runs tools/bench_rl.py --ppo in a child process of its own.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

CHUNK = 16          # steps per wave in k_gae (csrc/ongym_gae.hpp); the patterns below put terminations at its edges
SENT = 0x7FC0DEAD   # guard words around the outputs (a NaN payload no computation makes)
GUARD = 256


def gae_reference(reward, terminated, values, last_values, gamma, lam):
    """float64 sequential GAE: reward [T, B] (f64), terminated [T, B] (0/1), values [T, B], last_values [B] -> (A, returns)"""
    reward, values = np.asarray(reward, np.float64), np.asarray(values, np.float64)
    T = reward.shape[0]
    nnt = 1.0 - np.asarray(terminated, np.float64)
    A = np.zeros_like(values)
    a = np.zeros(values.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            vnext = np.asarray(last_values, np.float64) if t == T - 1 else values[t + 1]
            delta = reward[t] + gamma * vnext * nnt[t] - values[t]
            a = delta + gamma * lam * nnt[t] * a
            A[t] = a
    return A, A + values


def gae_sb3_f32(reward, terminated, values, last_values, gamma, lam):
    """SB3's RolloutBuffer.compute_returns_and_advantage loop in float32 (episode ends = terminated)"""
    reward, values, last_values = (np.asarray(x, np.float32) for x in (reward, values, last_values))
    T = reward.shape[0]
    nnt = (1.0 - np.asarray(terminated, np.float32)).astype(np.float32)
    g, gl = np.float32(gamma), np.float32(gamma * lam)
    A = np.zeros_like(values)
    a = np.zeros(values.shape[1], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            vnext = last_values if t == T - 1 else values[t + 1]
            delta = reward[t] + g * vnext * nnt[t] - values[t]
            a = delta + gl * nnt[t] * a
            A[t] = a
    return A


def gae_bound(A64, values, gamma, lam):
    """per column b: 2e-6 L (1 + max_t |A64| + max_t |V|), L = min(T, 64 / (1 - gamma lam)) (T when gamma lam = 1)"""
    T = A64.shape[0]
    gl = gamma * lam
    L = T if gl >= 1.0 else min(T, 64.0 / (1.0 - gl))
    with np.errstate(invalid="ignore"):
        return 2e-6 * L * (1.0 + np.nanmax(np.abs(A64), axis=0, initial=0.0) + np.nanmax(np.abs(values), axis=0, initial=0.0))


def excess(got, ref, bound):
    """max over the finite entries of |got - ref| / bound (columns), and whether the NaN patterns agree"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nan_same = bool(np.array_equal(np.isnan(got), np.isnan(ref)))
    fin = np.isfinite(ref) & np.isfinite(got)
    with np.errstate(invalid="ignore"):
        r = np.where(fin, np.abs(got - ref) / bound[None, :], 0.0)
    return float(r.max(initial=0.0)), nan_same


def main():
    import json
    import subprocess

    import torch

    from common import golden_tables, jocn_modulations
    from optical_networking_gym import _native as nat
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    from optical_networking_gym.rl import gae, masked_categorical

    dev = torch.device("cuda", 0)
    out = {}
    REC = nat.STEP_DTYPE.itemsize
    R_OFF, T_OFF = nat.STEP_DTYPE.fields["reward"][1], nat.STEP_DTYPE.fields["terminated"][1]
    envs = {}

    def make_env(B, S=320, mtc=None, episode_length=1000):
        key = (B, S, mtc, episode_length)
        if key not in envs:
            kw = dict(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=B, num_spectrum_resources=S,
                      capacity=1024, load=300.0, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), auto_reset=True,
                      episode_length=episode_length, io_device=True)
            if mtc:
                kw["modulations_to_consider"] = mtc
            env = BatchedQRMSAEnv(**kw)
            env.set_stream(torch.cuda.current_stream().cuda_stream)
            envs[key] = env
        return envs[key]

    def obs_dim(env):
        c = env.holder.struct
        return 3 + c.k_paths + c.k_paths * c.n_mods_consider * 12

    def guarded(T, B):
        whole = torch.full((T * B + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        return whole, whole[GUARD:GUARD + T * B].view(torch.float32).view(T, B)

    # ---------------------------------------------------------------------------------------------------------------- GAE
    def run_gae(tag, env, recs, values, last, gamma, lam):
        """recs uint8 [T, B, 56] on the device; values [T, B], last [B] float32 numpy"""
        T, B = values.shape
        v_d, l_d = torch.from_numpy(values).to(dev), torch.from_numpy(last).to(dev)
        before = (recs.clone(), v_d.clone(), l_d.clone())
        wa, adv = guarded(T, B)
        wr, ret = guarded(T, B)
        gae(env, recs, v_d, l_d, gamma, lam, out=(adv, ret))
        torch.cuda.synchronize()
        out[tag + "_inputs_kept"] = np.array(all(torch.equal(x.view(torch.uint8), y.view(torch.uint8))     # bitwise: NaN too
                                                 for x, y in zip(before, (recs, v_d, l_d))))
        out[tag + "_guards_kept"] = np.array(all(bool((w[:GUARD] == SENT).all() and (w[-GUARD:] == SENT).all())
                                                 for w in (wa, wr)))
        rc = recs.cpu().numpy().reshape(T, B, REC)
        reward = rc[:, :, R_OFF:R_OFF + 8].copy().view(np.float64)[:, :, 0]
        term = rc[:, :, T_OFF]
        A64, R64 = gae_reference(reward, term, values, last, gamma, lam)
        bound = gae_bound(A64, values, gamma, lam)
        out[tag + "_excess"], out[tag + "_nan_same"] = (np.array(x) for x in excess(adv.cpu().numpy(), A64, bound))
        out[tag + "_ret_excess"], out[tag + "_ret_nan_same"] = (np.array(x) for x in excess(ret.cpu().numpy(), R64, bound))
        out[tag + "_sb3_excess"], out[tag + "_sb3_nan_same"] = (
            np.array(x) for x in excess(gae_sb3_f32(reward, term, values, last, gamma, lam), A64, bound))
        out[tag + "_terminations"] = np.array(int(term.sum()))
        return adv.cpu().numpy(), ret.cpu().numpy()

    def synthetic(T, B, pattern, rng):
        rec = np.zeros((T, B), nat.STEP_DTYPE)
        rec["reward"] = rng.normal(0.0, 1.0, (T, B))
        t = np.arange(T)[:, None] + np.zeros((1, B), np.int64)
        term = {"none": np.zeros((T, B), bool), "all": np.ones((T, B), bool),
                "random": rng.random((T, B)) < 0.05,
                "chunk_m1": t % CHUNK == CHUNK - 1, "chunk": (t % CHUNK == 0) & (t > 0), "chunk_p1": t % CHUNK == 1,
                "last": t == T - 1}[pattern]
        rec["terminated"] = term
        values = rng.normal(0.0, 3.0, (T, B)).astype(np.float32)
        last = rng.normal(0.0, 3.0, B).astype(np.float32)
        recs = torch.from_numpy(rec.view(np.uint8).reshape(T, B, REC)).to(dev)
        return recs, values, last

    rng = np.random.default_rng(5)
    cases = []
    for T in (1, 2, 31, 32, 33, 257):
        for B in (1, 63, 64, 65):
            cases.append((T, B, "random", 0.99, 0.95))
    for p in ("none", "all", "chunk_m1", "chunk", "chunk_p1", "last"):
        cases.append((257, 65, p, 0.99, 0.95))
        cases.append((33, 64, p, 0.99, 0.95))
    for T in (2, 33, 257):
        cases.append((T, 65, "random", 1.0, 1.0))
        cases.append((T, 63, "none", 1.0, 1.0))
    cases += [(33, 64, "random", 0.0, 0.95), (257, 65, "random", 0.0, 0.95),
              (33, 64, "random", 0.99, 0.0), (257, 65, "random", 0.99, 0.0),
              (2048, 64, "random", 0.99, 0.95), (2048, 65, "chunk_m1", 0.99, 0.95),
              (128, 16384, "random", 0.99, 0.95), (2048, 16384, "random", 0.99, 0.95)]
    names = []
    for T, B, p, g, lam in cases:
        tag = f"gae_T{T}_B{B}_{p}_g{g}_l{lam}"
        names.append(tag)
        recs, values, last = synthetic(T, B, p, rng)
        adv, ret = run_gae(tag, make_env(B), recs, values, last, g, lam)
        if p == "last":                               # terminated at T - 1: last_values must not matter
            adv2, ret2 = guarded(T, B)[1], guarded(T, B)[1]
            gae(make_env(B), recs, torch.from_numpy(values).to(dev), torch.from_numpy(last * 7 + 1).to(dev), g, lam,
                out=(adv2, ret2))
            out[tag + "_last_ignored"] = np.array(bool(np.array_equal(adv, adv2.cpu().numpy()) and
                                                       np.array_equal(ret, ret2.cpu().numpy())))
        del recs
    # NaN in a value: at t0 it poisons A[t <= t0]; through a termination too (0 * NaN = NaN)
    T, B = 257, 65
    recs, values, last = synthetic(T, B, "random", rng)
    values[100, 7] = np.nan
    values[200, 3] = np.nan
    rc = recs.view(T, B, REC)
    rc[199, 3, T_OFF] = 1
    tag = "gae_nan"
    names.append(tag)
    adv, _ = run_gae(tag, make_env(B), recs, values, last, 0.99, 0.95)
    out[tag + "_nan_count"] = np.array(int(np.isnan(adv).sum()))
    # records written by ongym_step_actions: NSFNET-320, episode_length 40 (terminations spread through every chunk)
    T, B = 257, 1024
    env = make_env(B, episode_length=40)
    env.seed(3)
    env.reset()
    mask = torch.empty((B, env.num_actions), dtype=torch.uint8, device=dev)
    obs = torch.empty((B, obs_dim(env)), dtype=torch.float32, device=dev)
    acts = torch.empty(B, dtype=torch.int32, device=dev)
    recs = torch.empty((T, B, REC), dtype=torch.uint8, device=dev)
    for t in range(T):
        env._check(env.lib.ongym_observe(env._h, obs.data_ptr(), mask.data_ptr()), "observe")
        env._check(env.lib.ongym_sample_actions(env._h, mask.data_ptr(), 3, t, acts.data_ptr()), "sample")
        env._check(env.lib.ongym_step_actions(env._h, acts.data_ptr(), recs[t].data_ptr()), "step")
    values = rng.normal(0.0, 3.0, (T, B)).astype(np.float32)
    last = rng.normal(0.0, 3.0, B).astype(np.float32)
    tag = "gae_env"
    names.append(tag)
    run_gae(tag, env, recs, values, last, 0.99, 0.95)
    out["gae_cases"] = np.array(names)

    # --------------------------------------------------------------------------------------------------- head, packed masks
    def ref(logits, mask):
        m = mask.bool()
        lp = torch.log_softmax(logits.double().masked_fill(~m, -float("inf")), dim=1)
        lp0 = torch.where(m, lp, torch.zeros_like(lp))
        H = -(torch.where(m, lp0.exp(), torch.zeros_like(lp0)) * lp0).sum(1)
        return lp, H

    def packbits(mask):
        mk = (mask.cpu().numpy() != 0)
        R, n = mk.shape
        nw = (n + 31) // 32
        pad = np.zeros((R, nw * 32), bool)
        pad[:, :n] = mk
        return np.packbits(pad, axis=1, bitorder="little").view("<u4").view(np.int32)

    def all_outputs(env, logits, mask, g, actions=None, **kw):
        """(actions, log_prob, entropy) and, in evaluate mode, d(sum g0 lp + g1 H)/d logits"""
        x = logits.detach().clone().requires_grad_(actions is not None)
        a, lp, H = masked_categorical(env, x, mask, actions, **kw)
        res = [a.cpu().numpy(), lp.detach().cpu().numpy(), H.detach().cpu().numpy()]
        if actions is not None:
            (lp * g[0] + H * g[1]).sum().backward()
            res.append(x.grad.float().cpu().numpy())
        return res

    def same(xs, ys):
        return all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(xs, ys))

    lib = None
    for cfg, B, kw in (("nsf", 64, {}), ("mc2", 48, dict(S=160, mtc=2))):
        env = make_env(B, **kw)
        lib = env.lib
        env.seed(11)
        env.reset()
        env.step_policy(400, record=False)
        n, nw = env.num_actions, (env.num_actions + 31) // 32
        T = -(-4097 // B) + 1                       # a rollout holding >= 4097 and 3 B + 1 rows
        obs = torch.empty((B, obs_dim(env)), dtype=torch.float32, device=dev)
        mask = torch.empty((B, n), dtype=torch.uint8, device=dev)
        masks = torch.empty((T, B, n), dtype=torch.uint8, device=dev)
        bits = torch.empty((T, B, nw), dtype=torch.int32, device=dev)
        acts = torch.empty((T, B), dtype=torch.int32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(7)
        for t in range(T):                                  # the rollout: sample with mask_bits_out=bits[t], step
            env._check(env.lib.ongym_observe(env._h, obs.data_ptr(), mask.data_ptr()), "observe")
            masks[t].copy_(mask)
            a, _, _ = masked_categorical(env, torch.randn((B, n), generator=gen, device=dev), mask, seed=3,
                                         mask_bits_out=bits[t])
            acts[t].copy_(a)
            env._check(env.lib.ongym_step_actions(env._h, acts[t].data_ptr(), torch.empty((B, REC), dtype=torch.uint8,
                                                                                         device=dev).data_ptr()), "step")
        torch.cuda.synchronize()
        out[f"{cfg}_bits_match_packbits"] = np.array(bool(np.array_equal(bits.view(T * B, nw).cpu().numpy(),
                                                                         packbits(masks.view(T * B, n)))))
        mask0, bits0 = masks[T - 1], bits[T - 1]
        g = (torch.randn(B, generator=gen, device=dev), torch.randn(B, generator=gen, device=dev))
        ev = acts[T - 1].clone()
        ev[::8] = torch.multinomial((~mask0.bool()).float() + 1e-30, 1, generator=gen).squeeze(1).int()[::8]   # masked
        # bits vs bytes at R = B (the byte call goes through ongym_masked_categorical), every mode, both dtypes
        ok = True
        for dt in (torch.float32, torch.bfloat16):
            logits = (torch.randn((B, n), generator=gen, device=dev) * 3).to(dt)
            for mkw in (dict(seed=5, draw_index=2), dict(deterministic=True), dict(actions=ev)):
                aa = mkw.pop("actions", None)
                ok &= same(all_outputs(env, logits, mask0, g, aa, **mkw), all_outputs(env, logits, bits0, g, aa, **mkw))
        out[f"{cfg}_bits_equal_bytes_RB"] = np.array(ok)
        # ongym_masked_categorical_rows (R = B, bytes) against ongym_masked_categorical, raw calls, with the backward pair
        ok = True
        for dt, code in ((torch.float32, nat.DTYPE_F32), (torch.bfloat16, nat.DTYPE_BF16)):
            logits = (torch.randn((B, n), generator=gen, device=dev) * 3).to(dt)
            for mode in (nat.HEAD_SAMPLE, nat.HEAD_ARGMAX, nat.HEAD_EVALUATE):
                res = []
                for rows in (False, True):
                    o = [ev.clone(), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty((B, 2), device=dev),
                         torch.zeros((B, nw), dtype=torch.int32, device=dev), torch.empty_like(logits)]
                    p = [x.data_ptr() for x in o]
                    if rows:
                        env._check(lib.ongym_masked_categorical_rows(env._h, B, logits.data_ptr(), code, mask0.data_ptr(),
                                                                     nat.MASK_BYTES, mode, 9, 4, *p[:5]), "rows")
                        env._check(lib.ongym_masked_categorical_backward_rows(env._h, B, logits.data_ptr(), code, p[4], p[0],
                                                                              p[3], p[2], g[0].data_ptr(), g[1].data_ptr(),
                                                                              p[5]), "bwd rows")
                    else:
                        env._check(lib.ongym_masked_categorical(env._h, logits.data_ptr(), code, mask0.data_ptr(), mode, 9, 4,
                                                                *p[:5]), "head")
                        env._check(lib.ongym_masked_categorical_backward(env._h, logits.data_ptr(), code, p[4], p[0], p[3],
                                                                         p[2], g[0].data_ptr(), g[1].data_ptr(), p[5]), "bwd")
                    res.append([x.float().cpu().numpy() if x.is_floating_point() else x.cpu().numpy() for x in o])
                ok &= same(res[0], res[1])
        out[f"{cfg}_rows_equal_legacy"] = np.array(ok)
        # minibatches gathered from the rollout: R = 4097 and 3 B + 1 rows, packed vs bytes bit for bit, both against float64
        for R in (4097, 3 * B + 1):
            idx = torch.randperm(T * B, generator=gen, device=dev)[:R]
            mb_mask, mb_bits = masks.view(T * B, n)[idx], bits.view(T * B, nw)[idx]
            mb_act = acts.view(-1)[idx].clone()
            mb_act[::8] = torch.multinomial((~mb_mask.bool()).float() + 1e-30, 1, generator=gen).squeeze(1).int()[::8]
            gR = (torch.randn(R, generator=gen, device=dev), torch.randn(R, generator=gen, device=dev))
            gR[0][::8] = 0          # log_prob = -inf there: only the entropy term carries a gradient
            for dt in (torch.float32, torch.bfloat16):
                d = "f32" if dt == torch.float32 else "bf16"
                tag = f"{cfg}_mb{R}_{d}"
                logits = (torch.randn((R, n), generator=gen, device=dev) * 3).to(dt)
                got = all_outputs(env, logits, mb_bits, gR, mb_act)
                ok = same(got, all_outputs(env, logits, mb_mask, gR, mb_act))
                for mkw in (dict(seed=5, draw_index=2), dict(deterministic=True)):
                    ok &= same(all_outputs(env, logits, mb_bits, gR, **mkw), all_outputs(env, logits, mb_mask, gR, **mkw))
                out[tag + "_bits_equal_bytes"] = np.array(ok)
                x64 = logits.detach().double().requires_grad_(True)
                lp_all, H_ref = ref(x64, mb_mask)
                lp_ref = lp_all.gather(1, mb_act.long().unsqueeze(1)).squeeze(1)
                (torch.where(torch.isfinite(lp_ref), lp_ref, torch.zeros_like(lp_ref)) * gR[0].double()
                 + H_ref * gR[1].double()).sum().backward()
                lp_ref = lp_ref.detach().cpu().numpy()
                out[tag + "_outside"] = np.array(bool(np.array_equal(np.isneginf(got[1]), np.isneginf(lp_ref))
                                                      and np.isneginf(lp_ref[::8]).all()))
                fin = np.isfinite(lp_ref)
                out[tag + "_lp_err"] = np.array(float(np.abs(got[1][fin] - lp_ref[fin]).max()))
                H_ref = H_ref.detach().cpu().numpy()
                out[tag + "_H_err"] = np.array(float((np.abs(got[2] - H_ref) / np.maximum(1.0, H_ref)).max()))
                gr = x64.grad.cpu().numpy()
                out[tag + "_grad_err"] = np.array(float(np.abs(got[3] - gr).max()))
                out[tag + "_grad_scale"] = np.array(float(np.abs(gr).max()))
    torch.cuda.synchronize()

    # ----------------------------------------------------------------------------------------------------- PPO end to end
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bench_rl.py"), "--ppo", "--batch", "1024", "--n-steps", "8",
                          "--epochs", "1", "--minibatch", "2048", "--steps", "2", "--warmup", "50"],
                         capture_output=True, text=True, timeout=600)
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    out["ppo_rc"] = np.array(run.returncode)
    out["ppo_json"] = np.array(line[-1] if line else "")
    out["ppo_log"] = np.array((run.stdout[-2000:] + run.stderr[-3000:]) if run.returncode or not line else "")
    if line:
        json.loads(line[-1])
    np.savez(sys.argv[1], **out)
    print("rollout child ok")


if __name__ == "__main__":
    main()
