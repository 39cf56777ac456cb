"""Child process of tests/test_gpu_policy_head.py: every GPU computation of that module, in ONE fresh process (PyTorch's
HIP runtime and this library's must start together, see test_caller_stream_equals_own_stream), saved to an .npz that the
tests assert on.  The reference throughout is float64 torch: log_softmax over masked_fill(~mask, -inf), p log p = 0 where
masked.

    python tests/policy_head_child.py OUT.npz
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import numpy as np
import torch

from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from optical_networking_gym.rl import masked_categorical

dev = torch.device("cuda", 0)
out = {}


def make_env(B, S=320, mtc=None, load=300.0):
    kw = dict(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), batch_size=B, num_spectrum_resources=S,
              capacity=1024, load=load, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), auto_reset=True,
              io_device=True)
    if mtc:
        kw["modulations_to_consider"] = mtc
    env = BatchedQRMSAEnv(**kw)
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    return env


def observe(env, obs=None, mask=None):
    c = env.holder.struct
    if obs is None:
        obs = torch.empty((env.batch_size, 3 + c.k_paths + c.k_paths * c.n_mods_consider * 12), dtype=torch.float32, device=dev)
        mask = torch.empty((env.batch_size, env.num_actions), dtype=torch.uint8, device=dev)
    env._check(env.lib.ongym_observe(env._h, obs.data_ptr(), mask.data_ptr()), "observe")
    return obs, mask


def step(env, actions):
    recs = torch.empty((env.batch_size, nat.STEP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    env._check(env.lib.ongym_step_actions(env._h, actions.data_ptr(), recs.data_ptr()), "step")
    return recs


def ref(logits, mask):
    """float64 (log_prob of every entry, entropy) of the exact masked distribution"""
    m = mask.bool()
    lp = torch.log_softmax(logits.double().masked_fill(~m, -float("inf")), dim=1)
    lp0 = torch.where(m, lp, torch.zeros_like(lp))         # no -inf in the product: its gradient would be NaN
    H = -(torch.where(m, lp0.exp(), torch.zeros_like(lp0)) * lp0).sum(1)
    return lp, H


def loaded_env(tag, B, **kw):
    env = make_env(B, **kw)
    env.seed(11)
    env.reset()
    env.step_policy(400, record=False)         # a loaded network: a realistic, sparse mask
    _, mask = observe(env)
    torch.cuda.synchronize()
    out[f"{tag}_mask"] = mask.cpu().numpy()
    return env, mask


def save(name, t):
    out[name] = t.detach().float().cpu().numpy() if t.is_floating_point() else t.detach().cpu().numpy()


def run_config(tag, B, **kw):
    env, mask = loaded_env(tag, B, **kw)
    n = env.num_actions
    g = torch.Generator(device=dev).manual_seed(3)
    m = mask.bool()
    # 1. evaluate, f32 and bf16: valid actions, masked ones on every 8th row, one out of range
    acts = torch.multinomial(m.float(), 1, generator=g).squeeze(1).int()
    bad = torch.multinomial((~m).float() + 1e-30, 1, generator=g).squeeze(1).int()
    acts[::8] = bad[::8]
    acts[3] = n + 5
    save(f"{tag}_eval_actions", acts)
    for dt in (torch.float32, torch.bfloat16):
        logits = (torch.randn((B, n), generator=g, device=dev) * 3).to(dt)
        _, lp, H = masked_categorical(env, logits, mask, acts)
        lp_all, H_ref = ref(logits, mask)
        lp_ref = torch.where((acts >= 0) & (acts < n), lp_all.gather(1, acts.clamp(0, n - 1).long().unsqueeze(1)).squeeze(1),
                             torch.full_like(H_ref, -float("inf")))
        lp_ref = torch.where((acts >= 0) & (acts < n) & m.gather(1, acts.clamp(0, n - 1).long().unsqueeze(1)).squeeze(1),
                             lp_ref, torch.full_like(lp_ref, -float("inf")))
        d = "f32" if dt == torch.float32 else "bf16"
        out[f"{tag}_eval_{d}_lp"], out[f"{tag}_eval_{d}_H"] = lp.cpu().double().numpy(), H.cpu().double().numpy()
        out[f"{tag}_eval_{d}_lp_ref"], out[f"{tag}_eval_{d}_H_ref"] = lp_ref.cpu().numpy(), H_ref.cpu().numpy()
    # 2. sample: validity, determinism in (seed, draw), log-probs against the reference
    logits = torch.randn((B, n), generator=g, device=dev) * 2
    a1, lp1, H1 = masked_categorical(env, logits, mask, seed=5, draw_index=0)
    a2, _, _ = masked_categorical(env, logits, mask, seed=5, draw_index=0)
    a3, _, _ = masked_categorical(env, logits, mask, seed=5, draw_index=1)
    lp_all, H_ref = ref(logits, mask)
    save(f"{tag}_sample_a1", a1); save(f"{tag}_sample_a2", a2); save(f"{tag}_sample_a3", a3)
    save(f"{tag}_sample_lp", lp1); save(f"{tag}_sample_lp_ref", lp_all.gather(1, a1.long().unsqueeze(1)).squeeze(1))
    save(f"{tag}_sample_H", H1); save(f"{tag}_sample_H_ref", H_ref)
    # 3. argmax with constructed ties: integer logits, and the row's two first valid entries set to the row's max
    logits = torch.randint(-3, 4, (B, n), generator=g, device=dev).float()
    first2 = torch.topk(m.int() * torch.arange(n, 0, -1, device=dev).int(), 2, dim=1).indices
    top = logits.masked_fill(~m, -float("inf")).amax(1, keepdim=True) + 1
    logits.scatter_(1, first2.flip(1), top.expand(-1, 2))      # the second valid entry first: argmax must still pick the first
    for dt in (torch.float32, torch.bfloat16):
        a, _, _ = masked_categorical(env, logits.to(dt), mask, deterministic=True)
        d = "f32" if dt == torch.float32 else "bf16"
        save(f"{tag}_argmax_{d}", a)
        save(f"{tag}_argmax_{d}_ref", torch.argmax(logits.to(dt).double().masked_fill(~m, -float("inf")), dim=1))
    # 4. backward, both dtypes; the mask buffer is overwritten by a fresh observation between forward and backward
    for dt in (torch.float32, torch.bfloat16):
        d = "f32" if dt == torch.float32 else "bf16"
        x = (torch.randn((B, n), generator=g, device=dev) * 3).to(dt).requires_grad_(True)
        mask_before = mask.clone()
        a, lp, H = masked_categorical(env, x, mask)
        g_lp, g_H = torch.randn(B, generator=g, device=dev), torch.randn(B, generator=g, device=dev)
        step(env, a)
        observe(env, mask=mask, obs=torch.empty((B, 3 + env.holder.struct.k_paths * (1 + env.holder.struct.n_mods_consider * 12)),
                                                 device=dev))
        out[f"{tag}_bwd_{d}_mask_changed"] = np.array(bool((mask != mask_before).any().item()))
        (lp * g_lp + H * g_H).sum().backward()
        x64 = x.detach().double().requires_grad_(True)
        lp_all, H_ref = ref(x64, mask_before)
        (lp_all.gather(1, a.long().unsqueeze(1)).squeeze(1) * g_lp.double() + H_ref * g_H.double()).sum().backward()
        save(f"{tag}_bwd_{d}_grad", x.grad)
        out[f"{tag}_bwd_{d}_grad_ref"] = x64.grad.cpu().numpy()
        out[f"{tag}_bwd_{d}_mask"] = mask_before.cpu().numpy()
    # 5. edge rows: junk in masked entries changes nothing; reject-only row; all-zero row; the next call still works
    mask = observe(env)[1]
    logits = torch.randn((B, n), generator=g, device=dev)
    junk = logits.clone()
    nm = ~mask.bool()
    junk[0::3][nm[0::3]] = float("nan")
    junk[1::3][nm[1::3]] = float("inf")
    junk[2::3][nm[2::3]] = -float("inf")
    acts = torch.multinomial(mask.float(), 1, generator=g).squeeze(1).int()
    res = {}
    for name, lg in (("clean", logits), ("junk", junk)):
        r = [masked_categorical(env, lg, mask, seed=9, draw_index=4),
             masked_categorical(env, lg, mask, deterministic=True),
             masked_categorical(env, lg, mask, acts)]
        res[name] = torch.stack([torch.stack([t.float() for t in x]) for x in r])
    out[f"{tag}_edge_junk_equal"] = np.array(bool(torch.equal(res["clean"], res["junk"])))
    m2 = mask.clone()
    m2[0, :] = 0; m2[0, n - 1] = 1            # only the reject action
    m2[1, :] = 0                              # nothing valid (a caller error)
    a, lp, H = masked_categorical(env, logits, m2, seed=9, draw_index=5)
    ae, lpe, He = masked_categorical(env, logits, m2, torch.full((B,), n - 1, dtype=torch.int32, device=dev))
    save(f"{tag}_edge_a", a); save(f"{tag}_edge_lp", lp); save(f"{tag}_edge_H", H); save(f"{tag}_edge_eval_lp", lpe)
    a, lp, H = masked_categorical(env, logits, mask, seed=9, draw_index=6)     # the next call on the same env
    lp_all, H_ref = ref(logits, mask)
    save(f"{tag}_after_a", a); save(f"{tag}_after_lp", lp); save(f"{tag}_after_H", H)
    save(f"{tag}_after_lp_ref", lp_all.gather(1, a.long().unsqueeze(1)).squeeze(1)); save(f"{tag}_after_H_ref", H_ref)
    save(f"{tag}_after_mask", mask)
    return env, mask


def chi_square(env, mask):
    """rows cut to 11 valid entries (head and tail entries of the row among them), logits over -5..5, D draws"""
    B, n = env.batch_size, env.num_actions
    rng = np.random.default_rng(1)
    m = torch.zeros_like(mask)
    logits = torch.full((B, n), 50.0, device=dev)                 # masked entries: huge logits that must not count
    keep = np.zeros((B, 11), np.int64)
    for r in range(B):
        others = rng.choice(np.arange(3, n - 3), size=5, replace=False)
        keep[r] = np.concatenate([[0, 1, 2], others, [n - 3, n - 2, n - 1]])
    kt = torch.from_numpy(keep).to(dev)
    vals = torch.from_numpy(np.stack([rng.permutation(np.linspace(-5, 5, 11)) for _ in range(B)])).float().to(dev)
    m.scatter_(1, kt, 1)
    logits.scatter_(1, kt, vals)
    D = 20000
    acts = torch.stack([masked_categorical(env, logits, m, seed=21, draw_index=d)[0] for d in range(D)])
    acts = acts.cpu().numpy()
    counts = np.stack([(acts == keep[:, j][None, :]).sum(0) for j in range(11)], 1)
    out["chi_counts"], out["chi_total"] = counts, np.array(D)
    out["chi_valid"] = np.array(bool(np.isin(acts, keep).all() and all(np.isin(acts[:, r], keep[r]).all() for r in range(B))))
    out["chi_p"] = torch.softmax(vals.double(), 1).cpu().numpy()


def mean_log_prob(env, mask):
    """E[log p(a)] = -H for a ~ p: mean log-prob of the drawn actions over all rows of a full mask and many draws"""
    B, n = env.batch_size, env.num_actions
    logits = torch.randn((B, n), generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    lps = []
    for d in range(200):
        _, lp, H = masked_categorical(env, logits, mask, seed=33, draw_index=d)
        lps.append(lp)
    out["mlp_lp"] = torch.stack(lps).cpu().numpy()
    out["mlp_H"] = H.cpu().numpy()


def sharding(mask):
    """one env of 8 replicas vs two of 4 at replica_base 0 and 4: the same draws"""
    n = mask.shape[1]
    e8, e4a, e4b = make_env(8), make_env(4), make_env(4)
    e8.seed(1, 0); e4a.seed(1, 0); e4b.seed(1, 4)
    logits = torch.randn((8, n), generator=torch.Generator(device=dev).manual_seed(7), device=dev)
    m8 = mask[:8].clone()
    got8, got4 = [], []
    for dt in (torch.float32, torch.bfloat16):
        lg = logits.to(dt)
        for d in range(20):
            got8.append(masked_categorical(e8, lg, m8, seed=3, draw_index=d)[0])
            got4.append(torch.cat([masked_categorical(e4a, lg[:4].clone(), m8[:4].clone(), seed=3, draw_index=d)[0],
                                   masked_categorical(e4b, lg[4:].clone(), m8[4:].clone(), seed=3, draw_index=d)[0]]))
    out["shard_8"], out["shard_4x2"] = torch.stack(got8).cpu().numpy(), torch.stack(got4).cpu().numpy()


def end_to_end():
    """observe -> MLP (bf16 autocast) -> masked_categorical -> step, no host synchronisation; then a backward"""
    B = 256
    env = make_env(B)
    env.seed(2); env.reset(); env.step_policy(300, record=False)
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    obs, mask = observe(env)
    n = env.num_actions
    torch.manual_seed(0)
    body = torch.nn.Sequential(torch.nn.Linear(obs.shape[1], 128), torch.nn.Tanh(), torch.nn.Linear(128, n)).to(dev)
    masks, acts, flags, losses = [], [], [], []
    f_off = nat.STEP_DTYPE.fields["flags"][1]
    for t in range(6):
        observe(env, obs, mask)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = body(obs)
        a, lp, H = masked_categorical(env, logits, mask)
        masks.append(mask.clone()); acts.append(a.clone())
        recs = step(env, a)
        flags.append(recs[:, f_off].clone())
        losses.append(-(lp.mean() + 0.01 * H.mean()))
    torch.stack(losses).sum().backward()
    torch.cuda.synchronize()
    out["e2e_logits_dtype_bf16"] = np.array(logits.dtype == torch.bfloat16)
    out["e2e_valid"] = np.array(bool(all(mk.gather(1, a.long().unsqueeze(1)).all().item() for mk, a in zip(masks, acts))))
    out["e2e_flags"] = torch.stack(flags).cpu().numpy()
    out["e2e_grad_finite"] = np.array(bool(all(p.grad is not None and torch.isfinite(p.grad).all().item()
                                               for p in body.parameters())))


def main():
    env, mask = run_config("nsf", 64)
    run_config("mc2", 48, S=160, mtc=2)
    chi_square(env, mask)
    mean_log_prob(env, mask)
    sharding(mask)
    end_to_end()
    torch.cuda.synchronize()
    np.savez(sys.argv[1], **out)
    print("policy head child ok")


if __name__ == "__main__":
    main()
