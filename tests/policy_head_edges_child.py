"""Child process of tests/test_gpu_policy_head_edges.py: every GPU computation of that module, in ONE fresh process (PyTorch's
HIP runtime and this library's must start together), saved to an .npz that the tests assert on.  The head is called through
the C ABI with guarded output buffers, except where a test is about the autograd path (optical_networking_gym.rl).  The
reference throughout is float64 torch on the dtype-rounded logits: log_softmax over masked_fill(~mask, -inf), p log p = 0
where p = 0.

    python tests/policy_head_edges_child.py OUT.npz
"""
import ctypes as C
import itertools
import os
import sys
import tempfile
import traceback

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import numpy as np
import torch

from common import golden_tables, jocn_modulations
from optical_networking_gym import _native as nat
from optical_networking_gym._tables import StaticTables
from optical_networking_gym.envs.batched import BatchedQRMSAEnv
from optical_networking_gym.rl import masked_categorical
from optical_networking_gym.topology import get_topology

dev = torch.device("cuda", 0)
out = {}
GUARD = 5                      # guard rows past row B - 1 in every output buffer
SENT = 0x7F                    # sentinel byte of every output buffer
DTYPES = (("f32", torch.float32, nat.DTYPE_F32), ("bf16", torch.bfloat16, nat.DTYPE_BF16))

# Row-geometry shapes: (tag, topology, modulations_to_consider, S, batch).  n = k * Mc * S + 1 covers every residue of
# n mod 8 at three sizes: tiny rows (n = 2..9, shorter than one chunk: a 4-node ring with k = 1 path), ~2000 (NSFNET, k = 5,
# Mc = 1) and the largest (NSFNET, Mc = 5, S = 1016..1023: n = 25401..25576).  Batches 1, 4m + 1, 4m + 2, 4m + 3.
SHAPES = ([(f"t{s + 1}", "ring4k1", 1, s, b) for s, b in zip(range(1, 9), (1, 33, 34, 35, 37, 38, 39, 41))]
          + [(f"m{5 * s + 1}", "nsfnet", 1, s, b) for s, b in zip(range(400, 408), (5, 6, 7, 1, 9, 10, 11, 13))]
          + [(f"l{25 * s + 1}", "nsfnet", 5, s, b) for s, b in zip(range(1016, 1024), (6, 7, 1, 5, 3, 2, 9, 10))])


def topology(name, n_nodes, edges, k):
    f = os.path.join(tempfile.mkdtemp(prefix="policy_head_edges_"), name + ".txt")
    with open(f, "w") as fh:
        fh.write("\n".join([str(n_nodes), str(len(edges))] + [f"{u} {v} {w}" for u, v, w in edges]) + "\n")
    return StaticTables.from_topology(get_topology(f, None, jocn_modulations(), 80, 0.2, 4.5, k))


_tables = {}


def tables(name):
    if name not in _tables:
        if name == "nsfnet":
            _tables[name] = golden_tables("nsfnet")
        elif name == "ring4k1":
            _tables[name] = topology(name, 4, [(1, 2, 150), (2, 3, 160), (3, 4, 170), (4, 1, 180)], 1)
        else:                                  # "k6k<k>": complete graph on 6 nodes (65 simple paths per pair), k paths
            k = int(name[3:])
            _tables[name] = topology(name, 6, [(u, v, 150 + 10 * ((u + v) % 5)) for u, v in itertools.combinations(range(1, 7), 2)], k)
    return _tables[name]


def make_env(topo, B, S, mtc=None):
    kw = dict(tables=tables(topo), modulations=jocn_modulations(), batch_size=B, num_spectrum_resources=S, capacity=1024,
              load=300.0, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), auto_reset=True, io_device=True)
    if mtc:
        kw["modulations_to_consider"] = mtc
    env = BatchedQRMSAEnv(**kw)
    env.set_stream(torch.cuda.current_stream().cuda_stream)
    return env


def buf(rows, per_row, dtype):
    """[rows + GUARD, per_row] of `dtype` filled with the sentinel byte; returns (whole buffer, the first `rows` rows)"""
    nbytes = (rows + GUARD) * per_row * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((nbytes,), SENT, dtype=torch.uint8, device=dev).view(dtype).view(rows + GUARD, per_row)
    return whole, whole[:rows]


def guard_intact(whole, rows):
    return bool((whole[rows:].contiguous().view(torch.uint8) == SENT).all().item())


def all_written(view):
    """no element of `view` still holds the sentinel pattern"""
    b = view.contiguous().view(torch.uint8).view(view.shape[0], -1, view.element_size())
    return bool((b != SENT).any(-1).all().item())


def fwd(env, logits, code, mask, mode, seed=0, draw=0, actions=None):
    """one ongym_masked_categorical call on guarded outputs; a dict of numpy results + the guard / written checks"""
    B, n = logits.shape
    nw = (n + 31) // 32
    aw, a = buf(B, 1, torch.int32)
    if actions is not None:
        a.copy_(actions.view(B, 1))
    lw, lp = buf(B, 1, torch.float32)
    hw, H = buf(B, 1, torch.float32)
    sw, st = buf(B, 2, torch.float32)
    bw, bits = buf(B, nw, torch.int32)
    rc = env.lib.ongym_masked_categorical(env._h, C.c_void_p(logits.data_ptr()), code, C.c_void_p(mask.data_ptr()), mode,
                                          C.c_uint64(seed), C.c_uint64(draw), C.c_void_p(a.data_ptr()), C.c_void_p(lp.data_ptr()),
                                          C.c_void_p(H.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(bits.data_ptr()))
    torch.cuda.synchronize()
    r = dict(rc=rc, a=a.view(-1), lp=lp.view(-1), H=H.view(-1), stats=st, bits=bits)
    r["guard"] = all(guard_intact(w, B) for w in (aw, lw, hw, sw, bw))
    r["written"] = all(all_written(v) for v in ([] if mode == nat.HEAD_EVALUATE else [a]) + [lp, H, st])
    return r


def bwd(env, logits, code, f, g_lp, g_H):
    """ongym_masked_categorical_backward from forward result f on a guarded gradient buffer"""
    B, n = logits.shape
    gw, g = buf(B, n, logits.dtype)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
    rc = env.lib.ongym_masked_categorical_backward(env._h, p(logits), code, p(f["bits"]), p(f["a"]), p(f["stats"]), p(f["H"]),
                                                   p(g_lp), p(g_H), p(g))
    torch.cuda.synchronize()
    return dict(rc=rc, g=g, guard=guard_intact(gw, B), written=all_written(g))


def ref(logits, mask):
    """float64 log-probabilities of every entry (-inf where masked) and entropy; p log p = 0 where p = 0"""
    m = mask.bool()
    lp = torch.log_softmax(logits.double().masked_fill(~m, -float("inf")), dim=1)
    p = lp.exp()
    H = -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(1)
    return lp, H


def ref_grad(logits, mask, actions, g_lp, g_H):
    """float64 d(g_lp log p_a + g_H H)/dx: valid_j (g_lp (delta_ja - p_j) - g_H p_j (log p_j + H)), delta only for an action
    inside the mask; a valid entry of -inf counts as masked; either g may be None"""
    lp, H = ref(logits, mask)
    B, n = logits.shape
    valid = mask.bool() & (logits.double() != -float("inf"))
    p = lp.exp()
    g = torch.zeros((B, n), dtype=torch.float64, device=dev)
    if g_lp is not None:
        a = actions.long()
        inr = (a >= 0) & (a < n)
        delta = torch.zeros_like(g)
        delta[inr.nonzero().squeeze(1), a[inr]] = 1.0
        g += g_lp.double()[:, None] * (delta * valid - p)
    if g_H is not None:
        lp0 = torch.where(p > 0, lp, torch.zeros_like(lp))
        g -= g_H.double()[:, None] * p * (lp0 + H[:, None])
    return torch.where(valid, g, torch.zeros_like(g))


def packbits(mask):
    """the bit-packed mask as little-endian uint32 words, padding bits 0"""
    mk = (mask.cpu().numpy() != 0)
    B, n = mk.shape
    nw = (n + 31) // 32
    pad = np.zeros((B, nw * 32), bool)
    pad[:, :n] = mk
    return np.packbits(pad, axis=1, bitorder="little").view("<u4").view(np.int32)


def npy(t):
    return t.detach().cpu().double().numpy() if t.is_floating_point() else t.detach().cpu().numpy()


def row_masks(B, n, g):
    """uint8 masks with values 1, 2 and 255: row r % 4 = 0 sparse (~5 %), 1 dense (~95 %), 2 only entries in the partial
    head and tail chunks and on lane boundaries (8c - s0 - 1 / 8c - s0, 512c - 1 / 512c, both in row and in global chunk
    terms), 3 half; every row keeps at least one valid entry"""
    u = torch.rand((B, n), generator=g, device=dev)
    m = torch.zeros((B, n), dtype=torch.bool, device=dev)
    for r in range(B):
        kind = r % 4
        if kind == 0:
            m[r] = u[r] < 0.05
        elif kind == 1:
            m[r] = u[r] < 0.95
        elif kind == 3:
            m[r] = u[r] < 0.5
        else:
            s0 = (r * n) % 8                   # the row's offset in its first chunk
            edges = set(range(min(n, (8 - s0) % 8 or 8)))                 # partial head chunk (else the first chunk)
            edges |= set(range(max(0, n - ((s0 + n) % 8 or 8)), n))       # partial tail chunk (else the last chunk)
            for c in range(0, n + 512, 512):   # lane 63 -> lane 0, in row entries and in the row's chunk grid
                edges |= {c - 1, c, c - s0 - 1, c - s0}
            for c in range(0, n // 8 + 2, 7):  # neighbouring lanes
                edges |= {8 * c - s0 - 1, 8 * c - s0}
            m[r, sorted(j for j in edges if 0 <= j < n)] = True
        if not m[r].any():
            m[r, int(torch.randint(0, n, (1,), generator=g, device=dev))] = True
    vals = torch.tensor([1, 2, 255], dtype=torch.uint8, device=dev)[torch.randint(0, 3, (B, n), generator=g, device=dev)]
    return torch.where(m, vals, torch.zeros_like(vals))


def geometry(tag, env, g):
    """item 1 / 3 / 4: all three modes and the backward, f32 with a {1, 2, 255} uint8 mask and bf16 with a bool mask"""
    B, n = env.batch_size, env.num_actions
    mask8 = row_masks(B, n, g)
    m = mask8.bool()
    out[f"{tag}_mask"] = npy(mask8)
    for d, dt, code in DTYPES:
        mask = mask8 if d == "f32" else m
        x = (torch.randn((B, n), generator=g, device=dev) * 3).to(dt)
        lp_all, H_ref = ref(x, m)
        k = f"{tag}_{d}"
        fs = fwd(env, x, code, mask, nat.HEAD_SAMPLE, seed=5, draw=1)
        fa = fwd(env, x, code, mask, nat.HEAD_ARGMAX)
        # evaluate: valid actions (row % 5 in 0..2), a masked one (3), out of range (4: -1 or n + 3)
        acts = torch.multinomial(m.float(), 1, generator=g).squeeze(1).int()
        for r in range(B):
            if r % 5 == 3 and (~m[r]).any():
                acts[r] = int((~m[r]).nonzero()[0, 0])
            elif r % 5 == 4:
                acts[r] = -1 if (r // 5) % 2 else n + 3
        fe = fwd(env, x, code, mask, nat.HEAD_EVALUATE, actions=acts)
        g_lp, g_H = torch.randn(B, generator=g, device=dev), torch.randn(B, generator=g, device=dev)
        fb = bwd(env, x, code, fe, g_lp, g_H)
        out[k + "_rc"] = np.array([fs["rc"], fa["rc"], fe["rc"], fb["rc"]])
        out[k + "_guard"] = np.array([fs["guard"], fa["guard"], fe["guard"], fb["guard"]])
        out[k + "_written"] = np.array([fs["written"], fa["written"], fe["written"], fb["written"]])
        out[k + "_bits"] = np.stack([npy(f["bits"]) for f in (fs, fa, fe)])
        out[k + "_bits_ref"] = packbits(mask)
        out[k + "_sample_a"], out[k + "_sample_lp"], out[k + "_sample_H"] = npy(fs["a"]), npy(fs["lp"]), npy(fs["H"])
        out[k + "_sample_lp_ref"] = npy(lp_all.gather(1, fs["a"].long().clamp(0, n - 1).unsqueeze(1)).squeeze(1))
        out[k + "_argmax_a"], out[k + "_argmax_lp"], out[k + "_argmax_H"] = npy(fa["a"]), npy(fa["lp"]), npy(fa["H"])
        out[k + "_argmax_ref"] = npy(torch.argmax(x.double().masked_fill(~m, -float("inf")), dim=1))
        out[k + "_eval_lp"], out[k + "_eval_H"] = npy(fe["lp"]), npy(fe["H"])
        inr = (acts >= 0) & (acts < n)
        lpa = lp_all.gather(1, acts.long().clamp(0, n - 1).unsqueeze(1)).squeeze(1)
        out[k + "_eval_lp_ref"] = npy(torch.where(inr, lpa, torch.full_like(lpa, -float("inf"))))
        out[k + "_H_ref"] = npy(H_ref)
        out[k + "_grad"] = npy(fb["g"]).astype(np.float32)
        out[k + "_grad_ref"] = npy(ref_grad(x, m, acts, g_lp, g_H))


def argmax_ties(tag, env, g):
    """item 2: equal maxima where the merge order matters; row r % 6: split across lanes (the lower entry in the higher
    lane), inside one full chunk, in the partial head chunk, in the partial tail chunk, across the lane-63 -> lane-0 wrap,
    three-way over all of them"""
    B, n = env.batch_size, env.num_actions
    m = torch.rand((B, n), generator=g, device=dev) < 0.9
    for d, dt, code in DTYPES:
        x = torch.randn((B, n), generator=g, device=dev)
        for r in range(B):
            s0 = (r * n) % 8
            at = lambda c, e: 8 * c - s0 + e          # noqa: E731  row entry of element e of chunk c
            cases = [[at(40, 3), at(67, 1)], [at(10, 2), at(10, 5)], [0, 1] if s0 <= 6 else [0, 8],
                     [n - 2, n - 1], [at(63, 7), at(64, 0)], [at(40, 3), at(67, 1), at(63, 7), at(64, 0), n - 1]]
            ties = [j for j in cases[r % 6] if 0 <= j < n]
            x[r, ties] = x[r].abs().max() + 1.0
            m[r, ties] = True
        x = x.to(dt)
        f = fwd(env, x, code, m.to(torch.uint8), nat.HEAD_ARGMAX)
        out[f"{tag}_{d}_ties_a"] = npy(f["a"])
        out[f"{tag}_{d}_ties_ref"] = npy(torch.argmax(x.double().masked_fill(~m, -float("inf")), dim=1))


def value_edges(env, g):
    """item 5: common offsets, flat rows, a peaked row, a row spanning +-3e38"""
    B, n = env.batch_size, env.num_actions
    m = torch.rand((B, n), generator=g, device=dev) < 0.9
    m[:, n - 1] = True
    acts = torch.multinomial(m.float(), 1, generator=g).squeeze(1).int()
    g_lp, g_H = torch.randn(B, generator=g, device=dev), torch.randn(B, generator=g, device=dev)
    cases = [("f32", c) for c in (1e2, -1e2, 1e3, -1e3, 1e4, -1e4)] + [("bf16", 1e2), ("bf16", -1e2)]
    for d, c in cases:
        dt, code = (torch.float32, nat.DTYPE_F32) if d == "f32" else (torch.bfloat16, nat.DTYPE_BF16)
        x = (torch.randn((B, n), generator=g, device=dev) * 3 + c).to(dt)
        k = f"off_{d}_{c:+.0e}"
        fe = fwd(env, x, code, m.to(torch.uint8), nat.HEAD_EVALUATE, actions=acts)
        fb = bwd(env, x, code, fe, g_lp, g_H)
        lp_all, H_ref = ref(x, m)
        out[k + "_lp"], out[k + "_H"] = npy(fe["lp"]), npy(fe["H"])
        out[k + "_lp_ref"], out[k + "_H_ref"] = npy(lp_all.gather(1, acts.long().unsqueeze(1)).squeeze(1)), npy(H_ref)
        out[k + "_grad"], out[k + "_grad_ref"] = npy(fb["g"]).astype(np.float32), npy(ref_grad(x, m, acts, g_lp, g_H))
    # flat rows (every valid logit equal: H = log #valid), a peaked row (one entry 40 above the rest), a row over +-3e38
    x = torch.full((B, n), 1.5, device=dev)
    x[0] = torch.randn(n, generator=g, device=dev)
    x[0, int(m[0].nonzero()[len(m[0].nonzero()) // 2, 0])] += 40.0
    x[1] = (torch.rand(n, generator=g, device=dev) * 2 - 1) * 3e38
    x[2, :] = -7.25
    f = fwd(env, x, nat.DTYPE_F32, m.to(torch.uint8), nat.HEAD_EVALUATE, actions=acts)
    fs = fwd(env, x, nat.DTYPE_F32, m.to(torch.uint8), nat.HEAD_SAMPLE, seed=2)
    fb = bwd(env, x, nat.DTYPE_F32, f, g_lp, g_H)
    lp_all, H_ref = ref(x, m)
    out["vals_H"], out["vals_H_ref"], out["vals_nvalid"] = npy(f["H"]), npy(H_ref), npy(m.sum(1))
    out["vals_lp"], out["vals_lp_ref"] = npy(f["lp"]), npy(lp_all.gather(1, acts.long().unsqueeze(1)).squeeze(1))
    out["vals_sample_lp"] = npy(fs["lp"])
    out["vals_sample_lp_ref"] = npy(lp_all.gather(1, fs["a"].long().unsqueeze(1)).squeeze(1))
    out["vals_sample_a"], out["vals_mask"] = npy(fs["a"]), npy(m)
    out["vals_grad"], out["vals_grad_ref"] = npy(fb["g"]).astype(np.float32), npy(ref_grad(x, m, acts, g_lp, g_H))


def nonfinite(tag, env, g):
    """item 6: -inf in valid entries == those entries masked, bit for bit; all-(-inf) rows; NaN / +inf poison their row"""
    B, n = env.batch_size, env.num_actions
    assert B >= 6
    m = torch.rand((B, n), generator=g, device=dev) < 0.7
    m[:, n - 1] = True
    for d, dt, code in DTYPES:
        x = (torch.randn((B, n), generator=g, device=dev) * 3).to(dt)
        ninf = torch.rand((B, n), generator=g, device=dev) < 0.2
        for r in range(0, B, 2):               # every lane's first chunk (chunks 0..63) entirely -inf in the even rows
            ninf[r, : 8 * 64 - (r * n) % 8] = True
        ninf[B - 1] = True                     # every valid entry -inf: a row with no valid entry
        ninf &= m
        xi = x.masked_fill(ninf, -float("inf"))
        mo = m & ~ninf
        acts = torch.multinomial(mo.float() + 1e-30, 1, generator=g).squeeze(1).int()
        acts[1] = int(ninf[1].nonzero()[0, 0])  # evaluate an action whose logit is -inf
        g_lp, g_H = torch.randn(B, generator=g, device=dev), torch.randn(B, generator=g, device=dev)
        k = f"{tag}_{d}"
        res = {}
        for name, lg, mk in (("inf", xi, m), ("masked", x, mo)):
            fs = fwd(env, lg, code, mk.to(torch.uint8), nat.HEAD_SAMPLE, seed=3, draw=7)
            fa = fwd(env, lg, code, mk.to(torch.uint8), nat.HEAD_ARGMAX)
            fe = fwd(env, lg, code, mk.to(torch.uint8), nat.HEAD_EVALUATE, actions=acts)
            gr = bwd(env, lg, code, fe, g_lp, g_H)["g"]
            res[name] = (fs, fa, fe, gr)
            for mode, f in (("sample", fs), ("argmax", fa), ("eval", fe)):
                out[f"{k}_{name}_{mode}_a"], out[f"{k}_{name}_{mode}_lp"] = npy(f["a"]), npy(f["lp"])
                out[f"{k}_{name}_{mode}_H"] = npy(f["H"])
            out[f"{k}_{name}_grad"] = npy(gr).astype(np.float32)
        out[k + "_ninf"], out[k + "_mask"] = npy(ninf), npy(m)
        lp_all, H_ref = ref(xi, m)
        out[k + "_H_ref"] = npy(H_ref)
        out[k + "_eval_lp_ref"] = npy(lp_all.gather(1, acts.long().unsqueeze(1)).squeeze(1))
        # NaN (rows 1, 4) and +inf (rows 2, 5: one entry; row 5 also a NaN) in valid entries; the other rows must not change
        xp = x.clone()
        for r, vals in ((1, [float("nan")]), (2, [float("inf")]), (4, [float("nan")] * 3), (5, [float("inf"), float("nan")])):
            js = m[r].nonzero()[:, 0]
            pick = js[torch.randperm(len(js), generator=torch.Generator().manual_seed(r))[: len(vals)].to(dev)]
            xp[r, pick] = torch.tensor(vals, device=dev).to(dt)
        for name, lg in (("clean", x), ("poison", xp)):
            acts_p = torch.multinomial(m.float(), 1, generator=torch.Generator(device=dev).manual_seed(9)).squeeze(1).int()
            for mode, f in (("sample", fwd(env, lg, code, m.to(torch.uint8), nat.HEAD_SAMPLE, seed=4, draw=2)),
                            ("argmax", fwd(env, lg, code, m.to(torch.uint8), nat.HEAD_ARGMAX)),
                            ("eval", fwd(env, lg, code, m.to(torch.uint8), nat.HEAD_EVALUATE, actions=acts_p))):
                out[f"{k}_{name}_{mode}_a"], out[f"{k}_{name}_{mode}_lp"] = npy(f["a"]), npy(f["lp"])
                out[f"{k}_{name}_{mode}_H"] = npy(f["H"])
        out[k + "_poison_rows"] = np.array([1, 2, 4, 5])


def backward_edges(tag, env, g):
    """item 7: g_lp / g_H NULL one at a time; evaluate-mode autograd with masked, negative and >= n actions; reject-only
    and empty rows"""
    B, n = env.batch_size, env.num_actions
    m = torch.rand((B, n), generator=g, device=dev) < 0.5
    m[:, n - 1] = True
    m[0] = False
    m[0, n - 1] = True                         # only the reject entry
    m[1] = False                               # nothing valid
    for d, dt, code in DTYPES:
        k = f"{tag}_{d}"
        x = (torch.randn((B, n), generator=g, device=dev) * 3).to(dt)
        fs = fwd(env, x, code, m.to(torch.uint8), nat.HEAD_SAMPLE, seed=6)
        g_lp, g_H = torch.randn(B, generator=g, device=dev), torch.randn(B, generator=g, device=dev)
        for name, a, b in (("nolp", None, g_H), ("noH", g_lp, None), ("both", g_lp, g_H)):
            gr = bwd(env, x, code, fs, a, b)
            out[f"{k}_{name}_grad"] = npy(gr["g"]).astype(np.float32)
            out[f"{k}_{name}_grad_ref"] = npy(ref_grad(x, m, fs["a"], a, b))
            out[f"{k}_{name}_ok"] = np.array([gr["rc"] == 0, gr["guard"], gr["written"]])
        out[k + "_sample_a"], out[k + "_mask"] = npy(fs["a"]), npy(m)
        # evaluate through autograd: masked, negative and >= n actions get log_prob -inf and the gradient -g_lp p_j
        acts = torch.multinomial(m.float() + 1e-30, 1, generator=g).squeeze(1).int()
        for r in range(2, B):
            if r % 3 == 0:
                acts[r] = int((~m[r]).nonzero()[0, 0])
            elif r % 3 == 1:
                acts[r] = -3 if r % 2 else n + 7
        acts[0] = n - 1
        xr = x.detach().clone().requires_grad_(True)
        _, lp, H = masked_categorical(env, xr, m.to(torch.uint8), acts)
        torch.autograd.backward([lp, H], [g_lp, g_H])
        out[k + "_auto_lp"], out[k + "_auto_H"] = npy(lp), npy(H)
        out[k + "_auto_grad"] = npy(xr.grad).astype(np.float32)
        out[k + "_auto_grad_ref"] = npy(ref_grad(x, m, acts, g_lp, g_H))
        out[k + "_auto_acts"] = npy(acts)


def sampler(tag, env, g, D=20000):
    """item 8: chi-square of the draws on ~100 valid entries over every lane and both partial chunks, with ties between the
    even and odd entry of one counter pair"""
    B, n = env.batch_size, env.num_actions
    rng = np.random.default_rng(int(n))
    keeps = []
    for r in range(B):
        s0 = (r * n) % 8
        nch = (s0 + n + 7) // 8
        ks = {0, n - 1, n - 2}
        for lane in range(64):                 # one entry in each lane's chunks
            c = lane + 64 * int(rng.integers(0, max(1, (nch - lane + 63) // 64)))
            ks.add(min(n - 1, max(0, 8 * c - s0 + int(rng.integers(0, 8)))))
        while len(ks) < 96:
            ks.add(int(rng.integers(0, n)))
        pairs = []
        for p in rng.choice(np.arange(1, n // 2 - 1), size=2, replace=False):
            ks |= {2 * int(p), 2 * int(p) + 1}
            pairs.append(2 * int(p))
        keep = np.array(sorted(ks))
        vals = rng.uniform(-2, 2, len(keep))
        for p in pairs:                        # equal logits for the pair's even and odd entry
            vals[np.searchsorted(keep, p + 1)] = vals[np.searchsorted(keep, p)]
        keeps.append((keep, vals))
    K = max(len(k) for k, _ in keeps)
    m = torch.zeros((B, n), dtype=torch.uint8, device=dev)
    x = torch.full((B, n), 60.0, device=dev)   # masked entries: huge logits that must not count
    for r, (keep, vals) in enumerate(keeps):
        kt = torch.from_numpy(keep).to(dev)
        m[r, kt] = 1
        x[r, kt] = torch.from_numpy(vals).float().to(dev)
    nw = (n + 31) // 32
    a = torch.empty(B, dtype=torch.int32, device=dev)
    acts = torch.empty((D, B), dtype=torch.int32, device=dev)
    for dr in range(D):
        rc = env.lib.ongym_masked_categorical(env._h, C.c_void_p(x.data_ptr()), nat.DTYPE_F32, C.c_void_p(m.data_ptr()),
                                              nat.HEAD_SAMPLE, C.c_uint64(17), C.c_uint64(dr), C.c_void_p(a.data_ptr()),
                                              None, None, None, None)
        assert rc == 0
        acts[dr] = a
    acts = acts.cpu().numpy()
    counts = np.zeros((B, K), np.int64)
    probs = np.zeros((B, K))
    valid = True
    for r, (keep, vals) in enumerate(keeps):
        valid &= bool(np.isin(acts[:, r], keep).all())
        counts[r, : len(keep)] = (acts[:, r][:, None] == keep[None, :]).sum(0)
        probs[r, : len(keep)] = torch.softmax(torch.from_numpy(x[r].double().cpu().numpy()[keep]), 0).numpy()
    out[f"{tag}_chi_counts"], out[f"{tag}_chi_p"], out[f"{tag}_chi_valid"] = counts, probs, np.array(valid)
    out[f"{tag}_chi_total"], out[f"{tag}_chi_nw"] = np.array(D), np.array(nw)


def limit(g):
    """item 9: n_actions = 128 899 (k = 21 paths, 6 formats, S = 1023) runs; 135 037 (k = 22) is ONGYM_E_LIMIT before any
    launch (no output touched)"""
    for k, tag in ((21, "lim_ok"), (22, "lim_over")):
        env = make_env(f"k6k{k}", 2, 1023)
        B, n = env.batch_size, env.num_actions
        m = torch.rand((B, n), generator=g, device=dev) < 0.3
        x = torch.randn((B, n), generator=g, device=dev) * 3
        acts = torch.multinomial(m.float(), 1, generator=g).squeeze(1).int()
        f = fwd(env, x, nat.DTYPE_F32, m.to(torch.uint8), nat.HEAD_EVALUATE, actions=acts)
        lp_all, H_ref = ref(x, m)
        out[tag + "_n"], out[tag + "_rc"] = np.array(n), np.array(f["rc"])
        out[tag + "_guard"], out[tag + "_written"] = np.array(f["guard"]), np.array(f["written"])
        out[tag + "_untouched"] = np.array(all(bool((t.contiguous().view(torch.uint8) == SENT).all().item())
                                               for t in (f["lp"], f["H"], f["stats"], f["bits"])))
        out[tag + "_lp"], out[tag + "_H"] = npy(f["lp"]), npy(f["H"])
        out[tag + "_lp_ref"] = npy(lp_all.gather(1, acts.long().unsqueeze(1)).squeeze(1))
        out[tag + "_H_ref"] = npy(H_ref)
        out[tag + "_bits"], out[tag + "_bits_ref"] = npy(f["bits"]), packbits(m)
        env.close()


def section(name, fn, *args):
    try:
        fn(*args)
        out[f"ok_{name}"] = np.array(True)
    except Exception:                          # recorded for the test that reads this section; the others still run
        out[f"ok_{name}"] = np.array(False)
        out[f"err_{name}"] = np.array(traceback.format_exc()[-3000:])
        print(f"section {name} failed:\n{traceback.format_exc()}", file=sys.stderr)


def main():
    g = torch.Generator(device=dev).manual_seed(1234)
    envs = {}

    def geo(tag, topo, mtc, S, B):
        env = make_env(topo, B, S, mtc)
        envs[tag] = env
        out[f"{tag}_n"], out[f"{tag}_B"] = np.array(env.num_actions), np.array(B)
        geometry(tag, env, g)
    for tag, topo, mtc, S, B in SHAPES:
        section(f"geo_{tag}", geo, tag, topo, mtc, S, B)
    for tag in ("m2016", "m2021", "l25401", "l25576"):
        section(f"ties_{tag}", lambda t: argmax_ties(t, tie_env(t), g), tag)
    section("vals", lambda: value_edges(make_env("nsfnet", 7, 400, 1), g))
    for tag, S in (("m2001", 400), ("m2036", 407)):
        section(f"nonfinite_{tag}", lambda t=tag, s=S: nonfinite("nf_" + t, make_env("nsfnet", 7, s, 1), g))
        section(f"bwd_{tag}", lambda t=tag, s=S: backward_edges("be_" + t, make_env("nsfnet", 9, s, 1), g))
    for tag, S in (("m2016", 403), ("m2021", 404)):
        section(f"chi_{tag}", lambda t=tag, s=S: sampler(t, make_env("nsfnet", 5, s, 1), g))
    section("limit", limit, g)
    torch.cuda.synchronize()
    np.savez(sys.argv[1], **out)
    print("policy head edges child ok")


def tie_env(tag):
    """12-row NSFNET environments for the argmax ties (12 rows: each case at two row offsets s0)"""
    S, mtc = {"m2016": (403, 1), "m2021": (404, 1), "l25401": (1016, 5), "l25576": (1023, 5)}[tag]
    return make_env("nsfnet", 12, S, mtc)


if __name__ == "__main__":
    main()
