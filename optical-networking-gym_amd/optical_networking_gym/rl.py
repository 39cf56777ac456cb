"""Masked categorical action head on device: sample / argmax / evaluate a policy's logits over the environment's action mask;
GAE over a rollout of step records.

`masked_categorical` stands in for the action distribution of the reference's masked PPO training
(examples/ONDM_2025/train_multi_masked_ppo.py: sb3-contrib MaskablePPO, whose MaskableCategorical is a Categorical over the
logits with masked entries filled with -1e8).  It computes the exact masked distribution in one HIP pass per row
(ongym_masked_categorical, include/ongym.h): masked entries do not exist whatever their logit holds, log-probabilities are
normalised over the valid entries only and the entropy is -sum_valid p log p.  `log_prob` and `entropy` carry gradients to
the logits through ongym_masked_categorical_backward.

Non-finite logits in valid entries: -inf means probability 0, as in torch's Categorical (the same outputs, bit for bit, as with
that entry masked; its gradient is 0); a row whose valid entries are all -inf is a row with no valid entry (reject action, NaN
log_prob and entropy).  NaN or +inf makes that row's log_prob and entropy NaN, so a diverged policy shows; its action is still
a valid entry and the other rows are not affected.

    obs, mask = ...                                         # ongym_observe into torch tensors (io_device=True)
    logits = policy(obs)                                    # [B, n_actions], float32 or bfloat16
    actions, log_prob, entropy = masked_categorical(env, logits, mask)            # MaskableCategorical.sample()
    actions, _, _ = masked_categorical(env, logits, mask, deterministic=True)    # .mode()
    _, log_prob, entropy = masked_categorical(env, logits, mask, actions)        # evaluate_actions (PPO update)

A PPO rollout keeps the packed mask of every step (`mask_bits_out=bits[t]`, 8x smaller than the bytes) and evaluates
minibatches of any row count from it; `gae` turns the rollout's step records and values into advantages and returns:

    actions, log_prob, _ = masked_categorical(env, logits, mask, mask_bits_out=bits[t])       # rollout step t
    adv, ret = gae(env, recs, values, last_values, gamma=0.99, gae_lambda=0.95)             # after T steps
    _, log_prob, entropy = masked_categorical(env, logits_mb, bits.view(-1, nw)[idx], acts.view(-1)[idx])   # minibatch

Every launch goes on the environment's stream, which must be torch's current stream (`env.set_stream(
torch.cuda.current_stream().cuda_stream)`): nothing synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _native as nat

_DTYPES = {torch.float32: nat.DTYPE_F32, torch.bfloat16: nat.DTYPE_BF16}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _device(env) -> torch.device:
    return torch.device("cuda", env.holder.struct.device)


def _check_stream(env):
    handle = getattr(env, "stream_handle", None)
    if handle is None or handle != torch.cuda.current_stream().cuda_stream:
        raise ValueError("the environment must run on torch's current stream: "
                         "env.set_stream(torch.cuda.current_stream().cuda_stream)")


class _MaskedCategorical(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, env, mask, actions, mode, seed, draw_index, mask_bits_out=None):
        R, n = logits.shape
        dev = logits.device
        packed = mask.dtype == torch.int32
        out_actions = actions.clone() if actions is not None else torch.empty(R, dtype=torch.int32, device=dev)
        log_prob = torch.empty(R, dtype=torch.float32, device=dev)
        entropy = torch.empty(R, dtype=torch.float32, device=dev)
        stats = torch.empty((R, 2), dtype=torch.float32, device=dev)     # per row: max valid logit, log sum of e^(x - max)
        # the packed mask is saved, not the caller's byte mask: the next observation overwrites that buffer through a raw
        # pointer, which torch's version counter cannot see.  A packed mask given as input is saved as it is.
        if packed:
            bits = mask
        elif mask_bits_out is not None:
            bits = mask_bits_out
        else:
            bits = torch.empty((R, (n + 31) // 32), dtype=torch.int32, device=dev)
        # the environment's own shape (byte mask, one row per replica) keeps the original entry points
        ctx.rows = None if (not packed and R == env.batch_size) else R
        if ctx.rows is None:
            env._check(env.lib.ongym_masked_categorical(env._h, _ptr(logits), _DTYPES[logits.dtype], _ptr(mask), int(mode),
                                                        C.c_uint64(seed), C.c_uint64(draw_index), _ptr(out_actions),
                                                        _ptr(log_prob), _ptr(entropy), _ptr(stats), _ptr(bits)),
                       "ongym_masked_categorical")
        else:
            env._check(env.lib.ongym_masked_categorical_rows(env._h, R, _ptr(logits), _DTYPES[logits.dtype], _ptr(mask),
                                                             nat.MASK_BITS if packed else nat.MASK_BYTES, int(mode),
                                                             C.c_uint64(seed), C.c_uint64(draw_index), _ptr(out_actions),
                                                             _ptr(log_prob), _ptr(entropy), _ptr(stats),
                                                             None if packed else _ptr(bits)),
                       "ongym_masked_categorical_rows")
        ctx.env = env
        ctx.save_for_backward(logits, bits, out_actions, stats, entropy)
        ctx.mark_non_differentiable(out_actions)
        return out_actions, log_prob, entropy

    @staticmethod
    def backward(ctx, g_actions, g_log_prob, g_entropy):
        logits, bits, actions, stats, entropy = ctx.saved_tensors
        env = ctx.env
        _check_stream(env)
        g_lp = None if g_log_prob is None else g_log_prob.to(torch.float32).contiguous()
        g_h = None if g_entropy is None else g_entropy.to(torch.float32).contiguous()
        grad = torch.empty_like(logits, memory_format=torch.contiguous_format)
        if ctx.rows is None:
            env._check(env.lib.ongym_masked_categorical_backward(env._h, _ptr(logits), _DTYPES[logits.dtype], _ptr(bits),
                                                                 _ptr(actions), _ptr(stats), _ptr(entropy), _ptr(g_lp),
                                                                 _ptr(g_h), _ptr(grad)),
                       "ongym_masked_categorical_backward")
        else:
            env._check(env.lib.ongym_masked_categorical_backward_rows(env._h, ctx.rows, _ptr(logits), _DTYPES[logits.dtype],
                                                                      _ptr(bits), _ptr(actions), _ptr(stats), _ptr(entropy),
                                                                      _ptr(g_lp), _ptr(g_h), _ptr(grad)),
                       "ongym_masked_categorical_backward_rows")
        return grad, None, None, None, None, None, None, None


def masked_categorical(env, logits: torch.Tensor, mask: torch.Tensor, actions: Optional[torch.Tensor] = None, *,
                       deterministic: bool = False, seed: int = 0, draw_index: Optional[int] = None,
                       mask_bits_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(actions int32 [R], log_prob float32 [R], entropy float32 [R]) of the masked categorical distribution over `logits`
    ([R, n_actions], float32 or bfloat16, contiguous, on the environment's device; any R >= 1, e.g. a PPO minibatch)
    restricted to `mask`: [R, n_actions] uint8 or bool as the observation writes it, or int32 [R, ceil(n_actions / 32)]
    packed bits (bit j of row r = entry j, the layout of `mask_bits_out`).  `actions` given: evaluate them (log_prob = -inf
    outside the mask); else `deterministic`: the first valid entry with the largest logit; else a draw, deterministic in
    (seed, draw_index, replica_base + row) - `draw_index=None` takes the environment's next draw number.
    `mask_bits_out` (int32 [R, ceil(n_actions / 32)], byte masks only): the forward writes the packed mask there and the
    backward reads it, so a rollout keeps the 8x smaller bits of every step at no extra cost.  A packed input mask is read
    by the backward too: leave it unchanged until then."""
    if not env.holder.struct.io_device:
        raise ValueError("masked_categorical needs an environment created with io_device=True")
    n = env.num_actions
    nw = (n + 31) // 32
    dev = _device(env)
    if not isinstance(logits, torch.Tensor) or logits.dtype not in _DTYPES:
        raise ValueError("logits must be a float32 or bfloat16 tensor")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] != n or not logits.is_contiguous() or logits.device != dev:
        raise ValueError(f"logits must be a contiguous [R >= 1, {n}] tensor on {dev}")
    if logits.data_ptr() % 16:
        raise ValueError("logits must be 16-byte aligned")
    R = logits.shape[0]
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool, torch.int32):
        raise ValueError("mask must be a uint8 or bool tensor, or int32 packed bits")
    width = nw if mask.dtype == torch.int32 else n
    if tuple(mask.shape) != (R, width) or not mask.is_contiguous() or mask.device != dev:
        raise ValueError(f"mask must be a contiguous [{R}, {width}] tensor on {dev}")
    if mask.data_ptr() % (4 if mask.dtype == torch.int32 else 8):
        raise ValueError("mask must be 8-byte aligned (packed bits: 4-byte)")
    if mask_bits_out is not None:
        if mask.dtype == torch.int32:
            raise ValueError("mask_bits_out needs a byte mask: the mask is already packed")
        if (not isinstance(mask_bits_out, torch.Tensor) or mask_bits_out.dtype != torch.int32 or
                tuple(mask_bits_out.shape) != (R, nw) or not mask_bits_out.is_contiguous() or mask_bits_out.device != dev):
            raise ValueError(f"mask_bits_out must be a contiguous int32 [{R}, {nw}] tensor on {dev}")
    if actions is not None:
        if not isinstance(actions, torch.Tensor) or actions.dtype not in (torch.int32, torch.int64):
            raise ValueError("actions must be an int32 or int64 tensor")
        if tuple(actions.shape) != (R,) or actions.device != dev:
            raise ValueError(f"actions must be a [{R}] tensor on {dev}")
        actions = actions.to(torch.int32).contiguous()
    _check_stream(env)
    mode = nat.HEAD_EVALUATE if actions is not None else nat.HEAD_ARGMAX if deterministic else nat.HEAD_SAMPLE
    if draw_index is None:
        draw_index = getattr(env, "_head_draws", 0)
        if mode == nat.HEAD_SAMPLE:
            env._head_draws = draw_index + 1
    return _MaskedCategorical.apply(logits, env, mask, actions, mode, int(seed), int(draw_index), mask_bits_out)


def gae(env, recs: torch.Tensor, values: torch.Tensor, last_values: torch.Tensor, gamma: float = 0.99,
        gae_lambda: float = 0.95, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(advantages, returns), float32 [T, B]: generalised advantage estimation over a rollout in one HIP pass (ongym_gae),
    SB3's RolloutBuffer.compute_returns_and_advantage with the episode ends read from the step records.
    `recs`: uint8 [T, B, 56] (or [T, B * 56]), the records of T calls of ongym_step_actions in consecutive slices; `values`:
    float32 [T, B], the value of each step's observation; `last_values`: float32 [B], the value of the observation after the
    last step.  `out`: optional (advantages, returns) float32 [T, B] tensors to write; they must not overlap an input."""
    if not env.holder.struct.io_device:
        raise ValueError("gae needs an environment created with io_device=True")
    B, rec = env.batch_size, nat.STEP_DTYPE.itemsize
    dev = _device(env)
    if not isinstance(recs, torch.Tensor) or recs.dtype != torch.uint8:
        raise ValueError("recs must be a uint8 tensor of step records")
    if recs.dim() not in (2, 3) or recs.shape[0] < 1 or tuple(recs.shape[1:]) not in ((B, rec), (B * rec,)):
        raise ValueError(f"recs must be a [T >= 1, {B}, {rec}] or [T, {B * rec}] tensor")
    T = recs.shape[0]
    if not recs.is_contiguous() or recs.device != dev or recs.data_ptr() % 8:
        raise ValueError(f"recs must be contiguous, 8-byte aligned and on {dev}")
    for name, t, shape in (("values", values, (T, B)), ("last_values", last_values, (B,))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor")
        if tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous {list(shape)} tensor on {dev}")
    if not (0.0 <= gamma <= 1.0) or not (0.0 <= gae_lambda <= 1.0):
        raise ValueError("gamma and gae_lambda must lie in [0, 1]")
    if out is None:
        out = (torch.empty((T, B), dtype=torch.float32, device=dev), torch.empty((T, B), dtype=torch.float32, device=dev))
    adv, ret = out
    for name, t in (("advantages", adv), ("returns", ret)):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (T, B) or not t.is_contiguous()
                or t.device != dev):
            raise ValueError(f"out {name} must be a contiguous float32 [{T}, {B}] tensor on {dev}")
    _check_stream(env)
    env._check(env.lib.ongym_gae(env._h, T, _ptr(recs), _ptr(values), _ptr(last_values), float(gamma), float(gae_lambda),
                                 _ptr(adv), _ptr(ret)), "ongym_gae")
    return adv, ret
