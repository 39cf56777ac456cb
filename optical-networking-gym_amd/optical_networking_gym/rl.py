"""Masked categorical action head on device: sample / argmax / evaluate a policy's logits over the environment's action mask.

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


def _check_stream(env):
    handle = getattr(env, "stream_handle", None)
    if handle is None or handle != torch.cuda.current_stream().cuda_stream:
        raise ValueError("the environment must run on torch's current stream: "
                         "env.set_stream(torch.cuda.current_stream().cuda_stream)")


class _MaskedCategorical(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, env, mask, actions, mode, seed, draw_index):
        B, n = logits.shape
        dev = logits.device
        out_actions = actions.clone() if actions is not None else torch.empty(B, dtype=torch.int32, device=dev)
        log_prob = torch.empty(B, dtype=torch.float32, device=dev)
        entropy = torch.empty(B, dtype=torch.float32, device=dev)
        stats = torch.empty((B, 2), dtype=torch.float32, device=dev)     # per row: max valid logit, log sum of e^(x - max)
        # the packed mask is saved, not the caller's mask: the next observation overwrites that buffer through a raw pointer,
        # which torch's version counter cannot see
        bits = torch.empty((B, (n + 31) // 32), dtype=torch.int32, device=dev)
        env._check(env.lib.ongym_masked_categorical(env._h, _ptr(logits), _DTYPES[logits.dtype], _ptr(mask), int(mode),
                                                    C.c_uint64(seed), C.c_uint64(draw_index), _ptr(out_actions),
                                                    _ptr(log_prob), _ptr(entropy), _ptr(stats), _ptr(bits)),
                   "ongym_masked_categorical")
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
        env._check(env.lib.ongym_masked_categorical_backward(env._h, _ptr(logits), _DTYPES[logits.dtype], _ptr(bits),
                                                             _ptr(actions), _ptr(stats), _ptr(entropy), _ptr(g_lp), _ptr(g_h),
                                                             _ptr(grad)),
                   "ongym_masked_categorical_backward")
        return grad, None, None, None, None, None, None


def masked_categorical(env, logits: torch.Tensor, mask: torch.Tensor, actions: Optional[torch.Tensor] = None, *,
                       deterministic: bool = False, seed: int = 0,
                       draw_index: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(actions int32 [B], log_prob float32 [B], entropy float32 [B]) of the masked categorical distribution over `logits`
    ([B, n_actions], float32 or bfloat16, contiguous, on the environment's device) restricted to `mask` ([B, n_actions] uint8
    or bool, as the observation writes it).  `actions` given: evaluate them (log_prob = -inf outside the mask); else
    `deterministic`: the first valid entry with the largest logit; else a draw, deterministic in (seed, draw_index, global
    replica index) - `draw_index=None` takes the environment's next draw number."""
    if not env.holder.struct.io_device:
        raise ValueError("masked_categorical needs an environment created with io_device=True")
    B, n = env.batch_size, env.num_actions
    dev = torch.device("cuda", env.holder.struct.device)
    if not isinstance(logits, torch.Tensor) or logits.dtype not in _DTYPES:
        raise ValueError("logits must be a float32 or bfloat16 tensor")
    if tuple(logits.shape) != (B, n) or not logits.is_contiguous() or logits.device != dev:
        raise ValueError(f"logits must be a contiguous [{B}, {n}] tensor on {dev}")
    if logits.data_ptr() % 16:
        raise ValueError("logits must be 16-byte aligned")
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError("mask must be a uint8 or bool tensor")
    if tuple(mask.shape) != (B, n) or not mask.is_contiguous() or mask.device != dev:
        raise ValueError(f"mask must be a contiguous [{B}, {n}] tensor on {dev}")
    if mask.data_ptr() % 8:
        raise ValueError("mask must be 8-byte aligned")
    if actions is not None:
        if not isinstance(actions, torch.Tensor) or actions.dtype not in (torch.int32, torch.int64):
            raise ValueError("actions must be an int32 or int64 tensor")
        if tuple(actions.shape) != (B,) or actions.device != dev:
            raise ValueError(f"actions must be a [{B}] tensor on {dev}")
        actions = actions.to(torch.int32).contiguous()
    _check_stream(env)
    mode = nat.HEAD_EVALUATE if actions is not None else nat.HEAD_ARGMAX if deterministic else nat.HEAD_SAMPLE
    if draw_index is None:
        draw_index = getattr(env, "_head_draws", 0)
        if mode == nat.HEAD_SAMPLE:
            env._head_draws = draw_index + 1
    return _MaskedCategorical.apply(logits, env, mask, actions, mode, int(seed), int(draw_index))
