"""The masked categorical action head (ongym_masked_categorical / _backward, optical_networking_gym.rl) without a GPU: the
library exports it, the ctypes layer declares it, the Python module imports and rejects bad input before any launch."""
import ctypes

import pytest

from optical_networking_gym import _native as nat

NEW = ("ongym_masked_categorical", "ongym_masked_categorical_backward")


def test_library_exports_the_head():
    lib = nat.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is ctypes.c_int32


def test_native_declares_the_head():
    for name in NEW:
        assert name in nat.EXPORTED_SYMBOLS
    lib = nat.load_library()
    assert len(lib.ongym_masked_categorical.argtypes) == 12
    assert len(lib.ongym_masked_categorical_backward.argtypes) == 10
    assert (nat.DTYPE_F32, nat.DTYPE_BF16) == (0, 1)
    assert (nat.HEAD_SAMPLE, nat.HEAD_ARGMAX, nat.HEAD_EVALUATE) == (0, 1, 2)


def test_head_call_without_env_is_an_argument_error():
    lib = nat.load_library()
    assert lib.ongym_masked_categorical(None, None, 0, None, 0, 0, 0, None, None, None, None, None) == -1
    assert lib.ongym_masked_categorical_backward(None, None, 0, None, None, None, None, None, None, None) == -1


class _FakeEnv:
    """Just what masked_categorical validates before it touches the library."""
    def __init__(self, io_device):
        h = nat.ConfigHolder(__import__("common").golden_tables("nsfnet"), modulations=__import__("common").jocn_modulations(),
                             batch=2, load=300, io_device=io_device)
        self.holder, self.batch_size, self.num_actions = h, 2, h.reject_action + 1
        self.stream_handle = None


def test_rl_module_imports_and_validates():
    import torch
    from optical_networking_gym.rl import masked_categorical
    env = _FakeEnv(io_device=False)
    logits = torch.zeros((2, env.num_actions))
    mask = torch.ones((2, env.num_actions), dtype=torch.uint8)
    with pytest.raises(ValueError, match="io_device"):
        masked_categorical(env, logits, mask)
    env = _FakeEnv(io_device=True)
    with pytest.raises(ValueError, match="logits"):
        masked_categorical(env, logits.to(torch.float16), mask)
    with pytest.raises(ValueError, match="logits"):       # a CPU tensor is on the wrong device
        masked_categorical(env, logits, mask)


def test_abi_version_and_row_stats_in_the_header():
    """ABI 4: the per-row value saved for the backward is two floats (max valid logit, log sum), not one lse"""
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", header).group(1)) == nat.ABI_VERSION == 4
    assert nat.load_library().ongym_abi_version() == 4
    for name in NEW:
        decl = re.search(name + r"\s*\(([^)]*)\)", header).group(1)
        assert "float *row_stats" in decl and "lse" not in decl, name
    assert "row_stats float [batch][2]" in header


class _Ctx:
    def save_for_backward(self, *t):
        self.saved = t

    def mark_non_differentiable(self, *t):
        pass


class _RecordingLib:
    """stands in for the library: records the buffers ongym_masked_categorical is given"""
    def __init__(self):
        self.calls = []

    def ongym_masked_categorical(self, *args):
        self.calls.append(args)
        return 0


def test_rl_forward_allocates_two_row_stats_per_row():
    import torch
    from optical_networking_gym.rl import _MaskedCategorical
    env = _FakeEnv(io_device=True)
    env.lib, env._h = _RecordingLib(), None
    env._check = lambda rc, what: None
    B, n = env.batch_size, env.num_actions
    ctx = _Ctx()
    logits, mask = torch.zeros((B, n)), torch.ones((B, n), dtype=torch.uint8)
    _MaskedCategorical.forward(ctx, logits, env, mask, None, nat.HEAD_SAMPLE, 0, 0)
    saved_logits, bits, actions, stats, entropy = ctx.saved
    assert stats.shape == (B, 2) and stats.dtype == torch.float32 and stats.is_contiguous()
    assert bits.shape == (B, (n + 31) // 32) and actions.shape == (B,) and entropy.shape == (B,)
    args = env.lib.calls[0]
    assert len(args) == 12 and args[10].value == stats.data_ptr() and args[11].value == bits.data_ptr()
