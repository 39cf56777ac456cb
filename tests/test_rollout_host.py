"""The rollout pieces of on-device MaskablePPO without a GPU: ongym_masked_categorical_rows / _backward_rows and ongym_gae are
declared and exported, optical_networking_gym.rl routes every head call to the right entry point and checks gae's arguments
before any launch, and the float64 GAE reference of the GPU tests agrees with a case worked by hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from optical_networking_gym import _native as nat
from optical_networking_gym import rl

NEW = ("ongym_masked_categorical_rows", "ongym_masked_categorical_backward_rows", "ongym_gae")
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()
DECLS = {
    "ongym_masked_categorical_rows":
        "ongym_env *env, int32_t rows, const void *logits, int32_t dtype, const void *mask, int32_t mask_format, int32_t mode, "
        "uint64_t seed, uint64_t draw_index, int32_t *actions, float *log_prob, float *entropy, float *row_stats, "
        "uint32_t *mask_bits",
    "ongym_masked_categorical_backward_rows":
        "ongym_env *env, int32_t rows, const void *logits, int32_t dtype, const uint32_t *mask_bits, const int32_t *actions, "
        "const float *row_stats, const float *entropy, const float *grad_log_prob, const float *grad_entropy, void *grad_logits",
    "ongym_gae":
        "ongym_env *env, int32_t steps, const ongym_step_rec *recs, const float *values, const float *last_values, float gamma, "
        "float gae_lambda, float *advantages, float *returns",
}


def test_header_declares_the_rollout_functions():
    for name, params in DECLS.items():
        m = re.search(r"int " + name + r"\s*\(([^)]*)\);", HEADER)
        assert m, name
        assert " ".join(m.group(1).split()) == params, name
        assert HEADER.index(name + "(") > HEADER.index("int ongym_masked_categorical_backward("), name
    assert re.search(r"enum \{ ONGYM_MASK_BYTES = 0, ONGYM_MASK_BITS = 1 \};", HEADER)
    assert (nat.MASK_BYTES, nat.MASK_BITS) == (0, 1)


def test_library_exports_and_native_declares_them():
    lib = nat.load_library()
    for name in NEW:
        assert name in nat.EXPORTED_SYMBOLS
        assert hasattr(lib, name) and getattr(lib, name).restype is ctypes.c_int32, name
    assert len(lib.ongym_masked_categorical_rows.argtypes) == 14
    assert len(lib.ongym_masked_categorical_backward_rows.argtypes) == 11
    assert len(lib.ongym_gae.argtypes) == 9


def test_abi_is_still_4():
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == nat.ABI_VERSION == 4
    assert nat.load_library().ongym_abi_version() == 4


def test_calls_without_env_are_argument_errors():
    lib = nat.load_library()
    assert lib.ongym_masked_categorical_rows(None, 1, None, 0, None, 0, 0, 0, 0, None, None, None, None, None) == -1
    assert lib.ongym_masked_categorical_backward_rows(None, 1, None, 0, None, None, None, None, None, None, None) == -1
    assert lib.ongym_gae(None, 1, None, None, None, 0.99, 0.95, None, None) == -1


class _FakeEnv:
    """what rl validates before it touches the library"""
    def __init__(self, io_device, B=2):
        h = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                             io_device=io_device)
        self.holder, self.batch_size, self.num_actions = h, B, h.reject_action + 1
        self.stream_handle = None


@pytest.fixture
def on_cpu(monkeypatch):
    """rl's device checks against the CPU, so tensors made here pass them and the next check is reached"""
    monkeypatch.setattr(rl, "_device", lambda env: torch.device("cpu"))


def _gae_args(T=3, B=2):
    return (torch.zeros((T, B, nat.STEP_DTYPE.itemsize), dtype=torch.uint8), torch.zeros((T, B)), torch.zeros(B))


def test_gae_needs_io_device():
    with pytest.raises(ValueError, match="io_device"):
        rl.gae(_FakeEnv(io_device=False), *_gae_args())


def test_gae_checks_device_dtype_and_shape(on_cpu):
    env = _FakeEnv(io_device=True)
    recs, values, last = _gae_args()
    with pytest.raises(ValueError, match="recs"):
        rl.gae(env, recs.to(torch.int8), values, last)
    with pytest.raises(ValueError, match="recs"):
        rl.gae(env, recs[:, :1], values, last)
    with pytest.raises(ValueError, match="recs"):
        rl.gae(env, recs[:0], values[:0], last)
    with pytest.raises(ValueError, match="values"):
        rl.gae(env, recs, values.double(), last)
    with pytest.raises(ValueError, match="values"):
        rl.gae(env, recs, values[:2], last)
    with pytest.raises(ValueError, match="last_values"):
        rl.gae(env, recs, values, last[:1])
    with pytest.raises(ValueError, match="gamma"):
        rl.gae(env, recs, values, last, gamma=1.5)
    with pytest.raises(ValueError, match="gamma"):
        rl.gae(env, recs, values, last, gae_lambda=float("nan"))
    with pytest.raises(ValueError, match="advantages"):
        rl.gae(env, recs, values, last, out=(torch.zeros((3, 3)), torch.zeros((3, 2))))
    with pytest.raises(ValueError, match="stream"):
        rl.gae(env, recs, values, last)                                # shapes right: the stream is checked last
    with pytest.raises(ValueError, match="stream"):
        rl.gae(env, recs.view(3, -1), values, last)                    # [T, B * 56] is accepted too


def test_gae_rejects_a_cpu_tensor():
    env = _FakeEnv(io_device=True)
    with pytest.raises(ValueError, match="recs"):
        rl.gae(env, *_gae_args())


def test_head_accepts_packed_masks_and_any_row_count(on_cpu):
    env = _FakeEnv(io_device=True)
    n, nw = env.num_actions, (env.num_actions + 31) // 32
    for R, mask in ((5, torch.zeros((5, nw), dtype=torch.int32)), (5, torch.ones((5, n), dtype=torch.uint8)),
                    (2, torch.zeros((2, nw), dtype=torch.int32))):
        with pytest.raises(ValueError, match="stream"):                 # every argument check passed
            rl.masked_categorical(env, torch.zeros((R, n)), mask)
    with pytest.raises(ValueError, match="mask"):
        rl.masked_categorical(env, torch.zeros((5, n)), torch.zeros((5, nw + 1), dtype=torch.int32))
    with pytest.raises(ValueError, match="mask_bits_out"):
        rl.masked_categorical(env, torch.zeros((5, n)), torch.zeros((5, nw), dtype=torch.int32),
                              mask_bits_out=torch.zeros((5, nw), dtype=torch.int32))
    with pytest.raises(ValueError, match="mask_bits_out"):
        rl.masked_categorical(env, torch.zeros((5, n)), torch.ones((5, n), dtype=torch.uint8),
                              mask_bits_out=torch.zeros((4, nw), dtype=torch.int32))
    with pytest.raises(ValueError, match="logits"):
        rl.masked_categorical(env, torch.zeros((0, n)), torch.ones((0, n), dtype=torch.uint8))


class _Ctx:
    def save_for_backward(self, *t):
        self.saved_tensors = t

    def mark_non_differentiable(self, *t):
        pass


class _RecordingLib:
    """stands in for the library: records which head entry point gets which arguments"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ongym_"):
            raise AttributeError(name)

        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def _recording_env(B=2):
    env = _FakeEnv(io_device=True, B=B)
    env.lib, env._h = _RecordingLib(), None
    env._check = lambda rc, what: None
    env.stream_handle = 1
    return env


def _forward_backward(env, logits, mask, actions=None, bits_out=None):
    ctx = _Ctx()
    out = rl._MaskedCategorical.forward(ctx, logits, env, mask, actions, nat.HEAD_EVALUATE if actions is not None
                                        else nat.HEAD_SAMPLE, 3, 4, bits_out)
    import unittest.mock as mock
    with mock.patch.object(rl, "_check_stream", lambda env: None):
        grads = rl._MaskedCategorical.backward(ctx, None, torch.ones(logits.shape[0]), torch.ones(logits.shape[0]))
    assert len(grads) == 8 and grads[0].shape == logits.shape and all(g is None for g in grads[1:])
    return ctx, out


def test_byte_mask_at_batch_rows_keeps_the_original_entry_points():
    env = _recording_env()
    B, n = env.batch_size, env.num_actions
    logits, mask = torch.zeros((B, n)), torch.ones((B, n), dtype=torch.uint8)
    ctx, _ = _forward_backward(env, logits, mask)
    (fwd, fa), (bwd, ba) = env.lib.calls
    assert fwd == "ongym_masked_categorical" and len(fa) == 12
    assert bwd == "ongym_masked_categorical_backward" and len(ba) == 10
    assert fa[3].value == mask.data_ptr() and ba[3].value == fa[11].value == ctx.saved_tensors[1].data_ptr()


def test_byte_mask_at_batch_rows_writes_mask_bits_out():
    env = _recording_env()
    B, n = env.batch_size, env.num_actions
    bits = torch.zeros((B, (n + 31) // 32), dtype=torch.int32)
    ctx, _ = _forward_backward(env, torch.zeros((B, n)), torch.ones((B, n), dtype=torch.uint8), bits_out=bits)
    (fwd, fa), (bwd, ba) = env.lib.calls
    assert fwd == "ongym_masked_categorical" and fa[11].value == bits.data_ptr()
    assert ba[3].value == bits.data_ptr() and ctx.saved_tensors[1] is bits


@pytest.mark.parametrize("R", (1, 3, 7))
def test_other_row_counts_take_the_rows_pair(R):
    env = _recording_env()
    n, nw = env.num_actions, (env.num_actions + 31) // 32
    bits = torch.zeros((R, nw), dtype=torch.int32)
    mask = torch.ones((R, n), dtype=torch.uint8)
    _forward_backward(env, torch.zeros((R, n)), mask, torch.zeros(R, dtype=torch.int32), bits_out=bits)
    (fwd, fa), (bwd, ba) = env.lib.calls
    assert fwd == "ongym_masked_categorical_rows" and len(fa) == 14
    assert fa[1] == R and fa[4].value == mask.data_ptr() and fa[5] == nat.MASK_BYTES and fa[6] == nat.HEAD_EVALUATE
    assert fa[13].value == bits.data_ptr()
    assert bwd == "ongym_masked_categorical_backward_rows" and len(ba) == 11 and ba[1] == R and ba[4].value == bits.data_ptr()


@pytest.mark.parametrize("R", (2, 5))
def test_packed_mask_takes_the_rows_pair_and_is_saved(R):
    env = _recording_env()
    n, nw = env.num_actions, (env.num_actions + 31) // 32
    bits = torch.zeros((R, nw), dtype=torch.int32)
    ctx, _ = _forward_backward(env, torch.zeros((R, n)), bits)
    (fwd, fa), (bwd, ba) = env.lib.calls
    assert fwd == "ongym_masked_categorical_rows" and fa[1] == R and fa[4].value == bits.data_ptr()
    assert fa[5] == nat.MASK_BITS and fa[13] is None                # no bits out with bits in
    assert bwd == "ongym_masked_categorical_backward_rows" and ba[4].value == bits.data_ptr()
    assert ctx.saved_tensors[1] is bits


def test_gae_reference_against_a_hand_worked_case():
    """T = 3, B = 2, gamma = lambda = 0.5 (gamma lambda = 0.25); replica 0 terminates at t = 1.
    b = 0: t=2: delta = 3 + .5*4 - 2 = 3, A = 3;  t=1 (terminated): delta = 2 - 1 = 1, A = 1;  t=0: delta = 1 + .5*1 - .5 = 1,
           A = 1 + .25*1 = 1.25;  returns 1.75, 2, 5
    b = 1: t=2: delta = 1 + .5*2 = 2, A = 2;  t=1: A = .25*2 = .5;  t=0: A = .125;  returns = A (V = 0)"""
    from rollout_child import gae_reference, gae_sb3_f32
    reward = np.array([[1, 0], [2, 0], [3, 1]], np.float64)
    term = np.array([[0, 0], [1, 0], [0, 0]], np.uint8)
    values = np.array([[0.5, 0], [1, 0], [2, 0]], np.float32)
    last = np.array([4, 2], np.float32)
    A, ret = gae_reference(reward, term, values, last, 0.5, 0.5)
    np.testing.assert_array_equal(A, [[1.25, 0.125], [1, 0.5], [3, 2]])
    np.testing.assert_array_equal(ret, [[1.75, 0.125], [2, 0.5], [5, 2]])
    np.testing.assert_array_equal(gae_sb3_f32(reward, term, values, last, 0.5, 0.5), A)
    values_nan = values.copy()
    values_nan[2, 0] = np.nan                       # NaN at t = 2 reaches t = 1 through the termination (0 * NaN) and t = 0
    A, _ = gae_reference(reward, term, values_nan, last, 0.5, 0.5)
    assert np.isnan(A[:, 0]).all() and np.isfinite(A[:, 1]).all()
