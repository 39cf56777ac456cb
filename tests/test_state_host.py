"""Save, restore and fork of replica states without a GPU: ongym_state_size / _save / _load and ongym_fork are declared with
their exact parameter lists, exported and typed, and BatchedQRMSAEnv checks every argument before it calls the library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import common
from optical_networking_gym import _native as nat
from optical_networking_gym import rl
from optical_networking_gym.envs.batched import BatchedQRMSAEnv

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ongym.h")).read()
DECLS = {
    "ongym_state_size": "ongym_env *env, int32_t count, int64_t *bytes",
    "ongym_state_save": "ongym_env *env, int32_t count, const int32_t *replicas, void *out",
    "ongym_state_load": "ongym_env *env, int32_t count, const int32_t *replicas, const void *in, int32_t flags",
    "ongym_fork": "ongym_env *env, const int32_t *src, int32_t flags",
}
BLOCK = 1000


def test_header_declares_the_state_functions_and_flags():
    for name, params in DECLS.items():
        m = re.search(r"int " + name + r"\s*\(([^)]*)\);", HEADER)
        assert m, name
        assert " ".join(m.group(1).split()) == params, name
    assert re.search(r"enum \{ ONGYM_STATE_KEEP_STREAM = 1, ONGYM_STATE_KEEP_PARAMS = 2 \};", HEADER)
    assert (nat.STATE_KEEP_STREAM, nat.STATE_KEEP_PARAMS) == (1, 2)
    assert int(re.search(r"#define ONGYM_ABI_VERSION (\d+)", HEADER).group(1)) == 4


def test_library_exports_and_native_declares_them():
    lib = nat.load_library()
    for name in DECLS:
        assert name in nat.EXPORTED_SYMBOLS
        assert hasattr(lib, name) and getattr(lib, name).restype is ctypes.c_int32, name
    assert len(lib.ongym_state_size.argtypes) == 3
    assert len(lib.ongym_state_save.argtypes) == 4
    assert len(lib.ongym_state_load.argtypes) == 5
    assert len(lib.ongym_fork.argtypes) == 3


def test_calls_without_env_are_argument_errors():
    lib = nat.load_library()
    n = ctypes.c_int64(0)
    assert lib.ongym_state_size(None, 1, ctypes.byref(n)) == -1
    assert lib.ongym_state_save(None, 1, None, None) == -1
    assert lib.ongym_state_load(None, 1, None, None, 0) == -1
    assert lib.ongym_fork(None, None, 0) == -1


class _StubLib:
    """records the state calls; ongym_state_size answers 256 + count * BLOCK"""
    def __init__(self):
        self.calls = []

    def ongym_state_size(self, h, count, p):
        self.calls.append("size")
        p._obj.value = 256 + count * BLOCK
        return 0

    def __getattr__(self, name):
        if name.startswith("ongym_state_") or name == "ongym_fork":
            return lambda *a: self.calls.append(name) or 0
        raise AttributeError(name)


def _env(io_device, B=4):
    env = object.__new__(BatchedQRMSAEnv)
    env.holder = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                                  io_device=io_device)
    env.batch_size, env.lib, env._h, env.stream_handle = B, _StubLib(), None, None
    return env


def _library_calls(env):
    return [c for c in env.lib.calls if c != "size"]


def test_state_nbytes_checks_count():
    env = _env(False)
    assert env.state_nbytes() == 256 + 4 * BLOCK and env.state_nbytes(2) == 256 + 2 * BLOCK
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="count"):
            env.state_nbytes(bad)


def test_save_and_load_check_lists_and_blobs_before_the_library():
    env = _env(False)
    for bad in ([], [0, 4], [-1], [[0, 1]], [0.5], list(range(5))):
        with pytest.raises(ValueError, match="replica"):
            env.save_state(bad)
    blob = np.zeros(256 + 2 * BLOCK, np.uint8)
    with pytest.raises(ValueError, match="repeat"):
        env.load_state(blob, [1, 1])
    for bad in (blob[:200], blob.astype(np.int8), np.zeros(256 + 3 * BLOCK, np.uint8), blob.reshape(2, -1), blob[::2],
                torch.zeros(blob.size, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="state"):
            env.load_state(bad, [0, 1])
    ro = blob.copy()
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="out"):
        env.save_state([0, 1], out=ro)
    with pytest.raises(ValueError, match="out"):
        env.save_state([0, 1], out=np.zeros(10, np.uint8))
    assert _library_calls(env) == []
    env.load_state(blob, [0, 3], keep_stream=True)           # every check passed
    assert env.save_state([2, 2]).size == 256 + 2 * BLOCK    # a save list may repeat
    assert _library_calls(env) == ["ongym_state_load", "ongym_state_save"]


def test_fork_checks_src_before_the_library():
    env = _env(False)
    for bad in (np.zeros(3, np.int32), np.zeros((4, 1), np.int32), np.zeros(4, np.float32), np.array([0, 1, 2, 4])):
        with pytest.raises(ValueError, match="src"):
            env.fork(bad)
    assert _library_calls(env) == []
    env.fork(np.array([-1, 0, 0, 2]), keep_params=True)
    assert _library_calls(env) == ["ongym_fork"]


@pytest.fixture
def on_cpu(monkeypatch):
    monkeypatch.setattr(rl, "_device", lambda env: torch.device("cpu"))


def test_device_environment_takes_tensors_on_its_stream(on_cpu):
    env = _env(True)
    for bad in (np.zeros(4, np.int32), torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="src"):
            env.fork(bad)
    with pytest.raises(ValueError, match="stream"):          # shapes right: the shared stream is checked last
        env.fork(torch.zeros(4, dtype=torch.int32))
    n = 256 + 2 * BLOCK
    with pytest.raises(ValueError, match="state"):
        env.load_state(np.zeros(n, np.uint8), [0, 1])
    with pytest.raises(ValueError, match="state"):
        env.load_state(torch.zeros(n + 1, dtype=torch.uint8), [0, 1])
    with pytest.raises(ValueError, match="aligned"):
        env.load_state(torch.zeros(n + 1, dtype=torch.uint8)[1:], [0, 1])
    with pytest.raises(ValueError, match="stream"):
        env.load_state(torch.zeros(n, dtype=torch.uint8), [0, 1])
    with pytest.raises(ValueError, match="stream"):
        env.save_state([0, 1])
    assert _library_calls(env) == []
