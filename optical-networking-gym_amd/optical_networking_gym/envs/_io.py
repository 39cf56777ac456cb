"""Where BatchedQRMSAEnv's arrays live: the one place that tells a host environment (numpy in, new numpy arrays out) from an
io_device environment (torch tensors on the environment's device in, results written into the caller's `out`).

`io_for(env)` picks the helper once per call.  Both kinds have the same operations:
  array    a caller's array with a free dimension: type, dtype, admissible shapes, contiguity (and alignment on the device)
  fixed    an optional caller's array of one known shape
  constant a host array of the configuration, where the library reads it
  outputs  the arrays the library writes and what the method returns
  ptr      the address of any of them, or of None
  call     the library call; on the device torch's current stream is checked last, just before it
Every refusal is a ValueError raised before the library is called.  torch is imported on the device side only, and
rl._device / rl._check_stream are looked up when they are used."""
from __future__ import annotations

import ctypes as C

import numpy as np


def _free_dim(shape, shapes, min_free: int) -> int:
    """The free dimension (None in a pattern; 0 where the pattern has none) of the first of `shapes` that `shape` fits, or -1"""
    for pat in shapes:
        if len(pat) == len(shape) and all(p is None or p == s for p, s in zip(pat, shape)):
            free = [s for p, s in zip(pat, shape) if p is None]
            if not free:
                return 0
            if free[0] >= min_free:
                return free[0]
    return -1


class _HostIO:
    def __init__(self, env):
        self.env = env

    def array(self, x, name, dtype, shapes, says, *, column=False, min_free=0, align=True, host_too=None):
        """(x C-contiguous, its free dimension).  column: [n] counts as [n, 1].  host_too = (convert, what else the type
        refusal names, what else the shape refusal names): a form only a host environment takes, converted first."""
        convert, type_too, shape_too = host_too or (None, "", "")
        dtype = np.dtype(dtype)
        if convert is not None:
            x = convert(x)
        if not isinstance(x, np.ndarray) or x.dtype != dtype:
            raise ValueError(f"{name} must be a numpy {dtype.name} array{type_too}")
        if column and x.ndim == 1:
            x = x.reshape(-1, 1)
        free = _free_dim(x.shape, shapes, min_free)
        if free < 0:
            raise ValueError(f"{name} must have shape {shape_too}{says}")
        return np.ascontiguousarray(x), free

    def fixed(self, x, name, dtype, shape, inplace=False):
        """x (or None) of exactly `shape`; inplace: the library updates it, so it is taken as it is or not at all"""
        dtype = np.dtype(dtype)
        if x is None:
            return None
        ok = isinstance(x, np.ndarray) and x.dtype == dtype and x.shape == shape
        if inplace:
            if not ok or not x.flags.c_contiguous or not x.flags.writeable:
                raise ValueError(f"{name} must be a writeable C-contiguous {dtype.name} numpy array of shape {shape}")
            return x
        if not ok:
            raise ValueError(f"{name} must be a numpy {dtype.name} array of shape {shape}")
        return np.ascontiguousarray(x)

    def constant(self, x, attr):
        return x

    def outputs(self, out, specs, needs=None, *, detail=None, optional=False, align=None, host_form=tuple):
        """(arrays in library order, what the method returns) for specs = [(name, dtype, shape), ...].  detail None: the call
        always has all of them, as a tuple; False: the first alone (None for the rest); True: all, on the host as
        host_form(arrays).  See _DeviceIO.outputs for `needs`, `optional` and `align`."""
        if out is not None:
            raise ValueError("out is for io_device environments; a host environment returns "
                             + ("new arrays" if len(specs) > 1 else "a new array"))
        every = detail is None or detail
        arrays = [np.zeros(shape, dt) if i == 0 or every else None for i, (_, dt, shape) in enumerate(specs)]
        return arrays, tuple(arrays) if detail is None else host_form(arrays) if detail else arrays[0]

    @staticmethod
    def ptr(a):
        return a.ctypes.data if a is not None else None

    def call(self, name, *args):
        self.env._check(getattr(self.env.lib, name)(self.env._h, *args), name)


class _DeviceIO(_HostIO):
    def __init__(self, env):
        import torch
        from .. import rl
        self.env, self.torch, self.rl, self.dev = env, torch, rl, rl._device(env)

    def _dtypes(self, dtype):
        """(the torch dtypes that hold a numpy dtype, how a refusal names them); 64-bit masks come signed or unsigned"""
        torch, name = self.torch, np.dtype(dtype).name
        if name == "uint64":
            return (torch.int64,) + ((torch.uint64,) if hasattr(torch, "uint64") else ()), "torch.int64 or torch.uint64"
        return (getattr(torch, name),), f"torch.{name}"

    def array(self, x, name, dtype, shapes, says, *, column=False, min_free=0, align=True, host_too=None):
        dtypes, dtype_says = self._dtypes(dtype)
        if not isinstance(x, self.torch.Tensor) or x.dtype not in dtypes or x.device != self.dev:
            raise ValueError(f"{name} must be a {dtype_says} tensor on {self.dev}")
        if column and x.dim() == 1:
            x = x.reshape(-1, 1)
        free = _free_dim(tuple(x.shape), shapes, min_free)
        if free < 0 or not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous with shape {says}")
        if align and x.data_ptr() % x.element_size():
            raise ValueError(f"{name} must be aligned to its element size")
        return x, free

    def fixed(self, x, name, dtype, shape, inplace=False):
        if x is not None:
            self.env._check_tensor(x, name, self._dtypes(dtype)[0][0], shape, self.dev)
        return x

    def constant(self, x, attr):
        """x on the device, uploaded once per device and kept on the environment as `attr`"""
        if getattr(self.env, attr, None) is None or getattr(self.env, attr).device != self.dev:
            setattr(self.env, attr, self.torch.from_numpy(x).to(self.dev))
        return getattr(self.env, attr)

    def outputs(self, out, specs, needs=None, *, detail=None, optional=False, align=None, host_form=tuple):
        """The caller's `out`, checked: returned as it is (detail None: as a tuple).  needs: how the refusal of a missing `out`
        describes it; None with one output: one sentence refuses every fault of it.  optional: a tensor of the tuple may be
        None (not computed), not all.  align: bytes, for _check_tensor."""
        names = ", ".join(s[0] for s in specs)
        if detail is None:
            if out is None:
                raise ValueError(f"an io_device environment needs out=({names}) tensors")
            if not isinstance(out, (tuple, list)) or len(out) != len(specs):
                raise ValueError(f"out must be a tuple ({names})")
            if optional and all(t is None for t in out):
                raise ValueError(f"out: at least one of {names} must be a tensor")
            tensors, labels, ret = list(out), [s[0] for s in specs], tuple(out)
        elif needs is None:
            (_, dt, shape), = specs
            dtypes, dtype_says = self._dtypes(dt)
            if (not isinstance(out, self.torch.Tensor) or out.dtype not in dtypes or out.device != self.dev
                    or tuple(out.shape) != shape or not out.is_contiguous() or out.data_ptr() % out.element_size()):
                raise ValueError(f"an io_device environment needs out, a contiguous {dtype_says} tensor of shape {shape} on {self.dev}")
            return [out], out
        else:
            if out is None:
                raise ValueError(f"an io_device environment needs out, {needs}")
            if detail and (not isinstance(out, (tuple, list)) or len(out) != len(specs)):
                raise ValueError(f"with detail, out must be the {('pair', 'triple')[len(specs) - 2]} ({names})")
            tensors = list(out) if detail else [out] + [None] * (len(specs) - 1)
            labels, ret = [f"out[{i}]" if detail else "out" for i in range(len(specs))], out
        may_miss = optional if detail is None else not detail        # without detail the rest is None by construction
        for t, label, (_, dt, shape) in zip(tensors, labels, specs):
            if not (t is None and may_miss):
                self.env._check_tensor(t, label, self._dtypes(dt)[0][0], shape, self.dev, align=align)
        return tensors, ret

    @staticmethod
    def ptr(a):
        return C.c_void_p(a.data_ptr() if a is not None else None)

    def call(self, name, *args):
        self.rl._check_stream(self.env)
        super().call(name, *args)


def io_for(env):
    return (_DeviceIO if env.holder.struct.io_device else _HostIO)(env)
