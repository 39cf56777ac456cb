"""Call transcript of BatchedQRMSAEnv's twelve array-taking wrappers (observe_blocks ... playout): a driver, not a test.

It builds stub environments (no library, no GPU): object.__new__, a ConfigHolder on the golden nsfnet tables, B = 4,
capacity 128; host-side and io_device, each also with modulations_to_consider=3, and a host one with continuous bit rates.
The stub library knows from include/ongym.h which arguments of each call are input and output buffers and how many bytes
each holds for the call's scalar arguments.  It reads every non-null input at that size and records its digest, fills
every non-null output at that size with a fixed pattern, and records the name and the scalars.  For each call of the list
below the transcript holds what the library saw and what came back (type, dtype, shape, digest, whether it is the caller's
`out`), or for a refused call the exception's type and message and that the library saw nothing.

tests/test_batched_calls_host.py compares the transcript of the working tree with tests/golden/batched_calls.json, which
is the transcript of an earlier batched.py:
    python tests/batched_calls.py --write tests/golden/batched_calls.json --module <that batched.py>"""
import argparse
import ctypes
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "optical-networking-gym_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import common                                                   # noqa: E402
from optical_networking_gym import _native as nat               # noqa: E402
from optical_networking_gym import rl                           # noqa: E402

B, CAP = 4, 128
FILL = 0xA5
METHODS = ("observe_blocks", "link_metrics", "service_qot", "action_impact", "failure_impact", "failure_sets", "cut_links",
           "repair_links", "failed_links", "move_services", "admission_map", "playout")


def digest(data: bytes) -> str:
    return hashlib.sha1(data).hexdigest()[:16]


# ---- the recording stub library -----------------------------------------------------------------------------------------------
def signatures(c):
    """per function its arguments after the handle, in the order of include/ongym.h: (name, None) a scalar, or
    (name, "in" | "out" | "inout", bytes as a function of the scalars)"""
    E, K, N = c.n_links, c.k_paths, c.n_nodes
    Q = N * (N - 1) // 2
    one = lambda s: 16 * (B if s["per_replica"] else 1)                        # noqa: E731
    return {
        "ongym_observe_blocks": [("blocks", None), ("obs", "out", lambda s: 4 * B * (3 + 3 * K + 6 * K * s["blocks"])),
                                 ("mask", "out", lambda s: B * (K * s["blocks"] + 1)),
                                 ("action_map", "out", lambda s: 4 * B * (K * s["blocks"] + 1))],
        "ongym_link_metrics": [("link_out", "out", lambda s: 4 * B * E * 8), ("compactness", "out", lambda s: 8 * B),
                               ("link_stats", "inout", lambda s: 8 * B * E * 4)],
        "ongym_service_qot": [("svc_out", "out", lambda s: 8 * B * CAP * 4), ("replica_out", "out", lambda s: 8 * B * 6),
                              ("link_out", "out", lambda s: 4 * B * E * 3)],
        "ongym_action_impact": [("n_actions", None), ("actions", "in", lambda s: 4 * B * s["n_actions"]),
                                ("svc_in", "in", lambda s: 8 * B * CAP * 4), ("impact_out", "out", lambda s: 8 * B * s["n_actions"] * 8)],
        "ongym_failure_impact": [("n_fail", None), ("links", "in", lambda s: 4 * B * s["n_fail"]),
                                 ("link_out", "out", lambda s: 8 * B * s["n_fail"] * 10),
                                 ("svc_out", "out", lambda s: 4 * B * s["n_fail"] * CAP)],
        "ongym_failure_sets": [("n_sets", None), ("sets", "in", lambda s: 16 * s["n_sets"] * (B if s["per_replica"] else 1)),
                               ("per_replica", None), ("set_out", "out", lambda s: 8 * B * s["n_sets"] * 12),
                               ("svc_out", "out", lambda s: 4 * B * s["n_sets"] * CAP)],
        "ongym_cut_links": [("sets", "in", one), ("per_replica", None), ("flags", None), ("cut_out", "out", lambda s: 8 * B * 13),
                            ("svc_out", "out", lambda s: 4 * B * CAP), ("index_out", "out", lambda s: 4 * B * CAP)],
        "ongym_repair_links": [("sets", "in", one), ("per_replica", None), ("repaired_out", "out", lambda s: 4 * B)],
        "ongym_failed_links": [("failed_out", "out", lambda s: 16 * B)],
        "ongym_move_services": [("n_moves", None), ("moves", "in", lambda s: 8 * B * s["n_moves"]), ("flags", None),
                                ("move_out", "out", lambda s: 8 * B * s["n_moves"] * 6)],
        "ongym_admission_map": [("n_actions", None), ("actions", "in", lambda s: 4 * B * s["n_actions"]), ("n_rates", None),
                                ("rates", "in", lambda s: 4 * s["n_rates"]), ("weights", "in", lambda s: 8 * Q * s["n_rates"]),
                                ("summary_out", "out", lambda s: 8 * B * s["n_actions"] * 8),
                                ("map_out", "out", lambda s: 4 * B * s["n_actions"] * Q * s["n_rates"]),
                                ("margin_out", "out", lambda s: 4 * B * s["n_actions"] * Q * s["n_rates"])],
        "ongym_playout": [("n_actions", None), ("actions", "in", lambda s: 4 * B * s["n_actions"]), ("horizon", None),
                          ("policy", None), ("n_samples", None), ("seed", None), ("flags", None),
                          ("playout_out", "out", lambda s: 8 * B * s["n_actions"] * s["n_samples"] * 8)],
    }


def _address(p) -> int:
    if p is None:
        return 0
    if isinstance(p, ctypes.c_void_p):
        return p.value or 0
    return int(p)


class RecordingLib:
    def __init__(self, c):
        self.sig, self.calls = signatures(c), []

    def __getattr__(self, name):
        sig = self.__dict__["sig"].get(name)
        if sig is None:
            raise AttributeError(name)

        def call(handle, *args):
            assert handle is None and len(args) == len(sig), (name, len(args))
            scalars = {a[0]: int(getattr(v, "value", v)) for a, v in zip(sig, args) if a[1] is None}
            rec = {"function": name, "scalars": scalars, "buffers": {}}
            for a, v in zip(sig, args):
                if a[1] is None:
                    continue
                p, n = _address(v), int(a[2](scalars))
                if not p:
                    rec["buffers"][a[0]] = None
                    continue
                if a[1] in ("in", "inout"):
                    rec["buffers"][a[0]] = {"bytes": n, "digest": digest(ctypes.string_at(p, n))}
                if a[1] in ("out", "inout"):
                    ctypes.memset(p, FILL, n)
                    rec["buffers"].setdefault(a[0], {"bytes": n})["filled"] = True
            self.calls.append(rec)
            return 0
        return call


# ---- environments -------------------------------------------------------------------------------------------------------------
ENVS = {"host": dict(io_device=False), "device": dict(io_device=True),
        "host_window": dict(io_device=False, modulations_to_consider=3), "device_window": dict(io_device=True, modulations_to_consider=3),
        "host_continuous": dict(io_device=False, bit_rate_selection="continuous")}


def make_env(cls, kind):
    kw = dict(bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400))
    kw.update(ENVS[kind])
    env = object.__new__(cls)
    env.holder = nat.ConfigHolder(common.golden_tables("nsfnet"), modulations=common.jocn_modulations(), batch=B, load=300,
                                  capacity=CAP, **kw)
    env.batch_size, env.lib, env._h, env.stream_handle = B, RecordingLib(env.holder.struct), None, None
    return env


# ---- argument builders --------------------------------------------------------------------------------------------------------
NP = {torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8,
      torch.float16: np.float16}
if hasattr(torch, "uint64"):
    NP[torch.uint64] = np.uint64


def ints(shape, dtype=np.int32, mod=50):
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.int64) * 7 + 3) % mod).astype(dtype).reshape(shape)


def reals(shape, dtype=np.float64):
    n = int(np.prod(shape))
    return ((np.arange(n) % 97) / 97.0 + 0.25).astype(dtype).reshape(shape)


def strided(a):
    """a view with a's shape and content that is not C-contiguous (numpy array or torch tensor)"""
    if isinstance(a, np.ndarray):
        wide = np.zeros(a.shape + (2,), a.dtype)
    else:
        wide = torch.zeros(tuple(a.shape) + (2,), dtype=a.dtype)
    wide[..., 0] = a
    return wide[..., 0]


def misaligned(t):
    """a tensor with t's dtype, shape and content whose address is one byte past an aligned one"""
    a = t.numpy()
    raw = np.zeros(a.nbytes + 64, np.uint8)
    off = (-raw.ctypes.data) % 64 + 1
    view = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
    view[...] = a
    out = torch.from_numpy(view)
    assert out.data_ptr() % 2 == 1
    return out


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy())


def Z(shape, dtype):
    return torch.zeros(shape, dtype=dtype)


def bad_tensors(t, align_only_bytes=False):
    """label -> a tensor (or other object) that differs from the good tensor t in one respect"""
    out = {"dtype": t.to(torch.float16), "shape": t[:3], "numpy": t.numpy(), "none": None}
    if t.numel() > 1:
        out["strided"] = strided(t)
    if t.element_size() > 1 or align_only_bytes:
        out["misaligned"] = misaligned(t)
    return out


def cases(c):
    """the list of calls: dict(method, env, label, make: () -> (args, kwargs), device: what rl._device gives, stream: whether
    rl._check_stream is replaced by a no-op)"""
    E, K, N, M = c.n_links, c.k_paths, c.n_nodes, c.n_mods
    Q, R = N * (N - 1) // 2, 4
    f64, f32, i32, i64, u8 = torch.float64, torch.float32, torch.int32, torch.int64, torch.uint8
    u64 = getattr(torch, "uint64", torch.int64)
    out = []

    def add(method, env, label, make, device="cpu", stream=True):
        out.append(dict(method=method, env=env, label=label, make=make, device=device, stream=stream))

    def host(method, label, *args, env="host", **kw):
        add(method, env, label, lambda: (args, kw))

    def dev(method, label, make, **how):
        add(method, how.pop("env", "device"), label, make, **how)

    def device_family(method, good, outputs, inputs=(), align4=False, tag=""):
        """around good: () -> (args, kwargs) of an accepted device call: the call itself, every output and tensor input wrong in
        one respect, a device the tensors are not on, and the stream refusal.  outputs: indices into kwargs["out"] (None: out
        itself); inputs: ("arg", index) or ("kw", name)"""
        def dev(method, label, make, **how):
            add(method, "device", tag + label, make, **how)

        dev(method, "good", good)
        for i in outputs:
            a, kw = good()
            ref = kw["out"] if i is None else kw["out"][i]
            for what, bad in bad_tensors(ref, align4).items():
                def make(i=i, bad=bad):
                    a, kw = good()
                    if i is None:
                        kw["out"] = bad
                    else:
                        o = list(kw["out"])
                        o[i] = bad
                        kw["out"] = tuple(o)
                    return a, kw
                dev(method, f"out{'' if i is None else [i]} {what}", make)
        for where, key in inputs:
            a, kw = good()
            ref = a[key] if where == "arg" else kw[key]
            for what, bad in bad_tensors(ref).items():
                def make(where=where, key=key, bad=bad):
                    a, kw = good()
                    if where == "arg":
                        a = list(a)
                        a[key] = bad
                        a = tuple(a)
                    else:
                        kw[key] = bad
                    return a, kw
                dev(method, f"{key if where == 'kw' else 'argument %d' % key} {what}", make)
        dev(method, "another device", good, device="meta")
        dev(method, "stream is checked last", good, stream=False)

    # ---- observe_blocks
    m = "observe_blocks"
    for J in (1, 8, nat.MAX_BLOCKS, 0, nat.MAX_BLOCKS + 1):
        host(m, f"blocks {J}", J)
    host(m, "out passed", 8, out=(1, 2, 3))
    blocks_out = lambda J=8: (Z((B, 3 + 3 * K + 6 * K * J), f32), Z((B, K * J + 1), u8), Z((B, K * J + 1), i32))    # noqa: E731
    device_family(m, lambda: ((8,), dict(out=blocks_out())), (0, 1, 2), align4=True)
    dev(m, "out a list", lambda: ((3,), dict(out=list(blocks_out(3)))))
    dev(m, "blocks 0", lambda: ((0,), dict(out=blocks_out())))
    dev(m, "blocks too many", lambda: ((nat.MAX_BLOCKS + 1,), dict(out=blocks_out())))
    dev(m, "out missing", lambda: ((8,), {}))
    dev(m, "out too short", lambda: ((8,), dict(out=blocks_out()[:2])))
    dev(m, "out a tensor", lambda: ((8,), dict(out=blocks_out()[0])))

    # ---- link_metrics
    m = "link_metrics"
    stats = lambda: reals((B, E, 4))                                                  # noqa: E731
    host(m, "plain")
    host(m, "link_stats", link_stats=stats())
    host(m, "out passed", out=(1, 2))
    host(m, "link_stats a list", link_stats=stats().tolist())
    host(m, "link_stats a tensor", link_stats=T(stats()))
    host(m, "link_stats float32", link_stats=stats().astype(np.float32))
    host(m, "link_stats shape", link_stats=stats()[:3])
    host(m, "link_stats strided", link_stats=strided(stats()))
    ro = stats()
    ro.flags.writeable = False
    host(m, "link_stats read-only", link_stats=ro)
    metrics_out = lambda: (Z((B, E, 8), f32), Z((B,), f64))                           # noqa: E731
    device_family(m, lambda: ((), dict(out=metrics_out(), link_stats=T(stats()))), (0, 1), (("kw", "link_stats"),))
    dev(m, "no link_stats", lambda: ((), dict(out=metrics_out())))
    dev(m, "out missing", lambda: ((), dict(link_stats=T(stats()))))
    dev(m, "out too long", lambda: ((), dict(out=metrics_out() + (Z((B,), f64),))))

    # ---- service_qot
    m = "service_qot"
    host(m, "plain")
    host(m, "out passed", out=(None, None, None))
    qot_out = lambda: (Z((B, CAP, 4), f64), Z((B, 6), f64), Z((B, E, 3), f32))        # noqa: E731
    device_family(m, lambda: ((), dict(out=qot_out())), (0, 1, 2))
    dev(m, "svc alone", lambda: ((), dict(out=(qot_out()[0], None, None))))
    dev(m, "replica and link", lambda: ((), dict(out=(None,) + qot_out()[1:])))
    dev(m, "out missing", lambda: ((), {}))
    dev(m, "out too short", lambda: ((), dict(out=qot_out()[:2])))
    dev(m, "all None", lambda: ((), dict(out=(None, None, None))))

    # ---- the actions rule of action_impact, admission_map and playout
    def actions_rule(m, out_of, more={}, extra=None):
        """out_of(A): the device call's out for A actions; more: keyword arguments of every call; extra: those of the longest"""
        acts = lambda A: ints((B, A))                                                 # noqa: E731
        host(m, "actions [B]", ints((B,)), **more)
        host(m, "actions [B, 3]", acts(3), **more)
        host(m, "actions [B, 1]", acts(1), **more)
        host(m, "actions strided", ints((B, 6))[:, ::2], **more)
        host(m, "actions None", None, **more)
        host(m, "actions a list", acts(3).tolist(), **more)
        host(m, "actions a tensor", T(acts(3)), **more)
        host(m, "actions int64", ints((B, 3), np.int64), **more)
        host(m, "actions wrong leading", ints((3, 2)), **more)
        host(m, "actions 3-D", ints((B, 2, 2)), **more)
        host(m, "actions none per replica", ints((B, 0)), **more)
        host(m, "actions too many", ints((B, nat.MAX_IMPACT_ACTIONS + 1)), **more)
        host(m, "actions as many as allowed", ints((B, nat.MAX_IMPACT_ACTIONS)), **(extra or more))
        host(m, "out passed", acts(3), out=np.zeros(3), **more)
        device_family(m, lambda: ((T(acts(3)),), dict(out=out_of(3), **more)), (None,), (("arg", 0),))
        dev(m, "actions [B]", lambda: ((T(ints((B,))),), dict(out=out_of(1), **more)))
        dev(m, "actions None", lambda: ((None,), dict(out=out_of(1), **more)))
        dev(m, "actions wrong leading", lambda: ((T(ints((3, 2))),), dict(out=out_of(2), **more)))
        dev(m, "actions 3-D", lambda: ((T(ints((B, 2, 2))),), dict(out=out_of(2), **more)))
        dev(m, "actions none per replica", lambda: ((T(ints((B, 0))),), dict(out=out_of(0), **more)))
        dev(m, "actions too many", lambda: ((T(ints((B, nat.MAX_IMPACT_ACTIONS + 1))),),
                                            dict(out=out_of(nat.MAX_IMPACT_ACTIONS + 1), **more)))
        dev(m, "out missing", lambda: ((T(acts(3)),), dict(**more)))

    # ---- action_impact
    m = "action_impact"
    actions_rule(m, lambda A: Z((B, A, 8), f64))
    svc = lambda: reals((B, CAP, 4))                                                  # noqa: E731
    host(m, "svc", ints((B, 2)), svc())
    host(m, "svc strided", ints((B, 2)), strided(svc()))
    host(m, "svc a list", ints((B, 2)), svc().tolist())
    host(m, "svc float32", ints((B, 2)), svc().astype(np.float32))
    host(m, "svc shape", ints((B, 2)), svc()[:, :64])
    device_family(m, lambda: ((T(ints((B, 2))), T(svc())), dict(out=Z((B, 2, 8), f64))), (), (("arg", 1),), tag="svc: ")

    # ---- failure_impact
    m = "failure_impact"
    for label, links in (("links None", None), ("links [B]", ints((B,), mod=E)), ("links [B, 3]", ints((B, 3), mod=E)),
                         ("every link", ints((B, E), mod=E)), ("links strided", ints((B, 6), mod=E)[:, ::2])):
        host(m, label, links)
        host(m, label + " detail", links, detail=True)
    host(m, "format window", None, env="host_window")
    host(m, "out passed", None, out=np.zeros(3))
    host(m, "links a list", [[0], [1], [2], [3]])
    host(m, "links int64", ints((B, 3), np.int64))
    host(m, "links wrong leading", ints((3, 2)))
    host(m, "links 3-D", ints((B, 2, 2)))
    host(m, "no link", ints((B, 0)))
    host(m, "too many links", ints((B, E + 1)))
    fi_out = lambda F, detail=False: (Z((B, F, 10), f64), Z((B, F, CAP), i32)) if detail else Z((B, F, 10), f64)   # noqa: E731
    device_family(m, lambda: ((T(ints((B, 3), mod=E)),), dict(out=fi_out(3))), (None,), (("arg", 0),))
    device_family(m, lambda: ((T(ints((B, 3), mod=E)),), dict(out=fi_out(3, True), detail=True)), (0, 1), tag="detail: ")
    dev(m, "links None", lambda: ((), dict(out=fi_out(E))))
    dev(m, "links None detail, out a list", lambda: ((), dict(out=list(fi_out(E, True)), detail=True)))
    dev(m, "links [B]", lambda: ((T(ints((B,), mod=E)),), dict(out=fi_out(1))))
    dev(m, "format window", lambda: ((), dict(out=fi_out(E))), env="device_window")
    dev(m, "links wrong leading", lambda: ((T(ints((3, 2))),), dict(out=fi_out(2))))
    dev(m, "no link", lambda: ((T(ints((B, 0))),), dict(out=fi_out(0))))
    dev(m, "too many links", lambda: ((T(ints((B, E + 1))),), dict(out=fi_out(E + 1))))
    dev(m, "out missing", lambda: ((), {}))
    dev(m, "detail, out a tensor", lambda: ((), dict(out=fi_out(E), detail=True)))
    dev(m, "detail, out too long", lambda: ((), dict(out=fi_out(E, True) + (None,), detail=True)))

    # ---- failure_sets
    m = "failure_sets"
    sets = lambda *shape: ints(shape, np.uint64, mod=1 << 20)                         # noqa: E731
    lists = [[0, 1], [], range(3), (E - 1,), np.array([2, 5])]
    for label, s in (("shared list", sets(5, 2)), ("list per replica", sets(B, 3, 2)), ("index iterables", lists),
                     ("index iterables, a tuple", tuple(lists)), ("strided", strided(sets(5, 2))), ("one set", sets(1, 2))):
        host(m, label, s)
        host(m, label + " detail", s, detail=True)
    host(m, "format window", sets(5, 2), env="host_window")
    host(m, "out passed", sets(5, 2), out=np.zeros(3))
    host(m, "sets int64", sets(5, 2).astype(np.int64))
    host(m, "sets a tensor", T(sets(5, 2).astype(np.int64)))
    host(m, "sets None", None)
    host(m, "sets 1-D", sets(2))
    host(m, "sets of three words", sets(5, 3))
    host(m, "sets wrong leading", sets(3, 5, 2))
    host(m, "sets 4-D", sets(B, 5, 1, 2))
    host(m, "no set", sets(0, 2))
    host(m, "no set in a list", [])
    host(m, "too many sets", sets(nat.MAX_FAILURE_SETS + 1, 2))
    host(m, "index outside the links", [[0], [E]])
    fs_out = lambda F, detail=False: (Z((B, F, 12), f64), Z((B, F, CAP), i32)) if detail else Z((B, F, 12), f64)   # noqa: E731
    tsets = lambda *shape: T(sets(*shape).astype(np.int64))                           # noqa: E731
    device_family(m, lambda: ((tsets(5, 2),), dict(out=fs_out(5))), (None,), (("arg", 0),))
    device_family(m, lambda: ((tsets(B, 3, 2),), dict(out=fs_out(3, True), detail=True)), (0, 1), tag="detail: ")
    dev(m, "unsigned sets", lambda: ((tsets(5, 2).view(u64),), dict(out=fs_out(5))))
    dev(m, "format window", lambda: ((tsets(5, 2),), dict(out=fs_out(5))), env="device_window")
    dev(m, "index iterables", lambda: ((lists,), dict(out=fs_out(5))))
    dev(m, "sets int32", lambda: ((T(ints((5, 2))),), dict(out=fs_out(5))))
    dev(m, "sets 1-D", lambda: ((tsets(2),), dict(out=fs_out(1))))
    dev(m, "sets of three words", lambda: ((tsets(5, 3),), dict(out=fs_out(5))))
    dev(m, "sets wrong leading", lambda: ((tsets(3, 5, 2),), dict(out=fs_out(5))))
    dev(m, "no set", lambda: ((tsets(0, 2),), dict(out=fs_out(0))))
    dev(m, "too many sets", lambda: ((tsets(nat.MAX_FAILURE_SETS + 1, 2),), dict(out=fs_out(1))))
    dev(m, "out missing", lambda: ((tsets(5, 2),), {}))
    dev(m, "detail, out a tensor", lambda: ((tsets(5, 2),), dict(out=fs_out(5), detail=True)))
    dev(m, "detail, out too long", lambda: ((tsets(5, 2),), dict(out=fs_out(5, True) + (None,), detail=True)))

    # ---- cut_links, repair_links: one set per replica
    per_lists = [[0, 1], [], range(3), (E - 1,)]
    for m, more in (("cut_links", {}), ("repair_links", {})):
        for label, s in (("shared set", sets(2)), ("set per replica", sets(B, 2)), ("index iterables", per_lists),
                         ("index iterables, a tuple", tuple(per_lists)), ("strided", sets(B, 4)[:, ::2]), ("shared strided", sets(4)[::2])):
            host(m, label, s)
        host(m, "out passed", sets(2), out=np.zeros(3))
        host(m, "an iterable too few", per_lists[:3])
        host(m, "index outside the links", [[0], [E], [], []])
        host(m, "sets int64", sets(2).astype(np.int64))
        host(m, "sets a tensor", tsets(2))
        host(m, "sets None", None)
        host(m, "sets wrong leading", sets(3, 2))
        host(m, "sets of three words", sets(B, 3))
        host(m, "sets 3-D", sets(B, 1, 2))
    m = "cut_links"
    host(m, "no restoration", sets(2), restore=False)
    host(m, "detail", sets(B, 2), detail=True)
    host(m, "detail, no restoration", sets(B, 2), False, None, True)
    host(m, "format window", sets(2), env="host_window")
    cut_out = lambda detail=False: (Z((B, 13), f64), Z((B, CAP), i32), Z((B, CAP), i32)) if detail else Z((B, 13), f64)   # noqa: E731
    device_family(m, lambda: ((tsets(B, 2),), dict(out=cut_out())), (None,), (("arg", 0),))
    device_family(m, lambda: ((tsets(2),), dict(out=cut_out(True), detail=True, restore=False)), (0, 1, 2), tag="detail: ")
    dev(m, "unsigned sets", lambda: ((tsets(2).view(u64),), dict(out=cut_out())))
    dev(m, "format window", lambda: ((tsets(2),), dict(out=cut_out())), env="device_window")
    dev(m, "index iterables", lambda: ((per_lists,), dict(out=cut_out())))
    dev(m, "sets int32", lambda: ((T(ints((B, 2))),), dict(out=cut_out())))
    dev(m, "sets wrong leading", lambda: ((tsets(3, 2),), dict(out=cut_out())))
    dev(m, "sets 3-D", lambda: ((tsets(B, 1, 2),), dict(out=cut_out())))
    dev(m, "out missing", lambda: ((tsets(2),), {}))
    dev(m, "detail, out a tensor", lambda: ((tsets(2),), dict(out=cut_out(), detail=True)))
    dev(m, "detail, out too short", lambda: ((tsets(2),), dict(out=cut_out(True)[:2], detail=True)))
    m = "repair_links"
    device_family(m, lambda: ((tsets(B, 2),), dict(out=Z((B,), i32))), (None,), (("arg", 0),))
    dev(m, "shared set, unsigned", lambda: ((tsets(2).view(u64),), dict(out=Z((B,), i32))))
    dev(m, "index iterables", lambda: ((per_lists,), dict(out=Z((B,), i32))))
    dev(m, "sets wrong leading", lambda: ((tsets(3, 2),), dict(out=Z((B,), i32))))
    dev(m, "out missing", lambda: ((tsets(2),), {}))

    # ---- failed_links
    m = "failed_links"
    host(m, "plain")
    host(m, "out passed", out=np.zeros((B, 2), np.uint64))
    device_family(m, lambda: ((), dict(out=Z((B, 2), i64))), (None,))
    dev(m, "unsigned", lambda: ((), dict(out=Z((B, 2), u64))))
    dev(m, "out missing", lambda: ((), {}))
    dev(m, "out int32", lambda: ((), dict(out=Z((B, 2), i32))))
    dev(m, "out a tuple", lambda: ((), dict(out=(Z((B, 2), i64),))))

    # ---- move_services
    m = "move_services"
    moves = lambda *shape: ints(shape, mod=40) - 1                                    # noqa: E731
    host(m, "shared list", moves(3, 2))
    host(m, "list per replica", moves(B, 5, 2), own_route=True)
    host(m, "strided", moves(B, 8, 2)[:, ::2])
    host(m, "shared strided", moves(6, 2)[::2], True)
    host(m, "one move", moves(1, 2))
    host(m, "format window", moves(3, 2), env="host_window")
    host(m, "out passed", moves(3, 2), out=np.zeros(3))
    host(m, "moves int64", moves(3, 2).astype(np.int64))
    host(m, "moves a list", [[0, -1]])
    host(m, "moves a tensor", T(moves(B, 3, 2)))
    host(m, "moves None", None)
    host(m, "moves wrong leading", moves(3, 2, 2))
    host(m, "moves of three", moves(B, 3, 3))
    host(m, "shared moves of three", moves(3, 3))
    host(m, "no move", moves(0, 2))
    host(m, "no move per replica", moves(B, 0, 2))
    host(m, "moves 1-D", moves(2))
    host(m, "moves 4-D", moves(B, 3, 1, 2))
    tmoves = lambda *shape: T(moves(*shape))                                          # noqa: E731
    device_family(m, lambda: ((tmoves(B, 3, 2),), dict(out=Z((B, 3, 6), f64))), (None,), (("arg", 0),))
    dev(m, "own route, one move", lambda: ((tmoves(B, 1, 2), True), dict(out=Z((B, 1, 6), f64))))
    dev(m, "format window", lambda: ((tmoves(B, 3, 2),), dict(out=Z((B, 3, 6), f64))), env="device_window")
    dev(m, "shared list", lambda: ((tmoves(3, 2),), dict(out=Z((B, 3, 6), f64))))
    dev(m, "moves wrong leading", lambda: ((tmoves(3, 2, 2),), dict(out=Z((B, 2, 6), f64))))
    dev(m, "moves of three", lambda: ((tmoves(B, 3, 3),), dict(out=Z((B, 3, 6), f64))))
    dev(m, "no move", lambda: ((tmoves(B, 0, 2),), dict(out=Z((B, 0, 6), f64))))
    dev(m, "out missing", lambda: ((tmoves(B, 3, 2),), {}))

    # ---- admission_map
    m = "admission_map"
    am_out = lambda A, detail=False, R=R: ((Z((B, A, 8), f64), Z((B, A, Q, R), i32), Z((B, A, Q, R), f32)) if detail    # noqa: E731
                                           else Z((B, A, 8), f64))
    actions_rule(m, am_out)
    w = lambda R=R: reals((Q, R))                                                     # noqa: E731
    for label, kw in (("traffic", {}), ("uniform", dict(weights=None)), ("weights", dict(weights=w())),
                      ("weights strided", dict(weights=strided(w()))), ("rates, uniform", dict(rates=[10, 400.5], weights=None)),
                      ("rates, weights", dict(rates=np.array([25.0, 50.0, 75.0]), weights=w(3))),
                      ("rates a tuple of one", dict(rates=(100,), weights=None)),
                      ("as many rates as allowed", dict(rates=range(1, nat.MAX_ADMISSION_RATES + 1), weights=None))):
        host(m, label, **kw)
        host(m, label + " detail", ints((B, 2)), detail=True, **kw)
    host(m, "continuous rates, rates given", rates=[10, 40], weights=None, env="host_continuous")
    host(m, "continuous rates", env="host_continuous")
    host(m, "format window", env="host_window")
    host(m, "rates with traffic weights", rates=[10, 40])
    host(m, "no rate", rates=[], weights=None)
    host(m, "too many rates", rates=range(1, nat.MAX_ADMISSION_RATES + 2), weights=None)
    host(m, "a rate of zero", rates=[10, 0], weights=None)
    host(m, "a negative rate", rates=[10, -40], weights=None)
    host(m, "a rate not finite", rates=[10, float("inf")], weights=None)
    host(m, "a rate not a number", rates=[10, float("nan")], weights=None)
    host(m, "weights another word", weights="uniform")
    host(m, "weights a list", weights=w().tolist())
    host(m, "weights a tensor", weights=T(w()))
    host(m, "weights float32", weights=w().astype(np.float32))
    host(m, "weights shape", weights=w(3))
    host(m, "weights shape for the rates", rates=[10, 40], weights=w())
    device_family(m, lambda: ((T(ints((B, 2))),), dict(out=am_out(2, True), weights=T(w()), detail=True)), (0, 1, 2),
                  (("kw", "weights"),), tag="detail: ")
    dev(m, "traffic twice", lambda: ((), dict(out=am_out(1))))
    dev(m, "traffic twice (2)", lambda: ((), dict(out=am_out(1))))
    dev(m, "uniform", lambda: ((), dict(out=am_out(1), weights=None)))
    dev(m, "rates, weights", lambda: ((None, [25.0, 50.0, 75.0]), dict(out=am_out(1, R=3), weights=T(w(3)))))
    dev(m, "rates, uniform, detail, out a list",
        lambda: ((), dict(rates=(10, 40), out=list(am_out(1, True, 2)), weights=None, detail=True)))
    dev(m, "format window", lambda: ((), dict(out=am_out(1))), env="device_window")
    dev(m, "rates with traffic weights", lambda: ((), dict(rates=[10, 40], out=am_out(1))))
    dev(m, "too many rates", lambda: ((), dict(rates=range(1, nat.MAX_ADMISSION_RATES + 2), weights=None, out=am_out(1))))
    dev(m, "weights another word", lambda: ((), dict(weights="uniform", out=am_out(1))))
    dev(m, "weights host array", lambda: ((), dict(weights=w(), out=am_out(1))))
    dev(m, "detail, out a tensor", lambda: ((), dict(out=am_out(1), detail=True)))
    dev(m, "detail, out too short", lambda: ((), dict(out=am_out(1, True)[:2], detail=True)))

    # ---- playout
    m = "playout"
    po_out = lambda A, R=1: Z((B, A, R, 8), f64)                                      # noqa: E731
    actions_rule(m, po_out, extra=dict(horizon=2))
    host(m, "defaults")
    host(m, "samples, seed, policy", ints((B, 2)) - 5, 7, nat.POLICY_LOAD_BALANCING, 3, 12345)
    host(m, "negative seed", None, seed=-1)
    host(m, "seed beyond 64 bits", None, seed=(1 << 70) + 5)
    host(m, "own stream", None, own_stream=True, seed=9)
    host(m, "longest horizon, most samples", None, nat.MAX_PLAYOUT_HORIZON, samples=nat.MAX_PLAYOUT_SAMPLES)
    host(m, "as many scenarios as allowed", ints((B, nat.MAX_PLAYOUT_SCENARIOS // 64)), samples=64)
    host(m, "format window", env="host_window")
    host(m, "horizon 0", horizon=0)
    host(m, "horizon too long", horizon=nat.MAX_PLAYOUT_HORIZON + 1)
    host(m, "samples 0", samples=0)
    host(m, "too many samples", samples=nat.MAX_PLAYOUT_SAMPLES + 1)
    host(m, "own stream with samples", own_stream=True, samples=2)
    host(m, "too many scenarios", ints((B, nat.MAX_PLAYOUT_SCENARIOS // 64 + 1)), samples=64)
    dev(m, "samples, seed, policy", lambda: ((T(ints((B, 2)) - 5), 7, nat.POLICY_LOAD_BALANCING, 3, 12345), dict(out=po_out(2, 3))))
    dev(m, "own stream", lambda: ((), dict(own_stream=True, seed=-1, out=po_out(1))))
    dev(m, "format window", lambda: ((), dict(out=po_out(1))), env="device_window")
    dev(m, "horizon 0", lambda: ((), dict(horizon=0, out=po_out(1))))
    dev(m, "too many samples", lambda: ((), dict(samples=nat.MAX_PLAYOUT_SAMPLES + 1, out=po_out(1))))
    dev(m, "own stream with samples", lambda: ((), dict(own_stream=True, samples=2, out=po_out(1, 2))))
    dev(m, "too many scenarios", lambda: ((T(ints((B, nat.MAX_PLAYOUT_SCENARIOS // 64 + 1))),),
                                          dict(samples=64, out=po_out(nat.MAX_PLAYOUT_SCENARIOS // 64 + 1, 64))))
    dev(m, "out shape for the samples", lambda: ((), dict(samples=2, out=po_out(1))))
    return out


# ---- the transcript -----------------------------------------------------------------------------------------------------------
def describe(x, out):
    """what a returned object is: its type, dtype, shape and content, and whether it is the caller's `out` or a part of it"""
    if isinstance(x, (tuple, list)):
        return {"type": type(x).__name__, "is_out": x is out, "items": [describe(y, out) for y in x]}
    part = "out" if x is out else None
    if part is None and isinstance(out, (tuple, list)):
        part = next((f"out[{i}]" for i, y in enumerate(out) if y is x), None)
    if isinstance(x, np.ndarray):
        return {"type": "ndarray", "dtype": x.dtype.name, "shape": list(x.shape), "contiguous": bool(x.flags.c_contiguous),
                "digest": digest(x.tobytes()), "is_out": part}
    if isinstance(x, torch.Tensor):
        raw = x.contiguous().view(torch.uint8).numpy().tobytes() if x.numel() else b""
        return {"type": "Tensor", "dtype": str(x.dtype), "shape": list(x.shape), "digest": digest(raw), "is_out": part}
    return {"type": type(x).__name__, "repr": repr(x), "is_out": part}


def transcript(cls):
    envs = {}
    records = []
    saved = rl._device, rl._check_stream
    for case in cases(make_env(cls, "host").holder.struct):
        env = envs.setdefault(case["env"], make_env(cls, case["env"]))
        env.lib.calls.clear()
        args, kw = case["make"]()
        rec = {"method": case["method"], "env": case["env"], "label": case["label"], "device": case["device"],
               "stream_checked": not case["stream"]}
        try:
            rl._device = lambda env, d=case["device"]: torch.device(d)
            if case["stream"]:
                rl._check_stream = lambda env: None
            try:
                ret = getattr(env, case["method"])(*args, **kw)
                rec["returned"] = describe(ret, kw.get("out"))
                ls = kw.get("link_stats")
                if ls is not None:
                    rec["link_stats_after"] = describe(ls, None)
            except Exception as e:                                   # every refusal is recorded, whatever its type
                rec["refused"] = {"type": type(e).__name__, "message": str(e)}
        finally:
            rl._device, rl._check_stream = saved
        rec["library"] = list(env.lib.calls)
        records.append(rec)
    return records


def load_class(path=None):
    """BatchedQRMSAEnv of the package, or of another batched.py loaded as a module of the package"""
    if path is None:
        from optical_networking_gym.envs.batched import BatchedQRMSAEnv
        return BatchedQRMSAEnv
    import optical_networking_gym.envs                                      # noqa: F401
    spec = importlib.util.spec_from_file_location("optical_networking_gym.envs._batched_other", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.BatchedQRMSAEnv


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="PATH", required=True, help="where the transcript goes (JSON)")
    ap.add_argument("--module", metavar="FILE", help="the batched.py to drive (default: the package's)")
    a = ap.parse_args()
    recs = transcript(load_class(a.module))
    with open(a.write, "w") as f:
        json.dump(recs, f, indent=0, sort_keys=True)
        f.write("\n")
    refused = sum("refused" in r for r in recs)
    print(f"{len(recs)} calls, {refused} refused, {len(recs) - refused} accepted")
