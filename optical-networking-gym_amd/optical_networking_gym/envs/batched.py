"""Batched QRMSA environment: B independent replicas stepped by the HIP kernels behind include/ongym.h.

This is the host-side mirror of the reference's `QRMSAEnv` (envs/qrmsa.pyx:118-1644) for the hot path only:
constructor kwargs keep the reference's names (qrmsa.pyx:206-237) plus `batch_size`, `capacity`, `auto_reset`,
`device`; `reset()/step()` keep their meaning per replica; the first-fit heuristic
(heuristics/heuristics.py:923-966) is fused on device (`step_policy`).

The class is a thin ctypes shim: no arithmetic of the hot path happens in Python, and there is no CPU fallback —
constructing it without a built libongym_hip.so or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from .. import _native as nat
from .._tables import StaticTables
from ._io import io_for


class OngymError(RuntimeError):
    pass


class BatchedQRMSAEnv:
    def __init__(self, topology=None, *, tables: Optional[StaticTables] = None, batch_size: int = 1,
                 modulations: Optional[Sequence] = None, capacity: int = 1024, auto_reset: bool = True,
                 device: int = 0, io_device: bool = False, **kwargs):
        if tables is None:
            if topology is None:
                raise ValueError("need a topology graph (from get_topology) or StaticTables")
            tables = StaticTables.from_topology(topology)
        if modulations is None:
            modulations = topology.graph.get("modulations") if topology is not None else None
        if not modulations:
            raise ValueError("no modulations: pass `modulations=` or build the topology with them")
        modulations = list(modulations)
        # modulations_to_consider < len(modulations) (qrmsa.pyx:313): the action space addresses a window of that many formats
        # below max_modulation_idx (codec :801-834); observation() moves the window per request (:543-581, 712-717)
        mtc = min(int(kwargs.pop("modulations_to_consider", len(modulations))), len(modulations))
        kwargs["modulations_to_consider"] = mtc
        for dead in ("seed", "allow_rejection", "reset", "file_name", "blocks_to_consider", "gen_observation",
                     "bands", "bandwidth", "k_paths"):
            kwargs.pop(dead, None)
        self.holder = nat.ConfigHolder(tables, modulations=modulations, batch=batch_size, capacity=capacity,
                                       auto_reset=auto_reset, device=device, io_device=io_device, **kwargs)
        self.tables = tables
        self.modulations = modulations
        self.batch_size = int(batch_size)
        self.lib = nat.load_library()
        h = C.c_void_p()
        rc = self.lib.ongym_create(C.byref(self.holder.struct), C.byref(h))
        if rc != nat.OK:
            raise OngymError(f"ongym_create failed ({rc}): {self.lib.ongym_last_error(None).decode()}")
        self._h = h
        self._trace = None
        self.stream_handle = None       # the caller's stream given to set_stream (None: the environment's own)

    # ------------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.ongym_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != nat.OK:
            raise OngymError(f"{what} failed ({rc}): {self.lib.ongym_last_error(self._h).decode()}")

    @staticmethod
    def _check_tensor(t, name: str, dtype, shape, dev, what: Optional[str] = None, align: Optional[int] = None):
        """A torch tensor the library gets as a device pointer: its type, dtype, shape, contiguity and device, then its alignment
        (`align` bytes; None: its element size).  `what` words the tensor in the message where the default does not."""
        import torch
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
                or t.device != dev):
            raise ValueError(f"{name} must be a contiguous {what or f'{dtype} tensor of shape {shape}'} on {dev}")
        if t.data_ptr() % (align or t.element_size()):
            raise ValueError(f"{name} must be {f'{align}-byte aligned' if align else 'aligned to its element size'}")

    def _needs_every_format(self, who: str):
        """The refusal of a format window by a call that searches all formats; `who` leads the sentence in"""
        c = self.holder.struct
        if c.n_mods_consider < c.n_mods:
            raise ValueError(f"{who} every format: it needs modulations_to_consider == the number of modulations")

    def _actions(self, io, actions, required=False, samples=None):
        """(actions as the library takes them, A) of candidate step actions: int32 [B, A] or [B] (A = 1), 1 <= A <=
        nat.MAX_IMPACT_ACTIONS; None, unless `required`: no array, A = 1.  samples: playout's R, which bounds A R."""
        B, A = self.batch_size, 1
        if actions is not None or required:
            actions, A = io.array(actions, "actions", np.int32, [(B, None)], f"({B}, A) or ({B},)", column=True)
        if not 1 <= A <= nat.MAX_IMPACT_ACTIONS:
            raise ValueError(f"the number of actions per replica must lie in [1, {nat.MAX_IMPACT_ACTIONS}]")
        if samples is not None and A * samples > nat.MAX_PLAYOUT_SCENARIOS:
            raise ValueError(f"actions x samples per replica must not exceed {nat.MAX_PLAYOUT_SCENARIOS}")
        return actions, A

    @property
    def reject_action(self) -> int:
        return self.holder.reject_action

    @property
    def num_actions(self) -> int:
        return self.holder.reject_action + 1

    # ---- request sources -----------------------------------------------------------------------------------------
    def seed(self, seed: int, replica_base: int = 0):
        """Device traffic generator; local replica r uses stream (seed, replica_base + r) of include/ongym_traffic.h.
        `replica_base` = index of this environment's first replica in a batch sharded over several environments."""
        self.replica_base = int(replica_base)
        self._check(self.lib.ongym_seed_base(self._h, C.c_uint64(seed), C.c_uint64(replica_base)), "ongym_seed_base")

    def set_requests(self, requests: np.ndarray):
        """Trace replay: `requests` is a REQUEST_DTYPE array [batch, n] (or [n] for batch 1).  Every arrival_time must be finite
        with a clear sign bit (-0.0 is refused too), every holding_time not NaN with a clear sign bit (+inf is legal: the
        service never leaves); arrival times need not be monotone.  The library checks a host trace and raises OngymError on
        an entry outside this contract, with the earlier request source still installed.  A trace the library reads from device
        memory (ongym_set_requests of an io_device environment) is not checked: there the same contract is the caller's."""
        req = np.ascontiguousarray(requests, nat.REQUEST_DTYPE)
        if req.ndim == 1:
            req = req[None, :]
        if req.shape[0] != self.batch_size:
            raise ValueError("requests must have one row per replica")
        self._trace = req
        self._check(self.lib.ongym_set_requests(self._h, req.ctypes.data, req.shape[1]), "ongym_set_requests")

    # ---- reset / step -----------------------------------------------------------------------------------------------
    def reset(self, mask: Optional[np.ndarray] = None):
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.shape != (self.batch_size,):
                raise ValueError("mask must have one entry per replica")
        self._check(self.lib.ongym_reset(self._h, mask.ctypes.data if mask is not None else None), "ongym_reset")

    def reset_episode_counters(self, mask: Optional[np.ndarray] = None):
        """`reset(options={"only_episode_counters": True})` of the reference (qrmsa.pyx:427-464) per replica: episode counters
        and histograms to zero, the departure heap dropped (running services stay for good), nothing else touched."""
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.shape != (self.batch_size,):
                raise ValueError("mask must have one entry per replica")
        self._check(self.lib.ongym_reset_episode_counters(self._h, mask.ctypes.data if mask is not None else None),
                    "ongym_reset_episode_counters")

    def step_policy(self, nsteps: int = 1, record: bool = True, policy: int = nat.POLICY_FIRST_FIT,
                    out_device_ptr: Optional[int] = None):
        """`nsteps` x {heuristic `policy`; step}. Returns STEP_DTYPE [nsteps, batch] when `record`, else None.  With an
        environment created with io_device=True, `out_device_ptr` is the address of a device buffer of nsteps * batch step
        records (e.g. torch.Tensor.data_ptr()): the records stay on the device and the call returns without synchronising."""
        if out_device_ptr is not None:
            if not self.holder.struct.io_device:
                raise ValueError("out_device_ptr needs an environment created with io_device=True")
            self._check(self.lib.ongym_step_policy(self._h, policy, nsteps, C.c_void_p(out_device_ptr)), "ongym_step_policy")
            return None
        out = np.zeros((nsteps, self.batch_size), nat.STEP_DTYPE) if record else None
        self._check(self.lib.ongym_step_policy(self._h, policy, nsteps, out.ctypes.data if record else None),
                    "ongym_step_policy")
        return out

    def step(self, actions: np.ndarray) -> np.ndarray:
        actions = np.ascontiguousarray(actions, np.int32)
        if actions.shape != (self.batch_size,):
            raise ValueError("actions must have one entry per replica")
        out = np.zeros(self.batch_size, nat.STEP_DTYPE)
        self._check(self.lib.ongym_step_actions(self._h, actions.ctypes.data, out.ctypes.data), "ongym_step_actions")
        return out

    def step_bundle(self, actions: np.ndarray, next_policy: int = -1):
        """`step(actions)`, then fused policy `next_policy` on the new current requests (skipped when negative), everything
        behind one synchronisation (ongym_step_actions_bundle): (records, requests, stats, next_actions | None, next_flags | None)."""
        actions = np.ascontiguousarray(actions, np.int32)
        if actions.shape != (self.batch_size,):
            raise ValueError("actions must have one entry per replica")
        B = self.batch_size
        rec, req, st = np.zeros(B, nat.STEP_DTYPE), np.zeros(B, nat.REQUEST_DTYPE), np.zeros(B, nat.STATS_DTYPE)
        na, nf = (np.zeros(B, np.int32), np.zeros(B, np.uint8)) if next_policy >= 0 else (None, None)
        self._check(self.lib.ongym_step_actions_bundle(self._h, actions.ctypes.data, int(next_policy), rec.ctypes.data,
                                                       req.ctypes.data, st.ctypes.data,
                                                       na.ctypes.data if na is not None else None,
                                                       nf.ctypes.data if nf is not None else None), "ongym_step_actions_bundle")
        return rec, req, st, na, nf

    def policy_actions(self, policy: int = nat.POLICY_FIRST_FIT):
        actions = np.zeros(self.batch_size, np.int32)
        flags = np.zeros(self.batch_size, np.uint8)
        self._check(self.lib.ongym_policy_actions(self._h, policy, actions.ctypes.data, flags.ctypes.data),
                    "ongym_policy_actions")
        return actions, flags

    def sample_actions(self, mask: np.ndarray, seed: int, draw_index: int) -> np.ndarray:
        """One uniformly random valid action per replica from an action mask [batch, n_actions] (gymnasium's
        `action_space.sample(mask=...)` on the reference's Discrete space), drawn on device (ongym_sample_actions)."""
        mask = np.ascontiguousarray(mask, np.uint8)
        if mask.shape != (self.batch_size, self.num_actions):
            raise ValueError("mask must be [batch, n_actions]")
        actions = np.zeros(self.batch_size, np.int32)
        self._check(self.lib.ongym_sample_actions(self._h, mask.ctypes.data, C.c_uint64(seed), C.c_uint64(draw_index),
                                                  actions.ctypes.data), "ongym_sample_actions")
        return actions

    def observe(self):
        """observation() + action mask of every replica's current request: (float32 [B, obs_dim], uint8 [B, n_actions])."""
        c = self.holder.struct
        obs = np.zeros((self.batch_size, 3 + c.k_paths + c.k_paths * c.n_mods_consider * 12), np.float32)
        mask = np.zeros((self.batch_size, c.k_paths * c.n_mods_consider * c.n_slots + 1), np.uint8)
        self._check(self.lib.ongym_observe(self._h, obs.ctypes.data, mask.ctypes.data), "ongym_observe")
        return obs, mask

    # ---- block action space (ongym_observe_blocks, include/ongym.h) ------------------------------------------------------
    def block_obs_dim(self, blocks: int) -> int:
        k = self.holder.struct.k_paths
        return 3 + 3 * k + 6 * k * int(blocks)

    def observe_blocks(self, blocks: int, out=None):
        """The block action space of the current requests (DeepRMSA / optical-rl-gym; the reference's `blocks_to_consider`):
        (obs float32 [B, 3 + 3K + 6KJ], mask uint8 [B, KJ + 1], action_map int32 [B, KJ + 1]) for J = `blocks` in [1, 16].
        Entry k*J + j is block j of route k, decoded best format first; the last entry is the reject action.  action_map holds
        the full action index of every entry (the reject action where invalid): step(decode_block_actions(a, action_map)).
        Read-only.  A host environment returns numpy arrays.  An io_device environment writes into `out` = (obs, mask,
        action_map), torch tensors on its device, on torch's current stream (env.set_stream), without synchronising."""
        J = int(blocks)
        if not 1 <= J <= nat.MAX_BLOCKS:
            raise ValueError(f"blocks must lie in [1, {nat.MAX_BLOCKS}]")
        B, n = self.batch_size, self.holder.struct.k_paths * J + 1
        io = io_for(self)
        (obs, mask, amap), ret = io.outputs(out, [("obs", np.float32, (B, self.block_obs_dim(J))), ("mask", np.uint8, (B, n)),
                                                  ("action_map", np.int32, (B, n))], align=4)
        io.call("ongym_observe_blocks", J, io.ptr(obs), io.ptr(mask), io.ptr(amap))
        return ret

    @staticmethod
    def decode_block_actions(block_actions, action_map):
        """Full action indices [B] of block actions [B] through the action map of observe_blocks: one gather (numpy, or a torch
        gather that stays on the map's device)."""
        if isinstance(action_map, np.ndarray):
            a = np.asarray(block_actions)
            if a.shape != action_map.shape[:1] or not np.issubdtype(a.dtype, np.integer):
                raise ValueError("block_actions must be integers, one per row of action_map")
            if a.size and (a.min() < 0 or a.max() >= action_map.shape[1]):
                raise ValueError(f"block actions must lie in [0, {action_map.shape[1]})")
            return np.take_along_axis(action_map, a.astype(np.int64)[:, None], axis=1)[:, 0].astype(np.int32)
        import torch
        if not isinstance(block_actions, torch.Tensor) or block_actions.shape != action_map.shape[:1]:
            raise ValueError("block_actions must be a tensor with one entry per row of action_map")
        return torch.gather(action_map, 1, block_actions.to(device=action_map.device, dtype=torch.int64)[:, None])[:, 0]

    # ---- link metrics (ongym_link_metrics, include/ongym.h) ----------------------------------------------------------------
    def link_metrics(self, out=None, link_stats=None):
        """Spectrum fragmentation of every link of every replica: (link float32 [B, E, 8], compactness float64 [B]), links in
        table order, features nat.LINK_METRICS (on the free runs of each row), compactness = _get_network_compactness.
        `link_stats` float64 [B, E, 4] (nat.LINK_STATS), zeroed by the caller before the first call, is updated in place as
        _update_link_stats does for every link at each replica's current time.  Read-only.  A host environment returns numpy
        arrays (link_stats: a C-contiguous numpy array).  An io_device environment writes into `out` = (link, compactness) and
        link_stats, torch tensors on its device, on torch's current stream (env.set_stream), without synchronising."""
        B, E = self.batch_size, self.holder.struct.n_links
        io = io_for(self)
        (link, comp), ret = io.outputs(out, [("link", np.float32, (B, E, len(nat.LINK_METRICS))),
                                             ("compactness", np.float64, (B,))])
        link_stats = io.fixed(link_stats, "link_stats", np.float64, (B, E, len(nat.LINK_STATS)), inplace=True)
        io.call("ongym_link_metrics", io.ptr(link), io.ptr(comp), io.ptr(link_stats))
        return ret

    # ---- QoT of the running lightpaths (ongym_service_qot, include/ongym.h) ------------------------------------------------
    def service_qot(self, out=None):
        """Current GSNR of every running lightpath of every replica, each against all the others at the replica's launch power:
        (svc float64 [B, C, 4], replica float64 [B, 6], link float32 [B, E, 3]).  svc: nat.SERVICE_QOT (GSNR, ASE, NLI in dB,
        margin) of record i (the order of services()), NaN at and beyond the running count; replica: nat.REPLICA_QOT; link:
        nat.LINK_QOT, links in table order.  Read-only.  A host environment returns numpy arrays.  An io_device environment
        writes into `out` = (svc, replica, link), torch tensors on its device (any of them None: not computed, not all three),
        on torch's current stream (env.set_stream), without synchronising."""
        c = self.holder.struct
        B = self.batch_size
        io = io_for(self)
        (svc, rep, link), ret = io.outputs(out, [("svc", np.float64, (B, c.capacity, len(nat.SERVICE_QOT))),
                                                 ("replica", np.float64, (B, len(nat.REPLICA_QOT))),
                                                 ("link", np.float32, (B, c.n_links, len(nat.LINK_QOT)))], optional=True)
        io.call("ongym_service_qot", io.ptr(svc), io.ptr(rep), io.ptr(link))
        return ret

    # ---- effect of candidate actions on the running lightpaths (ongym_action_impact, include/ongym.h) -----------------------
    def action_impact(self, actions, svc=None, out=None):
        """What each candidate action would do to the running lightpaths: float64 [B, A, 8], columns nat.ACTION_IMPACT (status,
        victims, victims below minimum_osnr after, newly below it, newly below minimum_osnr + margin, lowest margin after,
        largest GSNR drop, record of the lowest margin), for int32 actions [B, A] (or [B]: A = 1) of full step action indices,
        1 <= A <= nat.MAX_IMPACT_ACTIONS.  svc: optionally the svc array of service_qot() on the same state, which saves the
        baseline pass.  Read-only.  A host environment takes and returns numpy arrays.  An io_device environment takes torch
        tensors on its device and writes into `out`, on torch's current stream (env.set_stream), without synchronising."""
        B = self.batch_size
        io = io_for(self)
        actions, A = self._actions(io, actions, required=True)
        svc = io.fixed(svc, "svc", np.float64, (B, self.holder.struct.capacity, len(nat.SERVICE_QOT)))
        (res,), ret = io.outputs(out, [("out", np.float64, (B, A, len(nat.ACTION_IMPACT)))],
                                 "a float64 tensor of shape (B, A, 8)", detail=False)
        io.call("ongym_action_impact", A, io.ptr(actions), io.ptr(svc), io.ptr(res))
        return ret

    # ---- weighted candidate scoring, weights per replica (ongym_score_actions, include/ongym_score.h) ----------------------
    def score_preset(self, name: str) -> np.ndarray:
        """float64 [10]: the weight vector nat.SCORE_PRESETS[name] for this configuration"""
        c = self.holder.struct
        return nat.score_preset(name, c.n_mods, c.n_slots)

    def score_actions(self, weights, out=None, detail=False):
        """The step action with the lowest w . x among the feasible placements of every replica's pending request: int32 [B].
        x are the ten features nat.SCORE_FEATURES of a candidate (route, hops, format rank, slots, slot-hops, start, route load,
        touch, GSNR, margin); the candidates are highest SNR's (every route, every format, every start with spectrum), feasible
        when they pass QoT with the replica's margin; no feasible candidate: the reject action.  weights: float64 [10] (one
        vector for every replica) or [B, 10] (a vector per replica: a population of heuristics in one launch);
        score_preset(name) gives the named ones.  detail=True returns (actions, best, counts): best float64 [B, 11], the
        winner's score and features (NaN without a winner), counts int32 [B, 3], columns nat.SCORE_COUNT_COLUMNS.  Read-only;
        `env.step(env.score_actions(W))` is one decision of the population.  A host environment takes and returns numpy arrays
        and refuses a weight that is not finite.  An io_device environment takes a torch.float64 tensor on its device and
        writes into `out` (the actions tensor, or with detail the triple (actions, best, counts)), on torch's current stream
        (env.set_stream), without synchronising; its weights are not inspected."""
        B, F = self.batch_size, len(nat.SCORE_FEATURES)
        self._needs_every_format("score_actions walks")
        io = io_for(self)
        weights, _ = io.array(weights, "weights", np.float64, [(F,), (B, F)], f"({F},) or ({B}, {F})",
                              host_too=(lambda w: np.asarray(w, np.float64) if isinstance(w, (list, tuple)) else w,
                                        " or a list of floats", ""))
        if isinstance(weights, np.ndarray) and not np.all(np.isfinite(weights)):
            raise ValueError("weights must be finite")
        (actions, best, counts), ret = io.outputs(out, [("actions", np.int32, (B,)), ("best", np.float64, (B, 1 + F)),
                                                        ("counts", np.int32, (B, len(nat.SCORE_COUNT_COLUMNS)))],
                                                  "an int32 tensor of shape (B,) (detail: with a float64 tensor of shape (B, 11) and "
                                                  "an int32 tensor of shape (B, 3), as a triple)", detail=bool(detail))
        io.call("ongym_score_actions", io.ptr(weights), int(weights.ndim == 2), io.ptr(actions), io.ptr(best), io.ptr(counts))
        return ret

    # ---- single-link failures and first-fit restoration (ongym_failure_impact, include/ongym.h) ----------------------------
    def failure_impact(self, links=None, out=None, detail=False):
        """What happens when a fibre is cut: float64 [B, F, 10], columns nat.FAILURE_IMPACT (status, victims, their capacity,
        restored, restored capacity, lost for want of spectrum, lost on QoT, extra hops, extra slot-hops, lowest margin of a
        restoration), one independent single-link failure per (replica, column) with first-fit restoration of the victims in
        record order.  links: int32 [B, F] (or [B]: F = 1) of link indices in table order, 1 <= F <= n_links; None: every link,
        F = n_links.  detail=True also returns int32 [B, F, C]: per record -1 (no victim), the reject action (lost) or the
        action index of its restoration - 4 F C bytes per replica, for small batches.  Read-only.  A host environment takes and
        returns numpy arrays.  An io_device environment takes torch tensors on its device and writes into `out` (the link
        tensor, or with detail the pair (link, svc)), on torch's current stream (env.set_stream), without synchronising."""
        c = self.holder.struct
        B, E = self.batch_size, c.n_links
        self._needs_every_format("failure_impact searches")
        io = io_for(self)
        F = E
        if links is not None:
            links, F = io.array(links, "links", np.int32, [(B, None)], f"({B}, F) or ({B},)", column=True)
        if not 1 <= F <= E:
            raise ValueError(f"the number of failed links per replica must lie in [1, {E}]")
        (res, svc), ret = io.outputs(out, [("link", np.float64, (B, F, len(nat.FAILURE_IMPACT))),
                                           ("svc", np.int32, (B, F, c.capacity))],
                                     "a float64 tensor of shape (B, F, 10) (detail: with an int32 tensor of shape (B, F, C), as a pair)",
                                     detail=bool(detail))
        io.call("ongym_failure_impact", F, io.ptr(links), io.ptr(res), io.ptr(svc))
        return ret

    # ---- failures of link sets: dual cuts, nodes, shared-risk groups (ongym_failure_sets, include/ongym.h) ------------------
    @staticmethod
    def pack_link_sets(lists, n_links: int) -> np.ndarray:
        """uint64 [F, 2] for F iterables of link indices in [0, n_links): bit e & 63 of word e >> 6 fails link e (the bit order
        of the library's path masks).  An empty iterable gives the empty set, which failure_sets skips (status 1)."""
        lists = list(lists)
        out = np.zeros((len(lists), 2), np.uint64)
        for f, links in enumerate(lists):
            for e in links:
                e = int(e)
                if not 0 <= e < min(int(n_links), 128):
                    raise ValueError(f"link index {e} of set {f} lies outside [0, {n_links})")
                out[f, e >> 6] |= np.uint64(1 << (e & 63))
        return out

    def node_link_sets(self) -> np.ndarray:
        """uint64 [N, 2]: per node (in table order) the set of its incident links, i.e. the node's failure"""
        c = self.holder.struct
        ends = np.asarray(self.holder.tables.link_nodes)
        return self.pack_link_sets([np.flatnonzero((ends[:, 0] == v) | (ends[:, 1] == v)) for v in range(c.n_nodes)], c.n_links)

    def link_pair_sets(self) -> np.ndarray:
        """uint64 [E (E - 1) / 2, 2]: every dual cut, in the order of itertools.combinations(range(E), 2)"""
        from itertools import combinations
        E = self.holder.struct.n_links
        return self.pack_link_sets(combinations(range(E), 2), E).reshape(-1, 2)

    def failure_sets(self, sets, out=None, detail=False):
        """What happens when several links fail at once: float64 [B, F, 12], columns nat.FAILURE_SETS (those of failure_impact,
        then lost_no_route - lost with no route of the node pair left at all, as the lightpaths that end at a failed node - and
        failed_links), one independent scenario per (replica, column): the victims are the records that cross ANY link of the
        set, each once, and first fit restores them in record order over the routes that cross NO link of it.  sets: uint64
        [F, 2] (one list for every replica) or [B, F, 2] (a list per replica), bit e & 63 of word e >> 6 fails link e, 1 <= F <=
        nat.MAX_FAILURE_SETS; or a list of F link-index iterables (pack_link_sets; node_link_sets() and link_pair_sets() make
        the usual lists).  The empty set and a set with a bit at an index >= n_links are skipped (status 1).  detail=True also
        returns int32 [B, F, C], encoded as failure_impact's.  Read-only.  A host environment takes and returns numpy arrays.
        An io_device environment takes a torch.int64 or torch.uint64 tensor on its device and writes into `out` (the set
        tensor, or with detail the pair (set, svc)), on torch's current stream (env.set_stream), without synchronising."""
        c = self.holder.struct
        B = self.batch_size
        self._needs_every_format("failure_sets searches")
        io = io_for(self)
        sets, F = io.array(sets, "sets", np.uint64, [(None, 2), (B, None, 2)], f"(F, 2) or ({B}, F, 2)",
                           host_too=(lambda s: self.pack_link_sets(s, c.n_links) if isinstance(s, (list, tuple)) else s,
                                      " or a list of link-index iterables", ""))
        if not 1 <= F <= nat.MAX_FAILURE_SETS:
            raise ValueError(f"the number of link sets per replica must lie in [1, {nat.MAX_FAILURE_SETS}]")
        (res, svc), ret = io.outputs(out, [("set", np.float64, (B, F, len(nat.FAILURE_SETS))),
                                           ("svc", np.int32, (B, F, c.capacity))],
                                     "a float64 tensor of shape (B, F, 12) (detail: with an int32 tensor of shape (B, F, C), as a pair)",
                                     detail=bool(detail))
        io.call("ongym_failure_sets", F, io.ptr(sets), int(sets.ndim == 3), io.ptr(res), io.ptr(svc))
        return ret

    # ---- link failures on live replicas (ongym_cut_links, ongym_repair_links, ongym_failed_links, include/ongym.h) ----------
    def _one_set_per_replica(self, io, sets, what: str):
        """(sets as the library takes them, per_replica) for one link set per replica: uint64 [2] (shared) or [B, 2], or B
        link-index iterables (pack_link_sets); on an io_device environment a torch.int64 / torch.uint64 tensor on its device"""
        B = self.batch_size

        def packed(s):
            if not isinstance(s, (list, tuple)):
                return s
            if len(s) != B:
                raise ValueError(f"{what} takes one link-index iterable per replica ({B})")
            return self.pack_link_sets(s, self.holder.struct.n_links)

        sets, _ = io.array(sets, "sets", np.uint64, [(2,), (B, 2)], f"(2,) or ({B}, 2)",
                           host_too=(packed, " or a list of link-index iterables, one per replica", ""))
        return sets, int(sets.ndim == 2)

    def cut_links(self, sets, restore=True, out=None, detail=False):
        """Fail a set of links on every replica ITSELF (failure_sets only asks "what if"): float64 [B, 13], columns
        nat.CUT_LINKS (failure_sets' twelve, then dropped).  The records that cross a failed link leave, first fit restores
        them one after the other in record order over the routes clear of the set (restore=False: none is tried, every victim
        is dropped), the failed rows lose every free slot and the state is stored: from then on every step, policy,
        observation and mask sees those links as full and nothing is placed on them, until repair_links returns them or a
        reset (reset(), or the auto reset at the end of an episode) rebuilds the spectrum.  A failed link is a full row that no
        record crosses: nothing else is stored, so save_state, load_state and fork carry failures.  An observation or mask
        taken before the call is stale after it.  sets: uint64 [2] (one set for every replica) or [B, 2], or B link-index
        iterables (pack_link_sets); the empty set and a set with a bit at an index >= n_links leave the replica untouched
        (status 1).  detail=True also returns (svc, index), both int32 [B, C] in pre-cut record order: svc encoded as
        failure_sets' (a dropped victim gets the reject action), index the post-cut record index (-1: lost, dropped, or not
        running).  A host environment takes and returns numpy arrays.  An io_device environment takes a torch.int64 or
        torch.uint64 tensor on its device and writes into `out` (the cut tensor, or with detail the triple (cut, svc,
        index)), on torch's current stream (env.set_stream), without synchronising."""
        c = self.holder.struct
        B = self.batch_size
        self._needs_every_format("cut_links searches")
        io = io_for(self)
        sets, per = self._one_set_per_replica(io, sets, "cut_links")
        (res, svc, idx), ret = io.outputs(out, [("cut", np.float64, (B, len(nat.CUT_LINKS))), ("svc", np.int32, (B, c.capacity)),
                                                ("index", np.int32, (B, c.capacity))],
                                          "a float64 tensor of shape (B, 13) (detail: with two int32 tensors of shape (B, C), as a triple)",
                                          detail=bool(detail), host_form=lambda a: (a[0], (a[1], a[2])))
        io.call("ongym_cut_links", io.ptr(sets), per, 0 if restore else nat.CUT_NO_RESTORE, io.ptr(res), io.ptr(svc), io.ptr(idx))
        return ret

    def repair_links(self, sets, out=None):
        """Return fibre: the links of each replica's set that are failed (cut_links) get their spectrum back, entirely free;
        healthy links of the set are ignored.  int32 [B], the links returned per replica.  sets as cut_links'.  An io_device
        environment writes into `out`, an int32 tensor of shape (B,), on torch's current stream, without synchronising."""
        io = io_for(self)
        sets, per = self._one_set_per_replica(io, sets, "repair_links")
        (n,), ret = io.outputs(out, [("out", np.int32, (self.batch_size,))], "an int32 tensor of shape (B,)", detail=False)
        io.call("ongym_repair_links", io.ptr(sets), per, io.ptr(n))
        return ret

    def failed_links(self, out=None):
        """uint64 [B, 2]: the failed links of every replica, bit e & 63 of word e >> 6 for link e (pack_link_sets' order).
        Link e is failed exactly when its row has no free slot and no running record crosses it.  Read-only.  An io_device
        environment writes into `out`, a torch.int64 or torch.uint64 tensor of shape (B, 2), on torch's current stream."""
        io = io_for(self)
        (f,), ret = io.outputs(out, [("out", np.uint64, (self.batch_size, 2))], detail=False)
        io.call("ongym_failed_links", io.ptr(f))
        return ret

    # ---- running lightpaths moved on live replicas (ongym_move_services, include/ongym.h) -----------------------------------
    def move_services(self, moves, own_route=False, out=None):
        """Move running lightpaths on every replica ITSELF: float64 [B, N, 6], columns nat.MOVE_COLUMNS.  moves is int32
        [B, N, 2] or [N, 2] (one list for every replica), rows (record, target), applied in order, each on the state the
        previous one left.  record: an index of services(), or nat.MOVE_TOP = the record no move of this call has attempted
        whose last slot is highest (ties: the lowest index).  target: a step action k M S + (M - 1 - m) S + start on the
        routes of the record's own node pair, or nat.MOVE_FIRST_FIT = where first fit places the service with its own spectrum
        counted as free (own_route=True: on its present route only).  The service keeps its capacity, so another format
        changes its slot count.  A target is taken only if its start is a candidate start of that state and it passes the
        step's QoT test with the replica's margin; otherwise the replica is exactly as before that move (status 1 invalid,
        2 unchanged, 3 no spectrum, 4 QoT).  A moved record keeps its index, release time and id; no statistic changes
        (with ids, episode_osnr_sum follows Service.OSNR).  A host environment takes and returns numpy arrays.  An io_device
        environment takes a contiguous torch.int32 tensor of shape (B, N, 2) on its device and writes into `out`, a float64
        tensor of shape (B, N, 6), on torch's current stream (env.set_stream), without synchronising."""
        B, ncol = self.batch_size, len(nat.MOVE_COLUMNS)
        self._needs_every_format("move_services searches")
        io = io_for(self)
        shared = lambda m: np.broadcast_to(m[None], (B,) + m.shape) if isinstance(m, np.ndarray) and m.ndim == 2 else m  # noqa: E731
        moves, N = io.array(moves, "moves", np.int32, [(B, None, 2)], f"({B}, N, 2), N >= 1", min_free=1, align=False,
                            host_too=(shared, "", "(N, 2) or "))
        (res,), ret = io.outputs(out, [("out", np.float64, (B, N, ncol))], f"a float64 tensor of shape ({B}, N, {ncol})",
                                 detail=False)
        io.call("ongym_move_services", N, io.ptr(moves), nat.MOVE_OWN_ROUTE if own_route else 0, io.ptr(res))
        return ret

    def defragment(self, n, own_route=True):
        """The classic sweep "highest service to first fit", n times per replica: move_services with n rows
        (nat.MOVE_TOP, nat.MOVE_FIRST_FIT).  Every move takes the record not yet attempted whose last slot is highest and
        places it where first fit would (own_route=True: on its present route).  Returns move_services' array.  A host
        environment only; an io_device environment calls move_services with its own tensors."""
        if self.holder.struct.io_device:
            raise ValueError("defragment builds a host move list: an io_device environment calls move_services")
        if int(n) < 1:
            raise ValueError("n must be at least 1")
        moves = np.tile(np.array([nat.MOVE_TOP, nat.MOVE_FIRST_FIT], np.int32), (int(n), 1))
        return self.move_services(moves, own_route=own_route)

    # ---- slot owners, batched records and the state audit (ongym_spectrum_map, include/ongym.h) -----------------------------
    def spectrum_map(self, out=None, owners=True, records=False, audit=True):
        """Who holds every slot, the running records of all replicas and an audit of the state, for every replica in one call:
        a dict of the arrays asked for.  owners: int16 [B, E, S] (2 E S bytes per replica), v >= 0 a signal cell of record v,
        nat.OWNER_FREE free, -2 - v the guard cell of record v, nat.OWNER_UNOWNED used and unclaimed (a failed link, or an
        orphan); decode_owners splits it.  records (with release): int32 [B, C, 6], columns nat.SPECTRUM_RECORD_COLUMNS, and
        float32 [B, C]; rows at and beyond the running count are -1 and NaN; record i is services(r)[i].  audit: int32 [B, 10],
        columns nat.SPECTRUM_AUDIT_COLUMNS: column 0 is zero exactly when the bitmap is the disjoint union of the records'
        provisioned ranges, every record is well-formed and none is wider than move_services may write.  The library refuses
        owners for a capacity above nat.MAX_OWNER_CAPACITY (the other outputs take any capacity).  Read-only.  A host
        environment returns numpy arrays.  An io_device environment writes into `out`, a dict of torch tensors on its device
        with exactly the keys asked for, on torch's current stream (env.set_stream), without synchronising."""
        c = self.holder.struct
        B, Cp = self.batch_size, c.capacity
        want = [("owners", np.int16, (B, c.n_links, c.n_slots))] if owners else []
        want += [("records", np.int32, (B, Cp, len(nat.SPECTRUM_RECORD_COLUMNS))), ("release", np.float32, (B, Cp))] if records else []
        want += [("audit", np.int32, (B, len(nat.SPECTRUM_AUDIT_COLUMNS)))] if audit else []
        if not want:
            raise ValueError("nothing to compute: ask for owners, records or audit")
        names = [w[0] for w in want]
        io = io_for(self)
        if out is not None and c.io_device:
            if not isinstance(out, dict) or sorted(out) != sorted(names):
                raise ValueError(f"out must be a dict with exactly the keys {names}")
            out = tuple(out[n] for n in names)
        arrays, _ = io.outputs(out, want)
        got = dict(zip(names, arrays))
        io.call("ongym_spectrum_map", *(io.ptr(got.get(n)) for n in ("owners", "records", "release", "audit")))
        return got

    @staticmethod
    def decode_owners(owners):
        """(record, kind) of an owners array of spectrum_map, both of its shape (numpy int32, or torch.int32 on its device):
        kind 0 free, 1 signal, 2 guard, 3 used and unclaimed; record is the holder's index, -1 where there is none."""
        if isinstance(owners, np.ndarray):
            if owners.dtype != np.int16:
                raise ValueError("owners must be an int16 array")
            o, where, xp = owners.astype(np.int32), np.where, np
        else:
            import torch
            if not isinstance(owners, torch.Tensor) or owners.dtype != torch.int16:
                raise ValueError("owners must be an int16 array or tensor")
            o, where, xp = owners.to(torch.int32), torch.where, torch
        kind = where(o >= 0, xp.ones_like(o), where(o == nat.OWNER_FREE, xp.zeros_like(o),
                                                    where(o == nat.OWNER_UNOWNED, xp.full_like(o, 3), xp.full_like(o, 2))))
        record = where(kind == 1, o, where(kind == 2, nat.OWNER_GUARD_BASE - o, xp.full_like(o, -1)))
        return record, kind

    def check_state(self):
        """The audit of spectrum_map alone, int32 [B, 10] as a numpy array (an io_device environment runs it on torch's
        current stream and copies it back): raises OngymError naming the first replica with a violation and its non-zero
        columns, returns the audit otherwise."""
        if self.holder.struct.io_device:
            import torch
            from .. import rl
            t = torch.empty((self.batch_size, len(nat.SPECTRUM_AUDIT_COLUMNS)), dtype=torch.int32, device=rl._device(self))
            audit = self.spectrum_map(out={"audit": t}, owners=False)["audit"].cpu().numpy()
        else:
            audit = self.spectrum_map(owners=False)["audit"]
        bad = np.flatnonzero(audit[:, 0])
        if bad.size:
            r = int(bad[0])
            cols = ", ".join(f"{n} = {int(v)}" for n, v in zip(nat.SPECTRUM_AUDIT_COLUMNS[2:7], audit[r, 2:7]) if v)
            if audit[r, 0] & 1:
                cols = "active outside [0, capacity]" + (", " + cols if cols else "")
            raise OngymError(f"check_state: {bad.size} of {self.batch_size} replicas violate the state invariants; the first is "
                             f"replica {r}: {cols}")
        return audit

    # ---- first-fit admission of every node pair and bit rate (ongym_admission_map, include/ongym.h) ------------------------
    @property
    def admission_pairs(self) -> np.ndarray:
        """int32 [Q, 2]: the unordered node pairs (s, d), s < d, in the order of admission_map's cells"""
        N = self.holder.struct.n_nodes
        return np.array([(s, d) for s in range(N) for d in range(s + 1, N)], np.int32).reshape(-1, 2)

    def admission_weights(self) -> np.ndarray:
        """float64 [Q, R]: the probability that the next request is for (pair q, configured bit rate r).  The pair's is
        p_s p_d / (1 - p_s) + p_d p_s / (1 - p_d), the two orders of the two-stage draw (source by node probability, destination
        among the others; qrmsa.pyx:1134-1148), from the differences of node_cum; the rate's from those of bit_rate_cum."""
        if self.holder.struct.bit_rate_mode != 0:
            raise ValueError("traffic weights need discrete bit rates")
        p = np.diff(self.holder._keep["node_cum"], prepend=0.0)
        p = p / p.sum()
        pr = np.diff(self.holder._keep["bit_rate_cum"], prepend=0.0)
        pr = pr / pr.sum()
        pair = np.array([p[s] * p[d] / (1.0 - p[s]) + p[d] * p[s] / (1.0 - p[d]) for s, d in self.admission_pairs])
        return np.ascontiguousarray(pair[:, None] * pr[None, :])

    def admission_map(self, actions=None, rates=None, weights="traffic", out=None, detail=False):
        """What the network could still carry: float64 [B, A, 8], columns nat.ADMISSION_MAP (status, admitted cells, blocked for
        want of spectrum, blocked on QoT, blocking probability, bit-rate blocking, lowest margin of an admitted cell, admitted on
        a route k > 0), first fit's admission decision for every cell (node pair q of admission_pairs, bit rate r) on the
        replica's state after each candidate action.  actions: int32 [B, A] (or [B]: A = 1) of full step action indices for the
        current request, 1 <= A <= nat.MAX_IMPACT_ACTIONS; None: the state as it is (A = 1).  rates: up to
        nat.MAX_ADMISSION_RATES bit rates in Gb/s (any sequence, always on the host); None: the configured discrete rates.
        weights: float64 [Q, R]; "traffic": the configuration's request probabilities (admission_weights; only with rates=None);
        None: uniform.  detail=True also returns the map int32 [B, A, Q, R] (k M S + (M-1-m) S + a admitted, K M S blocked for
        spectrum, K M S + 1 blocked on QoT, -1 status >= 2) and the margins float32 [B, A, Q, R] - 8 A Q R bytes per replica, for
        small batches.  Read-only.  A host environment takes and returns numpy arrays.  An io_device environment takes torch
        tensors on its device (actions, weights) and writes into `out` (the summary tensor, or with detail the triple (summary,
        map, margin)), on torch's current stream (env.set_stream), without synchronising."""
        c = self.holder.struct
        B, N = self.batch_size, c.n_nodes
        Q = N * (N - 1) // 2
        self._needs_every_format("admission_map searches")
        if rates is None:
            if c.bit_rate_mode != 0:
                raise ValueError("rates=None needs discrete bit rates: pass rates")
            R, rates_arr = int(c.n_bit_rates), None
        else:
            if isinstance(weights, str):
                raise ValueError('weights="traffic" describes the configured bit rates: with rates pass an array or None')
            rates_arr = np.ascontiguousarray(np.asarray(rates, np.float32).reshape(-1))
            R = int(rates_arr.size)
            if not 1 <= R <= nat.MAX_ADMISSION_RATES:
                raise ValueError(f"the number of rates must lie in [1, {nat.MAX_ADMISSION_RATES}]")
            if not np.all(np.isfinite(rates_arr)) or not np.all(rates_arr > 0):
                raise ValueError("every rate must be finite and positive")
        if isinstance(weights, str) and weights != "traffic":
            raise ValueError('weights must be "traffic", an array of shape (Q, R) or None')
        io = io_for(self)
        actions, A = self._actions(io, actions)
        if isinstance(weights, str):                        # the configuration's weights, uploaded once per device
            weights = io.constant(self.admission_weights(), "_admission_w")
        weights = io.fixed(weights, "weights", np.float64, (Q, R))
        (res, amap, mar), ret = io.outputs(out, [("summary", np.float64, (B, A, len(nat.ADMISSION_MAP))),
                                                 ("map", np.int32, (B, A, Q, R)), ("margin", np.float32, (B, A, Q, R))],
                                           "a float64 tensor of shape (B, A, 8) (detail: with an int32 and a float32 tensor of shape "
                                           "(B, A, Q, R), as a triple)", detail=bool(detail))
        io.call("ongym_admission_map", A, io.ptr(actions), R, rates_arr.ctypes.data if rates_arr is not None else None,
                io.ptr(weights), io.ptr(res), io.ptr(amap), io.ptr(mar))
        return ret

    # ---- playouts: candidate actions followed by H policy steps (ongym_playout, include/ongym.h) ------------------------------
    def playout(self, actions=None, horizon: int = 32, policy: int = nat.POLICY_FIRST_FIT, samples: int = 1, seed: int = 0,
                own_stream: bool = False, out=None):
        """What happens after each candidate action: float64 [B, A, R, 8], columns nat.PLAYOUT (status, first_accepted, steps,
        accepted, blocked, bit_rate_accepted, bit_rate_requested, active_end).  Every (replica, action, sample r) is one scenario
        on a private copy of the replica: the stream replaced as seed(seed + r, replica_base) replaces it, the candidate applied
        as step() applies it, then `horizon` iterations of step_policy(policy), ending early at the end of the episode or of the
        trace.  The candidates of a replica see the same future for the same r.  actions: int32 [B, A] (or [B]: A = 1) of full
        step action indices for the pending request, 1 <= A <= nat.MAX_IMPACT_ACTIONS; an index < 0, or None (A = 1): the policy
        decides the pending request too.  policy: first fit or load balancing.  samples: R, 1..nat.MAX_PLAYOUT_SAMPLES, with
        A R <= nat.MAX_PLAYOUT_SCENARIOS.  own_stream=True continues the replica's own generator or trace instead (the true
        future; samples must be 1, seed is ignored).  Read-only.  A host environment takes and returns numpy arrays.  An
        io_device environment takes a torch tensor on its device and writes into `out`, on torch's current stream
        (env.set_stream), without synchronising."""
        B = self.batch_size
        H, R, policy = int(horizon), int(samples), int(policy)
        self._needs_every_format("playout's policies search")
        if not 1 <= H <= nat.MAX_PLAYOUT_HORIZON:
            raise ValueError(f"horizon must lie in [1, {nat.MAX_PLAYOUT_HORIZON}]")
        if not 1 <= R <= nat.MAX_PLAYOUT_SAMPLES:
            raise ValueError(f"samples must lie in [1, {nat.MAX_PLAYOUT_SAMPLES}]")
        if own_stream and R != 1:
            raise ValueError("own_stream continues the replica's one true future: samples must be 1")
        flags = nat.PLAYOUT_OWN_STREAM if own_stream else 0
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        ncol = len(nat.PLAYOUT)
        io = io_for(self)
        actions, A = self._actions(io, actions, samples=R)
        (res,), ret = io.outputs(out, [("out", np.float64, (B, A, R, ncol))], f"a float64 tensor of shape (B, A, R, {ncol})",
                                 detail=False)
        io.call("ongym_playout", A, io.ptr(actions), H, policy, R, C.c_uint64(seed), flags, io.ptr(res))
        return ret

    # ---- queries (plugin API) ----------------------------------------------------------------------------------------
    def available_slots(self, replica: int, path_id: int) -> np.ndarray:
        out = np.zeros(self.holder.struct.n_slots, np.int32)
        self._check(self.lib.ongym_query_available(self._h, replica, path_id, out.ctypes.data), "ongym_query_available")
        return out

    def gsnr(self, replica: int, path_id: int, slot: int, nslots: int) -> np.ndarray:
        out = np.zeros(3, np.float64)
        self._check(self.lib.ongym_query_gsnr(self._h, replica, path_id, slot, nslots, out.ctypes.data),
                    "ongym_query_gsnr")
        return out

    def gsnr_many(self, replica: int, cands) -> np.ndarray:
        """`calculate_osnr` for many candidates `(path_id, slot, nslots)` of one replica in one launch -> [count][3] dB."""
        cands = np.ascontiguousarray(cands, np.int32).reshape(-1, 3)
        out = np.zeros((len(cands), 3), np.float64)
        self._check(self.lib.ongym_query_gsnr_many(self._h, replica, len(cands), cands.ctypes.data, out.ctypes.data),
                    "ongym_query_gsnr_many")
        return out

    def moves(self, replica: int):
        """Reallocations defragment() made during the replica's last step: (records, total count)."""
        out = np.zeros(nat.MOVE_LOG, nat.MOVE_DTYPE)
        n = C.c_int32(0)
        self._check(self.lib.ongym_query_moves(self._h, replica, out.ctypes.data, C.byref(n)), "ongym_query_moves")
        return out[:min(n.value, nat.MOVE_LOG)], n.value

    def candidates(self, row: np.ndarray, nslots: int) -> list:
        """`_get_candidates(row, nslots, len(row))` evaluated on device."""
        row = np.ascontiguousarray(row, np.int32)
        out = np.zeros(len(row), np.int32)
        n = C.c_int32(0)
        self._check(self.lib.ongym_query_candidates(self._h, row.ctypes.data, len(row), int(nslots), out.ctypes.data,
                                                    C.byref(n)), "ongym_query_candidates")
        return out[:n.value].tolist()

    def is_path_free(self, replica: int, path_id: int, slot: int, nslots: int) -> bool:
        out = C.c_int32(0)
        self._check(self.lib.ongym_query_path_free(self._h, replica, path_id, int(slot), int(nslots), C.byref(out)),
                    "ongym_query_path_free")
        return bool(out.value)

    def grid(self, replica: int) -> np.ndarray:
        c = self.holder.struct
        out = np.zeros((c.n_links, c.n_slots), np.int32)
        self._check(self.lib.ongym_query_grid(self._h, replica, out.ctypes.data), "ongym_query_grid")
        return out

    def services(self, replica: int) -> np.ndarray:
        out = np.zeros(self.holder.struct.capacity, nat.SERVICE_DTYPE)
        n = C.c_int32(0)
        self._check(self.lib.ongym_query_services(self._h, replica, out.ctypes.data, C.byref(n)),
                    "ongym_query_services")
        return out[:n.value]

    def request(self, replica: int):
        out = np.zeros(1, nat.REQUEST_DTYPE)
        self._check(self.lib.ongym_query_request(self._h, replica, out.ctypes.data), "ongym_query_request")
        return out[0]

    def stats(self) -> np.ndarray:
        out = np.zeros(self.batch_size, nat.STATS_DTYPE)
        self._check(self.lib.ongym_stats_get(self._h, out.ctypes.data), "ongym_stats_get")
        return out

    def occupancy(self, policy: int = nat.POLICY_FIRST_FIT) -> dict:
        """Resident replicas (wavefronts) per compute unit of the kernel step_policy(policy=...) launches, its LDS bytes per
        replica, and whether a lean kernel is the one that runs."""
        nb, lds, lean = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self.lib.ongym_query_occupancy_policy(self._h, int(policy), C.byref(nb), C.byref(lds), C.byref(lean)),
                    "ongym_query_occupancy_policy")
        return dict(blocks_per_cu=nb.value, lds_bytes=lds.value, lean_kernel=bool(lean.value))

    def link_weight_entry(self, path: int, links: int):
        """What a lean kernel fetches from the shared-link weight table for route `path` and an interferer with link mask
        `links`: dict(mult, index, bits, w1, w2), or None when the environment has no table."""
        out = (C.c_uint32 * 4)()
        entry = (C.c_double * 2)()
        self._check(self.lib.ongym_query_link_weight_entry(self._h, int(path), int(links) & 0xFFFFFFFF, out, entry),
                    "ongym_query_link_weight_entry")
        if not out[0]:
            return None
        return dict(mult=int(out[1]), index=int(out[2]), bits=int(out[3]), w1=float(entry[0]), w2=float(entry[1]))

    def path_rows(self, path: int) -> dict:
        """Route `path` as first fit's copy of the route records spells it out (ongym_query_path_rows): dict(hops, links (the
        four link fields), long (the route takes the link loop; its fields are 0), word (the dword as it lies in device memory))."""
        out = C.c_uint32(0)
        self._check(self.lib.ongym_query_path_rows(self._h, int(path), C.byref(out)), "ongym_query_path_rows")
        w = out.value
        return dict(hops=w & 0xFF, links=[(w >> (8 + 6 * r)) & 0x1F for r in range(4)],
                    long=bool(w >> 31), word=w)

    # ---- save / restore / fork replica states (ongym_state_*, ongym_fork; include/ongym.h) -----------------------------
    # A replica's state is its network, running services, clock, pending request, request counter, stream key, parameters and
    # ongym_stats, except the total_* work counters, which stay with the destination.  Python-side counters are not device
    # state: rl.masked_categorical's draw counter (`_head_draws`) stays where it is.
    def _state_replicas(self, replicas, distinct: bool):
        """(count, int32 array or None) of a save / load replica list, checked before any library call."""
        if replicas is None:
            return self.batch_size, None
        r = np.asarray(replicas)
        if r.ndim != 1 or r.size < 1 or r.size > self.batch_size:
            raise ValueError(f"replicas must be a 1-D list of 1..{self.batch_size} replica indices")
        if not np.issubdtype(r.dtype, np.integer):
            raise ValueError("replicas must be integers")
        if r.min() < 0 or r.max() >= self.batch_size:
            raise ValueError(f"replica indices must lie in [0, {self.batch_size})")
        if distinct and len(np.unique(r)) != r.size:
            raise ValueError("a load list must not repeat a replica")
        return int(r.size), np.ascontiguousarray(r, np.int32)

    def _state_flags(self, keep_stream: bool, keep_params: bool) -> int:
        return (nat.STATE_KEEP_STREAM if keep_stream else 0) | (nat.STATE_KEEP_PARAMS if keep_params else 0)

    def _check_blob(self, blob, nbytes: int, what: str, writable: bool):
        if self.holder.struct.io_device:
            import torch
            from .. import rl
            self._check_tensor(blob, what, torch.uint8, (nbytes,), rl._device(self), f"1-D uint8 tensor of {nbytes} bytes", 16)
            return C.c_void_p(blob.data_ptr())
        if (not isinstance(blob, np.ndarray) or blob.dtype != np.uint8 or blob.ndim != 1 or blob.size != nbytes
                or not blob.flags.c_contiguous or (writable and not blob.flags.writeable)):
            raise ValueError(f"{what} must be a contiguous 1-D numpy uint8 array of {nbytes} bytes")
        return C.c_void_p(blob.ctypes.data)

    def _check_shared_stream(self):
        if self.holder.struct.io_device:
            from .. import rl
            rl._check_stream(self)

    def state_nbytes(self, count: Optional[int] = None) -> int:
        """Bytes of a state blob of `count` replicas (None: all): a 256-byte header, then one block per replica."""
        count = self.batch_size if count is None else int(count)
        if not 1 <= count <= self.batch_size:
            raise ValueError(f"count must lie in [1, {self.batch_size}]")
        n = C.c_int64(0)
        self._check(self.lib.ongym_state_size(self._h, count, C.byref(n)), "ongym_state_size")
        return int(n.value)

    def save_state(self, replicas=None, out=None):
        """The states of `replicas` (host list of indices, None: all in order) as one blob: a numpy uint8 array, or with
        io_device a uint8 tensor on the environment's device, written on torch's current stream without synchronising.
        `out`: a blob of state_nbytes(len(replicas)) bytes to write instead of a new one."""
        count, r = self._state_replicas(replicas, distinct=False)
        nbytes = self.state_nbytes(count)
        if out is None:
            if self.holder.struct.io_device:
                import torch
                from .. import rl
                out = torch.empty(nbytes, dtype=torch.uint8, device=rl._device(self))
            else:
                out = np.empty(nbytes, np.uint8)
        ptr = self._check_blob(out, nbytes, "out", writable=True)
        self._check_shared_stream()
        self._check(self.lib.ongym_state_save(self._h, count, r.ctypes.data if r is not None else None, ptr),
                    "ongym_state_save")
        return out

    def load_state(self, state, replicas=None, *, keep_stream: bool = False, keep_params: bool = False):
        """Load a blob of save_state into `replicas` (host list of distinct indices, None: all in order).  The blob may come
        from another environment of the same configuration (batch, device, launch power, margin and load may differ).
        `keep_stream`: the replicas keep their own request streams; `keep_params`: their launch power, margin and load.
        With io_device the header is read back first: that one small copy waits for the stream."""
        count, r = self._state_replicas(replicas, distinct=True)
        ptr = self._check_blob(state, self.state_nbytes(count), "state", writable=False)
        self._check_shared_stream()
        self._check(self.lib.ongym_state_load(self._h, count, r.ctypes.data if r is not None else None, ptr,
                                              self._state_flags(keep_stream, keep_params)), "ongym_state_load")

    def fork(self, src, *, keep_stream: bool = False, keep_params: bool = False):
        """Replica j takes the pre-fork state of replica src[j] (any overlap: permutations, cycles, one into all); src[j] < 0 or
        == j leaves replica j as it is.  `src`: int32 [batch], a numpy array, or with io_device an int32 tensor on the device
        (then nothing synchronises, and entries >= batch leave their replica unchanged as well)."""
        B = self.batch_size
        flags = self._state_flags(keep_stream, keep_params)
        if self.holder.struct.io_device:
            import torch
            from .. import rl
            self._check_tensor(src, "src", torch.int32, (B,), rl._device(self), f"int32 [{B}] tensor", 4)
            rl._check_stream(self)
            self._check(self.lib.ongym_fork(self._h, C.c_void_p(src.data_ptr()), flags), "ongym_fork")
            return
        s = np.asarray(src)
        if s.shape != (B,) or not np.issubdtype(s.dtype, np.integer):
            raise ValueError(f"src must be an integer array of shape ({B},)")
        if s.max() >= B or s.min() < -2 ** 31:
            raise ValueError(f"src entries must lie in [-2^31, {B}) (negative: unchanged)")
        s = np.ascontiguousarray(s, np.int32)
        self._check(self.lib.ongym_fork(self._h, s.ctypes.data, flags), "ongym_fork")

    def set_stream(self, stream_handle: Optional[int]):
        """Run this environment's launches on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream); None
        returns to the environment's own stream.  See ongym_set_stream (include/ongym.h)."""
        if stream_handle is None:
            self._check(self.lib.ongym_set_stream(self._h, None, 1), "ongym_set_stream")
        else:       # 0 is HIP's default (null) stream: torch's default current stream
            self._check(self.lib.ongym_set_stream(self._h, C.c_void_p(int(stream_handle)), 0), "ongym_set_stream")
        self.stream_handle = None if stream_handle is None else int(stream_handle)   # None: the environment's own stream

    def sync(self):
        self._check(self.lib.ongym_sync(self._h), "ongym_sync")

    def last_kernel_ms(self) -> float:
        return float(self.lib.ongym_last_kernel_ms(self._h))
