"""VecEnv-shaped batched environment over the block action space (DeepRMSA / optical-rl-gym; the reference's
`blocks_to_consider`, envs/qrmsa.pyx:231, 242, and get_available_blocks, :1515-1531).

The agent picks a route k and one of the first J free spectrum blocks j of that route that fit the request: action k*J + j,
or K*J for reject.  The block is decoded best format first and placed at its start (BatchedQRMSAEnv.observe_blocks); the
step itself is the environment's ordinary ongym_step_actions.  Conventions as QRMSAVecEnv (envs/vec_env.py):
* `reset()` -> obs float32 [B, obs_dim], obs_dim = 3 + 3K + 6KJ
* `step(block_actions)` -> (obs, rewards float32 [B], dones bool [B], infos list[dict]) with the `episode` snapshot of a
  replica that terminated, and `qot_error` / `retry` flags (a masked agent never produces either)
* `action_masks()` -> bool [B, n_actions], n_actions = K*J + 1
* `protect_running=True`: `action_masks()` also clears every block action that would push a running lightpath that is not below
  its format's minimum_osnr now below it (BatchedQRMSAEnv.action_impact, column newly_below_minimum; reject stays allowed), and
  every info dict of `step` carries `disrupts`, that count for the action taken.  Default False: nothing changes.
* `action_lookahead()` -> float64 [B, n_actions]: the traffic-weighted probability that the NEXT request is blocked after each
  block action of the current observation (BatchedQRMSAEnv.admission_map); the reject column is the state as it is.
* `playout_lookahead(horizon, samples, seed)` -> float64 [B, n_actions]: the expected number of blocked requests among the
  pending one and the next `horizon`, first fit deciding those, after each block action (BatchedQRMSAEnv.playout); the reject
  column is the reject action.  `seed=None` numbers the calls on the Python side (as RolloutCollector numbers its draws): the
  counter is not device state, neither saved by save_state nor restored by load_state.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from .. import _native as nat
from .batched import BatchedQRMSAEnv


class QRMSABlockVecEnv:
    def __init__(self, topology=None, *, num_envs: int, blocks_to_consider: int = 8, seed: int = 0,
                 protect_running: bool = False, **kwargs):
        kwargs.setdefault("auto_reset", True)
        self.env = BatchedQRMSAEnv(topology, batch_size=num_envs, **kwargs)
        c = self.env.holder.struct
        if c.n_mods_consider < c.n_mods:
            raise ValueError("the block action space has no format window: modulations_to_consider must cover every format")
        self.blocks = int(blocks_to_consider)
        if not 1 <= self.blocks <= nat.MAX_BLOCKS:
            raise ValueError(f"blocks_to_consider must lie in [1, {nat.MAX_BLOCKS}]")
        self.num_envs = int(num_envs)
        self.obs_dim = self.env.block_obs_dim(self.blocks)
        self.n_actions = c.k_paths * self.blocks + 1
        self.env.seed(seed)
        self.protect_running = bool(protect_running)
        self._obs = self._mask = self._map = self._newly = None
        self._playout_seed, self._playout_calls = int(seed), 0

    def _observe(self):
        self._obs, mask, self._map = self.env.observe_blocks(self.blocks)
        self._mask = mask.astype(bool)
        if self.protect_running:
            newly = self.env.action_impact(self._map)[:, :, nat.ACTION_IMPACT.index("newly_below_minimum")]
            self._newly = np.nan_to_num(newly, nan=0.0).astype(np.int64)      # NaN: reject, or a block that is masked anyway
            self._mask &= self._newly == 0
        return self._obs

    def reset(self) -> np.ndarray:
        self.env.reset()
        return self._observe()

    def action_masks(self) -> np.ndarray:
        if self._mask is None:
            self._observe()
        return self._mask

    def action_lookahead(self) -> np.ndarray:
        """float64 [B, K*J + 1]: admission_map's blocking_probability (traffic weights) after each block action of the current
        observation, decoded through its action map; the reject column is the state as it is, masked-out blocks are NaN."""
        if self._map is None:
            self._observe()
        res = self.env.admission_map(np.ascontiguousarray(self._map, np.int32))
        out = res[:, :, nat.ADMISSION_MAP.index("blocking_probability")].copy()
        out[res[:, :, 0] >= 2] = np.nan
        out[:, :-1][~self._mask[:, :-1]] = np.nan
        return out

    def playout_lookahead(self, horizon: int = 32, samples: int = 4, seed=None) -> np.ndarray:
        """float64 [B, K*J + 1]: the mean over `samples` futures of (1 - first_accepted) + blocked of BatchedQRMSAEnv.playout, the
        expected number of blocked requests among the pending one and the next `horizon` with first fit deciding those, after
        each block action of the current observation; the futures are common to the actions of a replica.  The reject column is
        the reject action, masked-out blocks and actions the step would not take (status >= 2) are NaN.  seed=None: call n of
        this object uses seed (the constructor's seed + 1) * 2^32 + n * samples, so successive calls see fresh futures; the
        counter lives on the Python side, not in the device state."""
        if self._map is None:
            self._observe()
        if seed is None:
            seed = ((self._playout_seed + 1) << 32) + self._playout_calls * int(samples)
            self._playout_calls += 1
        res = self.env.playout(np.ascontiguousarray(self._map, np.int32), horizon=horizon, samples=samples, seed=seed)
        col = nat.PLAYOUT.index
        out = ((1.0 - res[..., col("first_accepted")]) + res[..., col("blocked")]).mean(axis=2)
        out[(res[..., 0] >= 2).any(axis=2)] = np.nan
        out[:, :-1][~self._mask[:, :-1]] = np.nan
        return out

    def step(self, block_actions: Sequence[int]):
        if self._map is None:
            self._observe()
        block_actions = np.asarray(block_actions, np.int64)
        actions = self.env.decode_block_actions(block_actions, self._map)
        disrupts = self._newly[np.arange(self.num_envs), block_actions] if self.protect_running else None
        rec = self.env.step(actions)
        rewards = rec["reward"].astype(np.float32)
        qot = (rec["flags"] & nat.F_QOT_ERROR) != 0
        rewards[qot] = -3.0
        dones = rec["terminated"].astype(bool)
        retry = rec["retry"] != 0
        infos = [{} for _ in range(self.num_envs)] if disrupts is None else [{"disrupts": int(d)} for d in disrupts]
        if dones.any() or qot.any() or retry.any():
            st = self.env.stats() if dones.any() else None
            for i in np.flatnonzero(dones | qot | retry):
                if qot[i]:
                    infos[i]["qot_error"] = True
                if retry[i]:
                    infos[i]["retry"] = True
                if dones[i]:
                    s = st[i]
                    infos[i]["episode"] = {
                        "episode_service_blocking_rate": float(s["last_episode_service_blocking_rate"]),
                        "episode_bit_rate_blocking_rate": float(s["last_episode_bit_rate_blocking_rate"]),
                        "episode_services_accepted": int(s["last_episode_accepted"]),
                        "mean_gsnr": float(s["last_mean_gsnr"]),
                    }
        return self._observe(), rewards, dones, infos

    def close(self):
        self.env.close()
