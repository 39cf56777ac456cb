#!/usr/bin/env python3
"""A small cross-entropy search over the weights of the on-device scoring policy (BatchedQRMSAEnv.score_actions).

One replica is one heuristic: replica r places every request where its own weight row W[r] scores lowest over the ten
features of a candidate placement (nat.SCORE_FEATURES).  All replicas are forked from one warmed-up replica, so every heuristic
of a generation, and every generation, meets the same network and the same requests; the loop is two launches per decision,
`env.step(env.score_actions(W))`.  After `steps` decisions the quarter of the population that blocked least gives the mean
and the spread the next generation is drawn from.

    python examples/weighted_policy_search.py [--batch 256] [--generations 10] [--steps 400] [--load 300] [--seed 1]

The script reports the blocking of every generation.  It is an illustration of the call, not a result: a few hundred requests
on one traffic sample say little about a heuristic, and nothing here is tuned."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "examples", "JOCN_Benchmark_2024")]

from jocn_common import load_topology  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv  # noqa: E402

# one unit of weight moves the score by about one unit of every feature's range (NSFNET, 320 slots)
SCALE = 1.0 / np.array([5, 4, 6, 8, 32, 320, 320, 2, 10, 10], np.float64)


def make_env(batch, load=300.0, slots=320, warmup=300, seed=1):
    """`batch` copies of one replica after `warmup` first-fit decisions: the same network, the same request stream"""
    env = BatchedQRMSAEnv(load_topology("nsfnet_chen.txt"), batch_size=batch, num_spectrum_resources=slots, capacity=512,
                          episode_length=10 ** 6, auto_reset=True, load=load, bit_rate_selection="discrete",
                          bit_rates=(10, 40, 100, 400))
    env.seed(seed)
    env.reset()
    env.step_policy(warmup, record=False)
    env.fork(np.zeros(batch, np.int32))
    return env


def evaluate(env, start, W, steps):
    """every replica from the state `start` (a blob of replica 0), `steps` decisions under its row of W: the step records"""
    env.load_state(start, replicas=[0])
    env.fork(np.zeros(env.batch_size, np.int32))
    return np.stack([env.step(env.score_actions(W)) for _ in range(steps)])


def search(batch=256, generations=10, steps=400, load=300.0, warmup=300, seed=1, log=print, keep_records=False):
    env = make_env(batch, load=load, warmup=warmup, seed=seed)
    start = env.save_state([0])
    rng = np.random.default_rng(seed)
    mean = env.score_preset("first_feasible") / (env.holder.struct.n_mods * env.holder.struct.n_slots)   # first fit over all starts
    std = SCALE.copy()
    res = dict(blocking=[], weights=[], records=[])
    for g in range(generations):
        W = mean + std * rng.normal(size=(batch, len(nat.SCORE_FEATURES)))
        W[0] = mean                                          # the current mean competes too
        rec = evaluate(env, start, W, steps)
        blocking = np.sum(rec["accepted"] == 0, axis=0) / steps
        elite = np.argsort(blocking, kind="stable")[:max(2, batch // 4)]
        mean, std = W[elite].mean(axis=0), W[elite].std(axis=0) + 0.05 * SCALE
        res["blocking"].append(blocking)
        res["weights"].append(W)
        if keep_records:
            res["records"].append(rec)
        log(f"generation {g}: blocking of {batch} heuristics over {steps} requests: best {blocking.min():.4f}, "
            f"mean row {blocking[0]:.4f}, median {np.median(blocking):.4f}, worst {blocking.max():.4f}")
    log("mean weights of the last elite: " + ", ".join(f"{n} {v:+.4f}" for n, v in zip(nat.SCORE_FEATURES, mean)))
    env.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--load", type=float, default=300.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    search(batch=a.batch, generations=a.generations, steps=a.steps, load=a.load, seed=a.seed)
