#!/usr/bin/env python3
"""Device time of ongym_admission_map for A = 1 (the state as it is) and A = 41 (the action map of observe_blocks(8)), with
the wavefront groups per scenario the host rule picks and with fixed ones, beside failure_impact() (all 22 links),
service_qot() and observe_blocks(8) on the same states: NSFNET-320 (capacity 448) after 600 first-fit steps, device buffers,
torch events on the environment's stream, the calls alternated round by round.

    python tools/time_admission_map.py [B ...]               (default 16384 65536)
    python tools/time_admission_map.py --host-loop [N]       (default 3 replicas)
    python tools/time_admission_map.py --probe-loop [B]      (default 16384)
    python tools/time_admission_map.py --lookahead [B STEPS] (default 1024 2000)

--host-loop times the way to the same answer on the host: services() and grid() of a replica, then the numpy restatement of
tests/admission_map_child.py with the CPU oracle's GN, for N sample replicas; it also counts the evaluated (route, format,
start) triples per scenario and compares its rows with the device's.
--probe-loop times the device alternative an application could write without the call: per cell load_state of the saved
replicas, set_requests with the cell as the next request, a step that rejects the current one, policy_actions - a sample of
cells, scaled to Q R.
--lookahead runs the block environment choosing the block with the lowest action_lookahead() against first fit on a twin
with the same seed, and reports both blocking rates and the env-steps/s of the lookahead loop.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv  # noqa: E402

ROUNDS = 7
J = 8
GROUPS = (1, 2, 4, 8)           # ONGYM_ADMISSION_GROUPS values tried beside the host rule
PART_ROWS = 262144              # scenarios x groups the library's partial-sum buffer holds (2 x kAdmissionFill, ongym_hip.hip)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def config():
    wl = bench.WORKLOADS["nsfnet320"]
    return bench.build_tables(wl["topology"]), dict(
        modulations=bench.jocn_modulations(), num_spectrum_resources=wl["S"], capacity=wl["capacity"], episode_length=1000,
        auto_reset=True, load=wl["load"], bit_rate_selection="discrete", bit_rates=wl["bit_rates"])


def make_env(B, io_device=True, groups=None):
    """groups: ONGYM_ADMISSION_GROUPS for this environment (the library reads it at create); None: the host rule"""
    tb, kw = config()
    os.environ.pop("ONGYM_ADMISSION_GROUPS", None)
    if groups is not None:
        os.environ["ONGYM_ADMISSION_GROUPS"] = str(groups)
    try:
        env = BatchedQRMSAEnv(tables=tb, batch_size=B, io_device=io_device, **kw)
    finally:
        os.environ.pop("ONGYM_ADMISSION_GROUPS", None)
    if io_device:
        env.set_stream(torch.cuda.current_stream().cuda_stream)
    env.seed(1)
    env.reset()
    env.step_policy(600, record=False)
    return env


def host_loop(N):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from admission_map_child import restate_replica, traffic_weights
    from oracle_lib import OracleEnv
    tb, kw = config()
    env = make_env(max(N, 64))
    out = torch.empty((env.batch_size, 1, 8), dtype=torch.float64, device="cuda")
    env.admission_map(out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    holder = nat.ConfigHolder(tb, batch=env.batch_size, **kw)
    rates, weights = tuple(float(x) for x in holder.bit_rates), traffic_weights(holder)
    secs, evals, same = [], 0, True
    for r in range(N):
        o = OracleEnv(holder, replica=r)
        t0 = time.perf_counter()
        svcs, grid = env.services(r), env.grid(r)
        log = []
        want = restate_replica(o, tb, holder, float(kw.get("margin", 0.0)), svcs, grid, env.request(r), None, rates, weights, log)[0]
        secs.append(time.perf_counter() - t0)
        evals += len(log)
        same &= bool(np.array_equal(got[r][:, :4], want[:, :4]) and np.allclose(got[r][:, 4:6], want[:, 4:6], rtol=0, atol=1e-12))
    per = float(np.mean(secs))
    res = {"replicas": N, "cells": int(weights.size), "host_seconds_per_scenario": per, "triples_per_scenario": evals / N,
           "rows_equal_device": same}
    print(f"host loop: {per:.3f} s per scenario ({weights.size} cells), {evals / N:.1f} evaluated (route, format, start) triples per "
          f"scenario (the device answers some of them with the ASE bound), rows equal the device's: {same}")
    for B in (16384, 65536):
        print(f"  scaled to B = {B}, A = 1: {per * B:.0f} s; A = 41: {per * B * 41:.0f} s")
    print(json.dumps(res))
    env.set_stream(None)
    env.close()


def probe_loop(B, sample=8):
    env = make_env(B, io_device=False)
    c = env.holder.struct
    pairs, rates = env.admission_pairs, env.holder.bit_rates
    reject = c.k_paths * c.n_mods * c.n_slots
    blob = env.save_state()
    rng = np.random.default_rng(0)
    secs = []
    for _ in range(sample + 1):
        q, r = int(rng.integers(len(pairs))), int(rng.integers(len(rates)))
        reqs = np.zeros((B, 2), nat.REQUEST_DTYPE)
        reqs["source"], reqs["destination"], reqs["bit_rate"], reqs["holding_time"] = pairs[q][0], pairs[q][1], rates[r], 1.0
        t0 = time.perf_counter()
        env.load_state(blob)
        env.set_requests(reqs)
        env.step(np.full(B, reject, np.int32))
        env.policy_actions()
        secs.append(time.perf_counter() - t0)
    per = float(np.median(secs[1:]))
    cells = len(pairs) * len(rates)
    print(f"probe loop, B = {B}: {per * 1e3:.2f} ms per cell (load_state + set_requests + reject step + policy_actions, host "
          f"buffers, median of {sample}); {cells} cells: {per * cells:.2f} s per scenario set")
    print(json.dumps({"B": B, "probe_seconds_per_cell": per, "cells": cells, "probe_seconds_all_cells": per * cells}))
    env.close()


def lookahead(B, steps):
    from optical_networking_gym.envs.block_vec_env import QRMSABlockVecEnv
    tb, kw = config()
    vec = QRMSABlockVecEnv(tables=tb, num_envs=B, blocks_to_consider=J, seed=1, **kw)
    vec.reset()
    accepted, t0 = 0.0, time.perf_counter()
    for _ in range(steps):
        la = vec.action_lookahead()
        la[:, -1] = np.inf                                     # reject only when no block is valid
        a = np.where(np.all(np.isnan(la[:, :-1]), axis=1), la.shape[1] - 1, np.nanargmin(np.nan_to_num(la, nan=np.inf), axis=1))
        _, rew, _, _ = vec.step(a)
        accepted += float(np.sum(rew == 0))                  # an accepted request has reward 0 (quirk Q1), a blocked one a negative one
    secs = time.perf_counter() - t0
    twin = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    twin.seed(1)
    twin.reset()
    ff = twin.step_policy(steps)
    res = {"B": B, "steps": steps, "lookahead_blocking": 1.0 - accepted / (B * steps),
           "first_fit_blocking": 1.0 - float(np.mean(ff["accepted"])), "lookahead_env_steps_per_s": B * steps / secs}
    print(f"lookahead, B = {B}, {steps} steps: blocking {res['lookahead_blocking']:.4f} choosing the lowest action_lookahead() block, "
          f"{res['first_fit_blocking']:.4f} with first fit on the twin; {res['lookahead_env_steps_per_s']:.0f} env-steps/s")
    print(json.dumps(res))
    vec.close()
    twin.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--host-loop":
        return host_loop(int(args[1]) if len(args) > 1 else 3)
    if args and args[0] == "--probe-loop":
        return probe_loop(int(args[1]) if len(args) > 1 else 16384)
    if args and args[0] == "--lookahead":
        return lookahead(int(args[1]) if len(args) > 1 else 1024, int(args[2]) if len(args) > 2 else 2000)
    for B in [int(a) for a in args] or [16384, 65536]:
        env = make_env(B)
        c = env.holder.struct
        K, E, dev = c.k_paths, c.n_links, torch.device("cuda", c.device)
        A = K * J + 1
        blocks = (torch.empty((B, env.block_obs_dim(J)), dtype=torch.float32, device=dev),
                  torch.empty((B, A), dtype=torch.uint8, device=dev), torch.empty((B, A), dtype=torch.int32, device=dev))
        env.observe_blocks(J, out=blocks)
        svc = torch.empty((B, c.capacity, 4), dtype=torch.float64, device=dev)
        rep = torch.empty((B, 6), dtype=torch.float64, device=dev)
        outE = torch.empty((B, E, 10), dtype=torch.float64, device=dev)
        out1 = torch.empty((B, 1, 8), dtype=torch.float64, device=dev)
        outA = torch.empty((B, A, 8), dtype=torch.float64, device=dev)
        active = float(np.mean(env.stats()["active"]))
        calls = {"service_qot": lambda: env.service_qot(out=(svc, rep, None)),
                 f"observe_blocks({J})": lambda: env.observe_blocks(J, out=blocks),
                 f"failure_impact F={E}": lambda: env.failure_impact(out=outE),
                 "admission_map A=1": lambda: env.admission_map(out=out1),
                 f"admission_map A={A}": lambda: env.admission_map(blocks[2], out=outA)}
        twins = {}                                               # the same states (same seed) with a forced group count each
        for g in GROUPS + ((16,) if B < 16384 else ()):
            if B * g > PART_ROWS:                                # beyond the partial-sum buffer the library lowers g itself
                continue
            twins[g] = make_env(B, groups=g)
            calls[f"admission_map A=1 G={g}"] = lambda e=twins[g]: e.admission_map(out=out1)
            if B * A * g <= PART_ROWS or g == 1:
                calls[f"admission_map A={A} G={g}"] = lambda e=twins[g]: e.admission_map(blocks[2], out=outA)
        for f in calls.values():                                   # warm-up: code objects, LDS limits
            f()
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, f in calls.items():
                ms[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        Q, R = len(env.admission_pairs), c.n_bit_rates
        st = outA[:, :, 0]
        res = {"B": B, "active": active, "cells": Q * R, **{f"{k}_ms": v for k, v in med.items()},
               "blocked_cells_A1": float((out1[:, :, 2] + out1[:, :, 3]).mean()), "blocking_probability_A1": float(out1[:, :, 4].mean()),
               "scenarios_applied_of_A": float((st == 0).float().mean()), "scenarios_refused_of_A": float((st >= 2).float().mean())}
        print(f"B={B}: {active:.0f} running services per replica; {Q * R} cells; state as it is: {res['blocked_cells_A1']:.1f} blocked "
              f"cells, blocking probability {res['blocking_probability_A1']:.4f}; of the {A} block actions "
              f"{100 * res['scenarios_applied_of_A']:.1f} % are applied, {100 * res['scenarios_refused_of_A']:.1f} % refused (status 2/3)")
        for k in calls:
            print(f"B={B}: {k:34s} {med[k]:9.3f} ms (median of {ROUNDS})")
        for k in ("admission_map A=1", f"admission_map A={A}"):
            n = B * (1 if k.endswith("A=1") else A)
            print(f"B={B}: {k}: {med[k] * 1e6 / n:.1f} ns per scenario, {med[k] * 1e6 / (n * Q * R):.3f} ns per cell (machine throughput)")
        print(json.dumps(res))
        for e in (env, *twins.values()):
            e.set_stream(None)
            e.close()
        del svc, outE, outA


if __name__ == "__main__":
    main()
