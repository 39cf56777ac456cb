#!/usr/bin/env python3
"""Device time of ongym_spectrum_map by output set (audit only, records + release, owners only, everything) on the bench
workload: NSFNET-320 as bench.py loads it, device buffers, the library's own events (ongym_last_kernel_ms).  check_state() runs
after 1 000 first-fit steps (step 1 000 ends the first episode: the auto reset has just run) and again 600 steps into the second
episode, the loaded state that is timed; it raises on any violation.  Two baselines from the same run: a torch fill_ of the
same output bytes, and link_metrics(), which reads the same state.  Last, the host loop the call replaces: grid(r) +
services(r) + the numpy restatement of tests/test_gpu_spectrum_map.py, per replica, on 64 replicas of a host environment.

    python tools/time_spectrum_map.py [--out FILE] [B ...]          (default 16384 65536; repository root, GPU)
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv  # noqa: E402
from test_gpu_spectrum_map import from_views  # noqa: E402

ROUNDS = 9
SETS = {"audit": ("audit",), "records+release": ("records", "release"), "owners": ("owners",),
        "everything": ("owners", "records", "release", "audit")}


def make(B, io_device, steps=1000):
    wl = bench.WORKLOADS["nsfnet320"]
    env = BatchedQRMSAEnv(tables=bench.build_tables(wl["topology"]), modulations=bench.jocn_modulations(), batch_size=B,
                          num_spectrum_resources=wl["S"], capacity=wl["capacity"], episode_length=1000, auto_reset=True,
                          load=wl["load"], bit_rate_selection="discrete", bit_rates=wl["bit_rates"], io_device=io_device)
    if io_device:
        env.set_stream(torch.cuda.current_stream().cuda_stream)
    env.seed(1)
    env.reset()
    env.step_policy(steps, record=False)
    return env


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    args = sys.argv[1:]
    say = print
    if "--out" in args:
        i = args.index("--out")
        log = open(args[i + 1], "w")
        del args[i:i + 2]

        def say(*a):
            print(*a, flush=True)
            print(*a, file=log, flush=True)
    for B in [int(a) for a in args] or [16384, 65536]:
        env = make(B, True)
        c = env.holder.struct
        E, S, Cp, dev = c.n_links, c.n_slots, c.capacity, torch.device("cuda", c.device)
        for more in (0, 600):              # step 1000 ends the first episode (auto reset): 600 more steps load the network again
            if more:
                env.step_policy(more, record=False)
            audit = env.check_state()                              # raises on any violation
            say(f"B={B}: check_state() after {1000 + more} first-fit steps: no violation; {audit[:, 1].mean():.0f} records and "
                f"{audit[:, 8].mean():.0f} claimed cells per replica, {int(audit[:, 7].sum())} failed links")
        t = dict(owners=torch.empty((B, E, S), dtype=torch.int16, device=dev), records=torch.empty((B, Cp, 6), dtype=torch.int32, device=dev),
                 release=torch.empty((B, Cp), dtype=torch.float32, device=dev), audit=torch.empty((B, 10), dtype=torch.int32, device=dev))
        link = torch.empty((B, E, 8), dtype=torch.float32, device=dev)
        comp = torch.empty((B,), dtype=torch.float64, device=dev)

        def call(names):
            env.spectrum_map(out={n: t[n] for n in names}, owners="owners" in names, records="records" in names, audit="audit" in names)

        res = {"B": B}
        for k, names in SETS.items():
            call(names)                                            # warm-up
        env.link_metrics(out=(link, comp))
        ms = {k: [] for k in list(SETS) + ["link_metrics"] + ["fill_ " + k for k in SETS]}
        for _ in range(ROUNDS):                                    # alternated round by round
            for k, names in SETS.items():
                call(names)
                ms[k].append(env.last_kernel_ms())
                ms["fill_ " + k].append(timed(lambda: [t[n].fill_(0) for n in names]))
            env.link_metrics(out=(link, comp))
            ms["link_metrics"].append(env.last_kernel_ms())
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k, names in SETS.items():
            nbytes = sum(t[n].numel() * t[n].element_size() for n in names)
            say(f"B={B}: {k:16s} {med[k]:8.3f} ms | {nbytes / 1e6:8.1f} MB out, {nbytes / med[k] / 1e9:5.2f} TB/s | fill_ of the same bytes "
                f"{med['fill_ ' + k]:7.3f} ms, ratio {med[k] / med['fill_ ' + k]:5.2f}")
        say(f"B={B}: link_metrics()   {med['link_metrics']:8.3f} ms | audit / link_metrics = {med['audit'] / med['link_metrics']:.2f}, "
            f"owners / fill_ = {med['owners'] / med['fill_ owners']:.2f}")
        res.update({k + "_ms": v for k, v in med.items()})
        say(json.dumps(res))
        env.set_stream(None)
        env.close()
        del t, link, comp
        torch.cuda.empty_cache()
    host = make(64, False, 1600)
    c = host.holder.struct
    t0 = time.perf_counter()
    views = [(host.grid(r), host.services(r)) for r in range(64)]
    t1 = time.perf_counter()
    rows = [from_views(host.tables, c.n_mods, c.n_slots, c.capacity, g, s, c.n_slots) for g, s in views]
    t2 = time.perf_counter()
    got = host.spectrum_map(owners=True, records=True, audit=True)
    t3 = time.perf_counter()
    same = all(np.array_equal(got["owners"][r], rows[r][0]) and np.array_equal(got["audit"][r], rows[r][1]) for r in range(64))
    say(f"host loop on 64 replicas: grid(r) + services(r) {(t1 - t0) / 64 * 1e3:.3f} ms per replica, numpy restatement "
        f"{(t2 - t1) / 64 * 1e3:.3f} ms per replica; the one call for all 64 through host buffers {(t3 - t2) * 1e3:.3f} ms; same arrays: {same}")
    host.close()


if __name__ == "__main__":
    main()
