#!/usr/bin/env python3
"""Device time of ongym_score_actions beside ongym_policy_actions(ONGYM_POLICY_HIGHEST_SNR) on the same states: NSFNET-320
(capacity 448) after 600 first-fit steps, device buffers, the library's own events (ongym_last_kernel_ms), the calls alternated
round by round.  The policy call is the step kernel doing the same enumeration (every route, format and start, one GN value
each) and keeping the highest GSNR: the yardstick.  Then the two-launch loop `step(score_actions(W))` in env-steps/s, beside
step_policy(policy=HIGHEST_SNR) over as many steps from the same saved state (one launch, the fused loop).

    python tools/time_score_actions.py [--out FILE] [B ...]          (default 16384; repository root, GPU)
"""
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), REPO, os.path.join(REPO, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from optical_networking_gym import _native as nat  # noqa: E402
from time_failure_impact import ROUNDS, make_env  # noqa: E402

LOOP = 200
SCALE = 1.0 / np.array([5, 4, 6, 8, 32, 320, 320, 2, 10, 10], np.float64)


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
    for B in [int(a) for a in args] or [16384]:
        env = make_env(B)
        c = env.holder.struct
        dev = torch.device("cuda", c.device)
        F = len(nat.SCORE_FEATURES)
        W = torch.from_numpy(np.random.default_rng(1).normal(size=(B, F)) * SCALE).to(dev)      # a population: a row per replica
        hs = torch.from_numpy(env.score_preset("highest_snr")).to(dev)
        hs_rows = hs.repeat(B, 1).contiguous()
        actions, pol = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        best, counts = torch.empty((B, 1 + F), dtype=torch.float64, device=dev), torch.empty((B, 3), dtype=torch.int32, device=dev)
        flags = torch.empty(B, dtype=torch.uint8, device=dev)
        recs = torch.empty(B * nat.STEP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())                                                 # noqa: E731

        def policy():
            env._check(env.lib.ongym_policy_actions(env._h, nat.POLICY_HIGHEST_SNR, ptr(pol), ptr(flags)), "ongym_policy_actions")

        calls = {"policy_actions(HIGHEST_SNR)": policy,
                 "score_actions, actions only, a row per replica": lambda: env.score_actions(W, out=actions),
                 "score_actions, all outputs, a row per replica": lambda: env.score_actions(W, out=(actions, best, counts), detail=True),
                 "score_actions, actions only, highest_snr per replica": lambda: env.score_actions(hs_rows, out=actions),
                 "score_actions, actions only, highest_snr shared": lambda: env.score_actions(hs, out=actions)}
        kms = {k: [] for k in calls}
        for rnd in range(ROUNDS + 1):                                  # round 0 warms up: code objects, LDS limits
            for k, f in calls.items():
                f()
                torch.cuda.synchronize()
                if rnd:
                    kms[k].append(env.last_kernel_ms())
        same = bool(torch.equal(actions, pol))                         # the last score call was the highest_snr row
        cnt = counts.cpu().numpy()
        active = float(np.mean(env.stats()["active"]))
        say(f"B={B}: {active:.0f} running services per replica; {cnt[:, 0].mean():.0f} candidates with spectrum per replica, "
            f"{cnt[:, 1].mean():.0f} feasible; highest_snr row == policy_actions(HIGHEST_SNR) on every replica: {same}")
        res = {"B": B, "active": active, "candidates": float(cnt[:, 0].mean()), "feasible": float(cnt[:, 1].mean()), "same": same}
        base = float(np.median(kms["policy_actions(HIGHEST_SNR)"]))
        for k in calls:
            med = float(np.median(kms[k]))
            res[k] = {"kernel_ms": med, "min_ms": float(min(kms[k])), "max_ms": float(max(kms[k])), "ratio_to_policy": med / base}
            say(f"B={B}: {k:54s} kernel {med:8.3f} ms ({min(kms[k]):.3f} .. {max(kms[k]):.3f})   x{med / base:.3f} of the policy call")
        # the loops: from the same saved state, timed with a host clock around work that ends in a synchronise
        blob = env.save_state()
        loops = {}
        for name in ("score + step, two launches", "step_policy(HIGHEST_SNR), fused") * 3:
            env.load_state(blob)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name.startswith("score"):
                for _ in range(LOOP):
                    env.score_actions(W, out=actions)
                    env._check(env.lib.ongym_step_actions(env._h, ptr(actions), ptr(recs)), "ongym_step_actions")
            else:
                env.step_policy(LOOP, record=False, policy=nat.POLICY_HIGHEST_SNR)
            torch.cuda.synchronize()
            loops.setdefault(name, []).append(B * LOOP / (time.perf_counter() - t0))
        for name, v in loops.items():
            res[name] = {"env_steps_per_s": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
            say(f"B={B}: {name:36s} {np.median(v):12.4g} env-steps/s ({min(v):.4g} .. {max(v):.4g}) over {LOOP} steps")
        say(json.dumps(res))
        env.set_stream(None)
        env.close()


if __name__ == "__main__":
    main()
