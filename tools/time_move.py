#!/usr/bin/env python3
"""Device time of ongym_move_services beside ongym_cut_links on the same states: NSFNET-320 (capacity 448) after 600 first-fit
steps (the setup of tools/time_link_cut.py), device buffers, the calls alternated round by round.

    python tools/time_move.py [B ...]              (default 16384)

Every timed call starts from the same saved state (load_state of one blob, outside the timed window).  Per call:
ongym_last_kernel_ms (the library's events around its kernel) and torch events around the whole call on the environment's
stream.  Moves: one explicit move per replica (record r % active one slot down on its own route and format); one
(TOP, FIRST_FIT) move; defragment's list of 32 (TOP, FIRST_FIT) rows on the own route.  Cuts: link r % E per replica, with and
without restoration."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), REPO, os.path.join(REPO, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from optical_networking_gym import _native as nat  # noqa: E402
from time_failure_impact import ROUNDS, config, make_env, timed  # noqa: E402


def main():
    for B in [int(a) for a in sys.argv[1:]] or [16384]:
        env = make_env(B)
        c = env.holder.struct
        E, M, S, dev = c.n_links, c.n_mods, c.n_slots, torch.device("cuda", c.device)
        link = torch.from_numpy(np.ascontiguousarray(env.pack_link_sets([[r % E] for r in range(B)], E)).view(np.int64)).to(dev)
        blob = env.save_state()
        active = float(np.mean(env.stats()["active"]))
        # record r % active one slot down on its own route and format (k: the route's place in its pair's list)
        k_of = {}
        for row in np.asarray(config()[0].pair_paths).reshape(-1, c.k_paths):
            for k, p in enumerate(row):
                k_of.setdefault(int(p), k)
        explicit = np.zeros((B, 1, 2), np.int32)
        for r in range(B):
            s = env.services(r)
            i = r % max(1, len(s))
            if len(s):
                explicit[r, 0] = i, k_of[int(s["path_id"][i])] * M * S + (M - 1 - int(s["modulation"][i])) * S + max(int(s["slot"][i]) - 1, 0)
        top = np.tile(np.array([nat.MOVE_TOP, nat.MOVE_FIRST_FIT], np.int32), (B, 1, 1))
        sweep = np.tile(np.array([nat.MOVE_TOP, nat.MOVE_FIRST_FIT], np.int32), (B, 32, 1))
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        explicit_t, top_t, sweep_t = to_dev(explicit), to_dev(top), to_dev(sweep)
        out1, out32 = (torch.empty((B, n, 6), dtype=torch.float64, device=dev) for n in (1, 32))
        cut = torch.empty((B, 13), dtype=torch.float64, device=dev)

        calls = {"move_services one record, one slot down": (lambda: env.move_services(explicit_t, out=out1), out1),
                 "move_services one (TOP, FIRST_FIT)": (lambda: env.move_services(top_t, out=out1), out1),
                 "defragment(32): 32 (TOP, FIRST_FIT), own route": (lambda: env.move_services(sweep_t, own_route=True, out=out32), out32),
                 "cut_links one link": (lambda: env.cut_links(link, out=cut), cut),
                 "cut_links one link, restore=False": (lambda: env.cut_links(link, restore=False, out=cut), cut)}
        res = {"B": B, "active": active, "state_bytes": int(blob.numel())}
        ms, kms, rows = {k: [] for k in calls}, {k: [] for k in calls}, {}
        for rnd in range(ROUNDS + 1):                                  # round 0 warms up: code objects, LDS limits
            for k, (f, o) in calls.items():
                env.load_state(blob)
                torch.cuda.synchronize()
                t = timed(f)
                if rnd:
                    ms[k].append(t)
                    kms[k].append(env.last_kernel_ms())
                rows[k] = o.cpu().numpy().copy()
        print(f"B={B}: {active:.0f} running services per replica, {blob.numel() / B:.0f} state bytes per replica")
        for k in calls:
            med, kmed = float(np.median(ms[k])), float(np.median(kms[k]))
            res[k] = {"kernel_ms": kmed, "kernel_min_ms": float(min(kms[k])), "kernel_max_ms": float(max(kms[k])),
                      "call_ms": med, "call_min_ms": float(min(ms[k])), "call_max_ms": float(max(ms[k]))}
            if k.startswith("cut_links"):
                res[k]["victims"], res[k]["restored"] = float(rows[k][:, 1].mean()), float(rows[k][:, 3].mean())
                note = f"   {res[k]['victims']:.1f} victims, {res[k]['restored']:.1f} restored"
            else:
                st = rows[k][:, :, 0].astype(int)
                res[k]["status_per_replica"] = [float(np.mean(np.sum(st == v, axis=1))) for v in range(5)]
                note = "   per replica: " + ", ".join(f"{n} {x:.2f}" for n, x in zip(("moved", "invalid", "unchanged", "no spectrum", "QoT"),
                                                                                   res[k]["status_per_replica"]))
            print(f"B={B}: {k:48s} kernel {kmed:8.3f} ms ({min(kms[k]):.3f} .. {max(kms[k]):.3f})   call {med:8.3f} ms "
                  f"({min(ms[k]):.3f} .. {max(ms[k]):.3f})" + note)
        print(json.dumps(res))
        env.set_stream(None)
        env.close()


if __name__ == "__main__":
    main()
