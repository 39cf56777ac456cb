#!/usr/bin/env python3
"""Device time of ongym_cut_links, ongym_repair_links and ongym_failed_links beside ongym_failure_sets with F = 1 on the same
states: NSFNET-320 (capacity 448) after 600 first-fit steps, device buffers, the calls alternated round by round.

    python tools/time_link_cut.py [B ...]              (default 16384)

A cut changes the replicas, so every timed call starts from the same saved state (load_state of one blob, outside the timed
window).  Per call: ongym_last_kernel_ms (the library's events around its kernel) and torch events around the whole call on the
environment's stream.  Sets, one per replica: link r % E; the links of node r % N.  The same sets go to failure_sets as a
[B, 1, 2] list.  Repair and the query run on the state the one-link cut left.  Last, a copy_ of the state bytes."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), REPO, os.path.join(REPO, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_failure_impact import ROUNDS, make_env, timed  # noqa: E402


def main():
    for B in [int(a) for a in sys.argv[1:]] or [16384]:
        env = make_env(B)
        c = env.holder.struct
        E, N, dev = c.n_links, c.n_nodes, torch.device("cuda", c.device)
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)      # noqa: E731
        link = to_dev(env.pack_link_sets([[r % E] for r in range(B)], E))
        node = to_dev(env.node_link_sets()[np.arange(B) % N])
        blob = env.save_state()
        spare = torch.empty_like(blob)
        cut, fs = torch.empty((B, 13), dtype=torch.float64, device=dev), torch.empty((B, 1, 12), dtype=torch.float64, device=dev)
        n, failed = torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int64, device=dev)
        active = float(np.mean(env.stats()["active"]))

        # name -> (the timed call, whether the one-link cut comes first).  The preparation (load_state, that cut) is not timed.
        calls = {"cut_links one link": (lambda: env.cut_links(link, out=cut), False),
                 "failure_sets one link F=1": (lambda: env.failure_sets(link.view(B, 1, 2), out=fs), False),
                 "cut_links node": (lambda: env.cut_links(node, out=cut), False),
                 "failure_sets node F=1": (lambda: env.failure_sets(node.view(B, 1, 2), out=fs), False),
                 "cut_links one link, restore=False": (lambda: env.cut_links(link, restore=False, out=cut), False),
                 "repair_links": (lambda: env.repair_links(link, out=n), True),
                 "failed_links": (lambda: env.failed_links(out=failed), True)}
        res = {"B": B, "active": active, "state_bytes": int(blob.numel())}
        ms, kms, rows = {k: [] for k in calls}, {k: [] for k in calls}, {}
        for rnd in range(ROUNDS + 1):                                  # round 0 warms up: code objects, LDS limits
            for k, (f, cut_first) in calls.items():
                env.load_state(blob)
                if cut_first:
                    env.cut_links(link, out=cut)
                torch.cuda.synchronize()
                t = timed(f)
                if rnd:
                    ms[k].append(t)
                    kms[k].append(env.last_kernel_ms())
                if k.startswith("cut_links"):
                    rows[k] = cut.cpu().numpy().copy()
                if k.startswith("failure_sets"):
                    rows[k] = fs[:, 0].cpu().numpy().copy()
        same = {w: bool(np.array_equal(np.delete(rows[f"cut_links {w}"][:, :12], 9, 1), np.delete(rows[f"failure_sets {w} F=1"], 9, 1)))
                for w in ("one link", "node")}
        res["cut_rows_equal_failure_sets"] = same
        print(f"B={B}: {active:.0f} running services per replica, {blob.numel() / B:.0f} state bytes per replica; "
              f"cut rows (columns 0-8, 10, 11) equal failure_sets': {same}")
        for k in calls:
            med, kmed = float(np.median(ms[k])), float(np.median(kms[k]))
            res[k] = {"kernel_ms": kmed, "kernel_min_ms": float(min(kms[k])), "kernel_max_ms": float(max(kms[k])),
                      "call_ms": med, "call_min_ms": float(min(ms[k])), "call_max_ms": float(max(ms[k]))}
            if k in rows and k.startswith("cut_links"):
                res[k]["victims"] = float(rows[k][:, 1].mean())
                res[k]["restored"] = float(rows[k][:, 3].mean())
            print(f"B={B}: {k:36s} kernel {kmed:8.3f} ms ({min(kms[k]):.3f} .. {max(kms[k]):.3f})   call {med:8.3f} ms "
                  f"({min(ms[k]):.3f} .. {max(ms[k]):.3f})" + (f"   {res[k]['victims']:.1f} victims, {res[k]['restored']:.1f} restored"
                                                              if "victims" in res[k] else ""))
        cp = []
        for rnd in range(ROUNDS + 1):
            t = timed(lambda: spare.copy_(blob))
            if rnd:
                cp.append(t)
        res["copy_ms"] = float(np.median(cp))
        print(f"B={B}: torch copy_ of the state bytes        {np.median(cp):8.3f} ms ({min(cp):.3f} .. {max(cp):.3f}), "
              f"{blob.numel() / np.median(cp) / 1e6:.0f} GB/s")
        print(json.dumps(res))
        env.set_stream(None)
        env.close()


if __name__ == "__main__":
    main()
