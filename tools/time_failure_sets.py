#!/usr/bin/env python3
"""Device time of ongym_failure_sets beside ongym_failure_impact on the same states: NSFNET-320 (capacity 448) after 600
first-fit steps, device buffers, torch events on the environment's stream, the calls alternated round by round.

    python tools/time_failure_sets.py [B ...]              (default 16384 65536)
    python tools/time_failure_sets.py --host-loop [N]      (default 3 replicas)

Per batch size it times failure_impact(links=None) and failure_sets with the E one-link sets (identical work per scenario:
the difference is held against the spread of failure_impact's own runs, and the rows are compared), then failure_sets with
every node's link set and with all E (E - 1) / 2 dual cuts.

--host-loop times the only way to the same answer without the call, the loop an application would write: services() and
grid() of a replica, then the numpy restatement of tests/failure_sets_child.py with the CPU oracle's GN, for the node sets and
for all dual cuts of N sample replicas; it also counts the evaluated (route, format, start) triples per scenario, which turn
the device's time per scenario into a time per triple, and compares its rows with the device's.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), REPO, os.path.join(REPO, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from optical_networking_gym import _native as nat  # noqa: E402
from time_failure_impact import ROUNDS, config, make_env, timed  # noqa: E402


def device_sets(env, sets):
    return torch.from_numpy(np.ascontiguousarray(sets).view(np.int64)).to(torch.device("cuda", env.holder.struct.device))


def host_loop(N):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from failure_sets_child import restate_sets
    from oracle_lib import OracleEnv
    tb, kw = config()
    env = make_env(max(N, 64))
    holder = nat.ConfigHolder(tb, batch=env.batch_size, **kw)
    res = {"replicas": N}
    for name, sets in (("node", env.node_link_sets()), ("dual", env.link_pair_sets())):
        F = len(sets)
        out = torch.empty((env.batch_size, F, 12), dtype=torch.float64, device="cuda")
        env.failure_sets(device_sets(env, sets), out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        secs, evals, victims, same = [], 0, 0, True
        for r in range(N):
            o = OracleEnv(holder, replica=r)
            t0 = time.perf_counter()
            svcs, grid = env.services(r), env.grid(r)
            log = []
            want, _ = restate_sets(o, tb, holder, float(kw.get("margin", 0.0)), svcs, grid, sets, log=log)
            secs.append(time.perf_counter() - t0)
            evals += len(log)
            victims += int(want[:, 1].sum())
            same &= bool(np.array_equal(np.delete(got[r], 9, axis=1), np.delete(want, 9, axis=1)))
        per = float(np.mean(secs))
        res[name] = {"scenarios": F, "host_seconds_per_replica": per, "triples_per_scenario": evals / (N * F),
                     "victims_per_scenario": victims / (N * F), "rows_equal_device": same}
        print(f"host loop, {name} sets: {per:.3f} s per replica ({F} scenarios), {victims / (N * F):.1f} victims and "
              f"{evals / (N * F):.1f} evaluated triples per scenario (the device answers some of them with the ASE bound), rows equal "
              f"the device's: {same}")
        for B in (16384, 65536):
            print(f"  scaled to B = {B}: {per * B:.0f} s")
    print(json.dumps(res))
    env.set_stream(None)
    env.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--host-loop":
        host_loop(int(args[1]) if len(args) > 1 else 3)
        return
    for B in [int(a) for a in args] or [16384, 65536]:
        env = make_env(B)
        c = env.holder.struct
        E, N, dev = c.n_links, c.n_nodes, torch.device("cuda", c.device)
        lists = {"one-link": env.pack_link_sets([[e] for e in range(E)], E), "node": env.node_link_sets(),
                 "dual": env.link_pair_sets()}
        sets = {k: device_sets(env, v) for k, v in lists.items()}
        outs = {k: torch.empty((B, len(v), 12), dtype=torch.float64, device=dev) for k, v in lists.items()}
        outE = torch.empty((B, E, 10), dtype=torch.float64, device=dev)
        active = float(np.mean(env.stats()["active"]))
        calls = {f"failure_impact F={E}": lambda: env.failure_impact(out=outE)}
        for k in lists:
            calls[f"failure_sets {k} F={len(lists[k])}"] = (lambda k=k: env.failure_sets(sets[k], out=outs[k]))
        for f in calls.values():                                   # warm-up: code objects, LDS limits
            f()
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["one-link"][:, :, :9], outE[:, :, :9])
                    and torch.equal(torch.nan_to_num(outs["one-link"][:, :, 9], nan=-1e9), torch.nan_to_num(outE[:, :, 9], nan=-1e9)))
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, f in calls.items():
                ms[k].append(timed(f))
        res = {"B": B, "active": active, "one_link_rows_equal_failure_impact": same}
        print(f"B={B}: {active:.0f} running services per replica; one-link sets equal failure_impact: {same}")
        for (k, v), F, o in zip(ms.items(), [E] + [len(x) for x in lists.values()], [outE] + list(outs.values())):
            med = float(np.median(v))
            res[k] = {"ms": med, "min_ms": float(min(v)), "max_ms": float(max(v)), "ns_per_scenario": med * 1e6 / (B * F),
                      "victims_per_scenario": float(o[:, :, 1].mean()), "restored_per_scenario": float(o[:, :, 3].mean()),
                      "lost_no_spectrum_per_scenario": float(o[:, :, 5].mean()), "lost_qot_per_scenario": float(o[:, :, 6].mean())}
            if o.shape[2] > 10:
                res[k]["lost_no_route_per_scenario"] = float(o[:, :, 10].mean())
            print(f"B={B}: {k:32s} {med:10.3f} ms (median of {ROUNDS}, {min(v):.3f} .. {max(v):.3f}), "
                  f"{res[k]['ns_per_scenario']:.1f} ns per scenario, {res[k]['victims_per_scenario']:.1f} victims per scenario")
        print(json.dumps(res))
        env.set_stream(None)
        env.close()
        del outs, outE, sets


if __name__ == "__main__":
    main()
