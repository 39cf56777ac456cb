"""Child process of tests/test_gpu_move.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP runtime
and this library's must start together), saved to an .npz that the tests assert on.

    python tests/move_child.py OUT.npz

It also holds the restatement of ongym_move_services (include/ongym.h) in plain numpy, `expected_moves`: one move after the
other on a copy of the records and the grid, with `release`, `provision`, `search`, `gn_running` and `route_of` of
tests/failure_impact_child.py, the valid starts from the oracle's `candidates` (_get_candidates) and every GN value from the
oracle's literal GN on explicit interferer lists: the other records in record order, the moved one left out.
tests/test_move_host.py runs it on the CPU oracles of the same cases and seeds.

Replica r's moves are drawn by `draw_moves` with default_rng(MOVE_SEED + r) from its pre-call services() and grid().
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402,F401  (before the library is loaded: the two HIP runtimes must start together)

from common import golden_tables, record_bytes  # noqa: E402
from failure_impact_child import (BAND, BASE, CASES, SEED, case_config, drive, free_row, gn_running, path_links_of, provision,  # noqa: E402,F401
                                  release, replica_margin, ring_tables, route_of, search, tab_nmax)
from link_cut_child import (FIELDS, OSNR, crossing, extend_trace, grid_of_records, links_of, make_env, replica_links,  # noqa: E402,F401
                            running_of, state_of, stats_same, svc_rows)
from optical_networking_gym import _native as nat  # noqa: E402

MOVE_SEED = 700                                  # replica r draws its moves with default_rng(MOVE_SEED + r)
TRAFFIC = ("nsfnet", "nobeleu", "odd", "ring4")  # the cases that go on with traffic after the moves
BOTH = ("nsfnet", "nobeleu")                     # the cases run on both step kernels
TOP, FIRST_FIT = nat.MOVE_TOP, nat.MOVE_FIRST_FIT
LEAN = ("ring4", "nsfnet", "odd")                # the cases whose configuration a lean step kernel can run
COVER = ("moved", "invalid", "unchanged", "no_spectrum", "qot", "other_route", "other_format", "shift_down", "ends_at_S",
         "namesake", "top_skips", "to_S", "too_wide")


# ---- the moves --------------------------------------------------------------------------------------------------------------
def encode(holder, k, m, start):
    c = holder.struct
    return k * c.n_mods * c.n_slots + (c.n_mods - 1 - m) * c.n_slots + start


def width_limit(holder, lean):
    """the widest record a move may write: where a lean step kernel may run on the environment, the widest slot count of the
    traffic table (the pair table's rows, tab_nmax), 32 in the narrow build (no slot count of the table above 32); else S"""
    S, nmax = holder.struct.n_slots, tab_nmax(holder)
    return min(nmax, 32 if nmax <= 32 else 512, S) if lean else S


def top_record(rows, attempted):
    """ONGYM_MOVE_TOP: the record outside `attempted` whose last slot is highest, the lowest index on a tie; -1 if none"""
    best, at = -1, -1
    for i, r in enumerate(rows):
        last = int(r[1]) + int(r[2]) - 1
        if i not in attempted and last > best:
            best, at = last, i
    return at


def draw_moves(o, tb, holder, svcs, grid, r, ids=False):
    """int32 [12, 2]: replica r's moves, drawn from its pre-call state.  One of each kind, in this order: a one-slot shift down
    that overlaps the old range; the pre-call top record to another route; TOP to first fit (which then skips that record if
    it stayed on top); another format on the own route; a random action; an invalid record or action; the present placement; the
    best format on the last route (QoT); a namesake (ids) or a record that ends at S to first fit; an own-route action that
    ends at S; two more TOP sweeps"""
    c = holder.struct
    K, M, S = c.k_paths, c.n_mods, c.n_slots
    se = np.asarray(holder.mod_se)
    rng = np.random.default_rng(MOVE_SEED + r)
    rows, routes, n = svc_rows(svcs), route_of(tb), len(svcs)
    moves = np.zeros((12, 2), np.int32)
    moves[:, 0], moves[:, 1] = TOP, FIRST_FIT
    if n == 0:
        return moves

    def freed(i):                                   # the pre-call grid with record i's own range free
        g = grid.copy()
        release(g, tb, int(rows[i, 0]), int(rows[i, 1]), int(rows[i, 2]))
        return g

    def place(i):
        p, s, nn, m = (int(x) for x in rows[i, :4])
        return p, s, nn, m, routes[p]

    def first_start(i, path, nn):
        st = o.candidates(free_row(freed(i), tb, path), nn) if 0 < nn <= S else []
        return int(st[0]) if st else int(rng.integers(S))

    # 0: one slot down, same route and format
    down = [i for i in range(n) if rows[i, 1] >= 1 and np.all(grid[path_links_of(tb, int(rows[i, 0])), int(rows[i, 1]) - 1] == 1)]
    i = int(rng.choice(down)) if down else int(rng.integers(n))
    p, s, nn, m, (_, _, k) = place(i)
    moves[0] = i, encode(holder, k, m, max(s - 1, 0))
    # 1: the top record to another route of its pair, same format
    i = top_record(rows, {int(moves[0, 0])} if n > 1 else set())
    p, s, nn, m, (src, dst, k) = place(i)
    ks = [kk for kk in range(K) if kk != k and tb.pair_paths[src, dst, kk] >= 0]
    k2 = int(rng.choice(ks)) if ks else k
    moves[1] = i, encode(holder, k2, m, first_start(i, int(tb.pair_paths[src, dst, k2]), nn))
    # 2: TOP, first fit (the defaults)
    # 3: another format on the own route: the next lower one (more slots), or the next higher
    i = int(rng.integers(n))
    p, s, nn, m, (_, _, k) = place(i)
    m2 = m - 1 if m > 0 else m + 1
    moves[3] = i, encode(holder, k, m2, first_start(i, p, -(-nn * int(se[m]) // int(se[m2]))))
    # 4: anything
    moves[4] = int(rng.integers(n)), int(rng.integers(K * M * S))
    # 5: invalid
    moves[5] = [(n + int(rng.integers(3)), FIRST_FIT), (-2, FIRST_FIT), (int(rng.integers(n)), K * M * S),
                (int(rng.integers(n)), -7)][r % 4]
    # 6: where it is
    i = int(rng.integers(n))
    p, s, nn, m, (_, _, k) = place(i)
    moves[6] = i, encode(holder, k, m, s)
    # 7: the best format on the pair's last route
    i = int(rng.integers(n))
    p, s, nn, m, (src, dst, k) = place(i)
    k2 = max(kk for kk in range(K) if tb.pair_paths[src, dst, kk] >= 0)
    moves[7] = i, encode(holder, k2, M - 1, first_start(i, int(tb.pair_paths[src, dst, k2]), -(-nn * int(se[m]) // int(se[M - 1]))))
    # 8: a namesake (ids), else a record that ends at S, else anything, to first fit
    sid = rows[:, 6].astype(np.int64)
    twice = [i for i in range(n) if ids and np.sum(sid == sid[i]) > 1]
    at_S = [i for i in range(n) if rows[i, 1] + rows[i, 2] == S]
    moves[8, 0] = int(rng.choice(twice)) if twice else int(rng.choice(at_S)) if at_S else int(rng.integers(n))
    # 9: to the end of the own route's row, where no guard slot is needed
    i = int(rng.integers(n))
    p, s, nn, m, (_, _, k) = place(i)
    moves[9] = i, encode(holder, k, m, S - nn)
    return moves


# ---- the restatement --------------------------------------------------------------------------------------------------------
def expected_moves(o, tb, holder, margin, svcs, grid, moves, ids=False, own_route=False, log=None, cover=None, limit=None):
    """(move_out [N, 6], post-call records [n, 8] in the columns FIELDS, post-call grid) of `moves` (int32 [N, 2]) on the state
    (svcs in record order, grid).  With ids the osnr column of a moved record is the new GSNR from the oracle's literal GN;
    without, it stays what it was.  log collects every evaluation's relative distance to its limit, cover what the moves do;
    limit is the widest record a move may write (width_limit; None: S)"""
    c = holder.struct
    K, M, S, n = c.k_paths, c.n_mods, c.n_slots, len(svcs)
    se, thr = np.asarray(holder.mod_se), np.asarray(holder.mod_thr)
    rows, grid, routes = svc_rows(svcs).copy(), grid.copy(), route_of(tb)
    cover = cover if cover is not None else {}
    out = np.zeros((len(moves), len(nat.MOVE_COLUMNS)))
    attempted = set()
    limit = S if limit is None else limit

    def count(name, v=1):
        cover[name] = cover.get(name, 0) + int(v)

    for t, (sel, target) in enumerate(np.asarray(moves).tolist()):
        out[t] = 1, -1, -1, -1, np.nan, 0
        if sel == TOP:
            i = top_record(rows, attempted)
            if i < 0:
                count("invalid")
                continue
            count("top_skips", i != top_record(rows, set()))
        elif 0 <= sel < n:
            i = sel
        else:
            count("invalid")
            continue
        attempted.add(i)
        out[t, 1] = i
        path, s, nn, m, sid = int(rows[i, 0]), int(rows[i, 1]), int(rows[i, 2]), int(rows[i, 3]), int(rows[i, 6])
        if path not in routes:
            count("invalid")
            continue
        src, dst, k0 = routes[path]
        out[t, 2] = out[t, 3] = k0 * M * S + (M - 1 - m) * S + s
        cap = nn * int(se[m])
        nslots = [-(-cap // int(x)) for x in se]
        count("too_wide", target != FIRST_FIT and 0 <= target < K * M * S and limit < nslots[M - 1 - (target // S) % M] <= S)
        count("too_wide", target == FIRST_FIT and any(limit < x <= S for x in nslots))
        nslots = [x if x <= limit else S + 1 for x in nslots]              # a format beyond the width limit is unusable
        others = [x for j, x in enumerate(running_of(rows)) if j != i]
        freed = grid.copy()
        release(freed, tb, path, s, nn)                                   # its own spectrum counts as free

        def gn(p, a, n2):
            return gn_running(o, tb, se, others, p, a, n2, sid if ids else None)[0]

        if target != FIRST_FIT:
            k, mm, start = target // (M * S), M - 1 - (target // S) % M, target % S
            p = int(tb.pair_paths[src, dst, k]) if 0 <= target < K * M * S else -1
            if p < 0:
                count("invalid")
                continue
            if (p, mm, start) == (path, m, s):
                out[t, 0] = 2
                count("unchanged")
                continue
            n2 = nslots[mm]
            if n2 > S or start not in o.candidates(free_row(freed, tb, p), n2):
                out[t, 0] = 3
                count("no_spectrum")
                continue
            g = gn(p, start, n2)
            if log is not None:
                log.append(abs(10.0 ** ((thr[mm] + margin - g) / 10.0) - 1.0))
            if not g >= thr[mm] + margin:
                out[t, 0] = 4
                count("qot")
                continue
        else:
            way = [(k0, path)] if own_route else []
            for k in range(0 if own_route else K):
                p = int(tb.pair_paths[src, dst, k])
                if p < 0:
                    break
                way.append((k, p))
            hit, evaluated = search(o, tb, thr, margin, nslots, way, freed, gn, log)
            if hit is None:
                out[t, 0] = 4 if evaluated else 3
                count("qot" if evaluated else "no_spectrum")
                continue
            k, mm, start, g = hit
            p, n2 = dict(way)[k], nslots[mm]
            if (p, mm, start) == (path, m, s):
                out[t, 0] = 2
                count("unchanged")
                continue
        grid = freed
        provision(grid, tb, p, start, n2)
        rows[i, :4] = p, start, n2, mm
        if ids:
            rows[i, OSNR] = g
        out[t] = 0, i, out[t, 2], k * M * S + (M - 1 - mm) * S + start, g - thr[mm] - margin, \
            n2 * int(tb.path_hops[p]) - nn * int(tb.path_hops[path])
        count("moved")
        count("other_route", p != path)
        count("other_format", mm != m and n2 != nn)
        count("shift_down", p == path and mm == m and start == s - 1)
        count("ends_at_S", s + nn == S)
        count("to_S", start + n2 == S)
        count("namesake", ids and any(x[4] == sid for x in others))
    return out, rows, grid


EXACT = [0, 1, 2, 3, 5]                           # the move_out columns compared exactly; 4 (margin) is a dB value


# ---- the GPU computations ---------------------------------------------------------------------------------------------------
def all_moves(ors, tb, holder, svcs, grids, ids):
    return np.ascontiguousarray(np.stack([draw_moves(o, tb, holder, svcs[r], grids[r], r, ids) for r, o in enumerate(ors)]))


def gpu_case(out, key):
    tb, kw, B, _, how = case_config(key)
    ids = how == "ids"
    env, twin = make_env(key), make_env(key)
    tb, kw, holder, ors = drive(key, env, oracles=False)          # the oracles only lend `candidates` and `gn_lists`
    drive(key, twin, oracles=False)
    if how == "trace":
        extend_trace(env, tb, kw, B)
    c = holder.struct
    E, S = tb.n_links, c.n_slots
    svcs0, grid0 = state_of(env, B)
    moves = all_moves(ors, tb, holder, svcs0, grid0, ids)
    lean = env.occupancy()["lean_kernel"]
    limit = width_limit(holder, lean)
    out[key + "_lean"], out[key + "_limit"] = lean, limit
    blob0, st0 = env.save_state(), env.stats()
    blobs0 = [env.save_state([r]).tobytes() for r in range(B)]
    twin.load_state(blob0)

    got = env.move_services(moves)
    out[key + "_kernel_ms"] = env.last_kernel_ms()
    st1 = env.stats()
    svcs1, grid1 = state_of(env, B)
    qot = env.service_qot()[0]
    blobs1 = [env.save_state([r]).tobytes() for r in range(B)]
    out[key + "_moves"], out[key + "_got"] = moves, got
    out[key + "_blob_same"] = np.array([blobs0[r] == blobs1[r] for r in range(B)])
    out[key + "_stats_same"] = stats_same(st0, st1, ("episode_osnr_sum",) if ids else ())
    out[key + "_osnr_sum"] = np.stack([st0["episode_osnr_sum"], st1["episode_osnr_sum"]])
    near, tot, delta = 0, {}, np.zeros(B)
    qot_margin = np.full((B, moves.shape[1]), np.nan)
    for r, o in enumerate(ors):
        log, cover = [], {}
        margin = replica_margin(kw, r)
        want, post, grid = expected_moves(o, tb, holder, margin, svcs0[r], grid0[r], moves[r], ids, False, log, cover, limit)
        k = f"{key}_r{r}"
        out[k + "_want"], out[k + "_post"], out[k + "_grid"] = want, post, grid
        out[k + "_pre"], out[k + "_got_post"], out[k + "_got_grid"] = svc_rows(svcs0[r]), svc_rows(svcs1[r]), grid1[r]
        near += int(np.sum(np.array(log) < BAND))
        if ids and len(svcs1[r]) == len(svcs0[r]):
            delta[r] = float(np.sum(svcs1[r]["osnr"] - svcs0[r]["osnr"]))
        ok = np.flatnonzero(got[r, :, 0] == 0)
        if len(ok):                                                   # the last move that succeeded: nothing changed after it
            t = int(ok[-1])
            qot_margin[r, t] = qot[r, int(got[r, t, 1]), 3] - margin
        for name in COVER:
            tot[name] = tot.get(name, 0) + cover.get(name, 0)
    out[key + "_band"], out[key + "_osnr_delta"], out[key + "_qot_margin"] = near, delta, qot_margin
    for name, v in tot.items():
        out[f"{key}_cond_{name}"] = v
    out[key + "_B"], out[key + "_E"], out[key + "_S"], out[key + "_ids"] = B, E, S, ids
    out[key + "_rec32"] = bool(tb.n_links <= 32 and len(tb.path_hops) <= 512)

    # the sweep on the twin, which holds the pre-call state: defragment(n) is n rows (TOP, FIRST_FIT) on the own route
    n = 6
    sweep = twin.defragment(n)
    blob_a = twin.save_state().tobytes()
    out[key + "_sweep"] = sweep
    rows_tf = np.tile(np.array([TOP, FIRST_FIT], np.int32), (n, 1))
    for r, o in enumerate(ors):
        want, post, grid = expected_moves(o, tb, holder, replica_margin(kw, r), svcs0[r], grid0[r], rows_tf, ids, True, limit=limit)
        k = f"{key}_r{r}_sweep"
        out[k + "_want"], out[k + "_post"], out[k + "_grid"] = want, post, grid
        out[k + "_got_post"], out[k + "_got_grid"] = svc_rows(twin.services(r)), twin.grid(r)
    twin.load_state(blob0)
    same = twin.move_services(rows_tf, own_route=True)
    out[key + "_sweep_same"] = bool(np.array_equal(same, sweep, equal_nan=True) and twin.save_state().tobytes() == blob_a)
    # every move again as a call of its own with the record it resolved to, service_qot() after each: the margin of EVERY moved
    # record on the state its move left
    twin.load_state(blob0)
    each, each_qot = np.zeros_like(got), np.full(got.shape[:2], np.nan)
    for t in range(moves.shape[1]):
        one = moves[:, t:t + 1].copy()
        one[:, 0, 0] = np.where(got[:, t, 1] >= 0, got[:, t, 1], -2).astype(np.int32)
        each[:, t] = twin.move_services(np.ascontiguousarray(one))[:, 0]
        q = twin.service_qot()[0]
        for r in np.flatnonzero(each[:, t, 0] == 0):
            each_qot[r, t] = q[r, int(each[r, t, 1]), 3] - replica_margin(kw, r)
    out[key + "_each"], out[key + "_each_qot"] = each, each_qot
    out[key + "_each_state_same"] = all(np.array_equal(twin.services(r), svcs1[r]) and np.array_equal(twin.grid(r), grid1[r])
                                        for r in range(B))
    twin.load_state(blob0)
    anywhere = twin.defragment(n, own_route=False)
    out[key + "_sweep_anywhere_differs"] = not np.array_equal(anywhere, sweep, equal_nan=True)
    twin.close()

    if key in TRAFFIC:                                               # traffic goes on after the moves
        moved = [[int(i) for i in got[r, got[r, :, 0] == 0, 1]] for r in range(B)]
        new = [{(float(svcs1[r]["release_time"][i]), int(svcs1[r]["path_id"][i]), int(svcs1[r]["slot"][i])) for i in moved[r]}
               for r in range(B)]
        grid_ok, left = [], []
        for _ in range(6):
            env.step_policy(50, record=False)
            s, g = state_of(env, B)
            grid_ok.append([np.array_equal(g[r], grid_of_records(tb, E, S, svc_rows(s[r]))) for r in range(B)])
            left.append(sum(len(new[r] & {(float(x["release_time"]), int(x["path_id"]), int(x["slot"])) for x in s[r]})
                            for r in range(B)))
        out[key + "_run_grid_ok"], out[key + "_run_moved_left"] = np.array(grid_ok), np.array(left)
        out[key + "_run_moved"] = sum(len(x) for x in new)
        out[key + "_run_steps"] = env.stats()["total_steps"] - st1["total_steps"]
    env.close()


def both_kernels(out, key):
    """the same moves after the same launch on the lean and on the generic step kernel, then five recorded launches of 50 steps
    with the grid invariant after each, on both"""
    tb, kw, B, _, how = case_config(key)
    recs, outs, ends, ok = [], [], [], []
    for generic in (False, True):
        env = make_env(key, generic=generic)
        tb, kw, holder, ors = drive(key, env, oracles=False)
        if how == "trace":
            extend_trace(env, tb, kw, B)
        c = holder.struct
        svcs, grids = state_of(env, B)
        outs.append(env.move_services(all_moves(ors, tb, holder, svcs, grids, how == "ids")))
        runs = []
        for _ in range(5):
            runs.append(env.step_policy(50))
            sv, g = state_of(env, B)
            ok.append([np.array_equal(g[r], grid_of_records(tb, tb.n_links, c.n_slots, svc_rows(sv[r]))) for r in range(B)])
        recs.append({f: np.concatenate([x[f] for x in runs]) for f in ("action", "accepted", "flags", "active", "osnr")})
        ends.append((sv, g))
        out[f"{key}_both_lean{int(generic)}"] = env.occupancy()["lean_kernel"]
        env.close()
    a, b = recs
    out[key + "_both_same"] = all(np.array_equal(a[f], b[f]) for f in ("action", "accepted", "flags", "active"))
    out[key + "_both_osnr"] = np.stack([a["osnr"], b["osnr"]])
    out[key + "_both_accepted"] = int(a["accepted"].sum())
    out[key + "_both_moves_same"] = bool(np.array_equal(outs[0][:, :, EXACT], outs[1][:, :, EXACT]) and np.any(outs[0][:, :, 0] == 0))
    out[key + "_both_grid_ok"] = np.array(ok)
    rest = [f for f in FIELDS if f != "osnr"]
    out[key + "_both_end_same"] = all(np.array_equal(ends[0][1][r], ends[1][1][r])
                                      and all(np.array_equal(ends[0][0][r][f], ends[1][0][r][f]) for f in rest) for r in range(B))


WIDE = dict(BASE, num_spectrum_resources=320, capacity=256, load=150.0)


def wide_guard(out, B=8):
    """A move that would write a record wider than the lean kernels carry: a 400 Gb/s service of a format above QPSK whose
    capacity needs more than 32 slots under BPSK, sent to BPSK on its own route at the first start with room.  A lean
    environment answers "no spectrum" and stays byte for byte; a forced-generic one of the same state takes it.  Then the same
    service goes to QPSK (at most 18 slots) on both, and four launches of 50 steps follow on the lean and the generic kernel"""
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb = golden_tables("nsfnet")
    envs = []
    for generic in (False, True):
        if generic:
            os.environ["ONGYM_FORCE_GENERIC"] = "1"
        try:
            envs.append(BatchedQRMSAEnv(tables=tb, batch_size=B, **WIDE))
        finally:
            os.environ.pop("ONGYM_FORCE_GENERIC", None)
        envs[-1].seed(21)
        envs[-1].reset()
        envs[-1].step_policy(200, record=False)
    lean, gen = envs
    holder = lean.holder
    c = holder.struct
    S, se, routes = c.n_slots, np.asarray(holder.mod_se), route_of(tb)
    out["wide_lean"], out["wide_generic_lean"] = lean.occupancy()["lean_kernel"], gen.occupancy()["lean_kernel"]
    out["wide_limit"] = width_limit(holder, True)
    out["wide_start_same"] = all(np.array_equal(lean.services(r), gen.services(r)) for r in range(B))

    def first_room(row, n):                              # _get_candidates' first start: n free slots and the guard unless at S
        for a in range(S - n + 1):
            if np.all(row[a:a + n] == 1) and (a + n == S or row[a + n] == 1):
                return a
        return -1

    wide, narrow, nwide = np.zeros((B, 1, 2), np.int32), np.zeros((B, 1, 2), np.int32), np.zeros(B, np.int32)
    room = np.zeros(B, bool)
    for r in range(B):
        sv, g = lean.services(r), lean.grid(r)
        cap = sv["nslots"].astype(int) * se[sv["modulation"].astype(int)]
        i = int(np.argmax(np.where(sv["modulation"] >= 2, cap, 0)))
        p, slot, n = int(sv["path_id"][i]), int(sv["slot"][i]), int(sv["nslots"][i])
        nwide[r] = int(cap[i])                           # slots under BPSK (spectral efficiency 1)
        release(g, tb, p, slot, n)
        row = free_row(g, tb, p)
        room[r] = first_room(row, int(cap[i])) >= 0
        wide[r, 0] = i, encode(holder, routes[p][2], 0, max(first_room(row, int(cap[i])), 0))
        narrow[r, 0] = i, encode(holder, routes[p][2], 1, max(first_room(row, -(-int(cap[i]) // 2)), 0))
    out["wide_slots"], out["wide_room"] = nwide, room
    before = lean.save_state().tobytes()
    out["wide_lean_out"], out["wide_generic_out"] = lean.move_services(wide), gen.move_services(wide)
    out["wide_lean_untouched"] = lean.save_state().tobytes() == before
    out["wide_generic_slots"] = np.array([int(gen.services(r)["nslots"][wide[r, 0, 0]]) for r in range(B)])
    gen.load_state(np.frombuffer(before, np.uint8).copy())          # back to the common state
    out["narrow_lean_out"], out["narrow_generic_out"] = lean.move_services(narrow), gen.move_services(narrow)
    recs, ok = [], []
    for e in (lean, gen):
        runs = []
        for _ in range(4):
            runs.append(e.step_policy(50))
            sv, g = state_of(e, B)
            ok.append([np.array_equal(g[r], grid_of_records(tb, tb.n_links, S, svc_rows(sv[r]))) for r in range(B)])
        recs.append({f: np.concatenate([x[f] for x in runs]) for f in ("action", "accepted", "flags", "active", "osnr")})
    a, b = recs
    out["wide_run_same"] = all(np.array_equal(a[f], b[f]) for f in ("action", "accepted", "flags", "active"))
    out["wide_run_osnr"] = np.stack([a["osnr"], b["osnr"]])
    out["wide_run_grid_ok"] = np.array(ok)
    out["wide_end_same"] = all(np.array_equal(lean.grid(r), gen.grid(r)) and np.array_equal(lean.services(r)["slot"], gen.services(r)["slot"])
                               for r in range(B))
    out["wide_still_lean"] = lean.occupancy()["lean_kernel"]
    for e in envs:
        e.close()


LOW = dict(BASE, num_spectrum_resources=128, capacity=128, load=3.0)


def noops(out, B=8):
    """a replica with only failing moves and a replica without records are left byte for byte; one shared list equals the list
    tiled per replica"""
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb = golden_tables("nsfnet")
    envs = [BatchedQRMSAEnv(tables=tb, batch_size=B, **LOW) for _ in range(2)]
    for e in envs:
        e.seed(11)
        e.reset()
    env, other = envs
    holder = env.holder
    c = holder.struct
    reject = c.k_paths * c.n_mods * c.n_slots
    start = env.save_state().tobytes()
    empty = env.move_services(np.array([[TOP, FIRST_FIT], [0, FIRST_FIT], [0, 5]], np.int32))
    out["empty_active"], out["empty_out"] = env.stats()["active"], empty
    out["empty_blob_same"] = env.save_state().tobytes() == start
    for e in envs:
        e.step_policy(40, record=False)
    routes = route_of(tb)
    moves = np.zeros((B, 4, 2), np.int32)
    for r in range(B):
        s = env.services(r)
        moves[r] = [(len(s), FIRST_FIT), (len(s) + 1, 3), (-3, 4), (0, reject)]
        if len(s):                                                   # record 0 to where it is
            p, slot, m = int(s["path_id"][0]), int(s["slot"][0]), int(s["modulation"][0])
            moves[r, 1] = 0, encode(holder, routes[p][2], m, slot)
    before = [env.save_state([r]).tobytes() for r in range(B)]
    res = env.move_services(moves)
    out["fail_out"], out["fail_active"] = res, env.stats()["active"]
    out["fail_blob_same"] = np.array([env.save_state([r]).tobytes() == before[r] for r in range(B)])
    shared = np.array([[TOP, FIRST_FIT], [0, FIRST_FIT], [TOP, FIRST_FIT]], np.int32)
    a = env.move_services(shared)
    b = other.move_services(np.ascontiguousarray(np.tile(shared[None], (B, 1, 1))))
    out["shared_same"] = bool(np.array_equal(a, b, equal_nan=True) and env.save_state().tobytes() == other.save_state().tobytes())
    out["shared_moved"] = int(np.sum(a[:, :, 0] == 0))
    for e in envs:
        e.close()


def state_calls(out, key="nsfnet"):
    """save / load / fork after a move"""
    tb, kw, B, _, _ = case_config(key)
    env, second = make_env(key), make_env(key)
    tb, kw, holder, ors = drive(key, env, oracles=False)
    second.seed(SEED)
    second.reset()
    svcs, grids = state_of(env, B)
    res = env.move_services(all_moves(ors, tb, holder, svcs, grids, False))
    out["state_moved"] = int(np.sum(res[:, :, 0] == 0))
    blob = env.save_state()
    want = env.step_policy(100)
    second.load_state(blob)
    out["state_records_same"] = record_bytes(second.step_policy(100)) == record_bytes(want)
    out["state_same"] = all(np.array_equal(second.services(r), env.services(r)) and np.array_equal(second.grid(r), env.grid(r))
                            for r in range(B))
    env.load_state(blob)
    one = env.save_state([1]).tobytes()
    src = np.arange(B, dtype=np.int32)
    src[3] = 0
    env.fork(src)
    out["fork_copies"] = bool(np.array_equal(env.services(3), env.services(0)) and np.array_equal(env.grid(3), env.grid(0))
                              and env.save_state([1]).tobytes() == one
                              and env.save_state([3]).tobytes() != one)
    env.close()
    second.close()


def after_cut(out, key="nsfnet"):
    """moves on a degraded network: nothing lands on a failed link, and the failed set stays"""
    tb, kw, B, _, _ = case_config(key)
    env = make_env(key)
    tb, kw, holder, ors = drive(key, env, oracles=False)
    c = holder.struct
    lists = [replica_links(tb, env.services(r), r) for r in range(B)]
    env.cut_links(lists)
    failed = env.failed_links()
    svcs, grids = state_of(env, B)
    moves = all_moves(ors, tb, holder, svcs, grids, False)
    res = env.move_services(moves)
    svcs1, grid1 = state_of(env, B)
    fl = [links_of(failed[r]) for r in range(B)]
    out["cut_failed_same"] = bool(np.array_equal(env.failed_links(), failed) and np.any(failed))
    out["cut_cross"] = sum(crossing(tb, svc_rows(svcs1[r]), fl[r]) for r in range(B))
    out["cut_grid_ok"] = np.array([np.array_equal(grid1[r], grid_of_records(tb, tb.n_links, c.n_slots, svc_rows(svcs1[r]), fl[r]))
                                   for r in range(B)])
    out["cut_moved"] = int(np.sum(res[:, :, 0] == 0))
    ok = True
    for r, o in enumerate(ors):
        want, post, grid = expected_moves(o, tb, holder, replica_margin(kw, r), svcs[r], grids[r], moves[r])
        ok &= bool(np.array_equal(res[r][:, EXACT], want[:, EXACT]) and np.array_equal(grid1[r], grid)
                   and np.array_equal(svc_rows(svcs1[r]), post))
    out["cut_restated"] = ok
    env.close()


NSF = dict(BASE, num_spectrum_resources=128, capacity=192, load=120.0)


def device_io(out, B=32):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    tb = golden_tables("nsfnet")
    host = BatchedQRMSAEnv(tables=tb, batch_size=B, **NSF)
    dev = BatchedQRMSAEnv(tables=tb, batch_size=B, io_device=True, **NSF)
    host.seed(5)
    host.reset()
    host.step_policy(220, record=False)
    rng = np.random.default_rng(MOVE_SEED)
    c = host.holder.struct
    moves = np.zeros((B, 5, 2), np.int32)
    moves[:, :, 0], moves[:, :, 1] = TOP, FIRST_FIT
    moves[:, 1, 0] = rng.integers(0, 20, B)
    moves[:, 3, 0], moves[:, 3, 1] = rng.integers(0, 20, B), rng.integers(0, c.k_paths * c.n_mods * c.n_slots, B)
    m_t = torch.from_numpy(moves).cuda()
    t = torch.full((B, 5, 6), 7.0, dtype=torch.float64, device="cuda")
    try:
        dev.move_services(m_t, out=t)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    want = host.move_services(moves)
    want_blob = host.save_state()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        dev.seed(5)
        dev.reset()
        dev.step_policy(220, record=False)
        r = dev.move_services(m_t, out=t)
        blob = dev.save_state()
        stream.synchronize()
        out["dev_same"] = bool(r is t and np.array_equal(t.cpu().numpy(), want, equal_nan=True))
        out["dev_moved"] = int(np.sum(want[:, :, 0] == 0))
        out["dev_state_same"] = blob.cpu().numpy().tobytes() == want_blob.tobytes()
        bad = []
        for call in (lambda: dev.move_services(m_t.long(), out=t),                  # dtype
                     lambda: dev.move_services(torch.from_numpy(moves), out=t),     # a host tensor
                     lambda: dev.move_services(moves, out=t),                       # not a tensor
                     lambda: dev.move_services(m_t),                                # no out
                     lambda: dev.move_services(m_t[:B - 1], out=t),                 # B - 1 replicas
                     lambda: dev.move_services(m_t[0], out=t),                      # a shared list
                     lambda: dev.move_services(m_t, out=t.float()),
                     lambda: dev.defragment(3)):
            try:
                call()
                bad.append(False)
            except ValueError:
                bad.append(True)
        out["dev_refusals"] = np.array(bad)
        dev.set_stream(None)
    host.close()
    dev.close()


def refusals(out):
    from dataclasses import replace
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    small = dict(NSF, capacity=128)
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, **small)
    env.seed(1)
    env.reset()
    moves, res = np.full((4, 2, 2), -1, np.int32), np.zeros((4, 2, 6))
    rc, msg = {}, {}

    def call(name, e, *a):
        rc[name] = e.lib.ongym_move_services(e._h, *a)
        msg[name] = e.lib.ongym_last_error(e._h).decode() if rc[name] else ""

    call("null_moves", env, 2, None, 0, res.ctypes.data)
    call("null_out", env, 2, moves.ctypes.data, 0, None)
    call("zero", env, 0, moves.ctypes.data, 0, res.ctypes.data)
    call("flags", env, 2, moves.ctypes.data, 2, res.ctypes.data)
    call("ok", env, 2, moves.ctypes.data, 0, res.ctypes.data)
    call("ok_own", env, 2, moves.ctypes.data, nat.MOVE_OWN_ROUTE, res.ctypes.data)
    env.close()
    narrow = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, modulations_to_consider=3, **small)
    call("window", narrow, 2, moves.ctypes.data, 0, res.ctypes.data)
    narrow.close()
    tb = ring_tables()                                               # one pair lists its two routes in the other order
    pp = tb.pair_paths.copy()
    pp[1, 0] = pp[1, 0][::-1]
    odd = BatchedQRMSAEnv(tables=replace(tb, pair_paths=pp), batch_size=4, **dict(BASE, num_spectrum_resources=40, capacity=64, load=10.0))
    call("pairs", odd, 2, moves.ctypes.data, 0, res.ctypes.data)
    odd.close()
    for k, v in rc.items():
        out["refuse_rc_" + k], out["refuse_msg_" + k] = v, msg[k]


def main():
    out = {}
    refusals(out)
    noops(out)
    state_calls(out)
    after_cut(out)
    device_io(out)
    wide_guard(out)
    for key in BOTH:
        both_kernels(out, key)
    for key in CASES:
        gpu_case(out, key)
        print(key, "done", flush=True)
    np.savez(sys.argv[1], **out)
    print("move child ok")


if __name__ == "__main__":
    main()
