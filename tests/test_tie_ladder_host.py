"""The near-tie ladders of tests/tie_ladder.py, on the CPU oracle alone: the conditions without which the GPU test
(tests/test_gpu_tie_ladder.py) would pass emptily.  For both cases, all three launch powers and both ladders:

  * every request is accepted;
  * every evaluated candidate is at least 2 dB from its admission threshold, so no admission decision moves along a ladder;
  * every non-laddered (odd, 0-based) decision has |delta| >= 1e-3 dB;
  * on every rung with |eps| >= 3e-11 every laddered decision is exact (|delta| >= 1e-11 dB); the rungs that may hold an exempt
    decision are the 7 of 21 with |eps| <= 2e-12;
  * on every exact laddered decision the oracle takes the route the sign of eps makes better, and where all of a run's laddered
    decisions are exact the whole route sequence alternates from that start;
  * at eps = 0 route 0 leads every laddered decision;
  * both routes and at least two formats appear among the winners of the +2 dBm replica.

Each ladder prints the range of every measured quantity.
"""
import numpy as np
import pytest

import tie_ladder as tl

LADDERS = [(c, l) for c in tl.CASES for l in tl.LADDERS]


def test_layout():
    assert len(tl.EPS) == 21 and tl.EPS[0] == 0.0 and len(set(tl.EPS)) == 21
    assert sum(abs(e) <= tl.MAY_BE_EXEMPT for e in tl.EPS) == 7
    assert min(abs(e) for e in tl.EPS if abs(e) > tl.MAY_BE_EXEMPT) == 3e-11
    tb = tl.base_tables()
    assert (tb.n_nodes, tb.n_links, tb.k_paths, tb.n_paths) == (4, 4, 2, 12)
    p0, p1 = (int(x) for x in tb.pair_paths[tl.SRC, tl.DST])
    assert tb.path_links[p0, :2].tolist() == [0, 1] and tb.path_links[p1, :2].tolist() == [2, 3]
    assert len(set(tb.link_nf.tolist())) == 1 and len(set(tb.link_alpha.tolist())) == 1
    for name, link in tl.LADDERS.items():
        up = tl.rung_tables(link, 1e-15)
        assert up.link_nf[link] > tb.link_nf[link] and np.array_equal(np.delete(up.link_nf, link), np.delete(tb.link_nf, link))
        assert np.array_equal(up.link_alpha, tb.link_alpha)
    assert [t for t in range(5) if tl.laddered(t)] == [0, 2, 4]


def test_topology_file_gives_the_rungs_tables(tmp_path):
    """The graph the compatibility view gets (rung_topology) compiles to the builder's tables, bit for bit."""
    from optical_networking_gym._tables import StaticTables
    for link, eps in ((3, 0.0), (3, -3e-11), (1, 1e-15)):
        got, want = StaticTables.from_topology(tl.rung_topology(tmp_path, link, eps)), tl.rung_tables(link, eps)
        assert (got.n_nodes, got.n_links, got.n_paths, got.k_paths, got.max_hops) == (4, 4, 12, 2, 3)
        for f in ("pair_paths", "path_hops", "path_links", "path_length", "link_nodes", "link_length", "link_nspans", "link_span_km",
                  "link_alpha", "link_nf"):
            assert np.array_equal(getattr(got, f), getattr(want, f)), (link, eps, f, getattr(got, f), getattr(want, f))


@pytest.mark.parametrize("case,ladder", LADDERS)
def test_ladder_is_not_vacuous(case, ladder):
    rungs = tl.find_ladder(case, ladder)
    n = tl.CASES[case]["n"]
    lad = np.array([tl.laddered(t) for t in range(n)])
    assert lad.sum() == (n + 1) // 2 and lad[0] and lad[-1]
    dist = min(float(r.dist.min()) for r in rungs)
    even = min(float(np.abs(r.delta[~lad]).min()) for r in rungs)
    ratio = {b: [] for b in range(tl.B)}
    may_be_exempt = 0
    for r in rungs:
        ctx = (case, ladder, r.eps)
        assert r.recs["accepted"].all(), ctx
        assert np.isfinite(r.delta).all(), ctx                  # both routes hold a passing candidate at every decision
        ex = r.exact()
        if abs(r.eps) > tl.MAY_BE_EXEMPT:
            assert ex[lad].all(), (ctx, np.abs(r.delta[lad]).min())
        else:
            may_be_exempt += 1
        want = tl.better_route(ladder, r.eps)
        for b in range(tl.B):
            routes = r.recs["route"][:, b]
            # the restated walk is the oracle's: its winner is the winner of the better route, or route 0's on an exact tie
            for t in range(n):
                k = int(routes[t])
                assert k == (1 if r.delta[t, b] > 0 else 0), (ctx, b, t, r.delta[t, b])
                w = r.best[t, b, k]
                for f in ("modulation", "slot", "nslots"):
                    assert r.recs[f][t, b] == w[f], (ctx, b, t, f)
                assert r.recs["osnr"][t, b] == w["osnr"], (ctx, b, t)
            assert np.all(routes[lad][ex[lad, b]] == want), (ctx, b, routes.tolist())
            if ex[lad, b].all():
                assert routes.tolist() == [want if tl.laddered(t) else 1 - want for t in range(n)], (ctx, b, routes.tolist())
            if r.eps == 0.0:
                assert np.all(routes[lad] == 0) and np.all(r.delta[lad, b] == 0.0), (ctx, b)
            else:
                assert np.all(np.sign(r.delta[lad, b][ex[lad, b]]) == (1 if want == 1 else -1)), (ctx, b)
                ratio[b] += (np.abs(r.delta[lad, b]) / abs(r.eps)).tolist() if abs(r.eps) >= 3e-11 else []
        hot = r.recs[:, tl.B - 1]
        assert set(hot["route"].tolist()) == {0, 1} and len(set(hot["modulation"].tolist())) >= 2, (ctx, hot["modulation"].tolist())
    assert may_be_exempt == 7
    first_exact = [r for r in rungs if abs(r.eps) == 3e-11]
    least = min(float(np.abs(r.delta[lad]).min()) for r in first_exact)
    print(f"{case} {ladder}: least distance of a candidate from its threshold {dist:.3f} dB; least |delta| of a non-laddered decision "
          f"{even:.3e} dB; least |delta| of a laddered decision at |eps| = 3e-11 {least:.3e} dB; |delta| / |eps| per replica "
          + ", ".join(f"{min(v):.2f}..{max(v):.2f}" for v in ratio.values()))
    assert dist >= 2.0
    assert even >= 1e-3
    assert least >= tl.ZONE_DB
