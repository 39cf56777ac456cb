"""The margin ladders of tests/threshold_ladder.py, on the CPU oracle alone: the conditions without which the GPU tests
(tests/test_gpu_threshold_ladder.py) would pass vacuously.  For every case of the table:

  * the 21 rungs' histories are bit-identical before t*;
  * the oracle's decision at t* differs between the lowest and the highest rung and changes exactly once along T_r, where
    g >= T_r stops holding;
  * no other accepted decision of any rung's run (t* + 40 diverged steps) lies within 1e-6 dB of its threshold, so the ladder's
    8.6e-8 dB span moves nothing else;
  * t* has at least 40 running services, except in the empty-network case.

Each case prints t*, g, the format and the next-closest distance.  The ladders on a state reached under the base margin
(max_modulation_idx, lowest fragmentation, service_qot, action_impact) are held the same way: the oracle's answer changes exactly
where g >= T_r stops holding, and is the ends' answer as far as 1e-6 dB out.
"""
import numpy as np
import pytest

import threshold_ladder as tl
from common import record_bytes
from optical_networking_gym import _native as nat


@pytest.mark.parametrize("name", list(tl.CASES))
def test_ladder_is_not_vacuous(name):
    case = tl.find_case(name)              # refuses a case whose history or decisions at t* are not what the recipe says
    t, recs = case.t, case.recs
    assert recs.shape == (case.steps, tl.B) and case.steps <= 340
    for r in range(tl.B):
        assert record_bytes(recs[:t, r]) == record_bytes(case.base[:t]), (name, r)
    acc = tl.accepted_m(case, recs[t])
    assert acc[0] and not acc[-1]
    k = tl.one_change(acc)
    assert k > 0, (name, acc)
    assert np.array_equal(acc, case.g >= case.T)
    assert np.all(np.diff(case.T) >= 0) and case.T[-1] - case.T[0] < 8.7e-8
    # the exempt zone is the ladder's, not the test's: the +-1e-11 rungs and everything farther out are held to the oracle
    ex = tl.exact_rungs(case)
    assert ex[0] and ex[-1] and int((~ex).sum()) <= 13 and k - 1 in np.flatnonzero(~ex) and k in np.flatnonzero(~ex)
    nearest = np.inf
    for r in range(tl.B):
        d = np.abs(tl.distances(recs[:, r], case.thr, case.margins[r]))
        d[t] = np.inf
        nearest = min(nearest, float(d.min()))
    base_d = np.abs(tl.distances(case.base, case.thr, case.cfg["m0"]))
    base_d[t] = np.inf
    print(f"{name}: t* {t} g {case.g!r} format {case.m} candidate (path, slot, n) {case.cand} distance at base margin {case.d:.3e} dB "
          f"next-closest accepted decision {float(base_d.min()):.3e} dB (on the rungs {nearest:.3e} dB) "
          f"running services {int(case.base['active'][t])} accepting rungs {int(acc.sum())}")
    assert nearest > tl.QUIET_DB, (name, nearest)
    if not case.cfg.get("empty"):
        assert int(case.base["active"][t]) >= 40, (name, int(case.base["active"][t]))
    else:
        assert t == 0 and case.m == len(case.thr) - 1 and case.cand[1] == 0 and case.route == 0
        assert case.g - case.thr[case.m] >= 0


def test_ladder_layout():
    g, thr = 13.251837219490534, 13.24
    margins, T = tl.ladder(g, thr)
    assert len(margins) == tl.B == 21 and np.array_equal(T, thr + margins)
    off = np.abs(T - g)
    assert (off < tl.ZONE_DB).sum() <= 13
    assert (off < tl.HALF_BAND_DB).sum() >= 15          # equality, ulps, deep inside the band and near its edges (2e-9)
    assert (off > 2 * tl.HALF_BAND_DB).sum() == 4       # 1e-8 just outside, 4.3e-8 ten band widths away
    assert abs(tl.HALF_BAND_DB - 4.34e-9) < 1e-11


def test_every_policy_has_a_ladder_on_which_its_answer_changes():
    """The pending states of POLICY_CASES, policy by policy: does the oracle's answer differ between the ladder's ends?"""
    seen = set()
    for name in tl.POLICY_CASES:
        ch = tl.changing_policies(name)
        print(f"{name}: policies whose answer changes along the ladder: {list(ch)}")
        assert ch, name                     # a case that cannot fail is not kept
        seen |= set(ch)
    assert seen == set(range(12)) - set(tl.NO_CHANGING_LADDER), sorted(seen)


def test_max_modulation_idx_ladder_is_not_vacuous():
    case = tl.mmi_case()
    got = [tl.oracle_mmi(case, o)[0] for o in case.oracles]
    k = tl.one_change([x == got[0] for x in got])
    print(f"max_modulation_idx: t {case.t} g {case.g!r} format {case.m} candidate {case.cand} along T_r {got}")
    assert k > 0 and got[0] == case.m and all(x == got[-1] for x in got[k:]) and got[-1] < case.m
    assert [x == got[0] for x in got] == (case.g >= case.T).tolist()
    assert len(case.oracles[0].services()) >= 40
    # nothing else of the scan lies within 1e-6 dB of the ladder: the ends' answers hold that far out
    o = case.oracles[0]
    for off, want in ((-tl.QUIET_DB, got[0]), (tl.QUIET_DB, got[-1])):
        o.set_margin(case.g - case.thr[case.m] + off)
        assert tl.oracle_mmi(case, o)[0] == want
    o.set_margin(case.margins[0])


def test_running_lightpath_ladders_are_not_vacuous():
    case = tl.service_case()
    thr_s = case.thr[case.svcs["modulation"]]
    below = [int(np.sum(case.want[:, 0] < thr_s + m)) for m in case.margins]
    others = np.delete(case.d, case.y)
    print(f"service_qot: t {case.t} running {len(case.svcs)} lowest GSNR - thr {case.d[case.y]:.6f} dB (g {case.g!r}) next {others.min():.6f} dB "
          f"below margin along T_r {below}")
    assert len(case.svcs) >= 40 and others.min() - case.d[case.y] > tl.QUIET_DB
    assert tl.one_change([b == below[0] for b in below]) > 0 and below[-1] == below[0] + 1
    assert [b == below[0] for b in below] == (case.g >= case.T).tolist()

    case = tl.impact_case()
    p, i = case.pairs, case.i
    M = case.g - p[i, 4]
    near_after = np.abs(np.delete(p[:, 3] - p[:, 4], i) - M)
    near_before = np.abs(p[:, 2] - p[:, 4] - M)
    print(f"action_impact: action {case.action} victims {len(p)} lowest margin after {M:.6f} dB (g {case.g!r}, before {p[i, 2]!r}) "
          f"nearest other after {near_after.min() if len(near_after) else np.inf:.3e} dB nearest before {near_before.min():.3e} dB")
    assert (len(near_after) == 0 or near_after.min() > tl.QUIET_DB) and near_before.min() > tl.QUIET_DB
    newly = [int(np.sum((p[:, 3] < p[:, 4] + m) & ~(p[:, 2] < p[:, 4] + m))) for m in case.margins]
    assert [n == newly[0] for n in newly] == (case.g >= case.T).tolist() and newly[-1] == newly[0] + 1


def test_lowest_fragmentation_ladder_is_not_vacuous():
    """Policy 10 has no first-fit ladder on which its answer changes (tl.NO_CHANGING_LADDER); this one is built on its own choice."""
    case = tl.policy_state_case(nat.POLICY_LOWEST_FRAGMENTATION)
    got = [o.policy(case.policy) for o in case.oracles]
    print(f"lowest fragmentation: t {case.t} g {case.g!r} format {case.m} answers along T_r {[x[0] for x in got]}")
    assert got[0] == case.first and got[-1] != case.first
    assert [x == got[0] for x in got] == (case.g >= case.T).tolist() and all(x == got[-1] for x in got if x != got[0])
    o = case.oracles[0]
    for off, want in ((-tl.QUIET_DB, got[0]), (tl.QUIET_DB, got[-1])):
        o.set_margin(case.g - case.thr[case.m] + off)
        assert o.policy(case.policy) == want
    o.set_margin(case.margins[0])
