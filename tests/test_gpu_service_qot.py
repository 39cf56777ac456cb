"""Current QoT of every running lightpath (ongym_service_qot through BatchedQRMSAEnv.service_qot).  Every GPU computation runs in
ONE fresh child process (tests/service_qot_child.py); the tests assert on the .npz it writes.

The restatements live here: the GN value of a running service from the oracle's literal GN (orc_gn_lists) on per-link
interferer lists built from the oracle's running services, itself (and, with id tracking, its namesakes, quirk Q12) left out;
and the per-replica and per-link aggregates of include/ongym.h from svc_out, the service records and the path tables.
tests/test_service_qot_host.py pins the first one to the oracle's own step records."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GN_RTOL = 1e-9
# "<traffic>_<topology>_<S>": the configurations compared with the oracle (service_qot_child.case_config builds them)
CASES = ("ff_nsfnet_320", "lb_cost239_160", "wide_nobeleu_320", "ff_germany50_100", "ff_nsfnet_768", "hsnr_nsfnet_100",
         "lf_nsfnet_320", "alpha_nsfnet_320", "cont_cost239_320", "trace_nsfnet_160", "defrag_nsfnet_320", "disr_nsfnet_320",
         "ids_nsfnet_320", "random_cost239_100")


# ---- the restatements -------------------------------------------------------------------------------------------------
def insertion_order(svcs):
    """the running services sorted by release time (the reference appends to a link's running list when it provisions; with
    one holding time for every request this is the order of the links' lists)"""
    return np.argsort(svcs["release_time"], kind="stable")


def interferer_lists(tables, mod_se, svcs, y, ids=None):
    """(counts per hop, flat (slot, n, se) triples) of running service y's path: on each of its links the other running services
    that cross it, in the order of svcs; y itself (and with ids, every service with y's id) left out"""
    path_links, path_hops = tables.path_links, tables.path_hops
    keep = np.ones(len(svcs), bool)
    keep[y] = False
    if ids is not None:
        keep &= ids != ids[y]
    paths = svcs["path_id"].astype(np.int64)
    counts, intf = [], []
    for l in path_links[paths[y], :path_hops[paths[y]]]:
        on = keep & np.any(path_links[paths] == l, axis=1)
        z = np.flatnonzero(on)
        counts.append(len(z))
        intf.append(np.stack([svcs["slot"][z], svcs["nslots"][z], np.asarray(mod_se)[svcs["modulation"][z]]], axis=1))
    return np.array(counts, np.int32), np.concatenate(intf).astype(np.int16) if intf else np.zeros((0, 3), np.int16)


def restate_gn(o, tables, mod_se, svcs, ids=None):
    """GSNR, ASE, NLI (dB) of every running service of svcs against the others, by the oracle's literal GN (orc_gn_lists, at
    the oracle's launch power)"""
    out = np.zeros((len(svcs), 3))
    for y in range(len(svcs)):
        counts, intf = interferer_lists(tables, mod_se, svcs, y, ids)
        out[y] = o.gn_lists(int(svcs["path_id"][y]), int(svcs["slot"][y]), int(svcs["nslots"][y]), counts, intf)
    return out


def restate_aggregates(svc, services, path_links, path_hops, mod_thr, margin, E):
    """(replica_out row, link_out rows) of one replica from its svc_out rows (record order), its records and the path tables,
    the "below" counts decided on the dB values"""
    n = len(services)
    g = svc[:n]
    thr = np.asarray(mod_thr)[services["modulation"]]
    below0 = g[:, 0] < thr
    belowm = g[:, 0] < thr + margin
    rep = np.array([n, below0.sum(), belowm.sum(), np.nan, np.nan, -1.0])
    if n:
        i = int(np.argmin(g[:, 3]))                                 # the first (lowest) index of the minimum
        rep[3:] = g[i, 3], np.mean(g[:, 0]), i
    link = np.zeros((E, 3), np.float64)
    link[:, 1] = np.nan
    for k in range(n):
        p = int(services["path_id"][k])
        for l in path_links[p, :path_hops[p]]:
            link[l, 0] += 1
            link[l, 1] = g[k, 3] if np.isnan(link[l, 1]) else min(link[l, 1], g[k, 3])
            link[l, 2] += below0[k]
    return rep, link


def match(dev_services, ora_services):
    """index into ora_services of every device record, matched by (path, slot)"""
    key = {(int(p), int(s)): i for i, (p, s) in enumerate(zip(ora_services["path_id"], ora_services["slot"]))}
    assert len(key) == len(ora_services)
    return np.array([key[(int(p), int(s))] for p, s in zip(dev_services["path_id"], dev_services["slot"])], np.int64)


# ---- the child's results ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("service_qot") / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "service_qot_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=1800)
    assert run.returncode == 0 and "service qot child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def replicas_of(res, key):
    return [int(r) for r in res[key + "_replicas"]]


def check_against_oracle(res, key):
    """svc_out of every sampled replica against the oracle restatement; the count columns of replica_out against the oracle's
    dB values (returns the number of services compared)"""
    n_checked = 0
    for r in replicas_of(res, key):
        k = f"{key}_r{r}"
        svc, dsvc, osvc, want = res[k + "_svc"], res[k + "_dsvc"], res[k + "_osvc"], res[k + "_want"]
        n = len(dsvc)
        assert len(osvc) == n, k
        assert np.all(np.isnan(svc[n:])), k
        j = match(dsvc, osvc)
        np.testing.assert_allclose(svc[:n, :3], want[j], rtol=GN_RTOL, atol=0, err_msg=k)
        thr = res[key + "_thr"][dsvc["modulation"]]
        np.testing.assert_allclose(svc[:n, 3], want[j, 0] - thr, rtol=GN_RTOL, atol=1e-12, err_msg=k)
        rep = res[k + "_rep"]
        assert rep[0] == n, k
        assert rep[1] == int(np.sum(want[:, 0] < res[key + "_thr"][osvc["modulation"]])), k
        assert rep[2] == int(np.sum(want[:, 0] < res[key + "_thr"][osvc["modulation"]] + float(res[k + "_margin"]))), k
        n_checked += n
    return n_checked


@pytest.mark.parametrize("key", CASES)
def test_service_gsnr_equals_the_oracle_literal_gn(res, key):
    assert check_against_oracle(res, key) > 0


def test_the_cases_exercise_what_they_claim(res):
    assert res["wide_nobeleu_320_wide"] > 0                      # services wider than 32 slots among the running ones
    assert res["trace_nsfnet_160_above_tab"] > 0                 # interferers beyond the pair table (the asinh path)
    assert res["ids_nsfnet_320_dup_ids"] > 0                     # running namesakes after the counters-only reset
    assert res["defrag_nsfnet_320_moves"] > 0
    assert res["disr_nsfnet_320_disrupted"] > 0
    assert not res["alpha_nsfnet_320_uniform"]
    assert res["any_below_margin"] > 0


@pytest.mark.parametrize("key", CASES + ("scale_65536", "scale_odd"))
def test_aggregates_equal_the_restatement(res, key):
    for r in replicas_of(res, key):
        k = f"{key}_r{r}"
        svc, dsvc = res[k + "_svc"], res[k + "_dsvc"]
        rep_w, link_w = restate_aggregates(svc, dsvc, res[key + "_path_links"], res[key + "_path_hops"], res[key + "_thr"],
                                           float(res[k + "_margin"]), res[k + "_link"].shape[0])
        rep, link = res[k + "_rep"], res[k + "_link"]
        assert np.array_equal(rep[[0, 1, 2, 5]], rep_w[[0, 1, 2, 5]]), (k, rep, rep_w)
        np.testing.assert_allclose(rep[3:5], rep_w[3:5], rtol=1e-12, err_msg=k)
        assert np.array_equal(link[:, [0, 2]], link_w[:, [0, 2]].astype(np.float32)), k
        assert np.array_equal(link[:, 1], link_w[:, 1].astype(np.float32), equal_nan=True), k


def test_below_minimum_services_are_in_the_disrupted_list(res):
    checks = 0
    for key in [k[:-len("_belowflag")] for k in res if k.endswith("_belowflag")]:
        below, flagged = res[key + "_belowflag"], res[key + "_flagged"]
        assert not np.any(below & ~flagged), key
        checks += int(below.sum())
    assert checks > 0                                            # some services are below minimum_osnr at the check points


def test_first_service_equals_its_step_record(res):
    got, want = res["fresh_svc"], res["fresh_rec"]
    assert len(got) >= 8
    np.testing.assert_allclose(got, want, rtol=GN_RTOL, atol=0)


def test_service_qot_is_read_only(res):
    assert res["ro_blob_same"] and res["ro_stats_same"] and res["ro_traj_same"] and res["ro_fork_same"]


@pytest.mark.parametrize("key", ["scale_65536", "scale_odd"])
def test_launch_scale_sampled_replicas_equal_the_oracle(res, key):
    assert check_against_oracle(res, key) > 0
    assert int(res[key + "_batch"]) in (65536, 1237)


def test_device_io_on_the_current_stream_equals_the_host_path(res):
    assert res["dev_same"] and res["dev_partial_same"] and res["dev_stream_refused"]


def test_refusals(res):
    assert int(res["refuse_null_rc"]) == -1 and "null" in str(res["refuse_null_msg"])
    for k in ("refuse_all_none", "refuse_dtype", "refuse_shape", "refuse_host_tensor", "refuse_out_on_host_env"):
        assert res[k], k
