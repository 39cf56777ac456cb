"""Child process of tests/test_gpu_action_impact.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP
runtime and this library's must start together), saved to an .npz that the tests assert on.

    python tests/action_impact_child.py OUT.npz

Covers ongym_action_impact (BatchedQRMSAEnv.action_impact): device replicas and CPU oracles driven with the same traffic on
eight configurations with the oracle restatement of every (action, victim) pair, with and without svc_in; forked steps of the
device itself as a second witness; the read-only property, fresh replicas, device I/O on torch's stream, the compat
environment, the library's refusals and QRMSABlockVecEnv(protect_running=True).
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402

from common import golden_tables, record_bytes  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv  # noqa: E402
from optical_networking_gym.envs.block_vec_env import QRMSABlockVecEnv  # noqa: E402
from optical_networking_gym.envs.qrmsa import QRMSAEnv  # noqa: E402
from service_qot_child import BASE, case_config  # noqa: E402
from test_gpu_action_impact import (BAND, CASES, COLS, J, REPLICAS, SEED, candidate_actions, drive, oracle_block_row,  # noqa: E402
                                    restate_replica)
from test_gpu_service_qot import insertion_order, match  # noqa: E402


def oracle_services(env, r, o):
    """the oracle's running services in the links' list order, completed by the records the counters-only reset dropped from
    its departure heap (service_qot_child.save_replica)"""
    dsvc, osvc = env.services(r), o.services()
    if len(osvc) < len(dsvc):
        assert np.array_equal(env.grid(r), o.grid())
        have = {(int(p), int(s)) for p, s in zip(osvc["path_id"], osvc["slot"])}
        kept = np.array([(int(p), int(s)) not in have for p, s in zip(dsvc["path_id"], dsvc["slot"])], bool)
        assert np.all(np.isinf(dsvc["release_time"][kept]))
        extra = dsvc[kept].copy()
        extra["service_id"], extra["reserved"] = -1, 0
        osvc = np.concatenate([extra, osvc])
    return dsvc, osvc[insertion_order(osvc)]


def oracle_case(out, key):
    B = REPLICAS.get(key, 3)
    tb, kw, how, _ = case_config(key)
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    tb, kw, holder, oracles = drive(key, B, SEED, env)
    _, _, amap = env.observe_blocks(J)
    actions = np.stack([candidate_actions(o, tb, holder, amap[r]) for r, o in enumerate(oracles)])
    impact = env.action_impact(actions)
    svc = env.service_qot()[0]
    impact_svc = env.action_impact(actions, svc=svc)
    st = env.stats()
    wide = namesakes = 0
    tab_nmax = int(np.ceil(100 / (min(holder.mod_se) * 12.5)))
    for r, o in enumerate(oracles):
        k = f"{key}_r{r}"
        dsvc, osvc = oracle_services(env, r, o)
        j = match(dsvc, osvc)                                        # oracle index of every device record
        record = np.empty(len(osvc), np.int64)
        record[j] = np.arange(len(dsvc))
        ids = cur_id = None
        if how == "ids":
            ids = np.empty(len(osvc), np.int64)
            ids[j] = dsvc["service_id"]
            cur_id = int(st[r]["episode_services_processed"]) - 1    # Service.service_id of the current request
            namesakes += int(np.sum(ids == cur_id))
        status, pairs = restate_replica(o, tb, holder, osvc, actions[r], ids, cur_id)
        out[k + "_actions"], out[k + "_impact"], out[k + "_impact_svc"] = actions[r], impact[r], impact_svc[r]
        out[k + "_status"], out[k + "_pairs"], out[k + "_record"] = status, pairs, record
        out[k + "_oracle_row"] = oracle_block_row(o, tb, holder)
        q = o.request()
        for a in np.flatnonzero(status == 0):
            _, m, _ = o.decode(int(actions[r, a]))
            wide += o.number_slots(float(q["bit_rate"]), m) > tab_nmax
    out[key + "_B"], out[key + "_margin"] = B, kw["margin"]
    out[key + "_wide_candidates"], out[key + "_namesakes"] = wide, namesakes
    out[key + "_uniform"] = bool(np.all(tb.link_alpha == tb.link_alpha[0]))
    out[key + "_links"] = tb.n_links
    env.close()


def forks(out, key="disr_nsfnet_320", nsrc=12, seed=5, steps=400):
    """nsrc source replicas, each forked over the K*J block actions of its row; the forks step, service_qot() gives every
    old record's new margin"""
    tb, kw, _, _ = case_config(key)
    K = nat.ConfigHolder(tb, batch=1, **kw).struct.k_paths
    A = K * J
    B = nsrc * (A + 1)
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    env.seed(seed)
    env.reset()
    env.step_policy(steps, record=False)
    _, _, amap = env.observe_blocks(J)
    amap = np.ascontiguousarray(amap[:, :A])
    impact = env.action_impact(amap)
    svc0 = env.service_qot()[0]
    thr, margin = np.asarray(env.holder.mod_thr), kw["margin"]
    old = [env.services(s) for s in range(nsrc)]
    src = np.full(B, -1, np.int32)
    acts = np.full(B, env.reject_action, np.int32)
    for s in range(nsrc):
        lo = nsrc + s * A
        src[lo:lo + A] = s
        acts[lo:lo + A] = amap[s]
    env.fork(src)
    rec = env.step(acts)
    svc1 = env.service_qot()[0]
    on_link = np.zeros((tb.n_paths if hasattr(tb, "n_paths") else len(tb.path_hops), tb.n_links), bool)
    for p in range(len(tb.path_hops)):
        on_link[p, tb.path_links[p, :tb.path_hops[p]]] = True
    got, want, band = [], [], []
    accepted = pairs = 0
    for s in range(nsrc):
        for a in range(A):
            f = nsrc + s * A + a
            if not rec["accepted"][f]:
                continue
            accepted += 1
            new = env.services(f)
            key_new = {(int(p), int(sl), int(n)): i for i, (p, sl, n) in enumerate(zip(new["path_id"], new["slot"], new["nslots"]))}
            if len(new) != len(old[s]) + 1 or any((int(p), int(sl), int(n)) not in key_new
                                                 for p, sl, n in zip(old[s]["path_id"], old[s]["slot"], old[s]["nslots"])):
                continue                                            # the step released something
            idx = np.array([key_new[(int(p), int(sl), int(n))] for p, sl, n in zip(old[s]["path_id"], old[s]["slot"], old[s]["nslots"])])
            cand = new[[i for i in range(len(new)) if i not in set(idx.tolist())][0]]
            v = np.flatnonzero(np.any(on_link[old[s]["path_id"]] & on_link[int(cand["path_id"])], axis=1))
            t = thr[old[s]["modulation"][v]]
            before, after = svc0[s, v, 0], svc1[f, idx[v], 0]
            row = np.full(8, np.nan)
            row[:5], row[7] = 0, -1
            row[1] = len(v)
            if len(v):
                mg = after - t
                row[2] = np.sum(after < t)
                row[3] = np.sum((after < t) & ~(before < t))
                row[4] = np.sum((after < t + margin) & ~(before < t + margin))
                row[5], row[6], row[7] = mg.min(), np.max(before - after), v[np.flatnonzero(mg == mg.min())].min()
            near = False
            for g in (before, after):
                for lim in (t, t + margin):
                    near |= bool(np.any(np.abs(10.0 ** ((lim - g) / 10.0) - 1.0) < BAND))
            got.append(impact[s, a])
            want.append(row)
            band.append(near)
            pairs += len(v)
    out["fork_accepted"], out["fork_qualified"], out["fork_pairs"] = accepted, len(got), pairs
    out["fork_got"], out["fork_want"], out["fork_band"] = np.array(got).reshape(-1, 8), np.array(want).reshape(-1, 8), np.array(band, np.uint8)
    env.close()


def read_only(out, B=64):
    kw = dict(BASE, num_spectrum_resources=320, load=300.0, measure_disruptions=True)
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    twin = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    for e in (env, twin):
        e.seed(4)
        e.reset()
        e.step_policy(200, record=False)
    blob0, st0 = env.save_state(), env.stats()
    _, _, amap = env.observe_blocks(J)
    env.action_impact(amap)
    env.action_impact(amap, svc=env.service_qot()[0])
    env.action_impact(env.policy_actions()[0])
    blob1, st1 = env.save_state(), env.stats()
    out["ro_blob_same"] = blob0.tobytes() == blob1.tobytes()
    out["ro_stats_same"] = st0.tobytes() == st1.tobytes()
    out["ro_traj_same"] = record_bytes(env.step_policy(100)) == record_bytes(twin.step_policy(100))
    env.close()
    twin.close()


def fresh(out, B=8):
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **dict(BASE, num_spectrum_resources=320, load=300.0))
    env.seed(3)
    env.reset()
    ff = env.policy_actions()[0]
    assert np.all(ff != env.reject_action)
    out["fresh_rows"] = env.action_impact(ff)[:, 0]
    env.close()


def device_io(out, B=64):
    kw = dict(BASE, num_spectrum_resources=320, load=300.0)
    host = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    dev = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, io_device=True, **kw)
    c = host.holder.struct
    A = c.k_paths * J + 1
    t = torch.full((B, A, 8), 7.0, dtype=torch.float64, device="cuda")
    try:
        dev.action_impact(torch.zeros((B, A), dtype=torch.int32, device="cuda"), out=t)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    host.seed(5)
    host.reset()
    host.step_policy(250, record=False)
    _, _, amap = host.observe_blocks(J)
    want = host.action_impact(amap)
    want1 = host.action_impact(np.ascontiguousarray(amap[:, 0]))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        dev.seed(5)
        dev.reset()
        dev.step_policy(250, record=False)
        dmap = torch.from_numpy(amap).cuda()
        r = dev.action_impact(dmap, out=t)
        svc = torch.empty((B, c.capacity, 4), dtype=torch.float64, device="cuda")
        dev.service_qot(out=(svc, None, None))
        t2 = torch.full((B, A, 8), 7.0, dtype=torch.float64, device="cuda")
        dev.action_impact(dmap, svc=svc, out=t2)
        t1 = torch.full((B, 1, 8), 7.0, dtype=torch.float64, device="cuda")
        dev.action_impact(dmap[:, 0].contiguous(), out=t1)
        stream.synchronize()
        out["dev_same"] = r is t and np.array_equal(t.cpu().numpy(), want, equal_nan=True)
        got2 = t2.cpu().numpy()
        out["dev_svc_same"] = (np.array_equal(got2[:, :, :5], want[:, :, :5], equal_nan=True)
                               and np.array_equal(got2[:, :, 7], want[:, :, 7], equal_nan=True)
                               and np.allclose(got2[:, :, 5:7], want[:, :, 5:7], rtol=0, atol=1e-9, equal_nan=True))
        out["dev_one_column_same"] = np.array_equal(t1.cpu().numpy(), want1, equal_nan=True)
        dev.set_stream(None)
    host.close()
    dev.close()


def compat(out):
    from common import jocn_modulations
    from optical_networking_gym.topology import bundled_topology_path, get_topology
    topology = get_topology(bundled_topology_path("nsfnet_chen.txt"), None, jocn_modulations(), 80, 0.2, 4.5, 5)
    single = QRMSAEnv(topology=topology, seed=9, load=300, episode_length=1000, num_spectrum_resources=320, launch_power_dbm=1.0,
                      margin=0.5, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), gen_observation=False)
    single.reset()
    for _ in range(150):
        single.step(single.first_fit_action()[0])
    a = single.first_fit_action()[0]
    d = single.action_impact(a)
    row = single._dev.action_impact(np.array([[a]], np.int32))[0, 0]
    same = list(d) == list(nat.ACTION_IMPACT) and d["status"] == 0 and isinstance(d["affected"], int) and d["affected"] > 0
    same = same and all(float(d[k]) == row[i] for i, k in enumerate(nat.ACTION_IMPACT))
    rej = single.action_impact(single._dev.reject_action)
    out["compat_same"] = bool(same and rej["status"] == 1 and np.isnan(rej["affected"]))
    single.close()


def refusals(out):
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, **dict(BASE, num_spectrum_resources=320, load=300.0))
    acts, res = np.zeros((4, 300), np.int32), np.zeros((4, 300, 8))
    out["refuse_zero_rc"] = env.lib.ongym_action_impact(env._h, 0, acts.ctypes.data, None, res.ctypes.data)
    out["refuse_zero_msg"] = env.lib.ongym_last_error(env._h).decode()
    out["refuse_257_rc"] = env.lib.ongym_action_impact(env._h, 257, acts.ctypes.data, None, res.ctypes.data)
    out["refuse_null_rc"] = env.lib.ongym_action_impact(env._h, 4, None, None, res.ctypes.data)
    env.close()


def protect(out, B=32, steps=300):
    tb, kw, _, _ = case_config("disr_nsfnet_320")
    ref = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    ref.seed(21)
    ref.reset()
    col = COLS["newly_below_minimum"]
    disrupted = {}
    cleared = 0
    all_disrupt = reject_ok = infos_ok = off_same = True
    for prot in (False, True):
        v = QRMSABlockVecEnv(tables=tb, num_envs=B, blocks_to_consider=J, seed=21, protect_running=prot, **kw)
        v.reset()
        rng = np.random.default_rng(2)
        for t in range(steps):
            mask = v.action_masks()
            if not prot and t == 0:
                off_same = np.array_equal(mask, ref.observe_blocks(J)[1].astype(bool))
            if prot:
                _, base, amap = v.env.observe_blocks(J)
                newly = v.env.action_impact(amap)[:, :, col]
                gone = base.astype(bool) & ~mask
                cleared += int(gone.sum())
                all_disrupt &= bool(np.all(newly[gone] > 0)) and not np.any(mask & (np.nan_to_num(newly) > 0))
                reject_ok &= bool(np.all(mask[:, -1]))
            acts = np.array([rng.choice(np.flatnonzero(row)) for row in mask])
            _, _, _, infos = v.step(acts)
            infos_ok &= all(("disrupts" in i) == prot and i.get("disrupts", 0) == 0 for i in infos)
        disrupted[prot] = int(np.sum(v.env.stats()["disrupted_services"]))
        v.close()
    ref.close()
    out["protect_off_masks_same"], out["protect_cleared"], out["protect_cleared_all_disrupt"] = off_same, cleared, all_disrupt
    out["protect_reject_allowed"], out["protect_infos_ok"] = reject_ok, infos_ok
    out["protect_disrupted_off"], out["protect_disrupted_on"] = disrupted[False], disrupted[True]


def main():
    out = {}
    refusals(out)
    fresh(out)
    read_only(out)
    device_io(out)
    compat(out)
    for key in CASES:
        oracle_case(out, key)
        print(key, "done", flush=True)
    forks(out)
    protect(out)
    np.savez(sys.argv[1], **out)
    print("action impact child ok")


if __name__ == "__main__":
    main()
