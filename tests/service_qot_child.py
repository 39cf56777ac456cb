"""Child process of tests/test_gpu_service_qot.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP
runtime and this library's must start together), saved to an .npz that the tests assert on.

    python tests/service_qot_child.py OUT.npz

Covers ongym_service_qot (BatchedQRMSAEnv.service_qot): device replicas and CPU oracles driven with the same traffic on many
configurations (with the oracle restatement of every running service), the disruption invariant along the reference's
measure_disruptions run and on random runs, the first service of an empty network, the read-only property, launch scale,
device I/O on torch's stream and the refusals.
"""
import copy
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402

from common import golden_tables, jocn_modulations, load_traj, record_bytes, traj_requests  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv  # noqa: E402
from oracle_lib import OracleEnv  # noqa: E402
from test_gpu_parity import make_env  # noqa: E402
from test_gpu_service_qot import CASES, insertion_order, match, restate_gn  # noqa: E402

BASE = dict(modulations=jocn_modulations(), capacity=512, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400),
            auto_reset=True, episode_length=1000, margin=0.5, launch_power_dbm=1.0)


def case_config(key):
    """(tables, keyword arguments, how the traffic is driven, steps)"""
    how, topo, S = key.split("_")
    topo = {"nobeleu": "nobel-eu"}.get(topo, topo)
    S = int(S)
    tb = golden_tables(topo)
    kw = dict(BASE, num_spectrum_resources=S, load=300.0 * S / 320)
    steps = 400
    if how == "wide":
        kw.update(bit_rates=(10, 40, 100, 400, 1000), capacity=1024)
    elif how == "ff" and topo == "germany50":
        kw.update(load=150.0)
        steps = 300
    elif how == "ff" and S == 768:
        kw.update(capacity=1024)
    elif how == "alpha":
        tb = copy.deepcopy(tb)
        tb.link_alpha = tb.link_alpha * np.linspace(0.85, 1.2, tb.n_links)
    elif how == "cont":
        kw.update(bit_rate_selection="continuous", bit_rate_lower_bound=25, bit_rate_higher_bound=300)
    elif how == "trace":
        kw.update(bit_rates=(10, 40, 100))
    elif how == "defrag":
        kw.update(defragmentation=True, n_defrag_services=4)
    elif how == "disr":
        kw.update(measure_disruptions=True, launch_power_dbm=3.0, load=500.0, margin=0.0)
    elif how == "ids":
        kw.update(track_service_ids=True)
    elif how == "random":
        kw.update(auto_reset=False, episode_length=10 ** 6, load=200.0)
    return tb, kw, how, steps


def save_replica(out, key, r, env, o, svc, rep, link, margin, tables, mod_se, ids_from_device):
    """one replica's device values, its records and the oracle restatement on the oracle's running services"""
    k = f"{key}_r{r}"
    dsvc = env.services(r)
    osvc = o.services()
    if len(osvc) < len(dsvc):
        # the oracle lists the services of its departure heap; the counters-only reset dropped the heap, so the services that
        # kept running are missing there (release time +inf on the device).  The grids are equal, so they are the same ones.
        assert np.array_equal(env.grid(r), o.grid())
        have = {(int(p), int(s)) for p, s in zip(osvc["path_id"], osvc["slot"])}
        kept = np.array([(int(p), int(s)) not in have for p, s in zip(dsvc["path_id"], dsvc["slot"])], bool)
        assert np.all(np.isinf(dsvc["release_time"][kept]))
        extra = dsvc[kept].copy()
        extra["service_id"], extra["reserved"] = -1, 0
        osvc = np.concatenate([extra, osvc])
    osvc = osvc[insertion_order(osvc)]
    ids = None
    if ids_from_device:
        ids = np.empty(len(osvc), np.int64)
        ids[match(dsvc, osvc)] = dsvc["service_id"]
    out[k + "_svc"], out[k + "_rep"], out[k + "_link"] = svc[r], rep[r], link[r]
    out[k + "_dsvc"], out[k + "_osvc"], out[k + "_margin"] = dsvc, osvc, margin
    out[k + "_want"] = restate_gn(o, tables, mod_se, osvc, ids)
    return dsvc, osvc


def save_tables(out, key, holder, tb):
    out[key + "_thr"] = np.asarray(holder.mod_thr, np.float64)
    out[key + "_path_links"], out[key + "_path_hops"] = tb.path_links, tb.path_hops


def oracle_case(out, key, B=3, seed=11):
    tb, kw, how, steps = case_config(key)
    holder = nat.ConfigHolder(tb, batch=B, **kw)
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    oracles = [OracleEnv(holder, replica=r) for r in range(B)]
    rng = np.random.default_rng(seed)
    if how == "trace":                  # bit rates beyond the configured table: slot counts above the pair table's range
        n = steps + 40
        reqs = np.zeros((B, n), nat.REQUEST_DTYPE)
        for r in range(B):
            reqs[r]["arrival_time"] = np.cumsum(rng.exponential(10800.0 / kw["load"], n)).astype(np.float32)
            reqs[r]["holding_time"] = rng.exponential(10800.0, n).astype(np.float32)
            src = rng.integers(0, tb.n_nodes, n)
            reqs[r]["source"], reqs[r]["destination"] = src, (src + rng.integers(1, tb.n_nodes, n)) % tb.n_nodes
            reqs[r]["bit_rate"] = rng.choice(np.array([10, 100, 400, 1000]), n)
        env.set_requests(reqs)
        for r, o in enumerate(oracles):
            o.set_trace(reqs[r])
    else:
        env.seed(seed)
        for o in oracles:
            o.seed(seed)
    env.reset()
    for o in oracles:
        o.reset()
    policy = {"lb": nat.POLICY_LOAD_BALANCING, "hsnr": nat.POLICY_HIGHEST_SNR, "lf": nat.POLICY_LOWEST_FRAGMENTATION}.get(how)
    if how == "random":
        warm = 150
        env.step_policy(warm, record=False)
        for o in oracles:
            o.run_first_fit(warm)
        for _ in range(steps - warm):
            ff, _ = env.policy_actions()
            u = rng.random(B)
            acts = np.where(u < 0.5, ff, np.where(u < 0.65, env.reject_action, rng.integers(0, env.reject_action + 1, B)))
            acts = acts.astype(np.int32)
            env.step(acts)
            for r, o in enumerate(oracles):
                o.step(int(acts[r]))
    elif how == "ids":                  # counters-only reset in the middle: ids restart under services that keep running
        half = steps // 2
        env.step_policy(half, record=False)
        env.reset_episode_counters()
        env.step_policy(steps - half, record=False)
        for o in oracles:
            o.run_first_fit(half)
            o.reset_counters()
            o.run_first_fit(steps - half)
    elif policy is not None:
        env.step_policy(steps, record=False, policy=policy)
        for o in oracles:
            o.run_policy(policy, steps)
    else:
        env.step_policy(steps, record=False)
        for o in oracles:
            o.run_first_fit(steps)
    svc, rep, link = env.service_qot()
    save_tables(out, key, holder, tb)
    out[key + "_replicas"] = np.arange(B)
    extra = 0
    for r, o in enumerate(oracles):
        dsvc, osvc = save_replica(out, key, r, env, o, svc, rep, link, kw["margin"], tb, holder.mod_se,
                                  how in ("ids", "defrag"))
        if how == "wide":
            extra += int(np.sum(dsvc["nslots"] > 32))
        elif how == "trace":
            tab_nmax = int(np.ceil(100 / (min(holder.mod_se) * 12.5)))
            extra += int(np.sum(dsvc["nslots"] > tab_nmax))
        elif how == "ids":
            extra += len(dsvc) - len(np.unique(dsvc["service_id"]))
        elif how == "disr":
            extra += int(np.sum(dsvc["reserved"] != 0))
    st = env.stats()
    out[key + "_wide"] = out[key + "_above_tab"] = out[key + "_dup_ids"] = out[key + "_disrupted"] = extra
    out[key + "_moves"] = int(np.sum(st["episode_service_reallocations"]))     # one episode: nothing reset the count
    out[key + "_uniform"] = bool(np.all(tb.link_alpha == tb.link_alpha[0]))
    out["any_below_margin"] = out.get("any_below_margin", 0) + int(np.sum(rep[:, 2]))
    env.close()


def disruption_invariant(out):
    """below minimum_osnr now => already in the disrupted list: along the reference's measure_disruptions run through both
    step kernels, and on random measure_disruptions runs"""
    meta, d = load_traj("traj_nsfnet320_disr")
    thr = None
    for generic in (False, True):
        if generic:
            os.environ["ONGYM_FORCE_GENERIC"] = "1"
        env = make_env(meta, auto_reset=True, measure_disruptions=True)
        os.environ.pop("ONGYM_FORCE_GENERIC", None)
        env.set_requests(traj_requests(d))
        for _ in range(meta["initial_resets"]):
            env.reset()
        thr = np.asarray(env.holder.mod_thr)
        below, flagged = [], []
        for chunk in (300, 400, 400, 500, 390):
            env.step_policy(chunk, record=False)
            svc, _, _ = env.service_qot()
            s = env.services(0)
            below.append(svc[0, :len(s), 0] < thr[s["modulation"]])
            flagged.append(s["reserved"] != 0)
        out[f"inv_traj_{int(generic)}_belowflag"], out[f"inv_traj_{int(generic)}_flagged"] = np.concatenate(below), np.concatenate(flagged)
        env.close()
    B = 16
    kw = dict(BASE, num_spectrum_resources=160, load=260.0, measure_disruptions=True, launch_power_dbm=4.0, margin=0.0,
              episode_length=400)
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    env.seed(77)
    env.reset()
    below, flagged = [], []
    for _ in range(4):
        env.step_policy(150, record=False)
        svc, _, _ = env.service_qot()
        for r in range(B):
            s = env.services(r)
            below.append(svc[r, :len(s), 0] < thr[s["modulation"]])
            flagged.append(s["reserved"] != 0)
    out["inv_random_belowflag"], out["inv_random_flagged"] = np.concatenate(below), np.concatenate(flagged)
    env.close()


def fresh(out, B=8):
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **dict(BASE, num_spectrum_resources=320, load=300.0))
    env.seed(3)
    env.reset()
    rec = env.step_policy(1)[0]
    svc, rep, _ = env.service_qot()
    acc = rec["accepted"] != 0
    out["fresh_svc"] = svc[acc, 0, :3]
    out["fresh_rec"] = np.stack([rec["osnr"][acc], rec["ase"][acc], rec["nli"][acc]], axis=1)
    assert np.all(rep[acc, 0] == 1)
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
    env.service_qot()
    env.service_qot()
    blob1, st1 = env.save_state(), env.stats()
    out["ro_blob_same"] = blob0.tobytes() == blob1.tobytes()
    out["ro_stats_same"] = st0.tobytes() == st1.tobytes()
    out["ro_traj_same"] = record_bytes(env.step_policy(100)) == record_bytes(twin.step_policy(100))
    src = np.roll(np.arange(B, dtype=np.int32), 1)
    env.fork(src)
    twin.fork(src)
    env.service_qot()
    out["ro_fork_same"] = record_bytes(env.step_policy(100)) == record_bytes(twin.step_policy(100))
    env.close()
    twin.close()


def scale(out, key, B, sample, steps=300):
    tb = golden_tables("nsfnet")
    kw = dict(BASE, num_spectrum_resources=320, load=300.0, capacity=448)
    holder = nat.ConfigHolder(tb, batch=B, **kw)
    env = BatchedQRMSAEnv(tables=tb, batch_size=B, **kw)
    env.seed(9)
    env.reset()
    env.step_policy(steps, record=False)
    svc, rep, link = env.service_qot()
    save_tables(out, key, holder, tb)
    out[key + "_replicas"], out[key + "_batch"] = np.array(sample), B
    for r in sample:
        o = OracleEnv(holder, replica=r)
        o.seed(9)
        o.reset()
        o.run_first_fit(steps)
        save_replica(out, key, r, env, o, svc, rep, link, kw["margin"], tb, holder.mod_se, False)
    del svc
    env.close()


def device_io(out, B=64):
    kw = dict(BASE, num_spectrum_resources=320, load=300.0)
    host = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, **kw)
    dev = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=B, io_device=True, **kw)
    C, E = host.holder.struct.capacity, host.holder.struct.n_links
    t = (torch.full((B, C, 4), 7.0, dtype=torch.float64, device="cuda"), torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda"),
         torch.full((B, E, 3), 7.0, dtype=torch.float32, device="cuda"))
    try:
        dev.service_qot(out=t)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    host.seed(5)
    host.reset()
    host.step_policy(250, record=False)
    hs, hr, hl = host.service_qot()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        dev.seed(5)
        dev.reset()
        dev.step_policy(250, record=False)
        r = dev.service_qot(out=t)
        part = torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda")
        dev.service_qot(out=(None, part, None))
        stream.synchronize()
        out["dev_same"] = (r[0] is t[0] and np.array_equal(t[0].cpu().numpy(), hs, equal_nan=True)
                           and np.array_equal(t[1].cpu().numpy(), hr, equal_nan=True)
                           and np.array_equal(t[2].cpu().numpy(), hl, equal_nan=True))
        out["dev_partial_same"] = np.array_equal(part.cpu().numpy(), hr, equal_nan=True)
        dev.set_stream(None)
    host.close()
    dev.close()


def refusals(out):
    kw = dict(BASE, num_spectrum_resources=320, load=300.0)
    env = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, **kw)
    out["refuse_null_rc"] = env.lib.ongym_service_qot(env._h, None, None, None)
    out["refuse_null_msg"] = env.lib.ongym_last_error(env._h).decode()
    try:
        env.service_qot(out=(np.zeros((4, 512, 4)), None, None))
        out["refuse_out_on_host_env"] = False
    except ValueError:
        out["refuse_out_on_host_env"] = True
    env.close()
    dev = BatchedQRMSAEnv(tables=golden_tables("nsfnet"), batch_size=4, io_device=True, **kw)
    C, E = dev.holder.struct.capacity, dev.holder.struct.n_links
    stream = torch.cuda.Stream()

    def refused(t):
        try:
            dev.service_qot(out=t)
        except ValueError:
            return True
        return False

    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        f64, f32 = torch.float64, torch.float32
        out["refuse_all_none"] = refused((None, None, None))
        out["refuse_dtype"] = refused((torch.empty((4, C, 4), dtype=f32, device="cuda"), None, None))
        out["refuse_shape"] = refused((None, torch.empty((4, 7), dtype=f64, device="cuda"), None))
        out["refuse_host_tensor"] = refused((None, None, torch.empty((4, E, 3), dtype=f32)))
        dev.set_stream(None)
    dev.close()


def main():
    out = {}
    refusals(out)
    fresh(out)
    read_only(out)
    device_io(out)
    disruption_invariant(out)
    for key in CASES:
        oracle_case(out, key)
    scale(out, "scale_odd", 1237, [0, 618, 1236])
    scale(out, "scale_65536", 65536, [0, 21845, 65535])
    np.savez(sys.argv[1], **out)
    print("service qot child ok")


if __name__ == "__main__":
    main()
