"""Child process of tests/test_gpu_blocks.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP runtime and
this library's must start together), saved to an .npz that the tests assert on.

    python tests/blocks_child.py OUT.npz

Covers ongym_observe_blocks (BatchedQRMSAEnv.observe_blocks / decode_block_actions, QRMSABlockVecEnv): golden trajectories driven
by block actions, device states with the GSNR of every block start for the restatement, forks that step every entry of a map,
the read-only property, the header against ongym_observe, device I/O on torch's stream, the VecEnv and the refusals.
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402

from common import golden_tables, jocn_modulations, load_traj, record_bytes, traj_requests  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402
from optical_networking_gym.envs.batched import BatchedQRMSAEnv, OngymError  # noqa: E402
from optical_networking_gym.envs.block_vec_env import QRMSABlockVecEnv  # noqa: E402
from test_gpu_blocks import STATE_BLOCKS, STATES, TRAJ, TRAJ_BLOCKS, block_candidates  # noqa: E402
from test_gpu_parity import make_env  # noqa: E402

STATE_KW = dict(capacity=1024, bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), episode_length=1000)
REQ = np.dtype([("source", "<i4"), ("destination", "<i4"), ("bit_rate", "<f4"), ("have", "?")])


def trajectories(out):
    for tag in TRAJ:
        meta, d = load_traj(tag)
        for J in TRAJ_BLOCKS:
            env = make_env(meta, auto_reset=True)
            env.set_requests(traj_requests(d))
            for _ in range(meta["initial_resets"]):
                env.reset()
            K = env.holder.struct.k_paths
            recs, valid = [], 0
            for _ in range(meta["n_steps"]):
                _, mask, amap = env.observe_blocks(J)
                first = np.flatnonzero(mask[0, :K * J:J])
                ba = int(first[0]) * J if len(first) else K * J
                valid += int(mask[0, :-1].sum())
                recs.append(env.step(env.decode_block_actions(np.array([ba]), amap)))
            out[f"traj_{tag}_J{J}"] = np.stack(recs).view(np.uint8)
            out[f"traj_{tag}_J{J}_valid"] = valid
            env.close()


def state_env(topo, S, seed, B=256, **over):
    kw = dict(STATE_KW, load=300 if S == 320 else 600)
    kw.update(over)
    env = BatchedQRMSAEnv(tables=golden_tables(topo), modulations=jocn_modulations(), batch_size=B, num_spectrum_resources=S,
                          **kw)
    env.seed(seed)
    env.reset()
    env.step_policy(300, record=False)
    return env


def state_cfg(env, tables):
    c, mods = env.holder.struct, jocn_modulations()
    return dict(K=c.k_paths, M=c.n_mods, S=c.n_slots, pair_paths=tables.pair_paths, path_links=tables.path_links,
                path_hops=tables.path_hops, se=np.array([m.spectral_efficiency for m in mods], np.int32),
                thr=np.array([m.minimum_osnr for m in mods], np.float64),
                width=c.nslots_channel_width if c.nslots_channel_width > 0 else c.channel_width, margin=c.margin)


def states(out):
    for topo, S, seed in STATES:
        key = f"st_{topo}_{S}_{seed}"
        tables = golden_tables(topo)
        env = state_env(topo, S, seed)
        cfg = state_cfg(env, tables)
        for k, v in cfg.items():
            out[f"{key}_cfg_{k}"] = v
        for J in STATE_BLOCKS:
            out[f"{key}_J{J}_obs"], out[f"{key}_J{J}_mask"], out[f"{key}_J{J}_map"] = env.observe_blocks(J)
        obs, _ = env.observe()
        out[key + "_obs_head"] = obs[:, :3 + cfg["K"]]
        B = env.batch_size
        grids, reqs, cand, gs = [], np.zeros(B, REQ), [], []
        for r in range(B):
            g = env.grid(r)
            q = env.request(r)
            reqs[r] = (q["source"], q["destination"], q["bit_rate"], True)
            grids.append(g.astype(np.int8))
            cs = block_candidates(cfg, g, reqs[r])
            if cs:
                gs.append(env.gsnr_many(r, cs)[:, 0])
                cand.append(np.column_stack([np.full(len(cs), r), np.array(cs)]))
        out[key + "_grids"], out[key + "_reqs"] = np.stack(grids), reqs
        out[key + "_cand"], out[key + "_gsnr"] = np.concatenate(cand).astype(np.int32), np.concatenate(gs)
        if (topo, S, seed) == STATES[0]:
            forks(out, env)
        if (topo, S, seed) == STATES[1]:
            read_only(out, env)
        env.close()


def forks(out, env, J=8):
    """one replica into K*J + 1 copies, copy i stepped with entry i of the replica's action map"""
    c = env.holder.struct
    K, M, S, B = c.k_paths, c.n_mods, c.n_slots, env.batch_size
    blob = env.save_state()
    obs, mask, amap = env.observe_blocks(J)
    rich = np.argsort(-mask[:, :-1].sum(axis=1), kind="stable")
    picks = [int(rich[0]), int(rich[1]), int(rich[B // 2])]
    for r in picks:
        env.load_state(blob)
        src = np.full(B, -1, np.int32)
        src[:K * J + 1] = r
        env.fork(src)
        acts = np.full(B, env.reject_action, np.int32)
        acts[:K * J + 1] = amap[r]
        rec = env.step(acts)
        out[f"fork_{r}_map"], out[f"fork_{r}_mask"] = amap[r], mask[r]
        out[f"fork_{r}_rec"] = rec[:K * J + 1].view(np.uint8).reshape(K * J + 1, -1)
        f = obs[r, 3 + 3 * K:].reshape(K * J, 6)
        out[f"fork_{r}_nslots"] = np.append(np.rint(f[:, 3].astype(np.float64) * S).astype(np.int32), 0)
    out["fork_replicas"] = np.array(picks)
    out["fork_M"], out["fork_S"], out["fork_reject"] = M, S, env.reject_action
    env.load_state(blob)


def read_only(out, env):
    blob0, st0 = env.save_state(), env.stats()
    for J in (1, 8, 16):
        env.observe_blocks(J)
    blob1, st1 = env.save_state(), env.stats()
    out["ro_blob_same"] = blob0.tobytes() == blob1.tobytes()
    out["ro_stats_same"] = st0.tobytes() == st1.tobytes()
    r1 = env.step_policy(100)
    env.load_state(blob0)
    env.observe_blocks(16)
    r2 = env.step_policy(100)
    out["ro_traj_same"] = record_bytes(r1) == record_bytes(r2)


def golden_header(out):
    meta, d = load_traj("obs_nsfnet320")
    env = make_env(meta, auto_reset=False)
    env.set_requests(traj_requests(d))
    for _ in range(meta["initial_resets"]):
        env.reset()
    K = env.holder.struct.k_paths
    a, b = [], []
    for i in range(meta["steps"] + 1):
        obs, _ = env.observe()
        bo = env.observe_blocks(4)[0]
        a.append(bo[0, :3 + K])
        b.append(obs[0, :3 + K])
        if i < meta["steps"]:
            env.step(np.array([d["action"][i]], np.int32))
    out["head_blocks"], out["head_observe"] = np.stack(a), np.stack(b)
    env.close()


def device_io(out, J=8, B=64, steps=20):
    host = state_env("nsfnet", 320, 5, B=B)
    dev = state_env("nsfnet", 320, 5, B=B, io_device=True)
    K = host.holder.struct.k_paths
    n = K * J + 1
    t = (torch.empty((B, host.block_obs_dim(J)), dtype=torch.float32, device="cuda"),
         torch.empty((B, n), dtype=torch.uint8, device="cuda"), torch.empty((B, n), dtype=torch.int32, device="cuda"))
    try:
        dev.observe_blocks(J, out=t)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)
    stream = torch.cuda.Stream()
    same = dict(obs=True, mask=True, map=True, rec=True)
    accepted = 0
    with torch.cuda.stream(stream):
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        for _ in range(steps):
            o, m, a = host.observe_blocks(J)
            ba = np.argmax(m, axis=1)
            rh = host.step(host.decode_block_actions(ba, a))
            dev.observe_blocks(J, out=t)
            bad = torch.argmax(t[1].to(torch.int32), dim=1)
            acts = dev.decode_block_actions(bad, t[2]).to(torch.int32).contiguous()
            recs = torch.empty((B, nat.STEP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
            dev._check(dev.lib.ongym_step_actions(dev._h, C.c_void_p(acts.data_ptr()), C.c_void_p(recs.data_ptr())), "step")
            stream.synchronize()
            same["obs"] &= np.array_equal(t[0].cpu().numpy().view(np.uint32), o.view(np.uint32))
            same["mask"] &= np.array_equal(t[1].cpu().numpy(), m)
            same["map"] &= np.array_equal(t[2].cpu().numpy(), a)
            rd = recs.cpu().numpy().reshape(-1).view(nat.STEP_DTYPE)
            same["rec"] &= record_bytes(rd) == record_bytes(rh)
            accepted += int(rh["accepted"].sum())
        dev.set_stream(None)
    for k, v in same.items():
        out[f"dev_{k}_same"] = v
    out["dev_accepted"] = accepted
    host.close()
    dev.close()


def vec_env(out, steps=200):
    v = QRMSABlockVecEnv(tables=golden_tables("nsfnet"), modulations=jocn_modulations(), num_envs=64, blocks_to_consider=8,
                         seed=3, num_spectrum_resources=320, load=300, bit_rate_selection="discrete",
                         bit_rates=(10, 40, 100, 400), episode_length=100, capacity=512)
    obs = v.reset()
    rng = np.random.default_rng(0)
    qot = retry = episodes = accepted = deep = 0
    for _ in range(steps):
        mask = v.action_masks()
        out["vec_mask_shape"] = np.array(mask.shape)
        deep += int(mask[:, :-1].reshape(64, 5, 8)[:, :, 1:].sum())
        acts = np.array([rng.choice(np.flatnonzero(row)) for row in mask])
        obs, rew, done, infos = v.step(acts)
        for i in infos:
            qot += "qot_error" in i
            retry += "retry" in i
            episodes += "episode" in i
            accepted += i["episode"]["episode_services_accepted"] if "episode" in i else 0
    out["vec_obs_shape"] = np.array(obs.shape)
    out["vec_n_actions"], out["vec_obs_dim"] = v.n_actions, v.obs_dim
    out["vec_qot"], out["vec_retry"], out["vec_episodes"], out["vec_accepted"], out["vec_deep"] = qot, retry, episodes, accepted, deep
    v.close()


def refusals(out):
    env = state_env("nsfnet", 320, 1, B=4, modulations_to_consider=4)
    K = env.holder.struct.k_paths
    obs, mask, amap = np.zeros((4, 3 + 3 * K + 6 * K * 4), np.float32), np.zeros((4, K * 4 + 1), np.uint8), np.zeros((4, K * 4 + 1), np.int32)
    out["refuse_mtc_rc"] = env.lib.ongym_observe_blocks(env._h, 4, obs.ctypes.data, mask.ctypes.data, amap.ctypes.data)
    out["refuse_mtc_msg"] = env.lib.ongym_last_error(env._h).decode()
    try:
        env.observe_blocks(4)
    except OngymError:
        pass
    env.close()
    env = state_env("nsfnet", 320, 1, B=4)
    out["refuse_j0_rc"] = env.lib.ongym_observe_blocks(env._h, 0, obs.ctypes.data, mask.ctypes.data, amap.ctypes.data)
    out["refuse_j17_rc"] = env.lib.ongym_observe_blocks(env._h, 17, obs.ctypes.data, mask.ctypes.data, amap.ctypes.data)
    env.close()


def main():
    out = {}
    refusals(out)
    golden_header(out)
    states(out)
    trajectories(out)
    device_io(out)
    vec_env(out)
    np.savez(sys.argv[1], **out)
    print("blocks child ok")


if __name__ == "__main__":
    main()
