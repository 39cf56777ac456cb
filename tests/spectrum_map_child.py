"""Child process of tests/test_gpu_spectrum_map.py: every GPU computation of that module in ONE fresh process (PyTorch's HIP
runtime and this library's must start together), saved to an .npz that the tests assert on.

    python tests/spectrum_map_child.py OUT.npz

The expected arrays come from the restatement of tests/test_gpu_spectrum_map.py on every replica's own grid(r) and
services(r).  The doctored states are made from a saved blob by the header's sec_off and sec_bytes; their expected arrays come
from the doctored blob itself, decoded in numpy (`blob_state`), after the undoctored blob's decoding has been compared with
grid(r) and services(r).  On a doctored environment only spectrum_map, check_state (which is spectrum_map), save_state and
close are called."""
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "optical-networking-gym_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402,F401  (before the library is loaded: the two HIP runtimes must start together)

from common import golden_tables, jocn_modulations, record_bytes  # noqa: E402
from failure_impact_child import BASE, tab_nmax  # noqa: E402
from optical_networking_gym import _native as nat  # noqa: E402
from test_gpu_spectrum_map import (decode, from_views, load_cases, pack, restate, restate_records, route_mask0)  # noqa: E402

NAMES = ("owners", "records", "release", "audit")
SECTIONS = ("occ", "svc_a", "svc_b", "svc_r", "svc_q", "svc_o", "move_log", "move_n", "env")   # StateSection, csrc/ongym_state.hpp
ACTIVE_IN_STATS = nat.STATS_DTYPE.fields["active"][1]


def make(tb, io_device=False, **kw):
    from optical_networking_gym.envs.batched import BatchedQRMSAEnv
    return BatchedQRMSAEnv(tables=golden_tables(tb), io_device=io_device, **dict(BASE, **kw))


def width_limit(env):
    """the width limit of ongym_move_services on `env`: the rows of the pair table (32 in the narrow build) where a lean kernel
    may run, else S"""
    n = tab_nmax(env.holder)
    return min(n, 512 if n > 32 else 32) if env.occupancy()["lean_kernel"] else env.holder.struct.n_slots


def expected(env):
    """the restated arrays of every replica of a host environment, from its own views"""
    c = env.holder.struct
    width = width_limit(env)
    rows = [from_views(env.tables, c.n_mods, c.n_slots, c.capacity, env.grid(r), env.services(r), width) for r in range(env.batch_size)]
    return {n: np.stack([row[i] for row in rows]) for i, n in enumerate(("owners", "audit", "records", "release"))}


def snapshot(out, k, env, want=None):
    got = env.spectrum_map(owners=True, records=True, audit=True)
    want = want or expected(env)
    for n in NAMES:
        out[f"{k}_{n}"], out[f"{k}_want_{n}"] = got[n], want[n]
    return got, want


def on_device(env, fn):
    """fn() with `env` on a side stream that is torch's current stream"""
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        env.set_stream(torch.cuda.current_stream().cuda_stream)
        res = fn()
        stream.synchronize()
        env.set_stream(None)
    return res


def device_tensors(env, names=NAMES, fill=7):
    c = env.holder.struct
    B, Cp = env.batch_size, c.capacity
    spec = dict(owners=((B, c.n_links, c.n_slots), torch.int16), records=((B, Cp, 6), torch.int32),
                release=((B, Cp), torch.float32), audit=((B, 10), torch.int32))
    return {n: torch.full(spec[n][0], fill, dtype=spec[n][1], device="cuda") for n in names}


# ---- 1. definition states -------------------------------------------------------------------------------------------------
DEFINITIONS = dict(
    ring4=("ring4", dict(num_spectrum_resources=64, capacity=128, load=40.0)),
    nsfnet320=("nsfnet", dict(num_spectrum_resources=320, capacity=448, load=300.0)),
    nsfnet100=("nsfnet", dict(num_spectrum_resources=100, capacity=256, load=140.0)),
    nobeleu320=("nobel-eu", dict(num_spectrum_resources=320, capacity=512, load=300.0)),
    germany100=("germany50", dict(num_spectrum_resources=100, capacity=256, load=200.0)),
    ids=("nsfnet", dict(num_spectrum_resources=320, capacity=448, load=300.0, track_service_ids=True)),
    defrag=("nsfnet", dict(num_spectrum_resources=320, capacity=448, load=300.0, defragmentation=True, n_defrag_services=4)))


def drive(env, seed, steps=(150, 40, 20)):
    """first fit (the lean kernel where the configuration has one), exact fit (the generic kernel), random valid external
    actions; returns how many of the last were accepted"""
    env.seed(seed)
    env.reset()
    env.step_policy(steps[0], record=False)
    env.step_policy(steps[1], record=False, policy=nat.POLICY_EXACT_FIT)
    accepted = 0
    for i in range(steps[2]):
        _, mask = env.observe()
        accepted += int(env.step(env.sample_actions(mask, seed, i))["accepted"].sum())
    return accepted


def definition_case(out, key, B=8):
    tb, kw = DEFINITIONS[key]
    host = make(tb, batch_size=B, **kw)
    k = f"def_{key}_host"
    out[f"def_{key}_external_accepted"] = drive(host, 31)
    out[f"def_{key}_lean"] = host.occupancy()["lean_kernel"]         # which kernels the two policies of `drive` ran on
    out[f"def_{key}_lean_generic_policy"] = host.occupancy(nat.POLICY_EXACT_FIT)["lean_kernel"]
    got, want = snapshot(out, k, host)
    blob = host.save_state()
    S = host.holder.struct.n_slots
    ends = sum(int(np.sum(host.services(r)["slot"].astype(int) + host.services(r)["nslots"] == S)) for r in range(B))
    dev = make(tb, io_device=True, batch_size=B, **kw)

    def run():
        dev.load_state(torch.from_numpy(blob).cuda())
        t = device_tensors(dev)
        ret = dev.spectrum_map(out=t, owners=True, records=True, audit=True)
        assert all(ret[n] is t[n] for n in NAMES)
        return t, dev.decode_owners(t["owners"])
    t, (drec, dkind) = on_device(dev, run)
    kd = f"def_{key}_device"
    for n in NAMES:
        out[f"{kd}_{n}"], out[f"{kd}_want_{n}"] = t[n].cpu().numpy(), want[n]
    hrec, hkind = host.decode_owners(got["owners"])
    for kk, (rec, kind) in ((k, (hrec, hkind)), (kd, (drec.cpu().numpy(), dkind.cpu().numpy()))):
        out[kk + "_dec_record"], out[kk + "_dec_kind"] = rec, kind
        out[kk + "_S"], out[kk + "_rec32"], out[kk + "_ends_at_S"] = S, bool(host.tables.n_links <= 32 and host.tables.n_paths <= 512), ends
    host.close()
    dev.close()


# ---- 2. after every state-changing call -----------------------------------------------------------------------------------
NSF = dict(num_spectrum_resources=320, capacity=448, load=300.0)


def after(out, k, env, **more):
    snapshot(out, "after_" + k, env)
    out[f"after_{k}_check_state"] = env.check_state()
    out[f"after_{k}_failed"] = env.failed_links()
    for name, v in more.items():
        out[f"after_{k}_{name}"] = v


def after_calls(out, B=16):
    env, twin = make("nsfnet", batch_size=B, **NSF), make("nsfnet", batch_size=B, **NSF)
    for e in (env, twin):
        e.seed(17)
        e.reset()
        e.step_policy(250, record=False)
    E = env.holder.struct.n_links
    sets = [[r % E, (5 * r + 3) % E] for r in range(B)]
    env.cut_links(sets)
    after(out, "cut", env)
    env.step_policy(50, record=False)
    env.repair_links(sets)
    after(out, "repair", env)
    env.step_policy(50, record=False)
    moves = np.tile(np.array([nat.MOVE_TOP, nat.MOVE_FIRST_FIT], np.int32), (4, 1))
    res = env.move_services(moves)
    after(out, "move", env, moved=int(np.sum(res[:, :, 0] == 0)))
    env.step_policy(50, record=False)
    res = env.defragment(8)
    after(out, "defragment", env, moved=int(np.sum(res[:, :, 0] == 0)))
    twin.cut_links(sets, restore=False)
    after(out, "cut_no_restore", twin)
    third = make("nsfnet", batch_size=B, **NSF)
    third.load_state(twin.save_state())
    after(out, "load", third)
    src = np.arange(B, dtype=np.int32)
    src[1::2] = 0
    third.fork(src)
    after(out, "fork", third)
    short = make("nsfnet", batch_size=B, **dict(NSF, episode_length=100))
    short.seed(17)
    short.reset()
    short.step_policy(250, record=False)
    after(out, "auto_reset", short, episodes=short.stats()["episodes_completed"])
    for e in (env, twin, third, short):
        e.close()


# ---- 3. read-only, subsets, refusals --------------------------------------------------------------------------------------
def subsets_equal(call, full):
    """the fifteen non-empty subsets of the four pointers through `call(dict of arrays or None)` against the full call"""
    ok = []
    for bits in range(1, 16):
        names = [n for i, n in enumerate(NAMES) if bits >> i & 1]
        got = call(names)
        ok.append(all(np.array_equal(got[n], full[n], equal_nan=True) for n in names))
    return np.array(ok)


def read_only(out, B=8):
    kw = dict(NSF, measure_disruptions=True)
    env, twin = make("nsfnet", batch_size=B, **kw), make("nsfnet", batch_size=B, **kw)
    for e in (env, twin):
        e.seed(5)
        e.reset()
        e.step_policy(200, record=False)
    blob0, st0 = env.save_state(), env.stats()
    full = env.spectrum_map(owners=True, records=True, audit=True)
    out["last_kernel_ms"] = env.last_kernel_ms()
    env.check_state()
    out["ro_blob_same"] = env.save_state().tobytes() == blob0.tobytes()
    st1 = env.stats()
    out["ro_stats_same"] = all(np.array_equal(st0[f], st1[f], equal_nan=True) for f in st0.dtype.names)
    out["ro_twin_records_same"] = record_bytes(env.step_policy(50)) == record_bytes(twin.step_policy(50))
    full = env.spectrum_map(owners=True, records=True, audit=True)
    c = env.holder.struct
    shapes = dict(owners=((B, c.n_links, c.n_slots), np.int16), records=((B, c.capacity, 6), np.int32),
                  release=((B, c.capacity), np.float32), audit=((B, 10), np.int32))

    def host_call(names):
        a = {n: np.full(shapes[n][0], 7, shapes[n][1]) for n in names}
        env._check(env.lib.ongym_spectrum_map(env._h, *(a[n].ctypes.data if n in a else None for n in NAMES)), "ongym_spectrum_map")
        return a
    out["subsets_host"] = subsets_equal(host_call, full)
    rc = env.lib.ongym_spectrum_map(env._h, None, None, None, None)
    out["refuse_all_null"], out["refuse_all_null_msg"] = rc, env.lib.ongym_last_error(env._h).decode()
    out["refuse_null_env"] = env.lib.ongym_spectrum_map(None, None, None, None, full["audit"].ctypes.data)

    dev = make("nsfnet", io_device=True, batch_size=B, **kw)
    blob = env.save_state()
    t = device_tensors(dev)
    try:
        dev.spectrum_map(out=t, records=True)
        out["dev_stream_refused"] = False
    except ValueError as e:
        out["dev_stream_refused"] = "stream" in str(e)

    def run():
        dev.load_state(torch.from_numpy(blob).cuda())

        def dev_call(names):
            a = device_tensors(dev, names)
            dev._check(dev.lib.ongym_spectrum_map(dev._h, *(a[n].data_ptr() if n in a else None for n in NAMES)), "ongym_spectrum_map")
            torch.cuda.current_stream().synchronize()
            return {n: v.cpu().numpy() for n, v in a.items()}
        ok = subsets_equal(dev_call, full)
        bad = []
        for call in (lambda: dev.spectrum_map(records=True),                                           # no out
                     lambda: dev.spectrum_map(out=t),                                                    # keys that were not asked for
                     lambda: dev.spectrum_map(out={"owners": t["owners"]}),                              # a key missing
                     lambda: dev.spectrum_map(out=(t["owners"], t["audit"])),                            # not a dict
                     lambda: dev.spectrum_map(out={"owners": t["owners"].int(), "audit": t["audit"]}),   # dtype
                     lambda: dev.spectrum_map(out={"owners": t["owners"].cpu(), "audit": t["audit"]}),   # a host tensor
                     lambda: dev.spectrum_map(out={"owners": t["owners"][:, :, 1:], "audit": t["audit"]}),   # shape
                     lambda: dev.spectrum_map(out={"audit": full["audit"]}, owners=False),               # numpy
                     lambda: dev.spectrum_map(out={}, owners=False, audit=False)):                       # nothing asked for
            try:
                call()
                bad.append(False)
            except ValueError:
                bad.append(True)
        same_check = np.array_equal(dev.check_state(), full["audit"])
        return ok, np.array(bad + [same_check])
    out["subsets_device"], out["dev_refusals"] = on_device(dev, run)
    for e in (env, twin, dev):
        e.close()


# ---- 4. doctored states ---------------------------------------------------------------------------------------------------
def blob_header(blob):
    """the layout facts of a state blob's 256-byte header (StateHeader, csrc/ongym_state.hpp)"""
    count, block = struct.unpack_from("<qq", blob, 24)
    rec32, track_ids, row_words, n_links, capacity, devenv_bytes, n_sections = struct.unpack_from("<7i", blob, 40)
    assert n_sections == len(SECTIONS)
    sec_bytes = struct.unpack_from("<9q", blob, 80)
    sec_off = struct.unpack_from("<9q", blob, 152)
    return dict(count=count, block=block, rec32=rec32, track_ids=track_ids, W=row_words, E=n_links, C=capacity, devenv=devenv_bytes,
                bytes=dict(zip(SECTIONS, sec_bytes)), off=dict(zip(SECTIONS, sec_off)))


def block_views(blob, h, k):
    """writable views into replica block k of the blob: occ uint64 [E, W], svc_a / svc_b uint32 [C], svc_r float32 [C], svc_q
    uint32 [C] or None, active int32 [1]"""
    base = 256 + k * h["block"]
    view = lambda s, dt, n: np.frombuffer(blob, dt, n, base + h["off"][s])   # noqa: E731
    v = dict(occ=view("occ", np.uint64, h["E"] * h["W"]).reshape(h["E"], h["W"]), svc_a=view("svc_a", np.uint32, h["C"]),
             svc_b=view("svc_b", np.uint32, h["C"]), svc_r=view("svc_r", np.float32, h["C"]),
             svc_q=view("svc_q", np.uint32, h["C"]) if h["bytes"]["svc_q"] else None)
    stats_bytes = nat.STATS_DTYPE.itemsize
    v["active"] = np.frombuffer(blob, np.int32, 1, base + h["off"]["env"] + h["devenv"] - stats_bytes + ACTIVE_IN_STATS)
    return v


def blob_state(tb, M, S, h, v, width):
    """(owners, audit, records, release) restated from the bytes of one replica block"""
    bits = (v["occ"][:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    grid = bits.reshape(h["E"], h["W"] * 64)[:, :S].astype(np.int32)
    fields = decode(h["rec32"], v["svc_a"], v["svc_b"])
    mask_ok = None
    if h["rec32"]:
        mask_ok = np.array([int(a) == route_mask0(tb, int(p)) for a, p in zip(v["svc_a"], fields[:, 0])])
    active = int(v["active"][0])
    owners, audit, bad = restate(tb, M, S, h["C"], grid, fields, active, width, mask_ok)
    ids = v["svc_q"].astype(np.int64).astype(np.int32) if v["svc_q"] is not None else np.full(h["C"], -1, np.int32)
    rec, rel = restate_records(h["C"], fields, ids, v["svc_r"], bad)
    return owners, audit, rec, rel


def set_bit(occ, e, s, free):
    if free:
        occ[e, s >> 6] |= np.uint64(1) << np.uint64(s & 63)
    else:
        occ[e, s >> 6] &= ~(np.uint64(1) << np.uint64(s & 63))


def doctored(out, codec):
    dims, recs, acts = load_cases()
    P, M, S, C = dims[codec]
    r32 = codec == "r32"
    tbname = "nsfnet" if r32 else "nobel-eu"
    tb = golden_tables(tbname)
    assert len(tb.path_hops) == P and len(jocn_modulations()) == M
    rows = [r for r in recs if r[1] == codec]
    # (name, the audit column that must be non-zero or -1, the edit)
    plan = []
    if r32:
        plan += [("claimed_set_free", 4), ("free_cleared", 5), ("idle_row_filled", 7), ("moved_onto_neighbour", 3), ("over_width", 6)]
        plan += [("active_" + a[0], 0 if a[3] else -1) for a in acts]
    plan += [(r[0], -1 if r[7] else 2) for r in rows]
    B = len(plan)
    kw = dict(num_spectrum_resources=S, capacity=C, load=300.0)
    src = make(tbname, batch_size=B, **kw)
    src.seed(3)
    src.reset()
    src.step_policy(16, record=False)                                # a few records: most replicas have an idle link
    width = width_limit(src)
    blob = src.save_state()
    h = blob_header(blob)
    assert (h["count"], bool(h["rec32"]), h["C"], h["E"]) == (B, r32, C, tb.n_links)
    views_same = True
    for r in range(B):
        own, aud, rec, rel = blob_state(tb, M, S, h, block_views(blob, h, r), width)
        w = from_views(tb, M, S, C, src.grid(r), src.services(r), width)
        views_same &= all(np.array_equal(x, y, equal_nan=True) for x, y in zip((own, aud, rec, rel), w)) and aud[0] == 0
    out[f"doc_{codec}_views_same"] = views_same
    src.close()
    by_name = {r[0]: r for r in rows}
    act_by_name = {"active_" + a[0]: a for a in acts}
    for r, (name, _) in enumerate(plan):
        v = block_views(blob, h, r)
        A = int(v["active"][0])
        f = decode(r32, v["svc_a"], v["svc_b"])[:A]
        links = [tb.path_links[p, :tb.path_hops[p]] for p in f[:, 0]]
        assert A >= 4
        if name == "claimed_set_free":
            set_bit(v["occ"], int(links[0][0]), int(f[0, 1]), True)
        elif name == "free_cleared":                                 # a free cell of a link that a record crosses
            e = int(links[0][0])
            s = max(s for s in range(S) if (int(v["occ"][e, s >> 6]) >> (s & 63)) & 1)
            set_bit(v["occ"], e, s, False)
        elif name == "idle_row_filled":
            idle = sorted(set(range(tb.n_links)) - set(int(l) for ls in links for l in ls))
            assert idle, "no idle link in this replica: choose another seed"
            v["occ"][idle[0], :] = 0
        elif name == "moved_onto_neighbour":                         # record j moves onto the range of a record it shares a link with
            i, j = next((i, j) for i in range(A) for j in range(i + 1, A) if set(links[i]) & set(links[j]))
            a, b = pack(r32, int(f[j, 0]), route_mask0(tb, int(f[j, 0])), int(f[i, 1]), int(f[j, 2]), int(f[j, 3]))
            v["svc_a"][j], v["svc_b"][j] = a, b
        elif name == "over_width":
            assert width < 40 and f[0, 1] + 40 <= S
            a, b = pack(r32, int(f[0, 0]), route_mask0(tb, int(f[0, 0])), int(f[0, 1]), 40, int(f[0, 3]))
            v["svc_a"][0], v["svc_b"][0] = a, b
        elif name in act_by_name:
            v["active"][0] = act_by_name[name][1]
        else:
            _, _, path, slot, n, mod, x, _ = by_name[name]
            a, b = pack(r32, path, route_mask0(tb, path) ^ x, slot, n, mod)
            v["svc_a"][1], v["svc_b"][1] = a, b
    want = [blob_state(tb, M, S, h, block_views(blob, h, r), width) for r in range(B)]
    doc = make(tbname, batch_size=B, **kw)
    doc.load_state(blob)
    got = doc.spectrum_map(owners=True, records=True, audit=True)
    try:
        doc.check_state()
        out[f"doc_{codec}_check_state_raises"], out[f"doc_{codec}_check_state_msg"] = False, ""
    except Exception as e:      # OngymError
        out[f"doc_{codec}_check_state_raises"], out[f"doc_{codec}_check_state_msg"] = type(e).__name__ == "OngymError", str(e)
    kept = doc.save_state()
    doc.close()
    out[f"doc_{codec}_blob_kept"] = all(
        np.array_equal(block_views(kept, h, r)[s], block_views(blob, h, r)[s]) for r in range(B) for s in ("occ", "svc_a", "svc_b", "active"))
    for i, n in enumerate(("owners", "audit", "records", "release")):
        out[f"doc_{codec}_{n}"], out[f"doc_{codec}_want_{n}"] = got[n], np.stack([w[i] for w in want])
    out[f"doc_{codec}_names"], out[f"doc_{codec}_column"] = np.array([p[0] for p in plan]), np.array([p[1] for p in plan])


# ---- 5. the single environment --------------------------------------------------------------------------------------------
def compat(out):
    from optical_networking_gym.envs.qrmsa import QRMSAEnv
    from optical_networking_gym.topology import bundled_topology_path, get_topology
    topology = get_topology(bundled_topology_path("nsfnet_chen.txt"), None, jocn_modulations(), 80, 0.2, 4.5, 5)
    kw = dict(seed=9, load=300, episode_length=1000, num_spectrum_resources=320, launch_power_dbm=1.0, margin=0.5,
              bit_rate_selection="discrete", bit_rates=(10, 40, 100, 400), gen_observation=False)
    single = QRMSAEnv(topology=topology, **kw)
    single.reset()
    for _ in range(200):
        single.step(single.first_fit_action()[0])
    S = 320
    want = np.full((topology.number_of_edges(), S), -1, np.int64)
    for svc in topology.graph["running_services"]:
        s, n = svc.initial_slot, svc.number_slots
        for link in svc.path.links:
            want[topology[link.node1][link.node2]["index"], s:min(s + n + 1, S)] = svc.service_id
    out["compat_allocation"], out["compat_want"] = single.spectrum_slots_allocation, want
    single.close()
    topology = get_topology(bundled_topology_path("nsfnet_chen.txt"), None, jocn_modulations(), 80, 0.2, 4.5, 5)
    plain = QRMSAEnv(topology=topology, track_service_ids=False, **kw)
    plain.reset()
    try:
        plain.spectrum_slots_allocation
        out["compat_no_ids_refused"] = False
    except ValueError:
        out["compat_no_ids_refused"] = True
    plain.close()


def main():
    out = {}
    read_only(out)
    for key in DEFINITIONS:
        definition_case(out, key)
        print(key, "done", flush=True)
    after_calls(out)
    compat(out)
    for codec in ("r32", "gen"):
        doctored(out, codec)
        print("doctored", codec, "done", flush=True)
    np.savez(sys.argv[1], **out)
    print("spectrum map child ok")


if __name__ == "__main__":
    main()
