"""The spectrum map on device (ongym_spectrum_map through BatchedQRMSAEnv.spectrum_map, decode_owners, check_state and
QRMSAEnv.spectrum_slots_allocation).  Every GPU computation runs in ONE fresh child process (tests/spectrum_map_child.py);
the tests assert on the .npz it writes.

This module also holds the restatement of the call's definitions (include/ongym.h) in plain numpy, `restate` and
`restate_records`, which tests/test_spectrum_map_host.py checks on hand-made cases and on CPU-oracle states.  The device is
held to it exactly: every output is an integer or a copy of a float32.  The expected arrays of every replica are built from
that replica's own grid(r) and services(r) (the doctored states: from the doctored blob, whose undoctored decoding is first
shown to equal grid(r) and services(r))."""
import os
import subprocess
import sys

import numpy as np
import pytest

from optical_networking_gym import _native as nat

HERE = os.path.dirname(os.path.abspath(__file__))
CASES_FILE = os.path.join(HERE, "spectrum_cases.txt")
AUDIT = {k: i for i, k in enumerate(nat.SPECTRUM_AUDIT_COLUMNS)}
DEFINITION_CASES = ("ring4", "nsfnet320", "nsfnet100", "nobeleu320", "germany100", "ids", "defrag")
AFTER_CALLS = ("cut", "cut_no_restore", "repair", "move", "defragment", "load", "fork", "auto_reset")


# ---- the restatement ------------------------------------------------------------------------------------------------------
def pack(r32, path, mask0, slot, n, mod):
    """the two stored words of a record (rec_pack, csrc/ongym_device.hpp)"""
    if r32:
        return int(mask0) & 0xFFFFFFFF, (slot | n << 10 | mod << 20 | path << 23) & 0xFFFFFFFF
    return (path | slot << 16) & 0xFFFFFFFF, (n | mod << 16) & 0xFFFFFFFF


def decode(r32, a, b):
    """int64 [n, 4] (path, slot, nslots, modulation) of the stored words a, b (uint32 arrays)"""
    a, b = np.asarray(a, np.uint32).astype(np.int64), np.asarray(b, np.uint32).astype(np.int64)
    if r32:
        return np.stack([b >> 23, b & 0x3FF, (b >> 10) & 0x3FF, (b >> 20) & 0x7], axis=1)
    return np.stack([a & 0xFFFF, a >> 16, b & 0xFFFF, (b >> 16) & 0xFF], axis=1)


def route_mask0(tb, path):
    """the low 32 bits of the link mask of route `path`; 0 where `path` is no route"""
    if not 0 <= path < len(tb.path_hops):
        return 0
    return sum(1 << int(l) for l in tb.path_links[path, :tb.path_hops[path]] if l < 32)


def restate(tb, M, S, C, grid, fields, stored_active, width, mask_ok=None):
    """(owners int16 [E, S], audit int32 [10], malformed bool [A]) of one replica by the definitions of ongym_spectrum_map:
    grid [E, S] with 1 = free, fields [>= A, 4] = (path, slot, nslots, modulation) as decoded from the stored words,
    stored_active the replica's `active`, width the width limit, mask_ok [>= A] the R32 mask test (None: it holds)"""
    E, P = tb.n_links, len(tb.path_hops)
    grid = np.asarray(grid)
    A = min(max(int(stored_active), 0), C)
    claims = np.zeros((E, S), np.int64)
    owners = np.where(grid != 0, nat.OWNER_FREE, nat.OWNER_UNOWNED).astype(np.int64)
    crossed, malformed, over = np.zeros(E, bool), np.zeros(A, bool), 0
    for i in range(A - 1, -1, -1):                                   # descending: the lowest index is written last and stays
        p, s, n, m = (int(x) for x in fields[i])
        ok = 0 <= p < P and n >= 1 and s + n <= S and m < M and (mask_ok is None or bool(mask_ok[i]))
        malformed[i] = not ok
        if not ok:
            continue
        over += n > width
        links = tb.path_links[p, :tb.path_hops[p]]
        crossed[links] = True
        claims[links, s:s + n] += 1
        owners[links, s:s + n] = i
        if s + n < S:
            claims[links, s + n] += 1
            owners[links, s + n] = nat.OWNER_GUARD_BASE - i
    failed = np.all(grid == 0, axis=1) & ~crossed
    a = np.zeros(len(AUDIT), np.int64)
    a[1], a[2], a[6], a[7] = A, malformed.sum(), over, failed.sum()
    a[3] = np.sum(claims >= 2)
    a[4] = np.sum((claims >= 1) & (grid != 0))
    a[5] = np.sum((claims == 0) & (grid == 0) & ~failed[:, None])
    a[8], a[9] = np.sum(claims >= 1), np.sum(grid == 0)
    a[0] = int(A != int(stored_active)) | sum(int(a[c] != 0) << (c - 1) for c in range(2, 7))
    return owners.astype(np.int16), a.astype(np.int32), malformed


def restate_records(C, fields, service_id, release, malformed):
    """(records int32 [C, 6], release float32 [C]) from the A decoded records: release carries the stored sign"""
    A = len(malformed)
    rec, rel = np.full((C, 6), -1, np.int32), np.full(C, np.nan, np.float32)
    rec[:A, :4] = np.asarray(fields)[:A]
    rec[:A, 4] = service_id[:A]
    release = np.asarray(release, np.float32)[:A]
    rec[:A, 5] = (release < 0) * nat.SPECTRUM_DISRUPTED + malformed * nat.SPECTRUM_MALFORMED
    rel[:A] = np.abs(release)
    return rec, rel


def from_views(tb, M, S, C, grid, svcs, width):
    """(owners, audit, records, release) of a replica from its grid() and services() views"""
    fields = np.stack([svcs[f].astype(np.int64) for f in ("path_id", "slot", "nslots", "modulation")], axis=1).reshape(-1, 4)
    owners, audit, bad = restate(tb, M, S, C, grid, fields, len(svcs), width)
    signed = np.where(svcs["reserved"] != 0, -1.0, 1.0).astype(np.float32) * svcs["release_time"]
    rec, rel = restate_records(C, fields, svcs["service_id"], signed, bad)
    return owners, audit, rec, rel


def decode_owners_restated(owners):
    o = owners.astype(np.int64)
    kind = np.where(o >= 0, 1, np.where(o == -1, 0, np.where(o == -32768, 3, 2)))
    return np.where(kind == 1, o, np.where(kind == 2, -2 - o, -1)), kind


def load_cases(path=CASES_FILE):
    """(dims {codec: (P, M, S, C)}, records [(name, codec, path, slot, n, mod, maskxor, ok)], actives [(name, active, A, violation)])"""
    dims, recs, acts = {}, [], []
    for line in open(path):
        t = line.split()
        if not t or t[0].startswith("#"):
            continue
        if t[0] == "dims":
            dims[t[1]] = tuple(int(x) for x in t[2:6])
        elif t[0] == "rec":
            recs.append((t[1], t[2]) + tuple(int(x) for x in t[3:7]) + (int(t[7], 16), t[8] == "ok"))
        elif t[0] == "act":
            acts.append((t[1], int(t[2]), int(t[3]), int(t[4])))
        else:
            raise ValueError(line)
    return dims, recs, acts


# ---- the GPU tests --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def res(tmp_path_factory):
    path = tmp_path_factory.mktemp("spectrum_map") / "out.npz"
    child = os.path.join(HERE, "spectrum_map_child.py")
    run = subprocess.run([sys.executable, child, str(path)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "spectrum map child ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    return dict(np.load(path, allow_pickle=False))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def check_against_views(res, k, want_records=True):
    """the four arrays of call `k` against the child's restatement from every replica's own views"""
    for name in ("owners", "audit") + (("records", "release") if want_records else ()):
        got, want = res[f"{k}_{name}"], res[f"{k}_want_{name}"]
        assert same(got, want), (k, name, np.argwhere(got != want)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("io", ("host", "device"))
@pytest.mark.parametrize("key", DEFINITION_CASES)
def test_definition_states(res, key, io):
    """1: owners, records, release and audit of all replicas equal the restatement; no violation; the column identity"""
    k = f"def_{key}_{io}"
    check_against_views(res, k)
    audit = res[k + "_audit"]
    assert audit.shape[0] == 8 and np.all(audit[:, 0] == 0), audit
    assert np.array_equal(audit[:, 9], audit[:, 8] + int(res[k + "_S"]) * audit[:, 7])
    assert np.all(audit[:, 1] > 0) and np.all(audit[:, 8] > 0)
    rec, kind = decode_owners_restated(res[k + "_owners"])
    assert np.array_equal(res[k + "_dec_record"], rec) and np.array_equal(res[k + "_dec_kind"], kind)
    assert np.any(kind == 1) and np.any(kind == 2) and np.any(kind == 0) and not np.any(kind == 3)
    assert bool(res[k + "_rec32"]) == (key not in ("nobeleu320", "germany100"))
    if key in ("ring4", "nsfnet100"):
        assert int(res[k + "_ends_at_S"]) > 0                      # a service without a guard slot
    if key in ("ids", "defrag"):
        assert np.all(res[k + "_records"][:, 0, 4] >= 0)
    else:
        assert np.all(res[k + "_records"][:, :, 4] == -1)
    print(k, "records", audit[:, 1].tolist(), "claimed cells", audit[:, 8].tolist())


@pytest.mark.gpu
def test_both_step_kernels_and_external_actions_were_used(res):
    assert res["def_nsfnet320_lean"] and not res["def_nobeleu320_lean_generic_policy"]
    assert int(res["def_nsfnet320_external_accepted"]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("what", AFTER_CALLS)
def test_after_every_state_changing_call(res, what):
    """2: NSFNET-320, B = 16: no violation after the call, everything as restated"""
    k = "after_" + what
    check_against_views(res, k)
    audit = res[k + "_audit"]
    assert audit.shape[0] == 16 and np.all(audit[:, 0] == 0), audit
    assert np.array_equal(audit[:, 9], audit[:, 8] + 320 * audit[:, 7])
    assert np.array_equal(res[k + "_check_state"], audit)
    failed = res[k + "_failed"]
    count = np.array([bin(int(w[0])).count("1") + bin(int(w[1])).count("1") for w in failed])
    assert np.array_equal(audit[:, 7], count)
    if what in ("cut", "cut_no_restore", "load", "fork"):
        assert count.sum() > 0
        for r in range(16):
            for e in range(res[k + "_owners"].shape[1]):
                if (int(failed[r][e >> 6]) >> (e & 63)) & 1:
                    assert np.all(res[k + "_owners"][r, e] == nat.OWNER_UNOWNED)
    if what in ("repair", "auto_reset"):
        assert count.sum() == 0
    if what in ("move", "defragment"):
        assert int(res[k + "_moved"]) > 0
    if what == "auto_reset":
        assert np.all(res[k + "_episodes"] >= 1)


@pytest.mark.gpu
def test_the_call_is_read_only(res):
    """3"""
    assert res["ro_blob_same"] and res["ro_stats_same"] and res["ro_twin_records_same"]


@pytest.mark.gpu
def test_every_output_subset_equals_the_full_call(res):
    """3: the fifteen non-empty subsets of the four pointers, on a host and on an io_device environment"""
    assert res["subsets_host"].shape == (15,) and np.all(res["subsets_host"])
    assert res["subsets_device"].shape == (15,) and np.all(res["subsets_device"])


@pytest.mark.gpu
def test_library_and_wrapper_refusals(res):
    assert int(res["refuse_all_null"]) == -1 and "nothing to compute" in str(res["refuse_all_null_msg"])
    assert int(res["refuse_null_env"]) == -1
    assert np.all(res["dev_refusals"]) and res["dev_stream_refused"]
    assert res["last_kernel_ms"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ("r32", "gen"))
def test_doctored_states(res, codec):
    """4: one doctoring per replica of a saved state, loaded into a second environment on which only spectrum_map, save_state
    and close are called.  tests/test_spectrum_map_host.py passes the same values through the shared header under the
    sanitizers first; the kernel is defined on them."""
    k = "doc_" + codec
    assert res[k + "_views_same"]                                    # the undoctored blob decodes to grid() and services()
    assert res[k + "_blob_kept"]                                     # the doctored environment still holds the doctored bytes
    names, column = [str(x) for x in res[k + "_names"]], res[k + "_column"]
    audit, want = res[k + "_audit"], res[k + "_want_audit"]
    assert len(names) == audit.shape[0] >= 8
    for r, name in enumerate(names):
        assert np.array_equal(audit[r], want[r]), (name, audit[r], want[r])
        if column[r] >= 0:
            assert audit[r, column[r]] != 0 and (audit[r, 0] != 0 or column[r] == 7), (name, audit[r])
    for name in ("owners", "records", "release"):
        assert same(res[f"{k}_{name}"], res[f"{k}_want_{name}"]), name
    dims, recs, acts = load_cases()
    bad = [n for n, c, *_, ok in recs if c == codec and not ok]
    assert set(bad) <= set(names)
    for n, c, *_, ok in recs:
        if c == codec:                                               # the table's verdict on the record the row replaced
            assert (audit[names.index(n), 2] == 0) == ok, n
    if codec == "r32":
        assert {"claimed_set_free", "free_cleared", "idle_row_filled", "moved_onto_neighbour", "over_width"} <= set(names)
        assert {"active_" + n for n, *_ in acts} <= set(names)
    assert res[k + "_check_state_raises"]


@pytest.mark.gpu
def test_spectrum_slots_allocation_of_the_single_environment(res):
    """5: after 200 steps, against the map built from topology.graph["running_services"]"""
    got, want = res["compat_allocation"], res["compat_want"]
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    assert np.sum(got >= 0) > 0 and res["compat_no_ids_refused"]


@pytest.mark.gpu
def test_check_state_reports_the_first_offender(res):
    msg = str(res["doc_r32_check_state_msg"])
    assert "replica 0" in msg and "claimed_free_cells" in msg
