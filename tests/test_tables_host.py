"""The host half of ongym_create (csrc/ongym_tables.hpp: config_check and derive_tables), checked on the CPU through
oracle/libongym_tables.so (oracle/ongym_tables_shim.cpp).  No GPU is involved: ongym_create uploads exactly these tables.
The library and the sanitised program are made here on first use (make -C oracle), as oracle_lib makes the oracle.

1. Integer and structural tables, exact: link masks, slot counts (against the oracle's get_number_slots), req_coef, the three
   layouts of the pair table, the link-weight table behind pair_tab2k, the route -> node-pair map and the two "same route list"
   checks.
2. Floating tables against a numpy fp64 restatement of the formulas (core/osnr.pyx:22-24, 52-55, 58-61, 68-93, 109-125;
   utils.pyx:61-79), relative difference <= 1e-13: libm and numpy each err by a few ulp (2e-16), which leaves two orders of
   magnitude, and the bound sits four orders below the QoT band of 1e-9.  The pair table's first entry is restated in the form
   create uses, log((U + sqrt(U^2 + 1)) / (V + sqrt(V^2 + 1))): asinh(U) - asinh(V) in fp64 cancels (asinh(U) is up to 9, the
   difference down to 3e-3) and is itself 3e-13 off the extended-precision value on NSFNET-320, so it cannot referee 1e-13.
3. ase_shortcut: 1 for every golden configuration; 0 for a configuration found here by stepping.  config_check derives a format's
   Phi from its spectral efficiency, so no configuration scales mod_phi53 alone: what the scan compares is
   mod_phi53 * l_eff / L, and the span length scales that (shorter spans: l_eff / L -> 1, and Phi * 5/3 > 1).
4. config_check: every refusal with its code and message, and the first of two violations is the one reported.
5. What lean eligibility is fed: max_n and rec32.
6. The same code as a stand-alone program on a built-in configuration, under AddressSanitizer + UBSan, exits 0.
"""
import copy
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from common import golden_tables, jocn_modulations
from optical_networking_gym._native import ConfigHolder, OngymConfig, CSRC_DIR
from oracle_lib import ORACLE_DIR, OracleEnv

E_ARG, E_LIMIT = -1, -5
RTOL = 1e-13
RATES = (10, 40, 100, 400)
with open(os.path.join(CSRC_DIR, "ongym_fast.hpp")) as _f:
    PITCH = int(re.search(r"constexpr int kTabPitch = (\d+);", _f.read()).group(1))

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", ORACLE_DIR, "libongym_tables.so"], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(ORACLE_DIR, "libongym_tables.so"))
        vp = C.c_void_p
        L.ogt_create.argtypes = [C.POINTER(OngymConfig), C.c_int, C.c_int, C.c_int, C.c_int]
        L.ogt_create.restype = vp
        L.ogt_destroy.argtypes = [vp]
        L.ogt_destroy.restype = None
        L.ogt_check_code.argtypes = [vp]
        L.ogt_check_msg.argtypes = [vp]
        L.ogt_check_msg.restype = C.c_char_p
        L.ogt_table.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.ogt_scalar.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double)]
        L.ogt_text.argtypes = [vp, C.c_char_p]
        L.ogt_text.restype = C.c_char_p
        _lib = L
    return _lib


DTYPES = dict(path_mask="<u8", mod_se="<i4", nreq_tab="<i4", lw_mult="<u4", lw_loc="<u4", path_pair="<i4")   # the others: f8


class Tables:
    """config_check's verdict and, if it passed, a copy of every table and scalar of HostTables."""

    def __init__(self, holder, no_lwtab=False):
        L = lib()
        h = L.ogt_create(C.byref(holder.struct), 0, 0, int(no_lwtab), PITCH)
        try:
            self.code, self.msg = L.ogt_check_code(h), L.ogt_check_msg(h).decode()
            if self.code:
                return
            for name in ("w1 w2 cl selfc path_mask path_ase path_w1 nli_coef self_asinh mod_se mod_thr mod_phi53 nreq_tab "
                         "req_coef plogp pair_tab pair_tab2k pair_tabp lw_mult lw_loc path_pair").split():
                p, n = C.c_void_p(), C.c_size_t()
                assert L.ogt_table(h, name.encode(), C.byref(p), C.byref(n)) == 0, name
                setattr(self, name, np.frombuffer(C.string_at(p.value, n.value) if n.value else b"", DTYPES.get(name, "<f8")))
            for name in "uniform ase_shortcut rec32 nslots_width tab_nmax tab_stride lw_tab_off lw_tab_bytes max_n".split():
                v = C.c_double()
                assert L.ogt_scalar(h, name.encode(), C.byref(v)) == 0, name
                setattr(self, name, v.value if name == "nslots_width" else int(v.value))
            self.path_pair_err = L.ogt_text(h, b"path_pair_err").decode()
            self.admission_pair_err = L.ogt_text(h, b"admission_pair_err").decode()
        finally:
            L.ogt_destroy(h)


def holder(topology="nsfnet", S=320, rates=RATES, selection="discrete", **kw):
    """On a private copy of the golden tables: ConfigHolder keeps the arrays it is given, and some tests edit them."""
    return ConfigHolder(copy.deepcopy(golden_tables(topology)), modulations=jocn_modulations(), num_spectrum_resources=S, load=300.0,
                        bit_rate_selection=selection, bit_rates=rates, **kw)


def nonuniform():
    h = holder()
    h._keep["link_alpha"][3] *= 1.01
    return h


CASES = {
    "nsfnet320": lambda: (holder(), False),
    "nobeleu320": lambda: (holder("nobel-eu"), False),
    "cost239_320": lambda: (holder("cost239"), False),
    "ring4_64": lambda: (holder("ring4", 64), False),
    "nsfnet70": lambda: (holder(S=70), False),
    "nsfnet_continuous": lambda: (holder(selection="continuous"), False),
    "nsfnet_nonuniform": lambda: (nonuniform(), False),
    "nsfnet_1t": lambda: (holder(rates=RATES + (1000,)), False),
    "nsfnet_no_lwtab": lambda: (holder(), True),
}
_made = {}


@pytest.fixture(params=list(CASES))
def case(request):
    """(holder, Tables) of one configuration; derived once, shared by the tests, never changed."""
    if request.param not in _made:
        h, no_lwtab = CASES[request.param]()
        t = Tables(h, no_lwtab)
        assert (t.code, t.msg) == (0, "")
        _made[request.param] = (h, t)
    return (request.param,) + _made[request.param]


def bits(a):
    return np.ascontiguousarray(a, "<f8").view("<u8")


def close(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape
    err = np.abs(got - want)
    worst = float(np.max(err / np.where(want == 0, 1.0, np.abs(want)), initial=0.0))
    assert (err <= RTOL * np.abs(want)).all(), worst
    return worst


# ---- 1. integer and structural tables ---------------------------------------------------------------------------------------
def test_path_mask_and_path_pair(case):
    _, h, t = case
    tb, c = h.tables, h.struct
    want = np.zeros((tb.n_paths, 2), np.uint64)
    for p in range(tb.n_paths):
        for l in tb.path_links[p, :tb.path_hops[p]]:
            want[p, int(l) >> 6] |= np.uint64(1 << (int(l) & 63))
    assert np.array_equal(t.path_mask.reshape(-1, 2), want)
    pair = np.full(tb.n_paths, -1, np.int64)
    flat = tb.pair_paths.reshape(c.n_nodes * c.n_nodes, c.k_paths)
    for pr in range(len(flat) - 1, -1, -1):                 # descending: the lowest pair that lists a route is written last
        pair[flat[pr][flat[pr] >= 0]] = pr
    assert np.array_equal(t.path_pair, pair)
    assert t.path_pair_err == "" and t.admission_pair_err == ""


def test_nreq_tab_and_req_coef(case):
    name, h, t = case
    c = h.struct
    want = np.zeros((max(c.n_bit_rates, 1), 8), np.int32)
    if c.bit_rate_mode == 0:
        o = OracleEnv(h)
        for b, rate in enumerate(h.bit_rates):
            for m in range(c.n_mods):
                want[b, m] = o.number_slots(float(rate), m)
        assert want.max() > 0
    else:
        assert name == "nsfnet_continuous" and c.n_bit_rates == 1
    assert np.array_equal(t.nreq_tab.reshape(-1, 8), want)
    coef = np.zeros((want.size, 2))
    n = want.reshape(-1)
    ok = (n >= 1) & (n <= c.n_slots)
    coef[ok, 0], coef[ok, 1] = t.nli_coef[n[ok]], t.self_asinh[n[ok]]
    assert np.array_equal(bits(t.req_coef.reshape(-1, 2)), bits(coef))
    assert t.max_n == (min(int(want.max()), c.n_slots) if c.bit_rate_mode == 0 else 0)


def test_pair_table_layouts(case):
    name, h, t = case
    S = h.struct.n_slots
    assert t.tab_stride == 2 * S + 1
    if name == "nsfnet_nonuniform":
        assert not t.uniform and t.tab_nmax == 0
        assert len(t.pair_tab) == len(t.pair_tab2k) == len(t.pair_tabp) == 0 and t.lw_tab_bytes == 0 and len(t.lw_mult) == 0
        return
    assert t.uniform and t.tab_nmax >= 1
    pt = bits(t.pair_tab).reshape(t.tab_nmax, t.tab_stride, 2)
    d = np.arange(t.tab_stride)
    for nk in range(1, t.tab_nmax + 1):
        assert not pt[nk - 1, :nk + 1].any()                # d <= nk: exactly (0, 0)
        assert pt[nk - 1, nk + 1:].all()
    rows = t.tab_nmax * PITCH
    t2 = bits(t.pair_tab2k[:rows * 2]).reshape(t.tab_nmax, PITCH, 2)
    want = np.zeros_like(t2)
    want[:, d] = pt
    assert np.array_equal(t2, want)
    tp = bits(t.pair_tabp).reshape(t.tab_nmax, PITCH, 2)
    want = np.zeros_like(tp)
    want[:, (d & 1) * (PITCH // 2) + (d >> 1)] = pt
    assert np.array_equal(tp, want)
    assert len(t.pair_tab2k) * 8 == rows * 16 + t.lw_tab_bytes
    assert t.lw_tab_off == (rows * 16 if t.lw_tab_bytes else 0)


def test_link_weight_table(case):
    name, h, t = case
    tb = h.tables
    if name in ("nobeleu320", "nsfnet_nonuniform", "nsfnet_no_lwtab"):      # two mask words / no pair table / switched off
        assert t.lw_tab_bytes == 0 and len(t.lw_mult) == 0 and len(t.lw_loc) == 0
        return
    assert t.rec32 and t.lw_tab_bytes > 0 and t.lw_tab_off % 32 == 0 and len(t.lw_mult) == len(t.lw_loc) == tb.n_paths
    blob = t.pair_tab2k
    end = t.lw_tab_off + t.lw_tab_bytes
    w1, w2 = t.w1.tolist(), t.w2.tolist()
    for p in range(tb.n_paths):
        links = sorted(int(l) for l in tb.path_links[p, :tb.path_hops[p]])
        mask, mult, loc = int(t.path_mask[2 * p]), int(t.lw_mult[p]), int(t.lw_loc[p])
        assert mult & 1 and mask == sum(1 << l for l in links)
        seen = set()
        for sub in range(1 << len(links)):
            chosen = [l for i, l in enumerate(links) if sub >> i & 1]
            x = sum(1 << l for l in chosen) | (~mask & 0xFFFFFFFF)          # links off the route do not matter
            idx = (((x & mask) * mult) & 0xFFFFFFFF) >> (loc & 31)          # lw_index, ongym_lwtab.hpp
            at = (loc & ~31) + 16 * idx
            assert t.lw_tab_off <= at and at + 16 <= end
            a = b = 0.0
            for l in chosen:                                                 # ascending links, plain adds from 0.0
                a, b = a + w1[l], b + w2[l]
            assert (blob[at // 8], blob[at // 8 + 1]) == (a, b), (p, chosen)
            seen.add(idx)
        assert len(seen) == 1 << len(links)


def _nsfnet_pairs(edit):
    h = holder(S=64)
    pp = h._keep["pair_paths"].reshape(h.struct.n_nodes, h.struct.n_nodes, h.struct.k_paths)
    assert h.struct.k_paths >= 2
    edit(pp)
    t = Tables(h)
    assert t.code == 0
    return h.struct.n_nodes, t


def test_route_listed_by_two_pairs_with_different_lists():
    def edit(pp):
        pp[0, 2, 0] = pp[2, 0, 0] = pp[0, 1, 0]
    route = int(golden_tables("nsfnet").pair_paths[0, 1, 0])
    _, t = _nsfnet_pairs(edit)
    assert t.path_pair_err == (f"route {route} is listed by node pairs 1 and 2 with different route lists: "
                               "no node pair for failure impact")
    assert t.admission_pair_err == ""


def test_pair_whose_directions_differ():
    def edit(pp):
        pp[0, 1, [0, 1]] = pp[0, 1, [1, 0]]
    _, t = _nsfnet_pairs(edit)
    assert t.admission_pair_err == ("node pair (0, 1) lists different routes in its two directions: "
                                    "no unordered pair for the admission map")
    assert t.path_pair_err.endswith("with different route lists: no node pair for failure impact")


# ---- 2. floating tables against numpy fp64 ----------------------------------------------------------------------------------
PI, BETA2, H_PLANCK, GAMMA = 3.14159265358979323846, 21.3e-27, 6.626e-34, 1.3e-3
PHI = np.array([1.0, 1.0, 2.0 / 3.0, 17.0 / 25.0, 69.0 / 100.0, 13.0 / 21.0])


def test_link_path_and_slot_tables(case):
    _, h, t = case
    tb, c = h.tables, h.struct
    a, L, ns = h._keep["link_alpha"], h._keep["link_span_km"], h._keep["link_nspans"].astype(float)
    l_eff = (1.0 - np.exp(-2.0 * a * L * 1e3)) / (2.0 * a)
    w1 = ns * l_eff
    ase = ns * H_PLANCK * (np.exp(2.0 * a * L * 1e3) - 1.0) * h._keep["link_nf"]
    close(t.w1, w1)
    close(t.w2, ns * l_eff * (l_eff / (L * 1e3)))
    close(t.cl, PI * PI * BETA2 * (1.0 / (2.0 * a)))
    close(t.selfc, PI * PI * BETA2 / (4.0 * a))
    routes = [tb.path_links[p, :tb.path_hops[p]] for p in range(tb.n_paths)]
    close(t.path_ase, [math.fsum(ase[r]) for r in routes])
    close(t.path_w1, [math.fsum(w1[r]) for r in routes])
    n = np.arange(c.n_slots + 2, dtype=float)
    bwn = c.slot_bandwidth * n
    nli = np.zeros(c.n_slots + 2)
    nli[1:] = (8.0 / (27.0 * PI * BETA2)) * (GAMMA * GAMMA) / (bwn[1:] * bwn[1:])
    close(t.nli_coef, nli)
    close(t.self_asinh, np.arcsinh(PI * PI * BETA2 / (4.0 * a[0]) * (bwn * bwn)))
    assert np.array_equal(t.mod_se, h.mod_se) and np.array_equal(bits(t.mod_thr), bits(h.mod_thr))
    close(t.mod_phi53, PHI[h.mod_se - 1] * (5.0 / 3.0))
    pr = np.arange(1, c.n_slots + 1) / c.n_slots
    close(t.plogp, np.concatenate([[0.0], pr * np.log(pr)]))


def test_pair_table_values(case):
    name, h, t = case
    if not t.uniform:
        return
    c = h.struct
    rate = max(h.bit_rates) if c.bit_rate_mode == 0 else c.bit_rate_hi
    assert t.tab_nmax == max(1, min(math.ceil(rate / (1 * 12.5)), c.n_slots))       # BPSK at 12.5 GHz is the widest format
    nk = np.arange(1, t.tab_nmax + 1, dtype=float)[:, None]
    d = np.arange(t.tab_stride, dtype=float)[None, :]
    bk = c.slot_bandwidth * nk
    ck = (PI * PI * BETA2 * (1.0 / (2.0 * h._keep["link_alpha"][0]))) * bk
    adf = np.broadcast_to((0.5 * c.slot_bandwidth) * d, (t.tab_nmax, t.tab_stride))
    U, V = ck * (adf + 0.5 * bk), ck * (adf - 0.5 * bk)
    live = d > nk
    with np.errstate(all="ignore"):
        x = np.where(live, np.log((U + np.sqrt(U * U + 1.0)) / (V + np.sqrt(V * V + 1.0))), 0.0)
        y = np.where(live, bk / adf, 0.0)
    got = t.pair_tab.reshape(t.tab_nmax, t.tab_stride, 2)
    print(f"{name}: pair table worst relative difference {close(got[..., 0], x):.3g} (asinh difference), "
          f"{close(got[..., 1], y):.3g} (Bk / |df|)")


# ---- 3. ase_shortcut --------------------------------------------------------------------------------------------------------
def test_ase_shortcut_holds_on_the_golden_configurations(case):
    assert case[2].ase_shortcut == 1


def test_ase_shortcut_breaks_when_an_interferer_term_turns_negative():
    h = holder("ring4", 64)
    span = h._keep["link_span_km"]
    base = span.copy()
    verdicts = []
    for step in range(12):                                  # spans of 1, 1/2, 1/4, ... of the golden length
        span[:] = base / 2 ** step
        verdicts.append(Tables(h).ase_shortcut)
        if not verdicts[-1]:
            break
    assert verdicts[0] == 1 and verdicts[-1] == 0, verdicts
    # the broken configuration's own numbers: some term asinh(U) - asinh(V) - Phi 5/3 (Bk / |df|) (l_eff / L) is <= 0
    t = Tables(h)
    ratio = t.w2 / t.w1
    pt = t.pair_tab.reshape(t.tab_nmax, t.tab_stride, 2)
    terms = pt[..., 0][None] - (t.mod_phi53[:, None, None] * ratio.max()) * pt[..., 1][None]
    live = np.arange(t.tab_stride)[None, :] > np.arange(1, t.tab_nmax + 1)[:, None]
    assert (terms[:, live] <= 0).any()
    print(f"ase_shortcut breaks at spans of 1/{2 ** (len(verdicts) - 1)} of ring4's: l_eff / L = {ratio.max():.3f}")


# ---- 4. config_check --------------------------------------------------------------------------------------------------------
def _set(field, value):
    return lambda h: setattr(h.struct, field, value)


def _poke(table, index, value):
    def f(h):
        h._keep[table].reshape(-1)[index] = value
    return f


REFUSALS = [
    (_set("n_nodes", 1), E_ARG, "non-positive size in ongym_config"),
    (_set("episode_length", 1), E_ARG, "non-positive size in ongym_config"),
    (_set("n_mods", 9), E_LIMIT, "n_mods > 8"),
    (_set("n_links", 129), E_LIMIT, "n_links > 128"),
    (_set("max_hops", 65), E_LIMIT, "max_hops > 64"),
    (_set("n_slots", 1024), E_LIMIT, "n_slots > 1023"),
    (_set("n_paths", 65536), E_LIMIT, "n_paths > 65535"),
    (_set("capacity", 100), E_ARG, "capacity must be a multiple of 64 in (0, 65535)"),
    (_set("capacity", 65536), E_ARG, "capacity must be a multiple of 64 in (0, 65535)"),
    (_set("node_cum", None), E_ARG, "null table pointer in ongym_config"),
    (_set("n_bit_rates", 0), E_ARG, "discrete bit-rate mode needs bit_rates/bit_rate_cum"),
    (_set("bit_rate_cum", None), E_ARG, "discrete bit-rate mode needs bit_rates/bit_rate_cum"),
    (_set("load", 0.0), E_ARG, "load and mean_holding_time must be positive"),
    (_poke("pair_paths", 7, -2), E_ARG, "pair_paths entry out of range"),
    (lambda h: _poke("pair_paths", 7, h.struct.n_paths)(h), E_ARG, "pair_paths entry out of range"),
    (_poke("path_hops", 3, 0), E_ARG, "path_hops entry out of range"),
    (lambda h: _poke("path_links", 0, h.struct.n_links)(h), E_ARG, "path_links entry out of range"),
    (_poke("mod_se", 2, 7), E_ARG, "spectral efficiency must be 1..6"),
    (_poke("link_alpha", 5, 0.0), E_ARG, "link span parameters must be positive"),
    (_poke("link_nspans", 5, 0), E_ARG, "link span parameters must be positive"),
    (lambda h: (_set("defragmentation", 1)(h), _set("n_defrag_services", -1)(h)), E_ARG, "n_defrag_services must be >= 0"),
    (lambda h: (_set("measure_disruptions", 1)(h), _poke("link_alpha", 3, 5e-5)(h)), E_LIMIT,
     "measure_disruptions needs uniform attenuation"),
    (lambda h: (_set("defragmentation", 1)(h), _poke("link_alpha", 3, 5e-5)(h)), E_LIMIT, "defragmentation needs uniform attenuation"),
    (lambda h: (_set("track_service_ids", 1)(h), _poke("link_alpha", 3, 5e-5)(h)), E_LIMIT,
     "track_service_ids needs uniform attenuation"),
    (_poke("rload", 2, 0.0), E_ARG, "per-replica load / launch power must be positive"),
    (_poke("rlp", 3, -1.0), E_ARG, "per-replica load / launch power must be positive"),
]


def _replicas():
    return holder(S=64, batch=4, replica_load=[100.0, 200.0, 300.0, 400.0], replica_launch_power_dbm=[0.0, 1.0, 2.0, 3.0])


@pytest.mark.parametrize("edit,code,msg", REFUSALS, ids=[f"{i}-{r[2][:28].replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_config_check_refuses(edit, code, msg):
    h = _replicas()
    assert Tables(h).code == 0
    edit(h)
    t = Tables(h)
    assert (t.code, t.msg) == (code, msg)


def test_config_check_reports_the_first_failure():
    h = _replicas()
    _poke("mod_se", 2, 7)(h)                                # a table check ...
    _poke("rload", 2, 0.0)(h)                               # ... and the last check of all
    t = Tables(h)
    assert (t.code, t.msg) == (E_ARG, "spectral efficiency must be 1..6")
    h.struct.capacity = 100                                 # ... and one before both
    t = Tables(h)
    assert (t.code, t.msg) == (E_ARG, "capacity must be a multiple of 64 in (0, 65535)")


# ---- 5. what lean eligibility is fed -----------------------------------------------------------------------------------------
def test_max_n_and_rec32(case):
    name, h, t = case
    if name == "nsfnet_1t":
        assert t.max_n == 80                                # 1 Tb/s BPSK at 12.5 GHz: the wide build
    elif name == "nsfnet_continuous":
        assert t.max_n == 0
    else:
        assert t.max_n == 32                                # 400 Gb/s BPSK at 12.5 GHz: the narrow build
    assert t.rec32 == (name != "nobeleu320")
    assert h.tables.n_links > 32 if name == "nobeleu320" else h.tables.n_links <= 32


# ---- 6. the stand-alone program under AddressSanitizer + UBSan ---------------------------------------------------------------
def test_standalone_program_is_clean_under_sanitizers():
    subprocess.run(["make", "-C", ORACLE_DIR, "tables_asan"], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ORACLE_DIR, "ongym_tables_asan")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ongym_tables: 30 routes")
