// ongym_tables.hpp — what ongym_create derives from an ongym_config before it touches the device: the argument checks and
// every table the kernels read, in fp64.  build() (ongym_hip.hip) uploads the tables in a fixed order;
// oracle/ongym_tables_shim.cpp hands them to the host tests.
// Plain C++ (no HIP), so that it can be compiled and checked on its own.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ongym.h"
#include "ongym_lwtab.hpp"

namespace ongym {

// Limits of the kernels (ongym_device.hpp holds the same values as kMaxMods, kMaxLinks, kMaxHops; ongym_hip.hip asserts it).
// kCfgMaxMods is also the row pitch of nreq_tab.
constexpr int kCfgMaxMods = 8, kCfgMaxLinks = 128, kCfgMaxHops = 64;

// Measurement knobs of create, read from the environment once (read_knobs, ongym_hip.hip)
struct CreateKnobs {
    bool force_generic = false;   // ONGYM_FORCE_GENERIC=1: no lean kernel
    bool force_wide = false;      // ONGYM_FORCE_WIDE=1: the wide build of the lean kernels
    bool no_lwtab = false;        // ONGYM_FAST_NO_LWTAB=1: no shared-link weight table behind pair_tab2k
};

inline int cfg_fail(std::string &msg, const char *text, int code = ONGYM_E_ARG) {
    msg = text;
    return code;
}

inline int check_sizes(const ongym_config *c, std::string &msg) {
    if (c->n_nodes <= 1 || c->n_links <= 0 || c->n_paths <= 0 || c->k_paths <= 0 || c->max_hops <= 0 ||
        c->n_mods <= 0 || c->n_slots <= 0 || c->batch <= 0 || c->episode_length <= 1)
        return cfg_fail(msg, "non-positive size in ongym_config");
    if (c->n_mods > kCfgMaxMods) return cfg_fail(msg, "n_mods > 8", ONGYM_E_LIMIT);
    if (c->n_links > kCfgMaxLinks) return cfg_fail(msg, "n_links > 128", ONGYM_E_LIMIT);
    if (c->max_hops > kCfgMaxHops) return cfg_fail(msg, "max_hops > 64", ONGYM_E_LIMIT);
    if (c->n_slots > 1023) return cfg_fail(msg, "n_slots > 1023", ONGYM_E_LIMIT);
    if (c->n_paths > 65535) return cfg_fail(msg, "n_paths > 65535", ONGYM_E_LIMIT);
    if (c->capacity <= 0 || c->capacity % 64 || c->capacity > 65535)
        return cfg_fail(msg, "capacity must be a multiple of 64 in (0, 65535)");
    if (!c->pair_paths || !c->path_hops || !c->path_links || !c->link_nspans || !c->link_span_km || !c->link_alpha ||
        !c->link_nf || !c->mod_se || !c->mod_min_osnr || !c->node_cum)
        return cfg_fail(msg, "null table pointer in ongym_config");
    if (c->bit_rate_mode == 0 && (!c->bit_rates || !c->bit_rate_cum || c->n_bit_rates <= 0))
        return cfg_fail(msg, "discrete bit-rate mode needs bit_rates/bit_rate_cum");
    if (c->load <= 0 || c->mean_holding_time <= 0) return cfg_fail(msg, "load and mean_holding_time must be positive");
    return ONGYM_OK;
}

// the tables' entries, before any kernel indexes with them
inline int check_tables(const ongym_config *c, std::string &msg) {
    const int N = c->n_nodes, E = c->n_links, NP = c->n_paths, K = c->k_paths, H = c->max_hops, M = c->n_mods;
    for (int i = 0; i < N * N * K; i++)
        if (c->pair_paths[i] < -1 || c->pair_paths[i] >= NP) return cfg_fail(msg, "pair_paths entry out of range");
    for (int p = 0; p < NP; p++) {
        if (c->path_hops[p] <= 0 || c->path_hops[p] > H) return cfg_fail(msg, "path_hops entry out of range");
        for (int h = 0; h < c->path_hops[p]; h++)
            if (c->path_links[p * H + h] < 0 || c->path_links[p * H + h] >= E)
                return cfg_fail(msg, "path_links entry out of range");
    }
    for (int m = 0; m < M; m++)
        if (c->mod_se[m] < 1 || c->mod_se[m] > 6) return cfg_fail(msg, "spectral efficiency must be 1..6");
    for (int e = 0; e < E; e++)
        if (!(c->link_alpha[e] > 0) || !(c->link_span_km[e] > 0) || c->link_nspans[e] <= 0)
            return cfg_fail(msg, "link span parameters must be positive");
    return ONGYM_OK;
}

inline bool uniform_alpha(const ongym_config *c) {
    for (int e = 0; e < c->n_links; e++)
        if (c->link_alpha[e] != c->link_alpha[0]) return false;
    return true;
}

// the options that need more than sizes and tables, and the per-replica parameters
inline int check_options(const ongym_config *c, std::string &msg) {
    if (c->defragmentation && c->n_defrag_services < 0) return cfg_fail(msg, "n_defrag_services must be >= 0");
    const bool uniform = uniform_alpha(c);
    if (c->measure_disruptions && !uniform) return cfg_fail(msg, "measure_disruptions needs uniform attenuation", ONGYM_E_LIMIT);
    if (c->defragmentation && !uniform) return cfg_fail(msg, "defragmentation needs uniform attenuation", ONGYM_E_LIMIT);
    if (c->track_service_ids && !uniform) return cfg_fail(msg, "track_service_ids needs uniform attenuation", ONGYM_E_LIMIT);
    for (int r = 0; r < c->batch; r++) {
        const double power = c->replica_launch_power_w ? c->replica_launch_power_w[r] : c->launch_power_w;
        const double load = c->replica_load ? c->replica_load[r] : c->load;
        if (!(load > 0) || !(power > 0)) return cfg_fail(msg, "per-replica load / launch power must be positive");
    }
    return ONGYM_OK;
}

// Every refusal of create that needs no device, in a fixed order: the first check that fails is the one reported.
inline int config_check(const ongym_config &c, std::string &msg) {
    if (const int rc = check_sizes(&c, msg)) return rc;
    if (const int rc = check_tables(&c, msg)) return rc;
    return check_options(&c, msg);
}

// Everything create computes on the host before its first upload.  Pairs of doubles are interleaved (x, y).
struct HostTables {
    std::vector<double> w1, w2, cl, selfc;             // per link: GN weights, asinh coefficients (cross, self)
    std::vector<uint64_t> path_mask;                    // per route: two link-mask words
    std::vector<double> path_ase, path_w1;              // per route: sums over its links, in hop order
    std::vector<double> nli_coef, self_asinh;           // per slot count 0 .. n_slots + 1
    std::vector<int32_t> mod_se;                        // per format
    std::vector<double> mod_thr, mod_phi53;
    std::vector<int32_t> nreq_tab;                      // [max(n_bit_rates, 1)][kCfgMaxMods] slots needed (discrete rates; else 0)
    std::vector<double> req_coef;                       // (nli_coef[n], self_asinh[n]) of every nreq_tab entry n in 1 .. n_slots
    std::vector<double> plogp;                          // per block length 0 .. n_slots
    bool uniform = true, ase_shortcut = false, rec32 = false;
    double nslots_width = 0.0;                          // the width get_number_slots divides by
    // (asinh difference, Bk/|df|) per (interferer slot count nk, centre distance d in half slots), uniform attenuation only:
    std::vector<double> pair_tab;                       // [tab_nmax][tab_stride]; empty: the kernels compute the terms
    int tab_nmax = 0, tab_stride = 0;
    std::vector<double> pair_tab2k;                     // the same with a row pitch of tab_pitch, the link-weight table behind it
    uint32_t lw_tab_off = 0, lw_tab_bytes = 0;          // ... its byte offset and size (0: none)
    std::vector<uint32_t> lw_mult, lw_loc;              // ... and LwTable::mult / loc per route
    std::vector<double> pair_tabp;                      // pitch tab_pitch, odd distances in the second half of a row
    std::vector<int32_t> path_pair;                     // route -> lowest node pair that lists it (-1: none)
    std::string path_pair_err, admission_pair_err;      // why failure impact / the admission map refuse (empty: they run)
    int max_n = 0;                                      // largest slot count of the traffic table, at most n_slots
};

// GN link weights in fp64 (core/osnr.pyx:22-24, 52-55, 58-61, 109-125) and the sums over every route's links
inline void derive_links(const ongym_config *c, HostTables &T) {
    const int E = c->n_links, NP = c->n_paths, H = c->max_hops;
    const double pi = 3.14159265358979323846, beta2 = 21.3e-27, h_planck = 6.626e-34;
    std::vector<double> ase_link(E);
    T.w1.resize(E); T.w2.resize(E); T.cl.resize(E); T.selfc.resize(E);
    T.uniform = true;
    for (int e = 0; e < E; e++) {
        double a = c->link_alpha[e], L = c->link_span_km[e];
        double l_eff = (1.0 - std::exp(-2.0 * a * L * 1e3)) / (2.0 * a);
        T.w1[e] = (double)c->link_nspans[e] * l_eff;
        T.w2[e] = (double)c->link_nspans[e] * l_eff * (l_eff / (L * 1e3));
        T.cl[e] = pi * pi * beta2 * (1.0 / (2.0 * a));
        T.selfc[e] = pi * pi * beta2 / (4.0 * a);
        ase_link[e] = (double)c->link_nspans[e] * h_planck * (std::exp(2.0 * a * L * 1e3) - 1.0) * c->link_nf[e];
        if (a != c->link_alpha[0]) T.uniform = false;
    }
    T.rec32 = E <= 32 && NP <= 512 && c->n_slots <= 1023;
    T.path_mask.assign((size_t)NP * 2, 0);
    T.path_ase.assign(NP, 0.0); T.path_w1.assign(NP, 0.0);
    for (int p = 0; p < NP; p++)
        for (int h = 0; h < c->path_hops[p]; h++) {
            int l = c->path_links[p * H + h];
            T.path_mask[2 * p + (l >> 6)] |= 1ull << (l & 63);
            T.path_ase[p] += ase_link[l];
            T.path_w1[p] += T.w1[l];
        }
}

// per slot count, per format, per (bit rate, format) and per block length
inline void derive_slot_tables(const ongym_config *c, HostTables &T) {
    const int M = c->n_mods;
    const double pi = 3.14159265358979323846, beta2 = 21.3e-27;
    T.nli_coef.assign((size_t)c->n_slots + 2, 0.0);
    for (int n = 1; n <= c->n_slots + 1; n++) {
        const double gamma = 1.3e-3, bwn = c->slot_bandwidth * n;
        T.nli_coef[n] = (8.0 / (27.0 * pi * beta2)) * (gamma * gamma) / (bwn * bwn);
    }
    T.self_asinh.assign((size_t)c->n_slots + 2, 0.0);   // uniform alpha only
    for (int n = 0; n <= c->n_slots + 1; n++) {
        double bwn = c->slot_bandwidth * n;
        T.self_asinh[n] = std::asinh(T.selfc[0] * (bwn * bwn));
    }
    static const double phi_mod[6] = {1.0, 1.0, 2.0 / 3.0, 17.0 / 25.0, 69.0 / 100.0, 13.0 / 21.0};
    T.mod_se.assign(c->mod_se, c->mod_se + M);
    T.mod_thr.assign(c->mod_min_osnr, c->mod_min_osnr + M);
    T.mod_phi53.resize(M);
    for (int m = 0; m < M; m++) T.mod_phi53[m] = phi_mod[c->mod_se[m] - 1] * (5.0 / 3.0);
    // link_shannon_entropy_ (utils.pyx:61-79): p = block / total_slots; p * math.log(p) — CPython's math.log is this log()
    T.plogp.assign((size_t)c->n_slots + 1, 0.0);
    for (int n = 1; n <= c->n_slots; n++) { const double pr = (double)n / (double)c->n_slots; T.plogp[n] = pr * std::log(pr); }
}

// slots needed per (discrete bit rate, modulation): get_number_slots, envs/qrmsa.pyx:1198-1205
inline void derive_requests(const ongym_config *c, HostTables &T) {
    const int M = c->n_mods;
    T.nslots_width = c->nslots_channel_width > 0 ? c->nslots_channel_width : c->channel_width;
    T.nreq_tab.assign((size_t)std::max(c->n_bit_rates, 1) * kCfgMaxMods, 0);
    T.max_n = 0;
    if (c->bit_rate_mode == 0)
        for (int b = 0; b < c->n_bit_rates; b++)
            for (int m = 0; m < M; m++) {
                const int32_t n = (int32_t)std::ceil((double)(float)c->bit_rates[b] / ((double)c->mod_se[m] * T.nslots_width));
                T.nreq_tab[(size_t)b * kCfgMaxMods + m] = n;
                T.max_n = std::max(T.max_n, std::min((int)n, (int)c->n_slots));
            }
    // (nli_coef[n], self_asinh[n]) of the slot count of every (discrete bit rate, modulation): lets the request draw
    // fetch them with the SAME index as nreq_tab instead of a second, dependent round trip through n
    T.req_coef.assign(T.nreq_tab.size() * 2, 0.0);
    for (size_t i = 0; i < T.nreq_tab.size(); i++) {
        const int32_t n = T.nreq_tab[i];
        if (n >= 1 && n <= c->n_slots) { T.req_coef[2 * i] = T.nli_coef[(size_t)n]; T.req_coef[2 * i + 1] = T.self_asinh[(size_t)n]; }
    }
}

// ASE-only rejection is exact iff no interferer term asinh(u)-asinh(v) - Phi*(5/3)*(Bk/|df|)*(l_eff/L) of
// core/osnr.pyx:68-93 can be negative: scan the whole discrete domain (slot counts x centre distances in half
// slots x modulation formats x distinct link classes) once.
inline void derive_ase_shortcut(const ongym_config *c, HostTables &T) {
    bool all_nonneg = true;
    std::vector<std::pair<double, double>> classes;   // (cl, l_eff/(L*1e3))
    for (int e = 0; e < c->n_links; e++) {
        std::pair<double, double> k(T.cl[e], T.w2[e] / T.w1[e]);
        bool seen = false;
        for (auto &q : classes) if (q == k) seen = true;
        if (!seen) classes.push_back(k);
    }
    const int S = c->n_slots;
    for (auto &cls : classes)
        for (int m = 0; m < c->n_mods && all_nonneg; m++) {
            const double K = T.mod_phi53[m] * cls.second;
            for (int nk = 1; nk <= S && all_nonneg; nk++) {
                const double bk = c->slot_bandwidth * nk, ck = cls.first * bk;
                for (int dfi = nk + 1; dfi <= 2 * S; dfi++) {
                    const double adf = 0.5 * c->slot_bandwidth * dfi;
                    const double t = (std::asinh(ck * (adf + 0.5 * bk)) - std::asinh(ck * (adf - 0.5 * bk))) - K * (bk / adf);
                    if (!(t > 0.0)) { all_nonneg = false; break; }
                }
            }
        }
    T.ase_shortcut = all_nonneg;
}

// (asinh difference, Bk/|df|) table of core/osnr.pyx:68-93 for uniform attenuation. Both factors depend only on the
// interferer's slot count nk and the centre distance in half slots: precompute them in fp64 with the device's own
// expressions. nk range: the largest slot count the configured traffic can produce (anything larger, e.g. from a
// replayed trace, is computed on the fly by the kernel).
inline void derive_pair_tab(const ongym_config *c, HostTables &T) {
    T.pair_tab.clear(); T.tab_nmax = 0; T.tab_stride = 2 * c->n_slots + 1;
    if (!T.uniform) return;
    double max_rate = 0.0;
    if (c->bit_rate_mode == 0) for (int b = 0; b < c->n_bit_rates; b++) max_rate = std::max(max_rate, c->bit_rates[b]);
    else max_rate = (double)c->bit_rate_hi;
    int min_se = 6;
    for (int m = 0; m < c->n_mods; m++) min_se = std::min(min_se, (int)c->mod_se[m]);
    int nmax = (int)std::ceil(max_rate / ((double)min_se * T.nslots_width));
    nmax = std::max(1, std::min(nmax, c->n_slots));
    size_t entries = (size_t)nmax * T.tab_stride;
    if (entries * 16 > (size_t)16 << 20) return;
    T.pair_tab.resize(entries * 2);
    for (int nk = 1; nk <= nmax; nk++) {
        const double bk = c->slot_bandwidth * nk, ck = T.cl[0] * bk;
        for (int d = 0; d < T.tab_stride; d++) {
            double x = 0.0, y = 0.0;
            if (d > nk) {   // allocations never overlap: |df| > Bk/2
                const double adf = (0.5 * c->slot_bandwidth) * (double)d;
                const double U = ck * (adf + 0.5 * bk), V = ck * (adf - 0.5 * bk);
                x = std::log((U + std::sqrt(std::fma(U, U, 1.0))) / (V + std::sqrt(std::fma(V, V, 1.0))));
                y = bk / adf;
            }
            const size_t e = (size_t)(nk - 1) * T.tab_stride + d;
            T.pair_tab[2 * e] = x; T.pair_tab[2 * e + 1] = y;
        }
    }
    T.tab_nmax = nmax;
}

// The pair table once more with a row pitch of tab_pitch entries (index = row * pitch | distance: one address instruction),
// used by the lean first-fit kernel and by the observation field builder; behind it the shared-link weight table of the lean
// kernels (ongym_lwtab.hpp) when the links fit one mask word.  One array: the kernels gather from both through the same base
// register.  pair_tabp: the same rows with the odd distances in the second half.
inline void derive_pair_layouts(const ongym_config *c, const CreateKnobs &knobs, int tab_pitch, HostTables &T) {
    const int NP = c->n_paths;
    T.pair_tab2k.clear(); T.pair_tabp.clear(); T.lw_tab_off = 0; T.lw_tab_bytes = 0; T.lw_mult.clear(); T.lw_loc.clear();
    if (T.pair_tab.empty() || T.tab_stride >= tab_pitch || (size_t)T.tab_nmax * tab_pitch * 16 > ((size_t)64 << 20)) return;
    std::vector<double> &t2 = T.pair_tab2k, &t3 = T.pair_tabp;
    t2.assign((size_t)T.tab_nmax * tab_pitch * 2, 0.0);
    t3.assign((size_t)T.tab_nmax * tab_pitch * 2, 0.0);
    for (int nk = 0; nk < T.tab_nmax; nk++)
        for (int d = 0; d < T.tab_stride; d++) {
            const size_t from = ((size_t)nk * T.tab_stride + d) * 2, e2 = (size_t)nk * tab_pitch + d;
            const size_t e3 = (size_t)nk * tab_pitch + (size_t)(d & 1) * (tab_pitch / 2) + (size_t)(d >> 1);
            t2[e2 * 2] = T.pair_tab[from]; t2[e2 * 2 + 1] = T.pair_tab[from + 1];
            t3[e3 * 2] = T.pair_tab[from]; t3[e3 * 2 + 1] = T.pair_tab[from + 1];
        }
    if (!T.rec32 || c->n_links > 32 || knobs.no_lwtab) return;
    std::vector<uint32_t> m32((size_t)NP);
    for (int p = 0; p < NP; p++) m32[(size_t)p] = (uint32_t)T.path_mask[2 * p];
    LwTable lwt = lw_build(m32, T.w1.data(), T.w2.data(), t2.size() * 8);
    if (!lwt.ok) return;
    T.lw_tab_off = (uint32_t)(t2.size() * 8); T.lw_tab_bytes = (uint32_t)(lwt.entries.size() * 8);
    t2.insert(t2.end(), lwt.entries.begin(), lwt.entries.end());
    T.lw_mult = std::move(lwt.mult); T.lw_loc = std::move(lwt.loc);
}

// route -> node pair for ongym_failure_impact.  Both directions of a pair share their routes in the same order
// (topology.pyx:310-355): every pair that lists a route must list the same K routes, or the call refuses
inline void derive_path_pair(const ongym_config *c, HostTables &T) {
    const int N = c->n_nodes, K = c->k_paths;
    std::vector<int32_t> &pp = T.path_pair;
    pp.assign((size_t)c->n_paths, -1);
    T.path_pair_err.clear();
    for (int pr = 0; pr < N * N && T.path_pair_err.empty(); pr++)
        for (int k = 0; k < K; k++) {
            const int p = c->pair_paths[(size_t)pr * K + k];
            if (p < 0) continue;
            if (pp[p] < 0) pp[p] = pr;
            else if (pp[p] != pr && !std::equal(c->pair_paths + (size_t)pr * K, c->pair_paths + (size_t)(pr + 1) * K,
                                                c->pair_paths + (size_t)pp[p] * K)) {
                T.path_pair_err = "route " + std::to_string(p) + " is listed by node pairs " + std::to_string(pp[p]) + " and " +
                                  std::to_string(pr) + " with different route lists: no node pair for failure impact";
                break;
            }
        }
}

// ongym_admission_map walks the unordered node pairs: both directions of a pair must list the same routes in the same order
inline void derive_admission_pairs(const ongym_config *c, HostTables &T) {
    const int N = c->n_nodes, K = c->k_paths;
    T.admission_pair_err.clear();
    for (int s = 0; s < N && T.admission_pair_err.empty(); s++)
        for (int d = s + 1; d < N; d++)
            if (!std::equal(c->pair_paths + ((size_t)s * N + d) * K, c->pair_paths + ((size_t)s * N + d + 1) * K,
                            c->pair_paths + ((size_t)d * N + s) * K)) {
                T.admission_pair_err = "node pair (" + std::to_string(s) + ", " + std::to_string(d) +
                                       ") lists different routes in its two directions: no unordered pair for the admission map";
                break;
            }
}

// Dword 0 of a route's record in first fit's copy of the record table (Params::path_rec_ff; ongym_fast.hpp, path_and): the hop
// count in the low byte and above it four 6-bit fields with the route's links in path_links order, so that the kernel reads the
// rows of all hops in one LDS trip (lane 16 r + w = word w of the row of field r).  Fields past the last hop repeat the first
// link: the AND of the rows is idempotent.  kCfgPathRowsLong marks a route for the link loop, its fields are 0: more than four
// hops, a row that with the virtual slot S does not fit 16 lanes (S >= 512), or link ids beyond one mask word.
constexpr uint32_t kCfgPathRowsLong = 1u << 31;
constexpr int kCfgPathRowsFields = 4, kCfgPathRowsShift = 8, kCfgPathRowsBits = 6, kCfgPathRowsLanes = 16;
inline uint32_t path_rows_word(const ongym_config *c, int p) {
    const int hops = c->path_hops[p];
    const uint32_t w = (uint32_t)hops & 0xFFu;
    if (hops > kCfgPathRowsFields || c->n_slots / 32 + 1 > kCfgPathRowsLanes || c->n_links > 32) return w | kCfgPathRowsLong;
    uint32_t f = 0;
    for (int r = 0; r < kCfgPathRowsFields; r++)
        f |= (uint32_t)c->path_links[(size_t)p * c->max_hops + (r < hops ? r : 0)] << (kCfgPathRowsShift + kCfgPathRowsBits * r);
    return w | f;
}

// `c` has passed config_check.  tab_pitch: kTabPitch of ongym_fast.hpp.
inline void derive_tables(const ongym_config &c, const CreateKnobs &knobs, int tab_pitch, HostTables &T) {
    derive_links(&c, T);
    derive_slot_tables(&c, T);
    derive_requests(&c, T);
    derive_ase_shortcut(&c, T);
    derive_pair_tab(&c, T);
    derive_pair_layouts(&c, knobs, tab_pitch, T);
    derive_path_pair(&c, T);
    derive_admission_pairs(&c, T);
}

}  // namespace ongym
