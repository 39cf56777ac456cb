// ongym_tables_shim.cpp — C interface to csrc/ongym_tables.hpp for the host tests (TEST INFRASTRUCTURE, never loaded by the
// product): config_check's verdict, and every table and scalar derive_tables makes, by name.
//   libongym_tables.so           tests/test_tables_host.py, through ctypes
//   -DONGYM_TABLES_MAIN          a stand-alone program on a built-in configuration, for the sanitizer build (make tables_asan)
#include <cstdio>
#include <cstring>
#include <map>

#include "../optical-networking-gym_amd/csrc/ongym_tables.hpp"

using namespace ongym;

namespace {
struct Span { const void *ptr; size_t bytes; };
struct Handle {
    int code = 0;
    std::string msg;
    HostTables T;
    std::map<std::string, Span> tables;
    std::map<std::string, double> scalars;
    std::map<std::string, const std::string *> texts;
};

template <class V> Span span(const std::vector<V> &v) { return Span{v.data(), v.size() * sizeof(V)}; }

void index_tables(Handle &h) {
    const HostTables &T = h.T;
    h.tables = {{"w1", span(T.w1)}, {"w2", span(T.w2)}, {"cl", span(T.cl)}, {"selfc", span(T.selfc)},
                {"path_mask", span(T.path_mask)}, {"path_ase", span(T.path_ase)}, {"path_w1", span(T.path_w1)},
                {"nli_coef", span(T.nli_coef)}, {"self_asinh", span(T.self_asinh)}, {"mod_se", span(T.mod_se)},
                {"mod_thr", span(T.mod_thr)}, {"mod_phi53", span(T.mod_phi53)}, {"nreq_tab", span(T.nreq_tab)},
                {"req_coef", span(T.req_coef)}, {"plogp", span(T.plogp)}, {"pair_tab", span(T.pair_tab)},
                {"pair_tab2k", span(T.pair_tab2k)}, {"pair_tabp", span(T.pair_tabp)}, {"lw_mult", span(T.lw_mult)},
                {"lw_loc", span(T.lw_loc)}, {"path_pair", span(T.path_pair)}};
    h.scalars = {{"uniform", T.uniform}, {"ase_shortcut", T.ase_shortcut}, {"rec32", T.rec32}, {"nslots_width", T.nslots_width},
                 {"tab_nmax", T.tab_nmax}, {"tab_stride", T.tab_stride}, {"lw_tab_off", T.lw_tab_off},
                 {"lw_tab_bytes", T.lw_tab_bytes}, {"max_n", T.max_n}};
    h.texts = {{"path_pair_err", &T.path_pair_err}, {"admission_pair_err", &T.admission_pair_err}};
}
}  // namespace

extern "C" {

// Never null.  The tables exist only when ogt_check_code() is 0.
void *ogt_create(const ongym_config *cfg, int force_generic, int force_wide, int no_lwtab, int tab_pitch) {
    Handle *h = new Handle();
    h->code = config_check(*cfg, h->msg);
    if (h->code) return h;
    CreateKnobs k;
    k.force_generic = force_generic != 0; k.force_wide = force_wide != 0; k.no_lwtab = no_lwtab != 0;
    derive_tables(*cfg, k, tab_pitch, h->T);
    index_tables(*h);
    return h;
}

void ogt_destroy(void *h) { delete static_cast<Handle *>(h); }
int ogt_check_code(void *h) { return static_cast<Handle *>(h)->code; }
const char *ogt_check_msg(void *h) { return static_cast<Handle *>(h)->msg.c_str(); }

// 0 and (pointer, byte length) of the named table, -1 for a name that is none
int ogt_table(void *h, const char *name, const void **ptr, size_t *bytes) {
    const auto &m = static_cast<Handle *>(h)->tables;
    const auto it = m.find(name);
    if (it == m.end()) return -1;
    *ptr = it->second.ptr; *bytes = it->second.bytes;
    return 0;
}

int ogt_scalar(void *h, const char *name, double *value) {
    const auto &m = static_cast<Handle *>(h)->scalars;
    const auto it = m.find(name);
    if (it == m.end()) return -1;
    *value = it->second;
    return 0;
}

// the named message ("" when the check behind it passed), null for a name that is none
const char *ogt_text(void *h, const char *name) {
    const auto &m = static_cast<Handle *>(h)->texts;
    const auto it = m.find(name);
    return it == m.end() ? nullptr : it->second->c_str();
}

}  // extern "C"

#ifdef ONGYM_TABLES_MAIN
// A 6-node ring with the chords 0-3 and 1-4; per node pair the two shortest of {clockwise arc, counter-clockwise arc, chord};
// S = 70 (row_words = ext_words = 2); two bit rates.  Every accessor runs once and every byte it hands out is read.
namespace {
constexpr int kN = 6, kK = 2, kH = 5;
struct Route { std::vector<int> links; };

std::vector<Route> routes_between(int s, int d) {
    std::vector<Route> r(2);
    for (int v = s; v != d; v = (v + 1) % kN) r[0].links.push_back(v);                  // ring link v: v -> v + 1
    for (int v = s; v != d; v = (v + kN - 1) % kN) r[1].links.push_back((v + kN - 1) % kN);
    if (s == 0 && d == 3) r.push_back(Route{{6}});
    if (s == 1 && d == 4) r.push_back(Route{{7}});
    std::stable_sort(r.begin(), r.end(), [](const Route &a, const Route &b) { return a.links.size() < b.links.size(); });
    r.resize(kK);
    return r;
}

uint64_t read_all(const void *p, size_t n) {
    uint64_t sum = 0;
    for (size_t i = 0; i < n; i++) sum += static_cast<const unsigned char *>(p)[i];
    return sum;
}
}  // namespace

int main() {
    std::vector<int32_t> pair_paths(kN * kN * kK, -1), hops, links;
    for (int s = 0; s < kN; s++)
        for (int d = s + 1; d < kN; d++)
            for (const Route &r : routes_between(s, d)) {
                const int p = (int)hops.size(), k = p % kK;
                pair_paths[(s * kN + d) * kK + k] = pair_paths[(d * kN + s) * kK + k] = p;
                hops.push_back((int32_t)r.links.size());
                for (int h = 0; h < kH; h++) links.push_back(h < (int)r.links.size() ? r.links[h] : 0);
            }
    const int32_t nspans[8] = {1, 2, 1, 3, 2, 1, 4, 2}, mod_se[3] = {1, 2, 4};
    const double span_km[8] = {80, 75, 60, 90, 100, 50, 85, 70}, nf[8] = {3.16, 3.16, 3.16, 3.16, 3.16, 3.16, 3.16, 3.16};
    double alpha[8];
    for (double &a : alpha) a = 0.2 / 4.343 / 1e3;
    const double thr[3] = {3.71, 6.72, 13.24}, rates[2] = {100, 400}, cum[2] = {0.5, 1.0}, node_cum[kN] = {1 / 6., 2 / 6., .5, 4 / 6., 5 / 6., 1};
    ongym_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = (int32_t)sizeof c; c.abi_version = ONGYM_ABI_VERSION;
    c.n_nodes = kN; c.n_links = 8; c.n_paths = (int32_t)hops.size(); c.k_paths = kK; c.max_hops = kH; c.n_mods = 3; c.n_slots = 70;
    c.batch = 2; c.capacity = 64; c.episode_length = 100; c.n_bit_rates = 2; c.bit_rate_lo = 25; c.bit_rate_hi = 100;
    c.frequency_start = 3e8 / 1565e-9; c.slot_bandwidth = 12.5e9; c.channel_width = 12.5; c.launch_power_w = 1e-3;
    c.load = 10; c.mean_holding_time = 100; c.max_bit_rate = 400;
    c.pair_paths = pair_paths.data(); c.path_hops = hops.data(); c.path_links = links.data(); c.link_nspans = nspans;
    c.link_span_km = span_km; c.link_alpha = alpha; c.link_nf = nf; c.mod_se = mod_se; c.mod_min_osnr = thr;
    c.bit_rates = rates; c.bit_rate_cum = cum; c.node_cum = node_cum;

    void *h = ogt_create(&c, 0, 0, 0, 2048);
    if (ogt_check_code(h)) { fprintf(stderr, "config_check: %s\n", ogt_check_msg(h)); return 1; }
    uint64_t sum = 0;
    int three_hops = 0;
    for (int32_t n : hops) three_hops += n == 3;
    Handle *hh = static_cast<Handle *>(h);
    for (const auto &t : hh->tables) {
        const void *p = nullptr; size_t n = 0;
        if (ogt_table(h, t.first.c_str(), &p, &n)) return 2;
        sum += read_all(p, n);
    }
    for (const auto &s : hh->scalars) { double v; if (ogt_scalar(h, s.first.c_str(), &v)) return 3; sum += (uint64_t)v; }
    for (const auto &t : hh->texts) { const char *m = ogt_text(h, t.first.c_str()); if (!m || m[0]) return 4; }
    double v;
    const void *p; size_t n;
    if (ogt_table(h, "no such table", &p, &n) != -1 || ogt_scalar(h, "no such scalar", &v) != -1 || ogt_text(h, "none")) return 5;
    const bool shape = three_hops >= 1 && hh->T.lw_tab_bytes > 0 && hh->T.tab_stride == 141 && hh->T.max_n == 32;
    ogt_destroy(h);
    c.n_mods = 9;                                        // ... and one refusal
    h = ogt_create(&c, 0, 0, 0, 2048);
    const bool refused = ogt_check_code(h) == ONGYM_E_LIMIT && !strcmp(ogt_check_msg(h), "n_mods > 8");
    ogt_destroy(h);
    printf("ongym_tables: %d routes, checksum %llu\n", (int)hops.size(), (unsigned long long)sum);
    return shape && refused ? 0 : 6;
}
#endif
