// ongym_lwtab.hpp — host side of the shared-link weight table of the lean kernels (ongym_fast.hpp).
//
// An interferer of route p contributes the GN link weights (w1, w2) of the links it shares with p, summed in ascending link
// order.  The sum depends only on p and on WHICH subset of p's links is shared, so it is tabulated at create: for every route
// with H links and link mask m one 16-byte entry (sum w1, sum w2) per subset s of m.  The device finds the entry with
//     idx = ((x & m) * mult_p) >> (32 - W_p)                       (x = the interferer's link mask, 32-bit product)
// a per-route multiplicative hash that is injective on the 2^H subsets of m (W_p >= H, as small as the search allows).  A
// route's 2^W_p entries are contiguous and 32-byte aligned, so its byte offset and the shift share one dword (`loc`).
// Plain C++ (no HIP), so that it can be compiled and checked on its own.
#pragma once
#include <cstdint>
#include <vector>

namespace ongym {

constexpr int kLwMaxHops = 10;          // routes with more links: no table (2^H entries per route)
constexpr int kLwSlack = 2;             // W_p <= H + kLwSlack
constexpr int kLwTrials = 1 << 14;      // multipliers tried per (route, W)

struct LwTable {
    std::vector<uint32_t> mult, loc;    // per route: multiplier (odd, never 0) | byte offset of the route's block + (32 - W_p)
    std::vector<double> entries;        // (sum w1, sum w2) interleaved; unused hash slots stay (0, 0)
    size_t touched_bytes = 0;           // sum over routes of 2^H * 16: the entries a kernel can ever read
    bool ok = false;
};

inline uint64_t lw_splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint32_t lw_index(uint32_t x, uint32_t mask, uint32_t mult, uint32_t loc) { return ((x & mask) * mult) >> (loc & 31u); }

// true iff `mult` maps the subsets of `mask` to distinct W-bit indices (`stamp`: 2^W words of scratch, `tag` unique per call)
inline bool lw_injective(uint32_t mask, uint32_t mult, int W, std::vector<uint32_t> &stamp, uint32_t tag) {
    uint32_t s = 0;
    do {
        const uint32_t i = (s * mult) >> (32 - W);
        if (stamp[i] == tag) return false;
        stamp[i] = tag;
        s = (s - mask) & mask;          // next subset of mask
    } while (s);
    return true;
}

// Deterministic, seeded (by the mask alone), bounded search.  H = popcount(mask) in 1..kLwMaxHops.
inline bool lw_find_mult(uint32_t mask, int H, uint32_t *mult, int *W) {
    std::vector<uint32_t> stamp;
    uint32_t tag = 0;
    for (int w = H; w <= H + kLwSlack; w++) {
        stamp.assign((size_t)1 << w, 0u);
        uint64_t seed = 0x6C77746162ull ^ ((uint64_t)mask << 8) ^ (uint64_t)w;
        for (int t = 0; t < kLwTrials; t++) {
            const uint64_t a = lw_splitmix(seed), b = lw_splitmix(seed);
            // sparse multipliers first (few partial products, few carries into the index bits), dense ones after
            const uint32_t m = (uint32_t)((t & 1) ? a : (a & b & (b >> 32))) | 1u;
            if (lw_injective(mask, m, w, stamp, ++tag)) { *mult = m; *W = w; return true; }
        }
    }
    return false;
}

// masks[p]: link mask of route p (links 0..31); w1 / w2: per-link weights.  `base_bytes`: where the table will lie relative to
// the address the kernels add `loc` to (a multiple of 32).
inline LwTable lw_build(const std::vector<uint32_t> &masks, const double *w1, const double *w2, size_t base_bytes) {
    LwTable T;
    const size_t NP = masks.size();
    T.mult.assign(NP, 0u); T.loc.assign(NP, 0u);
    size_t n_entries = 0;
    std::vector<int> Ws(NP, 0);
    for (size_t p = 0; p < NP; p++) {
        const uint32_t m = masks[p];
        const int H = __builtin_popcount(m);
        if (H < 1 || H > kLwMaxHops) return T;
        bool found = false;
        for (size_t q = 0; q < p && !found; q++)        // routes with the same link set share the multiplier (not the block)
            if (masks[q] == m) { T.mult[p] = T.mult[q]; Ws[p] = Ws[q]; found = true; }
        if (!found && !lw_find_mult(m, H, &T.mult[p], &Ws[p])) return T;
        const size_t off = base_bytes + n_entries * 16;
        if (off + ((size_t)16 << Ws[p]) > 0xFFFFFFFFull) return T;
        T.loc[p] = (uint32_t)off | (uint32_t)(32 - Ws[p]);
        n_entries += (size_t)1 << Ws[p];
        T.touched_bytes += (size_t)16 << H;
    }
    T.entries.assign(n_entries * 2, 0.0);
    for (size_t p = 0; p < NP; p++) {
        const uint32_t m = masks[p];
        const size_t first = ((T.loc[p] & ~31u) - base_bytes) / 16;
        uint32_t s = 0;
        do {
            double a = 0.0, b = 0.0;                    // the device loop's own sequence: ascending links, plain adds from 0.0
            for (uint32_t mm = s; mm; mm &= mm - 1) { const int l = __builtin_ctz(mm); a += w1[l]; b += w2[l]; }
            const size_t e = first + lw_index(s, m, T.mult[p], T.loc[p]);
            T.entries[2 * e] = a; T.entries[2 * e + 1] = b;
            s = (s - m) & m;
        } while (s);
    }
    T.ok = true;
    return T;
}

}  // namespace ongym
