// ongym_spectrum.hpp — the spectrum map of every replica (ongym_spectrum_map, include/ongym.h): who holds every slot of every
// link, the running records of all replicas, and an audit of the rule every state-changing kernel keeps: the bitmap's used cells
// are exactly the disjoint union of the running records' provisioned ranges [slot, min(slot + n + 1, S)) on the links of
// their routes.  Read-only: nothing of the replica is stored.
//
// Kernel: one wavefront per replica, grid (batch).  Record fields and st.active are bytes that ongym_state_load accepts as they
// come, so no address is formed from one before it has passed its range check (ongym_spectrum_core.hpp): a table index, an LDS
// index and a shift count only ever come from a well-formed record.
//   1. the replica's E x W row words to LDS (bits at and above S cleared), two more planes `claimed` and `twice` zeroed
//   2. lanes stride over the A records: decode, validate, write rec_out / release_out; a well-formed record ORs its range mask
//      into `claimed` on every link of its route with a returning 64-bit LDS atomic, and what the returned word already held
//      of the mask goes into `twice`
//   3. the audit columns are popcounts over the three planes; a failed link is a full row that no well-formed record crosses
//      (ongym_failed_links' rule), and its S unclaimed used cells are no orphans
//   4. owner_out only: link after link, lane l stores cells l, l + 64, ...: one coalesced 128-byte store per 64 cells.  A row
//      without a `twice` bit (every row of a sound state) has disjoint ranges, so a claimed cell belongs to the nearest range
//      start at or below it: every record that crosses the link writes its index at row[start] and one bit into a plane of
//      starts, and a lane finds its cell's holder with one bit scan.  A row with a `twice` bit takes the exact path: the
//      records write (index, guard) keys into every cell of their range with an LDS atomic minimum, the lowest index stays.
// Loops are bounded by A, C, E, the row words, or (contested rows) the validated width of one record (<= S).
//
// LDS: three planes of E x W words; with owner_out also W words of starts, the row u32[S] and two words per record (route,
// range).  NSFNET-320, C = 448: 2 640 B for the audit and the records, 7 544 B with the owners.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_cut.hpp"             // wave_or_u64
#include "ongym_spectrum_core.hpp"

namespace ongym {

__host__ __device__ inline size_t spectrum_lds_bytes(const Params &P, bool owners) {
    return (size_t)P.n_links * P.row_words * 24 + (owners ? (size_t)P.row_words * 8 + (size_t)P.n_slots * 4 + (size_t)P.capacity * 8 : 0);
}

constexpr uint32_t kNoRoute = 0xFFFFFFFFu;   // generic codec: the route word of a malformed record (R32: an empty mask)

template <bool R32>
__global__ __launch_bounds__(64) void k_spectrum_map(const Params *__restrict__ Pp, int width_limit, int16_t *__restrict__ owner_out,
                                                     int32_t *__restrict__ rec_out, float *__restrict__ release_out,
                                                     int32_t *__restrict__ audit_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    const int lane = threadIdx.x, replica = blockIdx.x;
    const int E = P.n_links, W = P.row_words, S = P.n_slots, C = P.capacity, EW = E * W;
    unsigned long long *occ = reinterpret_cast<unsigned long long *>(smem), *claimed = occ + EW, *twice = claimed + EW;
    unsigned long long *starts = twice + EW;                    // the four below only with owner_out
    uint32_t *row = reinterpret_cast<uint32_t *>(starts + W);
    uint32_t *route = row + S, *range = route + C;

    // ---- 1. the rows
    const uint64_t *g = P.occ + (size_t)replica * EW;
    for (int i = lane; i < EW; i += kWave) {
        occ[i] = g[i] & spectrum_word_mask(i % W, 0, S);
        claimed[i] = 0; twice[i] = 0;
    }
    wave_sync();

    // ---- 2. the records
    const int stored = uniform_i32(P.env[replica].st.active);
    const int A = spectrum_active(stored, C);
    const size_t off = (size_t)replica * C;
    const uint64_t links0 = E >= 64 ? ~0ull : (1ull << E) - 1ull, links1 = E <= 64 ? 0ull : E >= 128 ? ~0ull : (1ull << (E - 64)) - 1ull;
    uint64_t u0 = 0, u1 = 0;                                     // links that well-formed records cross
    int malformed = 0, wide = 0;
    for (int i = lane; i < A; i += kWave) {
        const uint32_t a = P.svc_a[off + i], b = P.svc_b[off + i];
        const SpectrumRec r = spectrum_decode(R32, a, b);
        bool ok = spectrum_fields_ok(r, P.n_paths, P.n_mods, S);
        uint64_t m0 = 0, m1 = 0;
        if (ok) {                                                // 0 <= path < n_paths
            m0 = G(P.path_mask)[2 * (size_t)r.path] & links0;
            m1 = G(P.path_mask)[2 * (size_t)r.path + 1] & links1;
            ok = spectrum_mask_ok(R32, a, m0);
        }
        if (!ok) { m0 = 0; m1 = 0; malformed++; }
        if (rec_out) {
            int32_t *o = rec_out + (off + i) * kSpectrumRec;
            o[0] = r.path; o[1] = r.slot; o[2] = r.n; o[3] = r.mod;
            o[4] = P.track_ids ? (int32_t)P.svc_q[off + i] : -1;
            o[5] = (P.svc_r[off + i] < 0.f ? 1 : 0) | (ok ? 0 : 2);
        }
        if (release_out) release_out[off + i] = fabsf(P.svc_r[off + i]);
        const int lo = ok ? r.slot : 0, sig = ok ? r.slot + r.n : 0, hi = ok ? spectrum_claim_end(r, S) : 0;   // 0 <= lo < sig <= hi <= S
        if (owner_out) { route[i] = ok ? (R32 ? a : (uint32_t)r.path) : (R32 ? 0u : kNoRoute); range[i] = (uint32_t)lo | ((uint32_t)sig << 16); }
        if (!ok) continue;
        wide += r.n > width_limit;
        u0 |= m0; u1 |= m1;
        const int w0 = lo >> 6, w1 = (hi - 1) >> 6;              // row words of the range: w1 < W
        for (int h = 0; h < 2; h++) {
            uint64_t m = h ? m1 : m0;
            while (m) {                                          // one turn per link of the route: bits below E only
                const int e = 64 * h + __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                for (int w = w0; w <= w1; w++) {
                    const unsigned long long mask = spectrum_word_mask(w, lo, hi);
                    const unsigned long long old = atomicOr(&claimed[e * W + w], mask);
                    if (old & mask) atomicOr(&twice[e * W + w], old & mask);
                }
            }
        }
    }
    for (int i = A + lane; i < C; i += kWave) {                  // the rows at and beyond A
        if (rec_out)
            for (int k = 0; k < kSpectrumRec; k++) rec_out[(off + i) * kSpectrumRec + k] = -1;
        if (release_out) release_out[off + i] = NAN;
    }
    wave_sync();

    // ---- 3. the audit
    if (audit_out) {
        u0 = wave_or_u64(u0); u1 = wave_or_u64(u1);
        int overlap = 0, claimed_free = 0, unclaimed = 0, cells = 0, used = 0;
        for (int i = lane; i < EW; i += kWave) {
            const unsigned long long o = occ[i], c = claimed[i];
            const unsigned long long u = ~o & spectrum_word_mask(i % W, 0, S);
            overlap += __popcll(twice[i]);
            claimed_free += __popcll(c & o);
            unclaimed += __popcll(u & ~c);
            cells += __popcll(c);
            used += __popcll(u);
        }
        bool full[2];
        for (int h = 0; h < 2; h++) {
            const int l = lane + 64 * h;
            unsigned long long any = 0;
            if (l < E)
                for (int w = 0; w < W; w++) any |= occ[l * W + w];
            full[h] = l < E && any == 0;
        }
        const uint64_t d0 = __ballot(full[0]) & ~u0, d1 = __ballot(full[1]) & ~u1;
        const int failed = __popcll((unsigned long long)d0) + __popcll((unsigned long long)d1);
        malformed = wave_sum_i32(malformed); wide = wave_sum_i32(wide);
        overlap = wave_sum_i32(overlap); claimed_free = wave_sum_i32(claimed_free);
        cells = wave_sum_i32(cells); used = wave_sum_i32(used);
        const int orphan = wave_sum_i32(unclaimed) - S * failed;   // no record crosses a failed link: its S used cells are unclaimed
        const int v[kSpectrumAudit] = {(stored != A ? 1 : 0) | (malformed ? 2 : 0) | (overlap ? 4 : 0) | (claimed_free ? 8 : 0) |
                                           (orphan ? 16 : 0) | (wide ? 32 : 0),
                                       A, malformed, overlap, claimed_free, orphan, wide, failed, cells, used};
        int r = v[0];
        for (int k = 1; k < kSpectrumAudit; k++) r = lane == k ? v[k] : r;
        if (lane < kSpectrumAudit) audit_out[(size_t)replica * kSpectrumAudit + lane] = r;
    }
    if (!owner_out) return;

    // ---- 4. the owners, link after link
    for (int e = 0; e < E; e++) {
        unsigned long long t = 0;
        for (int w = lane; w < W; w += kWave) { t |= twice[e * W + w]; starts[w] = 0; }
        const bool contested = __ballot(t != 0) != 0;            // wave-uniform
        if (contested)
            for (int s = lane; s < S; s += kWave) row[s] = ~0u;
        wave_sync();
        for (int i = lane; i < A; i += kWave) {
            const uint32_t rt = route[i];
            bool on;
            if (R32) on = (rt >> (e & 31)) & (e < 32);
            else on = rt != kNoRoute && ((G(P.path_mask)[2 * (size_t)rt + (e >> 6)] >> (e & 63)) & 1ull);   // rt: a validated path
            if (!on) continue;
            const int lo = (int)(range[i] & 0xFFFFu), sig = (int)(range[i] >> 16), hi = sig < S ? sig + 1 : sig;
            if (contested) {                                     // every cell: the lowest index stays
                for (int s = lo; s < hi; s++) atomicMin(&row[s], ((uint32_t)i << 1) | (uint32_t)(s == sig));
            } else {                                             // no cell of this row has two claimants: the ranges are disjoint,
                row[lo] = (uint32_t)i;                           // and a claimed cell belongs to the nearest start at or below it
                atomicOr(&starts[lo >> 6], 1ull << (lo & 63));
            }
        }
        wave_sync();
        int16_t *o = owner_out + ((size_t)replica * E + e) * S;
        for (int s = lane; s < S; s += kWave) {
            const int w = s >> 6, bit = s & 63;
            int v = ((occ[e * W + w] >> bit) & 1ull) ? kOwnerFree : kOwnerUnowned;
            if (contested) {
                const uint32_t k = row[s];
                if (k != ~0u) v = (k & 1u) ? -2 - (int)(k >> 1) : (int)(k >> 1);
            } else if ((claimed[e * W + w] >> bit) & 1ull) {
                int ww = w;
                unsigned long long m = starts[w] & (~0ull >> (63 - bit));   // the starts at or below s
                while (!m && ww > 0) m = starts[--ww];           // bounded by the row words
                if (m) {
                    const uint32_t i = row[ww * 64 + 63 - __clzll((long long)m)];
                    if (i < (uint32_t)A) v = s < (int)(range[i] >> 16) ? (int)i : -2 - (int)i;
                }
            }
            o[s] = (int16_t)v;
        }
        wave_sync();
    }
}

}  // namespace ongym
