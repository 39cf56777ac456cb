// ongym_metrics.hpp — per-link spectrum fragmentation metrics of every replica (ongym_link_metrics, include/ongym.h): the free
// and used runs of every link row, the metrics of utils.pyx:61-107 on the free runs, the network compactness of
// _get_network_compactness (envs/qrmsa.pyx:1150-1186) and, in place in a caller-owned buffer, the time-weighted link statistics
// of _update_link_stats (envs/qrmsa.pyx:1353-1480) with the reference's arithmetic and quirks.
//
// Kernel: one wavefront per replica.  The replica's n_links x row_words words of occ are staged into LDS (lane i loads word i,
// bits at and above S cleared), then every lane takes one link (e = lane, lane + 64, ...) and walks its row run by run: the
// next free slot at or after the position by a bit scan over the words, then the next used slot after it.  One walk gives the
// free-slot count, the free runs (count, longest, sum of squares, sum of p ln p from the entropy table of the lowest-fragmentation
// score), the used runs and the occupied span.  The slot-hops of the running services come from the lanes striding over the
// service records (rec_n, rec_path).  Nothing is stored back: replica state and statistics are untouched.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_device.hpp"

namespace ongym {

constexpr int kLinkMetrics = ONGYM_N_LINK_METRICS;   // link_out floats per link
constexpr int kLinkStats = ONGYM_N_LINK_STATS;       // link_stats doubles per link

__host__ __device__ inline size_t metrics_lds_bytes(const Params &P) { return (size_t)P.n_links * P.row_words * 8; }

// the first position >= pos of the row (W words) whose bit is set in x ^ flip, or `none`
__device__ __forceinline__ int next_bit(const uint64_t *row, int W, int pos, uint64_t flip, int none) {
    int w = pos >> 6;
    uint64_t x = (row[w] ^ flip) & (~0ull << (pos & 63));
    while (!x && ++w < W) x = row[w] ^ flip;
    return x ? w * 64 + (__ffsll((unsigned long long)x) - 1) : none;
}

struct LinkRuns {
    int free, nfree, lmax, sum2, nused, lo, hi;   // hi - lo: occupied span (lo = first used slot, hi = one past the last)
    double plogp;                                 // sum of (L/S) ln(L/S) over the free runs
};

// One link row (1 = free, nothing set at or above S): its runs, walked alternately free / used.  plogp[L] = (L/S) ln(L/S) (Params).
__device__ __forceinline__ LinkRuns link_runs(const uint64_t *row, int W, int S, const double *plogp) {
    LinkRuns r{0, 0, 0, 0, 0, 0, 0, 0.0};
    int pos = 0;
    while (pos < S) {
        const int a = next_bit(row, W, pos, 0ull, S);            // next free slot
        if (a > pos) {                                           // used run [pos, a)
            if (r.nused == 0) r.lo = pos;
            r.nused++;
            r.hi = a;
        }
        if (a >= S) break;
        const int b = min(next_bit(row, W, a, ~0ull, S), S);     // next used slot (the bits at and above S read as used)
        const int L = b - a;                                     // free run [a, b)
        r.free += L;
        r.nfree++;
        r.lmax = max(r.lmax, L);
        r.sum2 += L * L;
        r.plogp += G(plogp)[L];
        pos = b;
    }
    return r;
}

template <bool R32>
__global__ __launch_bounds__(64) void k_link_metrics(const Params *__restrict__ Pp, float *link_out, double *compactness,
                                                     double *link_stats) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    const int lane = threadIdx.x, replica = blockIdx.x;
    const int E = P.n_links, W = P.row_words, S = P.n_slots;
    uint64_t *occ = reinterpret_cast<uint64_t *>(smem);
    const uint64_t *g = P.occ + (size_t)replica * E * W;
    for (int i = lane; i < E * W; i += kWave) occ[i] = g[i] & word_range(i % W, 0, S);
    wave_sync();
    const DevEnv *de = P.env + replica;
    const double now = de->st.current_time;
    int occupied = 0, inner = 0;     // compactness: over the links with more than one used run
    for (int e = lane; e < E; e += kWave) {
        const LinkRuns r = link_runs(occ + (size_t)e * W, W, S, P.plogp);
        const size_t le = (size_t)replica * E + e;
        if (r.nused > 1) { occupied += r.hi - r.lo; inner += r.nused - 1; }   // one free run between two used runs
        if (link_out) {
            float *o = link_out + le * kLinkMetrics;
            o[0] = (float)r.free;
            o[1] = (float)r.nfree;
            o[2] = (float)r.lmax;
            o[3] = (float)r.nused;
            o[4] = (float)(r.nused ? r.hi - r.lo : 0);
            o[5] = r.free ? (float)(1.0 - (double)r.lmax / (double)r.free) : 0.f;
            o[6] = (float)(0.0 - r.plogp);
            o[7] = r.free ? (float)(sqrt((double)r.sum2) / (double)r.free) : 0.f;
        }
        if (link_stats) {            // _update_link_stats (envs/qrmsa.py:516-560), every product rounded on its own
            double *s = link_stats + le * kLinkStats;
            const double util = s[0], frag = s[1], comp = s[2], last = s[3];
            const double dt = now - last;
            const int used = S - r.free;
            double u = util;
            if (now > 0.0) u = (fp_barrier(util * last) + fp_barrier(((double)used / (double)S) * dt)) / now;
            const bool ends_only = r.nfree == 2 && (occ[(size_t)e * W] & 1ull) &&
                                   ((occ[(size_t)e * W + ((S - 1) >> 6)] >> ((S - 1) & 63)) & 1ull);
            const int max_empty = (r.nfree > 1 && !ends_only) ? r.lmax : 0;
            const double cf = r.free > 0 ? 1.0 - (double)max_empty / (double)used : 1.0;   // used = 0: 0/0 = NaN
            double cc = 1.0;
            if (r.nused > 1) cc = ((double)(r.hi - r.lo) / (double)used) * (1.0 / (double)r.nused);
            s[0] = u;
            s[1] = (fp_barrier(frag * last) + fp_barrier(cf * dt)) / now;
            s[2] = (fp_barrier(comp * last) + fp_barrier(cc * dt)) / now;
            s[3] = now;
        }
    }
    if (!compactness) return;
    // slot-hops of the running services: sum of nslots * hops (bounded by E * S, an int)
    const int active = de->st.active;
    const size_t off = (size_t)replica * P.capacity;
    int hops = 0;
    for (int i = lane; i < active; i += kWave) {
        const uint32_t a = P.svc_a[off + i], b = P.svc_b[off + i];
        hops += rec_n<R32>(a, b) * G(P.path_hops)[rec_path<R32>(a, b)];
    }
    occupied = wave_sum_i32(occupied);
    inner = wave_sum_i32(inner);
    hops = wave_sum_i32(hops);
    if (lane == 0) compactness[replica] = inner > 0 ? ((double)occupied / (double)hops) * ((double)E / (double)inner) : 1.0;
}

}  // namespace ongym
