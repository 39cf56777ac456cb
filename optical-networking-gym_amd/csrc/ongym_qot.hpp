// ongym_qot.hpp — current quality of transmission of every running lightpath of every replica (ongym_service_qot,
// include/ongym.h): the GSNR / ASE / NLI of core/osnr.pyx:21-142 of each running service at its own path, slot and slot count,
// against every other running service of the replica at the replica's current launch power, itself skipped (with id tracking:
// every running service with its service_id, quirk Q12, core/osnr.pyx:65), plus per-replica and per-link aggregates.
//
// Kernel: one wavefront per replica on the step kernels' set-up (Ctx, load_state).  The records are taken in chunks of 64:
// for record iy of the chunk (wave-uniform loop) the interferer list is built with iy left out (gn_build_list<R32, true>; with
// id tracking skip_id = sq[iy] leaves out iy and its namesakes) and gn_eval<UA, R32> gives its linear ASE / NLI, which lane
// iy - base keeps in registers.  After the chunk every lane converts its record to dB (four log10 across 64 lanes instead of
// one per wave-uniform service), decides the two "below" tests like the step does, folds the record into its per-lane replica
// aggregates and into the per-link accumulators in LDS (count and below count by ds_add_u32, the lowest margin as an
// order-preserving u32 key of its float32 value by ds_min_u32: the float32 of a minimum is the minimum of the float32s).
// Records at or beyond `active` are written as NaN.  Nothing is stored back: state, statistics and counters are untouched.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_device.hpp"

namespace ongym {

constexpr int kServiceQot = ONGYM_N_SERVICE_QOT;   // svc_out doubles per record: GSNR, ASE, NLI (dB), margin
constexpr int kReplicaQot = ONGYM_N_REPLICA_QOT;   // replica_out doubles per replica
constexpr int kLinkQot = ONGYM_N_LINK_QOT;         // link_out floats per link

// LDS: the state block | lim0 f64[8] | link count u32[E] | link below count u32[E] | link min-margin key u32[E]
__host__ __device__ inline size_t qot_lds_bytes(const Params &P) {
    return (lds_bytes(P) + 64 + (size_t)P.n_links * 12 + 15) & ~(size_t)15;
}

// below_minimum_osnr / qot_ok for a value per lane (theirs make the decision wave-uniform): 1/GSNR `acc` against the linear limit
// `lim` = 10^(-thr_db/10), inside the band kQotBand the reference's dB expression 10 log10(1/acc) < thr_db
__device__ __forceinline__ bool below_lane(double acc, double lim, double thr_db) {
    if (acc >= lim * (1.0 + kQotBand)) return true;
    if (acc <= lim * (1.0 - kQotBand)) return false;
    return 10.0 * log10(1.0 / acc) < thr_db;
}

// float32 -> u32 with the same order (no NaN reaches it)
__device__ __forceinline__ uint32_t f32_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// Linear ASE / NLI of running record iy (wave-uniform) at its own path, slot and slot count against every other running record
// of the replica: iy itself is left out of the interferer list; with id tracking, iy and every running namesake (quirk Q12),
// as gn_service_acc skips them
template <bool UA, bool R32>
__device__ __forceinline__ GnLin gn_running(Ctx &c, int iy) {
    const uint32_t ay = c.sa[iy], by = c.sb[iy];
    const int py = uniform_i32(rec_path<R32>(ay, by)), sy = uniform_i32(rec_slot<R32>(ay, by));
    const int ny = uniform_i32(rec_n<R32>(ay, by));
    const PathRef p = load_path(c, py);
    int L;
    if (c.P.track_ids) {
        c.skip_id = uniform_i32((int)c.sq[iy]);
        L = gn_build_list<R32>(c, p.m0, p.m1);
    } else {
        L = gn_build_list<R32, true>(c, p.m0, p.m1, iy);
    }
    return gn_eval<UA, R32>(c, p, L, sy, ny, coef_for_slots(c, ny));
}

template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_service_qot(const Params *__restrict__ Pp, double *svc_out, double *replica_out,
                                                    float *link_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    double *lim0 = reinterpret_cast<double *>(smem + lds_bytes(P));
    uint32_t *lcnt = reinterpret_cast<uint32_t *>(lim0 + 8), *lbel = lcnt + P.n_links, *lmin = lbel + P.n_links;
    const int E = P.n_links, C = P.capacity, lane = c.lane;
    for (int e = lane; e < E; e += kWave) { lcnt[e] = 0; lbel[e] = 0; lmin[e] = ~0u; }
    if (lane < P.n_mods) lim0[lane] = pow(10.0, -P.mod_thr[lane] / 10.0);   // the expression of load_state
    load_state(c);                                                          // (its wave_sync orders the stores above)
    const int active = c.active;
    const double margin = c.e->margin;
    int below0 = 0, belowm = 0, min_i = 0x7FFFFFFF;
    double sum_g = 0.0, min_m = INFINITY;
    for (int base = 0; base < C; base += kWave) {
        double la = 1.0, ln = 1.0;   // linear ASE / NLI of record base + lane
        const int nb = min(kWave, active - base);
        for (int j = 0; j < nb; j++) {
            const GnLin g = gn_running<UA, R32>(c, base + j);
            if (lane == j) { la = g.ase; ln = g.nli; }
        }
        const int i = base + lane;                                           // < C: capacity is a multiple of 64
        double *o = svc_out ? svc_out + ((size_t)c.replica * C + i) * kServiceQot : nullptr;
        if (i >= active) {
            if (o) { o[0] = NAN; o[1] = NAN; o[2] = NAN; o[3] = NAN; }
        } else {
            const uint32_t a = c.sa[i], b = c.sb[i];
            const int m = rec_mod<R32>(a, b);
            const double acc = la + ln;
            const double gsnr = -10.0 * log10(acc), mg = gsnr - P.mod_thr[m];    // gn_to_db
            if (o) { o[0] = gsnr; o[1] = -10.0 * log10(la); o[2] = -10.0 * log10(ln); o[3] = mg; }
            const bool b0 = below_lane(acc, lim0[m], P.mod_thr[m]);              // measure_disruptions' test (qrmsa.pyx:947)
            const bool bm = below_lane(acc, c.lim[m], P.mod_thr[m] + margin);     // !qot_ok
            below0 += b0;
            belowm += bm;
            sum_g += gsnr;
            if (mg < min_m) { min_m = mg; min_i = i; }                           // ascending i per lane: the lowest index on a tie
            if (link_out) {
                const uint32_t key = f32_key((float)mg);
                uint64_t m0, m1;
                if (R32) { m0 = a; m1 = 0; }
                else { const int pk = a & 0xFFFF; m0 = G(P.path_mask)[2 * pk]; m1 = G(P.path_mask)[2 * pk + 1]; }
                while (m0 | m1) {
                    int l;
                    if (m0) { l = __ffsll((unsigned long long)m0) - 1; m0 &= m0 - 1; }
                    else { l = 64 + __ffsll((unsigned long long)m1) - 1; m1 &= m1 - 1; }
                    atomicAdd(&lcnt[l], 1u);
                    if (b0) atomicAdd(&lbel[l], 1u);
                    atomicMin(&lmin[l], key);
                }
            }
        }
    }
    wave_sync();
    if (link_out) {
        float *lo = link_out + (size_t)c.replica * E * kLinkQot;
        for (int e = lane; e < E; e += kWave) {
            lo[kLinkQot * e] = (float)lcnt[e];
            lo[kLinkQot * e + 1] = lcnt[e] ? key_f32(lmin[e]) : NAN;
            lo[kLinkQot * e + 2] = (float)lbel[e];
        }
    }
    if (!replica_out) return;
    below0 = wave_sum_i32(below0);
    belowm = wave_sum_i32(belowm);
    sum_g = wave_sum(sum_g);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {                                      // (lowest margin, lowest index)
        const double om = __shfl_xor(min_m, s);
        const int oi = __shfl_xor(min_i, s);
        if (om < min_m || (om == min_m && oi < min_i)) { min_m = om; min_i = oi; }
    }
    if (lane < kReplicaQot) {
        const double v[kReplicaQot] = {(double)active, (double)below0, (double)belowm, active ? min_m : NAN,
                                       active ? sum_g / (double)active : NAN, active ? (double)min_i : -1.0};
        double r = v[0];
        for (int k = 1; k < kReplicaQot; k++) r = lane == k ? v[k] : r;
        replica_out[(size_t)c.replica * kReplicaQot + lane] = r;
    }
}

}  // namespace ongym
