// ongym_score.hpp — a weighted candidate-scoring policy with the weights given by the caller, one weight vector per replica
// (ongym_score_actions, include/ongym_score.h): every candidate placement of the pending request gets ten features, the
// candidate with the lowest w . x among those that pass QoT wins, and its step action index is returned.
//
// The candidates and their GSNR are policy_highest_snr's (ongym_device.hpp), expression for expression: routes k = 0..K-1 of
// the request's node pair, formats from the best down, every start of `_get_candidates` on the route row (the Vw words of
// build_field), 1/GSNR from one LDS read of the route's interferer field, qot_pass with the replica's margin.  What differs is
// the choice: highest SNR keeps the largest GSNR, this kernel the smallest weighted sum.
//
// Kernel: one wavefront per replica on the step kernels' set-up (Ctx, load_state), with the LDS block k_run has for highest
// SNR (the state block | Fx | Vw | xlist | needx).  Per route: the free row, its load (once), the field.  Per format: the
// products of the five features that only depend on (route, format) are summed once; then lanes run over starts, 64 per
// pass (one Vw word): GSNR, the QoT decision, `touch` from the route row words the lanes hold (four v_readlane pairs per
// pass: the words that hold cell s - 1 and cell s + n + 1 of any lane of the pass), the remaining five products, a wave
// minimum and a ballot for the first lane that has it.  The ten weights are wave-uniform: they are read through the constant
// address space into scalar registers.  Nothing is stored back: state, statistics and counters are untouched.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_device.hpp"
#include "ongym_fast.hpp"      // wave_min_f64

namespace ongym {

constexpr int kScoreFeatures = ONGYM_SCORE_FEATURES;   // weights per vector; best_out holds 1 + kScoreFeatures doubles per replica
constexpr int kScoreCounts = 3;                        // count_out int32 per replica: with spectrum, feasible, flags

// the field of highest SNR behind the state block, as k_run lays it out
__host__ __device__ inline size_t score_lds_bytes(const Params &P) {
    return ((lds_bytes(P) + ((size_t)2 * P.n_slots + 2) * (sizeof(double) + 2 + 1) + kMaxMods * kMaxRowWords * 8) + 15) & ~(size_t)15;
}

// bit `cell` of a lane-distributed row (word w in lane w) for a lane whose cell lies in word q0 or q0 + 1 (q0 wave-uniform)
__device__ __forceinline__ bool score_row_bit(uint64_t row, int q0, int cell) {
    const uint64_t a = readlane_u64(row, min(max(q0, 0), kWave - 1)), b = readlane_u64(row, min(max(q0 + 1, 0), kWave - 1));
    return (((cell >> 6) == q0 ? a : b) >> (cell & 63)) & 1ull;
}

template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_score_actions(const Params *__restrict__ Pp, const double *weights, int per_replica,
                                                     int32_t *actions, double *best_out, int32_t *count_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    c.fl.Fx = reinterpret_cast<double *>(smem + lds_bytes(P));
    c.fl.Vw = reinterpret_cast<uint64_t *>(c.fl.Fx + 2 * P.n_slots + 2);
    c.fl.xlist = reinterpret_cast<uint16_t *>(c.fl.Vw + kMaxMods * kMaxRowWords);
    c.fl.needx = reinterpret_cast<uint8_t *>(c.fl.xlist + 2 * P.n_slots + 2);
    c.fl.vs = kMaxRowWords;
    load_state(c);
    const int K = P.k_paths, M = P.n_mods, S = P.n_slots, max_mod = M - 1, W = P.row_words;
    double *bo = best_out ? best_out + (size_t)blockIdx.x * (1 + kScoreFeatures) : nullptr;
    int32_t *co = count_out ? count_out + (size_t)blockIdx.x * kScoreCounts : nullptr;
    if (!c.e->have_request) {   // as ongym_policy_actions answers it
        if (c.lane == 0) {
            actions[blockIdx.x] = -1;
            if (co) { co[0] = 0; co[1] = 0; co[2] = ONGYM_F_NO_REQUEST; }
        }
        if (bo && c.lane <= kScoreFeatures) bo[c.lane] = NAN;
        return;
    }
    // the replica's weights: a wave-uniform address in the constant address space, so scalar loads into scalar registers
    const auto *wv = (const __attribute__((address_space(4))) double *)(weights + (per_replica ? (size_t)blockIdx.x * kScoreFeatures : 0));
    double w[kScoreFeatures];
#pragma unroll
    for (int f = 0; f < kScoreFeatures; f++) w[f] = wv[f];
    const double band = kTieBandDb * (fabs(w[8]) + fabs(w[9]));
    const int src = c.e->cur_src, dst = c.e->cur_dst;
    const double margin = c.e->margin;

    int n_spec = 0, n_feas = 0, any_res = 0, any_osnr = 0;
    bool have = false;
    double best = INFINITY;
    int b_k = 0, b_mi = 0, b_s = 0, b_n = 0, b_hops = 0, b_touch = 0;
    double b_load = 0.0, b_gsnr = 0.0, b_margin = 0.0;
    for (int k = 0; k < K; k++) {
        const int path = k == 0 ? c.pre_id : G(P.pair_paths)[(src * P.n_nodes + dst) * K + k];
        if (path < 0) break;
        PathRef p;
        if (k == 0) { p.id = path; p.hops = c.pre_hops; p.mylink = c.pre_mylink; p.m0 = c.pre_m0; p.m1 = c.pre_m1; p.ase = c.pre_ase; p.w1 = c.pre_w1; }
        else p = load_path(c, path);
        const uint64_t free_ext = path_free_ext(c, p);
        // busy slots of the route row per hop, the quantity of policy_load_balancing (virtual guard bit excluded)
        const int freecnt = path_free_count(c, (c.lane == (S >> 6)) ? (free_ext & ~(1ull << (S & 63))) : free_ext);
        const double load = (double)(S - freecnt) / (double)p.hops;
        build_field<UA, R32>(c, p, free_ext, c.fl);
        const double pase = G(P.path_ase)[path];
        const double p6 = fp_barrier(w[6] * load);
        for (int m = max_mod; m >= 0; m--) {
            const int mi = max_mod - m;
            const int n = uniform_i32(c.nreq[m]);
            if (n <= 0) continue;
            const double thr = P.mod_thr[m] + margin, lim = c.lim[m], bw = P.slot_bw * n;
            const double self = path_self_term<UA>(c, p, n), nlic = G(P.nli_coef)[n] * c.rp[1];
            // x0..x4 only depend on (route, format): their part of the sum once, every product and sum rounded on its own
            double base = fp_barrier(w[0] * (double)k);
            base = fp_barrier(base + fp_barrier(w[1] * (double)p.hops));
            base = fp_barrier(base + fp_barrier(w[2] * (double)mi));
            base = fp_barrier(base + fp_barrier(w[3] * (double)n));
            base = fp_barrier(base + fp_barrier(w[4] * (double)(n * p.hops)));
            const int qe = (n + 1) >> 6;      // cell s + n + 1 of a start in word i lies in word i + qe or i + qe + 1
            int nvalid = 0;
            for (int i = 0; i < W; i++) {
                const uint64_t vw = c.fl.Vw[mi * c.fl.vs + i];
                if (!vw) continue;
                const int s = i * 64 + c.lane;
                const bool valid = ((vw >> c.lane) & 1ull) && s < S;
                nvalid += __popcll((unsigned long long)__ballot(valid));
                double osnr = 0.0;
                bool pass = false;
                if (valid) {
                    const double fc = P.f0 + (P.slot_bw * s) + (P.slot_bw * (n / 2.0));
                    const double acc = (bw * fc * pase) * c.rp[0] + nlic * (self + c.fl.Fx[2 * s + n]);
                    osnr = -10.0 * log10(acc);
                    pass = qot_pass(acc, lim, thr);
                }
                if (__ballot(valid && !pass)) any_osnr = 1;
                const uint64_t ebal = __ballot(valid && pass);
                n_feas += __popcll((unsigned long long)ebal);
                if (!ebal) continue;
                // touch: the cell left of the block and the cell right of its guard, from the route row (lane w = word w)
                const int e = min(s + n + 1, S);
                const bool lfree = score_row_bit(free_ext, i - 1, max(s - 1, 0)), rfree = score_row_bit(free_ext, i + qe, e);
                const bool left = s == 0 || !lfree, right = e == S || !rfree;
                const int touch = (left ? 1 : 0) + (right ? 1 : 0);
                const double mgn = osnr - thr;
                double t = fp_barrier(base + fp_barrier(w[5] * (double)s));
                t = fp_barrier(t + p6);
                t = fp_barrier(t + fp_barrier(w[7] * (double)touch));
                t = fp_barrier(t + fp_barrier(w[8] * osnr));
                t = fp_barrier(t + fp_barrier(w[9] * mgn));
                const bool elig = valid && pass && t == t;            // a NaN score never wins
                if (!__ballot(elig)) continue;
                const double v = elig ? t : INFINITY;
                const double vmin = wave_min_f64(v);
                if (!have || vmin < best - band) {                    // the first minimum of the pass; later passes only beyond the band
                    const int ln = __ffsll((unsigned long long)__ballot(elig && v == vmin)) - 1;
                    have = true;
                    best = vmin;
                    b_k = k; b_mi = mi; b_s = i * 64 + ln; b_n = n; b_hops = p.hops; b_load = load;
                    b_touch = __builtin_amdgcn_readlane(touch, ln);
                    b_gsnr = readlane_f64(osnr, ln); b_margin = readlane_f64(mgn, ln);
                }
            }
            if (nvalid == 0) any_res = 1;
            n_spec += nvalid;
        }
    }
    int flags = 0;
    if (!have) {
        if (any_osnr) any_res = 0;
        flags = (any_res ? ONGYM_F_BLOCKED_RESOURCES : 0) | (any_osnr ? ONGYM_F_BLOCKED_OSNR : 0);
    }
    if (c.lane == 0) {
        actions[blockIdx.x] = have ? b_k * M * S + b_mi * S + b_s : K * M * S;
        if (co) { co[0] = n_spec; co[1] = n_feas; co[2] = flags; }
        if (bo) {
            const double x[1 + kScoreFeatures] = {best, (double)b_k, (double)b_hops, (double)b_mi, (double)b_n, (double)(b_n * b_hops),
                                                  (double)b_s, b_load, (double)b_touch, b_gsnr, b_margin};
#pragma unroll
            for (int f = 0; f <= kScoreFeatures; f++) bo[f] = have ? x[f] : NAN;
        }
    }
}

}  // namespace ongym
