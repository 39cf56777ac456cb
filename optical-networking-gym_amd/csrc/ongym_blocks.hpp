// ongym_blocks.hpp — the block action space (ongym_observe_blocks, include/ongym.h): for every replica's current request, the
// first J free spectrum blocks of every candidate route that fit the request, their decoded format and GSNR, the mask and the map
// from block action to the full action index of ongym_step_actions.  The action space of DeepRMSA / optical-rl-gym, which the
// reference still carries as `blocks_to_consider` and get_available_blocks (envs/qrmsa.pyx:231, 242, 1515-1531).
//
// Definition (per replica, request (src, dst, bit rate), K routes, M formats, S slots):
//   row(k)        AND of the free bits of route k's links (get_available_slots)
//   n(m)          get_number_slots(request, m), exactly as the step computes it (load_state)
//   Blocks(k, m)  the maximal free runs [a, a+L) of row(k), in increasing a, that hold a candidate of _get_candidates
//                 (envs/qrmsa.pyx:515-541): L >= n(m) if the run ends at S, else L >= n(m) + 1 (the guard slot); the first J
//   decode (k, j) best format first: the first m with Blocks(k, m)[j] = (a, L) whose calculate_osnr at (route k, slot a,
//                 n(m)) passes qot_ok; first fit's order (heuristics.py:923-966).  So block (k, 0) is first fit on route k.
//
// Kernel: one wavefront per replica on k_observe's set-up (Ctx, load_state: the step's n(m), acceptance limits, GN
// coefficients and interferer skip id).  Per route: the row's words one per lane (path_free_ext), run starts
// free & ~(free << 1), fitting starts = run starts & run_and(row + virtual slot S, n + 1); the j-th fitting start by a scan of
// the per-lane popcounts, and its run length by a walk over the row's words in LDS.  The QoT decisions go through
// gn_build_list / gn_eval / qot_ok with the step kernel's template arguments, so a valid block action is never refused by the
// step.  Nothing is stored back: replica state and statistics are untouched.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_device.hpp"

namespace ongym {

constexpr int kMaxBlocks = ONGYM_MAX_BLOCKS;

// LDS behind the state block: row u64[kMaxRowWords] | start u16[kMaxMods][kMaxBlocks] | length u16[kMaxMods][kMaxBlocks] |
// count i32[kMaxMods]
__host__ __device__ inline size_t blocks_lds_offset(const Params &P) { return (lds_bytes(P) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t blocks_lds_bytes(const Params &P) {
    const size_t extra = (size_t)kMaxRowWords * 8 + (size_t)2 * kMaxMods * kMaxBlocks * 2 + (size_t)kMaxMods * 4;
    return (blocks_lds_offset(P) + extra + 15) & ~(size_t)15;
}

__host__ __device__ inline int blocks_obs_dim(int K, int J) { return 3 + 3 * K + 6 * K * J; }

// position of the r-th set bit (0-based) of w, r < popcount(w)
__device__ __forceinline__ int nth_set_bit(uint64_t w, int r) {
    int pos = 0;
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        const uint64_t lo = w & ((1ull << h) - 1ull);
        const int c = __popcll((unsigned long long)lo);
        if (r >= c) { r -= c; w >>= h; pos += h; }
        else w = lo;
    }
    return pos;
}

template <bool UNIFORM_ALPHA, bool R32>
__device__ __forceinline__ void observe_blocks_env(Ctx &c, int J, uint64_t *row, uint16_t *bst, uint16_t *blen, int *bcnt,
                                                   float *obs, uint8_t *mask, int32_t *amap) {
    const Params &P = c.P;
    const int K = P.k_paths, M = P.n_mods, S = P.n_slots, N = P.n_nodes, W = P.row_words;
    const int KJ = K * J;
    const int reject = K * M * S;
    const DevEnv *e = c.e;
    const bool have = e->have_request != 0;
    const int src = e->cur_src, dst = e->cur_dst;
    const double margin = e->margin;
    float *pfeat = obs + 3 + K;            // 2 per route
    float *bfeat = obs + 3 + 3 * K;        // 6 per (route, block), route-major
    if (c.lane == 0) {                     // ongym_observe's first 3 + K entries (zeros without a request)
        obs[0] = have ? (float)((double)e->cur_br / P.max_bit_rate) : 0.f;
        obs[1] = have ? (float)((double)src / (double)(N - 1)) : 0.f;
        obs[2] = have ? (float)((double)dst / (double)(N - 1)) : 0.f;
        mask[KJ] = 1;
        amap[KJ] = reject;
    }
    for (int k = 0; k < K; k++) {
        const int path = have ? uniform_i32(G(P.pair_paths)[(src * N + dst) * K + k]) : -1;
        if (c.lane == 0) obs[3 + k] = path >= 0 ? (float)P.path_len_norm[path] : 0.f;
        if (path < 0) {
            if (c.lane == 0) { pfeat[2 * k] = -1.f; pfeat[2 * k + 1] = -1.f; }
            if (c.lane < J) {
                float *f = bfeat + 6 * (k * J + c.lane);
                f[0] = 0.f; f[1] = -1.f; f[2] = -1.f; f[3] = -1.f; f[4] = -1.f; f[5] = -1.f;
                mask[k * J + c.lane] = 0;
                amap[k * J + c.lane] = reject;
            }
            continue;
        }
        PathRef p = load_path(c, path);
        const uint64_t ext = path_free_ext(c, p);
        // the row itself: no virtual slot S, nothing at or past S
        const uint64_t aw = ext & word_range(c.lane, 0, S);
        if (c.lane < kMaxRowWords) row[c.lane] = aw;
        const int tot = wave_sum_i32(c.lane < W ? __popcll((unsigned long long)aw) : 0);
        const int longest = longest_run(aw);
        const uint64_t starts = aw & ~shift_left1(aw);
        if (c.lane == 0) { pfeat[2 * k] = (float)((double)tot / (double)S); pfeat[2 * k + 1] = (float)((double)longest / (double)S); }
        wave_sync();
        // ---- Blocks(k, m) of every format: starts and run lengths of the first J, and their count
        uint64_t runs = ext;
        int r = 1;
        for (int m = M - 1; m >= 0; m--) {
            const int n = uniform_i32(c.nreq[m]);
            int cnt = 0;
            if (n > 0 && n <= S) {
                if (n + 1 < r) { runs = ext; r = 1; }
                runs = run_and(runs, r, n + 1);
                const uint64_t fit = runs & starts;
                const int pc = __popcll((unsigned long long)fit);
                int incl = pc;
#pragma unroll
                for (int d = 1; d < kMaxRowWords; d <<= 1) { const int u = __shfl_up(incl, d); if (c.lane >= d) incl += u; }
                cnt = __builtin_amdgcn_readlane(incl, kMaxRowWords - 1);
                const int pre = incl - pc;
                if (c.lane < kMaxRowWords && pc > 0 && pre < J) {
                    const int take = min(pc, J - pre);
                    for (int t = 0; t < take; t++) {
                        const int a = c.lane * 64 + nth_set_bit(fit, t);
                        int w = a >> 6;
                        uint64_t z = ~row[w] & (~0ull << (a & 63));          // used slots at or after a
                        while (!z && ++w < W) z = ~row[w];
                        const int end = z ? min(w * 64 + (__ffsll((unsigned long long)z) - 1), S) : S;
                        bst[m * kMaxBlocks + pre + t] = (uint16_t)a;
                        blen[m * kMaxBlocks + pre + t] = (uint16_t)(end - a);
                    }
                }
            }
            if (c.lane == 0) bcnt[m] = cnt;
        }
        wave_sync();
        // ---- decode every block action of the route: best format first, first pass wins
        int L = -1;                        // interferer list of the route, built on the first evaluation
        int last_a = -1, last_n = -1;      // formats of equal slot count share the evaluation of a start
        GnLin last_g{0.0, 0.0};
        for (int j = 0; j < J; j++) {
            int vm = -1, va = 0, vl = 0, vn = 0;
            GnLin vg{0.0, 0.0};
            for (int m = M - 1; m >= 0; m--) {
                if (uniform_i32(bcnt[m]) <= j) continue;
                const int a = uniform_i32(bst[m * kMaxBlocks + j]);
                const int n = uniform_i32(c.nreq[m]);
                GnLin g;
                if (a == last_a && n == last_n) {
                    g = last_g;
                } else {
                    if (P.ase_shortcut) {      // the exact lower bound of policy_first_fit: a fail here fails gn_eval too
                        const double bw = P.slot_bw * n;
                        const double fc = P.f0 + (P.slot_bw * a) + (P.slot_bw * (n / 2.0));
                        double lb = (bw * fc * p.ase) * c.rp[0];
                        if (UNIFORM_ALPHA) lb += c.nlic[m] * (p.w1 * c.selfa[m]);
                        if (uniform_i32(lb >= c.lim[m] * (1.0 + kQotBand))) continue;
                    }
                    if (L < 0) L = gn_build_list<R32>(c, p.m0, p.m1);
                    g = gn_eval<UNIFORM_ALPHA, R32>(c, p, L, a, n, coef_for_mod(c, m));
                    g.ase = uniform_f64(g.ase); g.nli = uniform_f64(g.nli);
                    last_a = a; last_n = n; last_g = g;
                }
                if (qot_ok(c, g, m, margin)) {
                    vm = m; va = a; vn = n; vg = g;
                    vl = uniform_i32(blen[m * kMaxBlocks + j]);
                    break;
                }
            }
            if (c.lane == 0) {
                float *f = bfeat + 6 * (k * J + j);
                if (vm >= 0) {
                    const double gsnr = -10.0 * log10(vg.ase + vg.nli);              // gn_to_db
                    f[0] = 1.f; f[1] = (float)((double)va / (double)S); f[2] = (float)((double)vl / (double)S);
                    f[3] = (float)((double)vn / (double)S); f[4] = (float)((double)(vm + 1) / (double)M);
                    f[5] = (float)((gsnr - P.mod_thr[vm] - margin) / 10.0);
                    mask[k * J + j] = 1;
                    amap[k * J + j] = k * M * S + (M - 1 - vm) * S + va;   // get_action_index, max_modulation_idx = M - 1
                } else {
                    f[0] = 0.f; f[1] = -1.f; f[2] = -1.f; f[3] = -1.f; f[4] = -1.f; f[5] = -1.f;
                    mask[k * J + j] = 0;
                    amap[k * J + j] = reject;
                }
            }
        }
        wave_sync();                       // row / bst / blen / bcnt are rewritten for the next route
    }
}

template <bool UNIFORM_ALPHA, bool R32>
__global__ __launch_bounds__(64) void k_observe_blocks(const Params *__restrict__ Pp, int J, float *obs, uint8_t *mask,
                                                       int32_t *amap) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    load_state(c);
    unsigned char *x = smem + blocks_lds_offset(P);
    uint64_t *row = reinterpret_cast<uint64_t *>(x);
    uint16_t *bst = reinterpret_cast<uint16_t *>(row + kMaxRowWords);
    uint16_t *blen = bst + kMaxMods * kMaxBlocks;
    int *bcnt = reinterpret_cast<int *>(blen + kMaxMods * kMaxBlocks);
    const size_t nout = (size_t)P.k_paths * J + 1;
    observe_blocks_env<UNIFORM_ALPHA, R32>(c, J, row, bst, blen, bcnt, obs + (size_t)c.replica * blocks_obs_dim(P.k_paths, J),
                                           mask + (size_t)c.replica * nout, amap + (size_t)c.replica * nout);
}

}  // namespace ongym
