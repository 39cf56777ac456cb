// ongym_policy_head.hpp — masked categorical action head (ongym_masked_categorical / _backward, include/ongym.h).
//
// The distribution sb3-contrib's MaskableCategorical builds over the env's action mask (the reference's
// examples/ONDM_2025/train_multi_masked_ppo.py), evaluated exactly: masked entries do not exist, whatever their logit holds.
// One wavefront per row, one pass over the row:
//   forward   online softmax  m = max x,  s = sum e^(x-m),  t = sum e^(x-m)(x-m)   (on a max move m -> m':
//             t <- e^(m-m')(t + (m-m')s), s <- e^(m-m')s),  log p_j = (x_j - m) - log s,  H = log s - t/s;
//             sample mode draws by Gumbel-max in the same pass, argmax mode keeps the first largest valid logit;
//             the chosen / given action's logit is read once more after the pass (one element per row);
//             the row stats (m, log s) are saved for the backward: x - m is exact near m, so log p does not lose
//             ulp(m) to a rounded m + log s (shift invariance, as torch's log_softmax)
//   backward  grad_j = valid_j ? g_lp (delta_ja - p_j) - g_H p_j (log p_j + H) : 0,  log p_j = (x_j - m) - log s
// Non-finite valid logits: -inf adds e^-inf = 0 to s and nothing to t (no 0 * inf: the running max starts at -FLT_MAX, and
// e^d d is taken at max(d, -FLT_MAX)), so the row is the one with that entry masked, bit for bit; its gradient is 0.
// NaN or +inf makes s NaN; a state merges whenever s != 0, so the NaN reaches the row's log_prob and entropy.
// The row length n = k*Mc*S + 1 is odd, so rows start at any element.  A lane works on CHUNKS of 8 elements aligned on
// the GLOBAL element index (logits base 16-byte aligned, mask base 8-byte aligned: one 16 B (bf16) or two 16 B (f32) loads
// plus one 8 B mask load per chunk); the first and last chunk of a row are partial and read element by element.
// The forward also reads the mask as packed bits (HeadMask<ONGYM_MASK_BITS>, ongym_masked_categorical_rows): a chunk's 8 bits
// are cut from one or two words, as the backward cuts them.  The row count is an argument of both kernels (any R).
// Uniforms of the Gumbel draws: the counter-based generator of include/ongym_traffic.h.  Key of (row, draw) =
// stream_key(stream_key(seed ^ kHeadDomain, global replica), draw_index): every draw is a stream of its own, so the counters
// of one draw run 0, 1, 2, ... (a counter of draw * 2^32 + pair leaves the low half of the finaliser's input the same in
// every draw).  One 64-bit word per PAIR of entries (counter = entry / 2, upper half for the even entry), 24 bits each
// (head_gumbel).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/ongym.h"
#include "../../include/ongym_traffic.h"

namespace ongym {

constexpr uint64_t kHeadDomain = 0xD1B54A32D192ED03ull;   // ongym_sample_actions keys its stream with another constant
constexpr int kHeadWaves = 4;                             // rows (wavefronts) per workgroup

template <int DT> struct HeadElem;
template <> struct HeadElem<ONGYM_DTYPE_F32> {
    using T = float;
    __device__ static inline float get(const float *p, long long i) { return p[i]; }
    __device__ static inline void load8(const float *p, long long g, float x[8]) {      // g % 8 == 0
        const float4 a = *reinterpret_cast<const float4 *>(p + g), b = *reinterpret_cast<const float4 *>(p + g + 4);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    }
    __device__ static inline void put(float *p, long long i, float v) { p[i] = v; }
    __device__ static inline void store8(float *p, long long g, const float v[8]) {
        *reinterpret_cast<float4 *>(p + g) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4 *>(p + g + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
};
template <> struct HeadElem<ONGYM_DTYPE_BF16> {
    using T = uint16_t;
    __device__ static inline float cvt(uint32_t h) { return __uint_as_float(h << 16); }
    __device__ static inline uint32_t rne(float v) {         // f32 -> bf16, round to nearest even (NaN kept quiet)
        const uint32_t u = __float_as_uint(v);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
        return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    }
    __device__ static inline float get(const uint16_t *p, long long i) { return cvt(p[i]); }
    __device__ static inline void load8(const uint16_t *p, long long g, float x[8]) {
        const uint4 w = *reinterpret_cast<const uint4 *>(p + g);
        const uint32_t a[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; i++) { x[2 * i] = __uint_as_float(a[i] << 16); x[2 * i + 1] = __uint_as_float(a[i] & 0xFFFF0000u); }
    }
    __device__ static inline void put(uint16_t *p, long long i, float v) { p[i] = (uint16_t)rne(v); }
    __device__ static inline void store8(uint16_t *p, long long g, const float v[8]) {
        uint4 w;
        w.x = rne(v[0]) | (rne(v[1]) << 16); w.y = rne(v[2]) | (rne(v[3]) << 16);
        w.z = rne(v[4]) | (rne(v[5]) << 16); w.w = rne(v[6]) | (rne(v[7]) << 16);
        *reinterpret_cast<uint4 *>(p + g) = w;
    }
};

// 8 mask bytes -> 8 bits (nonzero = valid)
__device__ static inline uint32_t head_mask_bits(uint2 w) {
    uint32_t b = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        b |= ((w.x >> (8 * e)) & 0xFFu) ? 1u << e : 0u;
        b |= ((w.y >> (8 * e)) & 0xFFu) ? 1u << (e + 4) : 0u;
    }
    return b;
}

// Gumbel noise -log(-log u) from 24 random bits, u = (k + 1/2) 2^-24 strictly inside (0, 1): above 1/2 the sum rounds to
// an even k (the value stays the centre of the two k it stands for), and k = 2^24 - 1 would round to 1, hence the clamp.
// The inner log is the accurate one: for u near 1, -log u is tiny and the hardware log's error is large relative to it.
__device__ static inline float head_gumbel(uint32_t bits24) {
    const float u = fminf(((float)bits24 + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
    return -__logf(-logf(u));
}

// Per-lane running state of the forward pass
struct HeadAcc {
    float m = -FLT_MAX, s = 0.f, t = 0.f;      // online softmax + entropy (s = 0: nothing folded; s NaN: poisoned)
    float key = -INFINITY;                     // best Gumbel key / logit
    int idx = 0x7FFFFFFF;                      // its entry (first on ties)
};

// move the lane's max to mm > a.m.  d = -inf (an f32 overflow of the difference) gives r = 0: the guard keeps 0 * inf out of t.
// A NaN s stays NaN.
__device__ static inline void head_rescale(HeadAcc &a, float mm) {
    const float d = a.m - mm, r = __expf(d);
    a.t = r > 0.f ? r * (a.t + d * a.s) : 0.f;
    a.s *= r;
    a.m = mm;
}

// fold valid entries {x[e] : bit e of vb} at row entries j0 + e into the lane state
template <int MODE>
__device__ static inline void head_fold(HeadAcc &a, const float x[8], uint32_t vb, long long j0, uint64_t key) {
    float cm = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; e++) cm = ((vb >> e) & 1u) ? fmaxf(cm, x[e]) : cm;
    if (cm > a.m) head_rescale(a, cm);         // the max moves
    uint64_t hw[5];
    if (MODE == ONGYM_HEAD_SAMPLE) {
        const long long p0 = j0 >> 1;          // j0 >= 0 here; entries j0..j0+7 span pairs p0..p0+4
#pragma unroll
        for (int q = 0; q < 5; q++)
            hw[q] = (q < 4 || (j0 & 1)) ? ongym_mix64(key + ((uint64_t)(p0 + q) + 1) * 0x9E3779B97F4A7C15ull) : 0;
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
        if (!((vb >> e) & 1u)) continue;
        const float d = x[e] - a.m, p = __expf(d);
        a.s += p;
        a.t = fmaf(p, fmaxf(d, -FLT_MAX), a.t);        // x = -inf: p = 0, d = -inf
        const int j = (int)(j0 + e);
        float k = x[e];
        if (MODE == ONGYM_HEAD_SAMPLE) {
            const bool odd = j0 & 1;                         // entry j0 + e lies in pair p0 + (e + odd) / 2
            const uint64_t w = odd ? hw[(e + 1) >> 1] : hw[e >> 1];
            k += head_gumbel((uint32_t)((((j & 1) ? w : (w >> 32)) & 0xFFFFFFFFull) >> 8));
        }
        if (k > a.key) { a.key = k; a.idx = j; }      // entries rise within a lane: strict > keeps the first
    }
}

// the same for a partial chunk, element by element (any j0, some entries outside the row: vb already excludes them)
template <int MODE>
__device__ static inline void head_fold_one(HeadAcc &a, float x, long long j, uint64_t key) {
    if (x > a.m) head_rescale(a, x);
    const float d = x - a.m, p = __expf(d);
    a.s += p;
    a.t = fmaf(p, fmaxf(d, -FLT_MAX), a.t);
    float k = x;
    if (MODE == ONGYM_HEAD_SAMPLE) {
        const uint64_t w = ongym_mix64(key + ((uint64_t)(j >> 1) + 1) * 0x9E3779B97F4A7C15ull);
        k += head_gumbel((uint32_t)((((j & 1) ? w : (w >> 32)) & 0xFFFFFFFFull) >> 8));
    }
    if (k > a.key) { a.key = k; a.idx = (int)j; }      // as in head_fold (a key of -inf is never taken)
}

// combine two lane states (b into a).  s != 0, not s > 0: a NaN s (a NaN or +inf logit) must reach the result.
__device__ static inline void head_merge(HeadAcc &a, float m, float s, float t, float key, int idx) {
    if (s != 0.f) {
        if (a.s != 0.f) {
            const float mm = fmaxf(a.m, m), da = a.m - mm, db = m - mm, ra = __expf(da), rb = __expf(db);
            a.t = (ra > 0.f ? ra * (a.t + da * a.s) : 0.f) + (rb > 0.f ? rb * (t + db * s) : 0.f);
            a.s = ra * a.s + rb * s;
            a.m = mm;
        } else { a.m = m; a.s = s; a.t = t; }
    }
    if (key > a.key || (key == a.key && idx < a.idx)) { a.key = key; a.idx = idx; }
}

// 8 bits of a packed row (entries j0 .. j0+7, 0 <= j0, j0 + 8 <= nact): they may straddle two words, and word w + 1 exists
// whenever they do
__device__ static inline uint32_t head_bits8(const uint32_t *rb, long long j0) {
    const int w = (int)(j0 >> 5), sh = (int)(j0 & 31);
    uint64_t v = rb[w];
    if (sh > 24) v |= (uint64_t)rb[w + 1] << 32;
    return (uint32_t)(v >> sh) & 0xFFu;
}

// The caller's mask in either format (ONGYM_MASK_BYTES: uint8 [rows][nact]; ONGYM_MASK_BITS: uint32 [rows][nw], the layout
// the forward writes to mask_bits).  `full` reads the 8 entries of a whole chunk, `one` a single entry of the row.
template <int MF> struct HeadMask;
template <> struct HeadMask<ONGYM_MASK_BYTES> {
    using T = uint8_t;
    __device__ static inline uint32_t full(const uint8_t *m, long long gc8, long long, long long, int) {
        return head_mask_bits(*reinterpret_cast<const uint2 *>(m + gc8));
    }
    __device__ static inline bool one(const uint8_t *m, long long g0, long long, long long j, int) { return m[g0 + j] != 0; }
};
template <> struct HeadMask<ONGYM_MASK_BITS> {
    using T = uint32_t;
    __device__ static inline uint32_t full(const uint32_t *m, long long, long long row, long long j0, int nw) {
        return head_bits8(m + row * nw, j0);
    }
    __device__ static inline bool one(const uint32_t *m, long long, long long row, long long j, int nw) {
        return (m[row * nw + (j >> 5)] >> (j & 31)) & 1u;
    }
};

// Forward: grid (ceil(rows / kHeadWaves)), block 64 * kHeadWaves, dynamic LDS kHeadWaves * nwords * 4 (mask bits out).
// MODE: ONGYM_HEAD_SAMPLE / _ARGMAX / _EVALUATE (actions read).  MF: format of the caller's mask (bits_out is null with bits).
template <int DT, int MODE, int MF>
__global__ __launch_bounds__(64 * kHeadWaves) void k_head_fwd(const typename HeadElem<DT>::T *__restrict__ logits,
                                                              const typename HeadMask<MF>::T *__restrict__ mask, int batch, int nact,
                                                              uint64_t seed, uint64_t replica_base, uint64_t draw,
                                                              int32_t *__restrict__ actions, float *__restrict__ log_prob,
                                                              float *__restrict__ entropy, float *__restrict__ stats_out,
                                                              uint32_t *__restrict__ bits_out) {
    using E = HeadElem<DT>;
    using M = HeadMask<MF>;
    extern __shared__ __align__(16) uint32_t head_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * kHeadWaves + wave;
    const int nw = (nact + 31) >> 5;
    uint32_t *bits = head_lds + wave * nw;
    const bool live = row < batch;
    if (bits_out)
        for (int i = lane; i < nw; i += 64) bits[i] = 0;
    __syncthreads();
    HeadAcc a;
    const long long g0 = (long long)row * nact;               // first element of the row
    const int s0 = (int)(g0 & 7);                             // its offset in the first chunk
    const int nch = (s0 + nact + 7) >> 3;                     // chunks touched by the row
    const uint64_t key = ongym_stream_key(ongym_stream_key(seed ^ kHeadDomain, replica_base + (uint64_t)row), draw);
    const long long gc = g0 - s0;                             // global index of chunk 0
    if (live) {
        for (int c = lane; c < nch; c += 64) {
            const long long j0 = 8ll * c - s0;                // row entry of the chunk's element 0
            uint32_t vb;
            float x[8];
            if (j0 >= 0 && j0 + 8 <= nact) {
                vb = M::full(mask, gc + 8ll * c, row, j0, nw);
                if (vb) {
                    E::load8(logits, gc + 8ll * c, x);
                    head_fold<MODE>(a, x, vb, j0, key);
                }
            } else {
                vb = 0;
                for (int e = 0; e < 8; e++) {
                    const long long j = j0 + e;
                    if (j < 0 || j >= nact || !M::one(mask, g0, row, j, nw)) continue;
                    vb |= 1u << e;
                    head_fold_one<MODE>(a, E::get(logits, g0 + j), j, key);
                }
            }
            if (bits_out && vb) {                             // bits j0 .. j0+7 of the row (j0 may be negative)
                const long long b = j0 + 32;                  // one word up keeps the bit position positive
                const uint64_t v = (uint64_t)vb << (b & 31);
                const int w = (int)(b >> 5) - 1;
                if (w >= 0 && (uint32_t)v) atomicOr(&bits[w], (uint32_t)v);
                if (w + 1 < nw && (uint32_t)(v >> 32)) atomicOr(&bits[w + 1], (uint32_t)(v >> 32));
            }
        }
    }
    // wave reduction of the lane states
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m = __shfl_xor(a.m, o), s = __shfl_xor(a.s, o), t = __shfl_xor(a.t, o), k = __shfl_xor(a.key, o);
        const int i = __shfl_xor(a.idx, o);
        head_merge(a, m, s, t, k, i);
    }
    __syncthreads();
    if (!live) return;
    if (bits_out) {
        uint32_t *dst = bits_out + (size_t)row * nw;
        for (int i = lane; i < nw; i += 64) dst[i] = bits[i];
    }
    if (lane != 0) return;
    const bool any = a.s != 0.f;                              // NaN s (poisoned row) included
    const bool ok = a.s > 0.f;                                // some finite valid logit, no NaN / +inf
    const float ls = __logf(a.s);
    const float H = any ? ls - a.t / a.s : NAN;
    int act;
    float lp;
    if (MODE == ONGYM_HEAD_EVALUATE) {
        act = actions[row];
        lp = (act >= 0 && act < nact && M::one(mask, g0, row, act, nw)) ? (E::get(logits, g0 + act) - a.m) - ls : -INFINITY;
    } else {
        act = (any && a.idx < nact) ? a.idx : nact - 1;        // no valid finite entry (a caller error): reject, NaN
        lp = (E::get(logits, g0 + act) - a.m) - ls;
        actions[row] = act;
    }
    if (!ok) lp = NAN;
    if (log_prob) log_prob[row] = lp;
    if (entropy) entropy[row] = H;
    if (stats_out) {
        stats_out[2 * (size_t)row] = any ? a.m : NAN;
        stats_out[2 * (size_t)row + 1] = any ? ls : NAN;
    }
}

// Backward: same geometry, no LDS.  g_lp / g_H may be null (zero).
template <int DT>
__global__ __launch_bounds__(64 * kHeadWaves) void k_head_bwd(const typename HeadElem<DT>::T *__restrict__ logits,
                                                              const uint32_t *__restrict__ bits, int batch, int nact,
                                                              const int32_t *__restrict__ actions, const float *__restrict__ stats,
                                                              const float *__restrict__ entropy, const float *__restrict__ g_lp,
                                                              const float *__restrict__ g_H,
                                                              typename HeadElem<DT>::T *__restrict__ grad) {
    using E = HeadElem<DT>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * kHeadWaves + wave;
    if (row >= batch) return;
    const int nw = (nact + 31) >> 5;
    const uint32_t *rb = bits + (size_t)row * nw;
    const long long g0 = (long long)row * nact;
    const int s0 = (int)(g0 & 7);
    const int nch = (s0 + nact + 7) >> 3;
    const long long gc = g0 - s0;
    const float M = stats[2 * (size_t)row], LS = stats[2 * (size_t)row + 1], H = entropy[row];
    const float glp = g_lp ? g_lp[row] : 0.f, gH = g_H ? g_H[row] : 0.f;
    const int act = actions[row];
    for (int c = lane; c < nch; c += 64) {
        const long long j0 = 8ll * c - s0;
        if (j0 >= 0 && j0 + 8 <= nact) {
            const uint32_t vb = head_bits8(rb, j0);
            float g[8];
            if (vb) {
                float x[8];
                E::load8(logits, gc + 8ll * c, x);
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const float lp = (x[e] - M) - LS, p = __expf(lp);
                    const float d = (j0 + e == act) ? 1.f : 0.f;
                    const float h = p == 0.f ? 0.f : p * (lp + H);        // p = 0: lp may be -inf
                    g[e] = (((vb >> e) & 1u) && x[e] != -INFINITY) ? glp * (d - p) - gH * h : 0.f;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++) g[e] = 0.f;
            }
            E::store8(grad, gc + 8ll * c, g);
        } else {
            for (int e = 0; e < 8; e++) {
                const long long j = j0 + e;
                if (j < 0 || j >= nact) continue;
                float gv = 0.f;
                const float x = E::get(logits, g0 + j);
                if (((rb[j >> 5] >> (j & 31)) & 1u) && x != -INFINITY) {
                    const float lp = (x - M) - LS, p = __expf(lp);
                    gv = glp * ((j == act ? 1.f : 0.f) - p) - gH * (p == 0.f ? 0.f : p * (lp + H));
                }
                E::put(grad, g0 + j, gv);
            }
        }
    }
}

}  // namespace ongym
