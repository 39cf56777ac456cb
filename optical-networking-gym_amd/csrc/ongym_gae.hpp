// ongym_gae.hpp — generalised advantage estimation over a rollout of step records (ongym_gae, include/ongym.h).
//
// SB3's RolloutBuffer.compute_returns_and_advantage with the episode ends taken from the records: for t = T-1 .. 0
//   nnt = 1 - terminated[t],  delta_t = reward[t] + gamma V[t+1] nnt - V[t],  A_t = delta_t + c_t A_{t+1},  c_t = gamma lambda nnt
// (V[T] = last_values, A_T = 0).  An affine scan along t, independent per replica b.
// Geometry: one lane per replica (64 replicas per workgroup: every load and store is coalesced along b), up to kGaeWaves waves
// per workgroup splitting T into chunks of kGaeChunk steps held in registers, so every byte is read from HBM once.
// A SUPER-SEGMENT is the waves' chunks side by side (waves * kGaeChunk steps); they are walked from the end of the rollout:
//   1. each wave loads its chunk (delta, V, nnt in registers) and folds it with a zero carry into (prod c, A at the chunk start);
//   2. the summaries meet in LDS; each wave combines those of the chunks after its own with the super-segment's carry
//      (A after its last step, kept in LDS) into its own carry, then replays the recurrence from it and stores A and A + V;
//   3. wave 0's first A is the carry of the next super-segment.
// Steps past T and lanes past the batch are identities (delta 0, c 1): every wave takes every barrier.  Workgroups never talk
// to each other.  The replay is the sequential recurrence itself, so NaN / inf follow it (0 * NaN = NaN through c = 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ongym.h"

namespace ongym {

constexpr int kGaeWaves = 16;       // waves per workgroup at most
constexpr int kGaeChunk = 16;       // steps per wave and super-segment

// grid (ceil(batch / 64)), block 64 * waves (waves = min(kGaeWaves, ceil(steps / kGaeChunk)))
__global__ __launch_bounds__(64 * kGaeWaves) void k_gae(const uint8_t *__restrict__ recs, const float *__restrict__ values,
                                                        const float *__restrict__ last_values, int steps, int batch, int waves,
                                                        float gamma, float gl, float *__restrict__ adv, float *__restrict__ ret) {
    __shared__ float s_prod[kGaeWaves][64], s_part[kGaeWaves][64], s_carry[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + lane;
    const bool live = b < batch;
    const int bc = live ? b : batch - 1;                      // loads stay in bounds without a branch
    const int seg = waves * kGaeChunk;
    if (wave == 0) s_carry[lane] = 0.f;                       // A_T = 0
    for (int t_seg = (steps - 1) / seg * seg; t_seg >= 0; t_seg -= seg) {
        const int t0 = t_seg + wave * kGaeChunk;
        float d[kGaeChunk], v[kGaeChunk], n[kGaeChunk];
#pragma unroll
        for (int i = 0; i < kGaeChunk; i++) {
            const int tc = min(t0 + i, steps - 1);
            const size_t k = (size_t)tc * batch + bc;
            v[i] = values[k];
            const uint8_t *rec = recs + k * sizeof(ongym_step_rec);
            d[i] = (float)*reinterpret_cast<const double *>(rec + offsetof(ongym_step_rec, reward));
            n[i] = 1.f - (float)rec[offsetof(ongym_step_rec, terminated)];
        }
        const float v_after = t0 + kGaeChunk < steps ? values[(size_t)(t0 + kGaeChunk) * batch + bc] : last_values[bc];
#pragma unroll
        for (int i = 0; i < kGaeChunk; i++) {
            const float vn = t0 + i + 1 >= steps ? last_values[bc] : i + 1 < kGaeChunk ? v[i + 1] : v_after;
            const bool in = live && t0 + i < steps;
            d[i] = in ? d[i] + gamma * vn * n[i] - v[i] : 0.f;
            n[i] = in ? gl * n[i] : 1.f;                        // from here on n holds c_t
        }
        float part = 0.f, prod = 1.f;
#pragma unroll
        for (int i = kGaeChunk - 1; i >= 0; i--) { part = d[i] + n[i] * part; prod *= n[i]; }
        s_part[wave][lane] = part;
        s_prod[wave][lane] = prod;
        __syncthreads();
        float a = s_carry[lane];
        for (int w = waves - 1; w > wave; w--) a = s_part[w][lane] + s_prod[w][lane] * a;
#pragma unroll
        for (int i = kGaeChunk - 1; i >= 0; i--) {
            a = d[i] + n[i] * a;
            if (live && t0 + i < steps) {
                const size_t k = (size_t)(t0 + i) * batch + b;
                adv[k] = a;
                ret[k] = a + v[i];
            }
        }
        __syncthreads();                                      // every wave has read s_carry and the summaries
        if (wave == 0) s_carry[lane] = a;
    }
}

}  // namespace ongym
