// ongym_playout.hpp — playouts (ongym_playout, include/ongym.h): per replica, per candidate action of a caller's list and per
// sample, the candidate applied to the pending request and then H requests decided by a policy, on a future of the scenario's
// own.  What comes back is a handful of counters: how many of those requests were blocked, how much bit rate was carried.
//
// Kernel: one wavefront per (replica b, action a, sample r) on the step kernels' set-up (Ctx, load_state).  Every wavefront
// works on its own LDS copy of the replica and stores nothing back; the LDS is the state block and nothing else.
//   0. unless the replica's own source continues: the stream's key and counter in the LDS DevEnv are replaced as ongym_seed_base
//      replaces them in memory, key = ongym_stream_key(seed + r, replica_base + b), counter 0.  The pending request, the clock
//      and everything else stay.  The A candidates of a replica get the same key: they see the same future.
//   1. the first step as k_run's action step takes it: evaluate_action on the candidate, or the policy for an index < 0, then
//      apply_step (provision, bookkeeping, disruptions, next request, departures).  Retry and QoT error end the scenario: the
//      step would not consume the request.
//   2. up to H iterations of k_run's policy step: policy_first_fit or policy_load_balancing, apply_step.  The scenario ends
//      after the terminal step of the episode and when the source has no further request.
//   3. lanes 0..7 store the eight columns.
// apply_step runs with rec = nullptr (no record, no per-step log10) and LOCAL = true (no terminal snapshot, no auto reset).
// The counters are wave-uniform registers.  Stores to global memory: the eight columns and nothing else (DESIGN section 17
// lists every device function the loop reaches).  Every loop is bounded by H, K, M or the loaded `active`.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ongym_device.hpp"

namespace ongym {

constexpr int kPlayout = ONGYM_N_PLAYOUT;   // playout_out doubles per (replica, action, sample)
constexpr int kMaxPlayoutActions = ONGYM_MAX_PLAYOUT_ACTIONS;
constexpr int kMaxPlayoutSamples = ONGYM_MAX_PLAYOUT_SAMPLES;
constexpr int kMaxPlayoutScenarios = ONGYM_MAX_PLAYOUT_SCENARIOS;   // A * R per replica: the second grid dimension when replicas are fastest
constexpr int kMaxPlayoutHorizon = ONGYM_MAX_PLAYOUT_HORIZON;

template <bool UA, bool R32, int POLICY>
__device__ __forceinline__ int playout_policy(Ctx &c, Choice &ch) {
    const DevEnv *e = c.e;
    const int src = e->cur_src, dst = e->cur_dst;
    const double lp = e->launch_power, mg = e->margin;
    if (POLICY == ONGYM_POLICY_LOAD_BALANCING) policy_load_balancing<UA, R32>(c, src, dst, lp, mg, ch);
    else policy_first_fit<UA, R32>(c, src, dst, lp, mg, ch);
    return ch.route >= 0 ? 0 : 1;           // neither policy proposes busy slots (k_run's outcome 2 is exact fit's)
}

// by_replica: grid (batch, A * R), the replicas fastest in dispatch order; else grid (batch * A * R), a replica's scenarios
// adjacent (DESIGN section 17 has both measured)
template <bool UA, bool R32, int POLICY>
__global__ __launch_bounds__(64) void k_playout(const Params *__restrict__ Pp, int A, int R, int by_replica,
                                                const int32_t *__restrict__ actions, int H, uint64_t seed, uint64_t replica_base,
                                                int own_stream, double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    const int AR = A * R;
    const int b = by_replica ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)AR);
    const int ar = by_replica ? (int)blockIdx.y : (int)(blockIdx.x % (unsigned)AR);
    const int a = ar / R, r = ar % R;
    Ctx c(P);
    ctx_open(c, smem, b);
    const int lane = c.lane;
    double *o = out + ((size_t)b * AR + ar) * kPlayout;
    load_state(c);
    DevEnv *e = c.e;

    int status = 4, first = 0, steps = 0, acc = 0;
    double br_acc = 0.0, br_req = 0.0;
    if (uniform_i32(e->have_request)) {
        if (!own_stream) {
            if (lane == 0) { e->rng_key = ongym_stream_key(seed + (uint64_t)r, replica_base + (uint64_t)b); e->req_index = 0; }
            wave_sync();
        }
        // ---- 1. the first step
        const int action = actions ? uniform_i32(G(actions)[(size_t)b * A + a]) : -1;
        Choice ch;
        int outcome;
        if (action >= 0) {
            outcome = uniform_i32(evaluate_action<UA, R32>(c, e->cur_src, e->cur_dst, e->launch_power, e->margin, action, ch));
            status = outcome >= 2 ? outcome : 0;
        } else {
            outcome = uniform_i32(playout_policy<UA, R32, POLICY>(c, ch));
            status = 1;
        }
        if (status < 2) {
            first = outcome == 0 && c.active < P.capacity;                   // apply_step rejects at capacity (overflow)
            apply_step<R32, false, true>(c, ch, outcome, nullptr);
            // apply_step's own test of the terminal step, on the counter the draw of the next request advanced
            bool done = uniform_i32((int)e->st.episode_services_processed) == P.episode_length;
            // ---- 2. the policy's steps
            for (int it = 0; it < H && !done; ++it) {
                if (!uniform_i32(e->have_request)) break;                    // the source has no further request
                const double br = (double)uniform_f32(e->cur_br);            // before apply_step consumes the request
                Choice cp;
                const int oc = uniform_i32(playout_policy<UA, R32, POLICY>(c, cp));
                const int ok = oc == 0 && c.active < P.capacity;
                apply_step<R32, false, true>(c, cp, oc, nullptr);
                steps++;
                acc += ok;
                br_req += br;
                if (ok) br_acc += br;
                done = uniform_i32((int)e->st.episode_services_processed) == P.episode_length;
            }
        }
    }
    // ---- 3. the eight columns, one per lane
    double v = (double)status;
    v = lane == 1 ? (double)first : v;
    v = lane == 2 ? (double)steps : v;
    v = lane == 3 ? (double)acc : v;
    v = lane == 4 ? (double)(steps - acc) : v;
    v = lane == 5 ? br_acc : v;
    v = lane == 6 ? br_req : v;
    v = lane == 7 ? (double)c.active : v;
    if (status >= 2 && lane > 0) v = NAN;
    if (lane < kPlayout) o[lane] = v;
}

}  // namespace ongym
