// ongym_hip.hip — kernels + C ABI (include/ongym.h) of the MI355X-native batched QRMSA environment.
// Build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared -o libongym_hip.so ongym_hip.hip   (see __graft_entry__.build)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include <map>
#include <mutex>
#include <utility>

#include "ongym_device.hpp"
#include "ongym_host.hpp"
#include "ongym_fast.hpp"      // fast_lds_bytes, PathRec (the kernels themselves: ongym_fast.hip)
#include "ongym_tables.hpp"    // config_check, derive_tables: the host half of create (with ongym_lwtab.hpp)
#include "ongym_scored.hpp"
#include "ongym_policy_head.hpp"   // masked categorical action head (ongym_masked_categorical)
#include "ongym_gae.hpp"           // GAE over a rollout (ongym_gae)
#include "ongym_state.hpp"         // save / restore / fork of replica states (ongym_state_*, ongym_fork)
#include "ongym_blocks.hpp"        // block action space: observation, mask and action map (ongym_observe_blocks)
#include "ongym_metrics.hpp"       // per-link fragmentation metrics and link statistics (ongym_link_metrics)
#include "ongym_qot.hpp"           // current QoT of every running lightpath (ongym_service_qot)
#include "ongym_impact.hpp"        // effect of candidate actions on the running lightpaths (ongym_action_impact)
#include "ongym_failure.hpp"       // link failures and first-fit restoration (ongym_failure_impact, ongym_failure_sets)
#include "ongym_cut.hpp"           // link failures on live replicas (ongym_cut_links, ongym_repair_links, ongym_failed_links)
#include "ongym_spectrum.hpp"      // slot owners, batched records and the state audit (ongym_spectrum_map)
#include "ongym_move.hpp"          // running lightpaths moved on live replicas (ongym_move_services)
#include "ongym_admission.hpp"     // first-fit admission of every node pair and bit rate (ongym_admission_map)
#include "ongym_playout.hpp"       // candidate actions followed by H policy steps on a private copy (ongym_playout)
#include "ongym_score.hpp"         // weighted candidate scoring, weights per replica (ongym_score_actions)

using namespace ongym;

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
// WAVES = waves per SIMD the register allocation is bounded for: 5 when the replica's LDS block is <= 8 KiB (20 replicas
// per CU), else 4
constexpr int kPolicyMisc = 3;   // template value of the shared instantiation for policy ids >= ONGYM_POLICY_LOWEST_SPECTRUM

template <bool UA, bool R32, int WAVES, int POLICY, bool DEFRAG = false>
__global__ __launch_bounds__(64, WAVES) void k_run(const Params *__restrict__ Pp, int run_mode, int nsteps, const int32_t *actions, int32_t *act_out,
                                            uint8_t *flag_out, ongym_step_rec *out, int policy_id) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
#ifdef ONGYM_STAMPS
    for (int i = 0; i < ONGYM_NSTAMPS; i++) c.stamp_acc[i] = 0;
    c.stamp_last = __builtin_amdgcn_s_memtime();
#endif
    if (POLICY == ONGYM_POLICY_HIGHEST_SNR) {   // extra LDS: Fx f64[2S+2] | Vw u64[8*16] | xlist u16[2S+2] | needx u8[2S+2]
        c.fl.Fx = reinterpret_cast<double *>(smem + lds_bytes(P));
        c.fl.Vw = reinterpret_cast<uint64_t *>(c.fl.Fx + 2 * P.n_slots + 2);
        c.fl.xlist = reinterpret_cast<uint16_t *>(c.fl.Vw + kMaxMods * kMaxRowWords);
        c.fl.needx = reinterpret_cast<uint8_t *>(c.fl.xlist + 2 * P.n_slots + 2);
        c.fl.vs = kMaxRowWords;
    }
    load_state(c);
    STAMP(c, 8);
    for (int it = 0; it < nsteps; ++it) {
        DevEnv *e = c.e;
        // kModeActionThenPolicy (the single-environment surface, ongym_step_actions_bundle): iteration 0 applies the action,
        // iteration 1 evaluates the policy on the request that step drew - the same code, no second launch
        const int mode = run_mode == kModeActionThenPolicy ? (it == 0 ? kModeActionStep : kModePolicyOnly) : run_mode;
        ongym_step_rec *rec = (out && mode != kModePolicyOnly) ? out + (size_t)it * P.batch + c.replica : nullptr;
        if (!e->have_request) {   // no request source / trace exhausted: the step is a no-op
            if (c.lane == 0) {
                e->st.flags |= ONGYM_F_NO_REQUEST;
                if (rec) { memset(rec, 0, sizeof(*rec)); rec->action = -1; rec->route = rec->modulation = rec->slot = -1;
                           rec->flags = ONGYM_F_NO_REQUEST; rec->active = c.active; }
                if (mode == kModePolicyOnly) { act_out[c.replica] = -1; if (flag_out) flag_out[c.replica] = ONGYM_F_NO_REQUEST; }
            }
            wave_sync();
            continue;
        }
        int src = e->cur_src, dst = e->cur_dst;
        float br = e->cur_br;
        double lp = e->launch_power, mg = e->margin;
        (void)br;
        STAMP(c, 0);
        Choice ch;
        int outcome;
        if (mode == kModeActionStep) {
            outcome = evaluate_action<UA, R32>(c, src, dst, lp, mg, actions[c.replica], ch);
        } else {
            if (POLICY == ONGYM_POLICY_HIGHEST_SNR) policy_highest_snr<UA, R32>(c, src, dst, lp, mg, ch);
            else if (POLICY == ONGYM_POLICY_LOAD_BALANCING) policy_load_balancing<UA, R32>(c, src, dst, lp, mg, ch);
            else if (POLICY == kPolicyMisc) policy_misc<UA, R32>(c, policy_id, src, dst, mg, ch);
            else if (POLICY == kPolicyScored)
                policy_scored<UA, R32>(c, policy_id, src, dst, mg, ch, reinterpret_cast<int32_t *>(smem + ((lds_bytes(P) + 15) & ~(size_t)15)));
            else policy_first_fit<UA, R32>(c, src, dst, lp, mg, ch);
            outcome = ch.route >= 0 ? (ch.busy ? 2 : 0) : 1;
            if (POLICY == kPolicyScored && mode == kModePolicyStep && ch.route >= 0) {
                // `env.step(action)` evaluates the GN model itself, at the width the format needs (lowest fragmentation asked
                // for one slot more): the reference raises ValueError if that fails (envs/qrmsa.pyx:925-929) — a fused
                // episode rejects the request instead and flags it
                outcome = evaluate_action<UA, R32>(c, src, dst, lp, mg, ch.action, ch);
                if (outcome == 3) {
                    outcome = 1;
                    ch.action = P.k_paths * P.n_mods * P.n_slots; ch.route = -1; ch.mod = -1; ch.slot = -1; ch.n = 0;
                    ch.flags = ONGYM_F_QOT_ERROR | ONGYM_F_BLOCKED_OSNR;
                }
            }
            // modulations_to_consider < n_mods: `env.step(action)` decodes the heuristic's action index with the window codec
            // (envs/qrmsa.pyx:801-834), which need not give back what the heuristic meant (heuristics.py:36-54 encodes formats
            // outside the window past the codec's range): do what the reference's loop does
            if (P.n_mods_consider < P.n_mods && mode == kModePolicyStep && ch.route >= 0)
                outcome = evaluate_action<UA, R32>(c, src, dst, lp, mg, ch.action, ch);
        }
        if (mode == kModePolicyOnly) {
            if (c.lane == 0) { act_out[c.replica] = ch.action; if (flag_out) flag_out[c.replica] = (uint8_t)ch.flags; }
            continue;
        }
        apply_step<R32, DEFRAG>(c, ch, outcome, rec);
    }
    if (run_mode != kModePolicyOnly) store_state(c);
    STAMP(c, 9);
#ifdef ONGYM_STAMPS
    if (c.lane == 0 && P.dbg)
        for (int i = 0; i < ONGYM_NSTAMPS; i++) atomicAdd(&P.dbg[i], c.stamp_acc[i]);
#endif
}

__global__ __launch_bounds__(64) void k_reset(const Params *__restrict__ Pp, const uint8_t *mask) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (mask && !mask[blockIdx.x]) return;
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
    load_state(c);
    reset_env(c);
    store_state(c);
}

#ifndef ONGYM_OBS_WAVES
#define ONGYM_OBS_WAVES 3
#endif
template <bool UA, bool R32>
__global__ __launch_bounds__(64, ONGYM_OBS_WAVES) void k_observe(const Params *__restrict__ Pp, float *obs, uint8_t *mask) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, blockIdx.x);
#ifdef ONGYM_STAMPS
    for (int i = 0; i < ONGYM_NSTAMPS; i++) c.stamp_acc[i] = 0;
    c.stamp_last = __builtin_amdgcn_s_memtime();
#endif
    load_state(c);
    STAMPW(c, 0);
    const size_t obs_dim = 3 + P.k_paths + (size_t)P.k_paths * P.n_mods_consider * 12;
    const size_t nact = (size_t)P.k_paths * P.n_mods_consider * P.n_slots + 1;
    const ObsLayout lay = obs_layout(P);          // ongym_observe sizes the block with the same function
    double *Fx = reinterpret_cast<double *>(smem + lay.fx);
    uint16_t *xlist = reinterpret_cast<uint16_t *>(smem + lay.xlist);
    uint64_t *Vw = reinterpret_cast<uint64_t *>(smem + lay.vw);
    uint8_t *needx = smem + lay.needx;
    c.list = reinterpret_cast<uint16_t *>(smem + lay.list);
    wave_sync();
    c.fl = FieldLds{Fx, Vw, xlist, needx, lay.vs};
    observe_env<UA, R32>(c, Fx, Vw, xlist, needx, lay.vs, obs + (size_t)c.replica * obs_dim, mask + (size_t)c.replica * nact);
#ifdef ONGYM_STAMPS
    STAMPW(c, 15);
    if (c.lane == 0 && P.dbg)
        for (int i = 0; i < ONGYM_NSTAMPS; i++) atomicAdd(&P.dbg[i], c.stamp_acc[i]);
#endif
}

__global__ void k_seed(Params P, uint64_t seed, uint64_t replica_base) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.batch) return;
    P.env[r].rng_key = ongym_stream_key(seed, replica_base + (uint64_t)r);
    P.env[r].req_index = 0;
}

// reset(options={"only_episode_counters": True}) (qrmsa.pyx:427-464): the episode counters and histograms go to zero and the
// departure heap is DROPPED (self._events = []): the services that are running stay in the network for good (release time
// +inf; the 'disrupted' sign bit is kept).  Grid, running services, totals, clock and the current request are untouched.
__global__ void k_reset_counters(Params P, const uint8_t *mask) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.batch || (mask && !mask[r])) return;
    DevEnv &e = P.env[r];
    ongym_stats &s = e.st;
    e.svc_list_extra += s.episode_services_processed;   // len(graph["services"]) keeps growing from where it was
    s.episode_bit_rate_requested = 0.0; s.episode_bit_rate_provisioned = 0.0;
    s.episode_services_processed = 0; s.episode_services_accepted = 0;
    s.episode_disrupted_services = 0; s.rejected = 0;
    s.episode_defrag_cycles = 0; s.episode_service_reallocations = 0;
    for (int m = 0; m < 8; m++) s.episode_modulation_hist[m] = 0;
    s.max_modulation_idx = P.n_mods - 1;                          // :437
    float *rr = P.svc_r + (size_t)r * P.capacity;
    for (int i = 0; i < s.active; i++) rr[i] = copysignf(INFINITY, rr[i]);
}

// ongym_sample_actions: one wave per replica.  The mask bytes are 0/1: the row is read as aligned dwords (lane-contiguous,
// popcount of w & 0x01010101) plus at most six head / tail bytes; any fixed order of the entries gives a uniform choice, so
// the order is "by lane, then by the lane's strided dwords": pass 1 counts per lane, a wave scan picks the lane that holds the
// r-th valid entry, pass 2 (the same loads, L2-resident) finds it.
__global__ __launch_bounds__(64) void k_sample_mask(const uint8_t *__restrict__ mask, long long nact, uint64_t seed, uint64_t replica_base,
                                                    uint64_t draw, int32_t *__restrict__ actions) {
    const int lane = threadIdx.x;
    const long long replica = blockIdx.x;
    const uint8_t *row = mask + replica * nact;
    const uintptr_t a0 = ((uintptr_t)row + 3) & ~(uintptr_t)3, a1 = ((uintptr_t)(row + nact)) & ~(uintptr_t)3;
    const long long head = (long long)(a0 - (uintptr_t)row);                      // bytes before the aligned middle (0..3)
    const long long ndw = a1 > a0 ? (long long)((a1 - a0) >> 2) : 0;               // aligned dwords
    const long long tail0 = head + 4 * ndw;                                        // first tail byte (element index)
    const uint32_t *mid = reinterpret_cast<const uint32_t *>(a0);
    // lanes 0..2: one head byte each, lanes 3..5: one tail byte each
    long long extra = -1;
    if (lane < 3 && lane < head) extra = lane;
    if (lane >= 3 && lane < 6 && tail0 + (lane - 3) < nact) extra = tail0 + (lane - 3);
    int cnt = (extra >= 0 && row[extra]) ? 1 : 0;
    for (long long j = lane; j < ndw; j += 64) cnt += __popc(mid[j] & 0x01010101u);
    // inclusive scan of the per-lane counts
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(incl, d); if (lane >= d) incl += u; }
    const int total = __shfl(incl, 63);
    int choice = (int)(nact - 1);                                                  // the reject action (always valid)
    if (total > 0) {
        const double u = ongym_uniform(ongym_stream_key(seed ^ 0x9E3779B97F4A7C15ull, replica_base + (uint64_t)replica), draw);
        int r = (int)(u * (double)total);
        r = r >= total ? total - 1 : r;
        const uint64_t at = __ballot(incl > r);                                    // first lane whose inclusive count exceeds r
        const int owner = __builtin_ctzll(at);
        if (lane == owner) {
            int k = r - (incl - cnt);                                              // k-th valid entry of this lane (0-based)
            long long found = -1;
            if (extra >= 0 && row[extra]) { if (k == 0) found = extra; k--; }
            for (long long j = lane; j < ndw && found < 0; j += 64) {
                uint32_t w = mid[j] & 0x01010101u;
                const int c = __popc(w);
                if (k < c) {
                    for (int b = 0; b < 4; b++)
                        if ((w >> (8 * b)) & 1u) { if (k == 0) { found = head + 4 * j + b; break; } k--; }
                } else k -= c;
            }
            if (found >= 0) choice = (int)found;
            actions[replica] = choice;
        }
    } else if (lane == 0) actions[replica] = choice;
}

__global__ void k_rewind(Params P) {   // new trace: cursor back to 0
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.batch) return;
    P.env[r].req_index = 0;
}

// calculate_osnr for MANY candidates of one replica: one wavefront per candidate (cand = {path_id, slot, nslots}).
template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_query_gsnr_many(const Params *__restrict__ Pp, int replica, int count,
                                                        const int32_t *__restrict__ cand, double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    if ((int)blockIdx.x >= count) return;
    Ctx c(P);
    ctx_open(c, smem, replica);
    load_state(c);
    const int path = cand[3 * blockIdx.x], slot = cand[3 * blockIdx.x + 1], n = cand[3 * blockIdx.x + 2];
    PathRef p = load_path(c, path);
    int L = gn_build_list<R32>(c, p.m0, p.m1);
    GnLin lin = gn_eval<UA, R32>(c, p, L, slot, n);
    double g[3];
    gn_to_db(lin, g);
    if (c.lane == 0) { out[3 * blockIdx.x] = g[0]; out[3 * blockIdx.x + 1] = g[1]; out[3 * blockIdx.x + 2] = g[2]; }
}

enum { kQAvailable, kQGrid, kQServices, kQRequest, kQCandidates, kQPathFree };

// One wavefront answers one plugin-API query on one replica.  Each case has its own typed arguments: `row` (kQCandidates: the
// caller's row), `out_i` (flags per slot, the grid's bits, one flag, or the service count), `svc`, `req`; the others are null.
template <bool UA, bool R32>
__global__ __launch_bounds__(64) void k_query(const Params *__restrict__ Pp, int what, int replica, int path, int slot, int n,
                                              const int32_t *row, int32_t *out_i, ongym_service *svc, ongym_request *req) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Params &P = *Pp;
    Ctx c(P);
    ctx_open(c, smem, replica);
    load_state(c);
    if (what == kQAvailable) {          // get_available_slots(path), envs/qrmsa.pyx:1482-1512
        PathRef p = load_path(c, path);
        uint64_t x = path_free_ext(c, p);
        for (int j = 0; j < P.n_slots; j++) {
            uint64_t w = __shfl((unsigned long long)x, j >> 6);
            if (c.lane == 0) out_i[j] = (int32_t)((w >> (j & 63)) & 1ull);
        }
    } else if (what == kQGrid) {        // topology.graph["available_slots"]
        for (int i = c.lane; i < P.n_links * P.n_slots; i += kWave) {
            int l = i / P.n_slots, j = i % P.n_slots;
            out_i[i] = (int32_t)((c.occ[l * P.row_words + (j >> 6)] >> (j & 63)) & 1ull);
        }
    } else if (what == kQServices) {    // running services: the count, then the records
        if (c.lane == 0) out_i[0] = c.active;
        for (int i = c.lane; i < c.active; i += kWave) {
            uint32_t a = c.sa[i], b = c.sb[i];
            svc[i].path_id = rec_path<R32>(a, b); svc[i].slot = (int16_t)rec_slot<R32>(a, b);
            svc[i].nslots = (int16_t)rec_n<R32>(a, b); svc[i].modulation = (int16_t)rec_mod<R32>(a, b);
            svc[i].reserved = c.sr[i] < 0.f ? 1 : 0;   // 1: in the disrupted list (measure_disruptions)
            svc[i].release_time = fabsf(c.sr[i]);
            svc[i].service_id = P.track_ids ? (int32_t)c.sq[i] : -1; svc[i].pad_ = 0;
            svc[i].osnr = P.track_ids ? c.so[i] : 0.0;
        }
    } else if (what == kQCandidates) {  // _get_candidates on a caller-supplied row: path = total_slots, n = nslots
        const int total = path;
        uint64_t x = 0;
        for (int j = 0; j < 64; j++) {
            int sl = c.lane * 64 + j;
            if (sl < total && row[sl] != 0) x |= 1ull << j;
        }
        if (c.lane == (total >> 6)) x |= 1ull << (total & 63);
        int rr = 1;
        x = run_and(x, rr, n + 1);
        for (int j = 0; j < 64; j++) {
            int sl = c.lane * 64 + j;
            if (sl < total) out_i[sl] = (int32_t)((x >> j) & 1ull);
        }
    } else if (what == kQPathFree) {    // is_path_free, envs/qrmsa.pyx:1248-1264
        PathRef p = load_path(c, path);
        int rr = 1;
        uint64_t ok = run_and(path_free_ext(c, p), rr, n + 1);
        uint64_t w = __shfl((unsigned long long)ok, slot >> 6);
        if (c.lane == 0) out_i[0] = (int32_t)((w >> (slot & 63)) & 1ull);
    } else if (what == kQRequest) {
        if (c.lane == 0) {
            req->arrival_time = c.e->cur_at; req->holding_time = c.e->cur_ht; req->bit_rate = c.e->cur_br;
            req->source = (int16_t)c.e->cur_src; req->destination = (int16_t)c.e->cur_dst;
        }
    }
}

static std::string g_create_error;

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static std::mutex g_lds_mutex;
hipError_t raise_lds_limit(int device, const void *kernel, size_t bytes) {
    static std::map<std::pair<int, const void *>, size_t> limit;
    if (bytes <= 64 * 1024) return hipSuccess;        // the default limit covers it
    std::lock_guard<std::mutex> lock(g_lds_mutex);
    size_t &cur = limit[std::make_pair(device, kernel)];
    if (bytes <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) cur = bytes;
    return e;
}

// Every launch of a kernel with dynamic LDS: the kernel's limit is raised first (a no-op up to the default 64 KiB), then it runs
// with one wavefront per workgroup.
template <class... KArgs, class... Args>
static int launch_lds(ongym_env *env, void (*kernel)(KArgs...), dim3 grid, size_t lds, Args... args) {
    HIP_TRY(env, raise_lds_limit(env->cfg.device, reinterpret_cast<const void *>(kernel), lds));
    hipLaunchKernelGGL(kernel, grid, dim3(64), lds, env->stream, args...);
    HIP_TRY(env, hipGetLastError());
    return 0;
}

// A runtime value as a compile-time constant: f(std::integral_constant<T, V>) for the V of Vs equal to v (the last V if none
// is; callers validate v first).  Each V instantiates f once.
template <class T, T V, T... Vs, class F>
static auto dispatch(T v, F &&f) {
    if constexpr (sizeof...(Vs) > 0)
        if (v != V) return dispatch<T, Vs...>(v, f);
    return f(std::integral_constant<T, V>{});
}

// f(UA, R32): the state layout of the environment (uniform attenuation, 32-bit service records) as template arguments
template <class F>
static auto with_layout(const Params &P, F &&f) {
    return dispatch<bool, true, false>(P.uniform_alpha != 0, [&](auto UA) {
        return dispatch<bool, true, false>(P.rec32 != 0, [&](auto R32) { return f(UA, R32); });
    });
}

// The lean units (ongym_fast.hip): the policies that have one, each with its narrow and its wide build.  prepare_lean() prepares them
// in this order; without the first row (first fit) no lean kernel runs.
struct LeanFns {
    int (*prepare)(ongym_env *);
    int (*launch)(ongym_env *, int, ongym_step_rec *);
    int (*occupancy)(ongym_env *, int *, int *);
};
static const struct { int policy; LeanFns narrow, wide; } kLeanUnits[] = {
    {ONGYM_POLICY_FIRST_FIT, {fast_prepare_p0, fast_launch_p0, fast_occupancy_p0},
     {fast_prepare_p0w, fast_launch_p0w, fast_occupancy_p0w}},
    {ONGYM_POLICY_LOAD_BALANCING, {fast_prepare_p1, fast_launch_p1, fast_occupancy_p1},
     {fast_prepare_p1w, fast_launch_p1w, fast_occupancy_p1w}},
    {ONGYM_POLICY_HIGHEST_SNR, {fast_prepare_p2, fast_launch_p2, fast_occupancy_p2},
     {fast_prepare_p2w, fast_launch_p2w, fast_occupancy_p2w}},
    {ONGYM_POLICY_LOWEST_FRAGMENTATION, {fast_prepare_p10, fast_launch_p10, fast_occupancy_p10},
     {fast_prepare_p10w, fast_launch_p10w, fast_occupancy_p10w}},
};

// The lean unit (narrow or wide build) ongym_step_policy(policy) runs, or nullptr: the generic kernel runs.
static const LeanFns *lean_unit(const ongym_env *env, int policy) {
    if (!env->fast_ok || env->trace_used) return nullptr;
    if (!(env->P.req_mode == kReqRng || (env->P.req_mode == kReqTrace && env->trace_fast_ok))) return nullptr;
    for (const auto &u : kLeanUnits)
        if (u.policy == policy && (env->lean_policies >> policy & 1u)) return env->fast_wide ? &u.wide : &u.narrow;
    return nullptr;
}

// k_run's POLICY template argument: own instantiations for first fit, load balancing and highest SNR, one shared by the scored
// policies (ongym_scored.hpp) and one by the other ids
static int run_class(int policy) {
    if (policy == ONGYM_POLICY_HIGHEST_SNR || policy == ONGYM_POLICY_LOAD_BALANCING) return policy;
    if (policy >= ONGYM_POLICY_LOWEST_FRAGMENTATION) return kPolicyScored;
    return policy >= ONGYM_POLICY_LOWEST_SPECTRUM ? kPolicyMisc : ONGYM_POLICY_FIRST_FIT;
}

// k_run's dynamic LDS: the state block, plus the field of highest SNR (Fx, Vw, xlist, needx) or the capacity-loss scratch of
// MSCL (scored_lds_bytes; lowest fragmentation needs none)
static size_t run_lds(const ongym_env *env, int policy) {
    const Params &P = env->P;
    if (policy == ONGYM_POLICY_HIGHEST_SNR)
        return ((env->lds + ((size_t)2 * P.n_slots + 2) * (sizeof(double) + 2 + 1) + kMaxMods * kMaxRowWords * 8) + 15) & ~(size_t)15;
    if (policy == ONGYM_POLICY_MSCL) return ((env->lds + 15) & ~(size_t)15) + scored_lds_bytes(P.row_words);
    return env->lds;
}

// f(kernel, dynamic LDS bytes) of the generic step kernel that runs `policy` on this environment (action steps: first fit)
template <class F>
static int with_run_kernel(const ongym_env *env, int policy, F &&f) {
    const Params &P = env->P;
    const size_t lds = run_lds(env, policy);
    return dispatch<int, ONGYM_POLICY_HIGHEST_SNR, ONGYM_POLICY_LOAD_BALANCING, kPolicyScored, kPolicyMisc, ONGYM_POLICY_FIRST_FIT>(
        run_class(policy), [&](auto POL) {
            if (P.track_ids)   // defragmentation / service-id tracking (uniform attenuation, checked at create)
                return dispatch<bool, true, false>(P.rec32 != 0, [&](auto R32) { return f(k_run<true, R32, 4, POL, true>, lds); });
            return with_layout(P, [&](auto UA, auto R32) {
                if constexpr (POL == ONGYM_POLICY_FIRST_FIT)   // 5 waves per SIMD when the state block is <= 8 KiB
                    if (env->lds <= 8192) return f(k_run<UA, R32, 5, POL>, lds);
                return f(k_run<UA, R32, 4, POL>, lds);
            });
        });
}

static int push_params(ongym_env *env) {
    HIP_TRY(env, hipMemcpyAsync(env->d_P, &env->P, sizeof(Params), hipMemcpyHostToDevice, env->stream));
    return 0;
}

template <typename T>
static int upload(ongym_env *env, const T *src, size_t n, const T **dst) {
    void *d = nullptr;
    HIP_TRY(env, hipMalloc(&d, n ? n * sizeof(T) : sizeof(T)));
    env->allocs.push_back(d);
    if (n) HIP_TRY(env, hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T *>(d);
    return 0;
}

template <typename T>
static int dev_alloc(ongym_env *env, size_t n, T **dst, bool zero) {
    void *d = nullptr;
    HIP_TRY(env, hipMalloc(&d, n ? n * sizeof(T) : sizeof(T)));
    env->allocs.push_back(d);
    if (zero && n) HIP_TRY(env, hipMemset(d, 0, n * sizeof(T)));
    *dst = static_cast<T *>(d);
    return 0;
}

static int fail_arg(ongym_env *env, const char *msg, int code = ONGYM_E_ARG) {
    env->err = msg;
    return code;
}

static int need_source(ongym_env *env) {
    return fail_arg(env, "no request source: call ongym_seed or ongym_set_requests first", ONGYM_E_STATE);
}

// f() launches kernels on the environment's stream: ongym_last_kernel_ms reports the time between the two events
template <class F>
static int timed_launch(ongym_env *env, F &&f) {
    HIP_TRY(env, hipEventRecord(env->ev0, env->stream));
    if (const int rc = f()) return rc;
    HIP_TRY(env, hipEventRecord(env->ev1, env->stream));
    env->timed = true;
    return 0;
}

// One array of a call: the caller's pointer (null: an optional array that is not asked for), its size, whether the kernel
// reads it (kIn), writes it (kOut) or both, and, after stage_open, the pointer the kernel gets.
enum { kIn = 1, kOut = 2 };
struct Span {
    const void *host; size_t bytes; int dir;
    void *dev;
    template <class T> T *as() const { return static_cast<T *>(dev); }
};

// Device pointers for the arrays of a call, given in layout order.  With io_device they are the caller's, unless the call
// always takes host buffers (`always`: the queries).  Otherwise the arrays lie in `st` at 256-byte offsets (an array that is not
// asked for takes no room and gets a null pointer, which the kernels branch on), `st` is grown if it is too small, and the kIn
// arrays are copied in.
template <size_t N>
static int stage_open(ongym_env *env, Stage &st, Span (&sp)[N], bool always = false) {
    if (env->cfg.io_device && !always) {
        for (Span &s : sp) s.dev = const_cast<void *>(s.host);
        return 0;
    }
    size_t off[N], total = 0;
    for (size_t i = 0; i < N; i++) {
        if (!sp[i].host) sp[i].bytes = 0;
        off[i] = (total + 255) & ~(size_t)255;
        total = off[i] + sp[i].bytes;
    }
    if (st.bytes < total) {
        if (st.base) { (void)hipFree(st.base); st.base = nullptr; st.bytes = 0; }
        HIP_TRY(env, hipMalloc(&st.base, total));
        st.bytes = total;
    }
    for (size_t i = 0; i < N; i++) {
        Span &s = sp[i];
        s.dev = s.host ? static_cast<char *>(st.base) + off[i] : nullptr;
        if (s.host && (s.dir & kIn)) HIP_TRY(env, hipMemcpyAsync(s.dev, s.host, s.bytes, hipMemcpyHostToDevice, env->stream));
    }
    return 0;
}

// After the launch: the kOut arrays back to the caller and one synchronisation (nothing where stage_open staged nothing)
template <size_t N>
static int stage_close(ongym_env *env, const Span (&sp)[N], bool always = false) {
    if (env->cfg.io_device && !always) return ONGYM_OK;
    for (const Span &s : sp)
        if (s.host && (s.dir & kOut))
            HIP_TRY(env, hipMemcpyAsync(const_cast<void *>(s.host), s.dev, s.bytes, hipMemcpyDeviceToHost, env->stream));
    HIP_TRY(env, hipStreamSynchronize(env->stream));
    return ONGYM_OK;
}

// Wavefronts per scenario of k_admission_map: the pairs are split into 2, 4, 8 or 16 groups until scenarios x
// groups reach kAdmissionFill wavefronts.  Measured on NSFNET-320 (profiles/r16_admission_map.txt): 16 384 scenarios run 6 to 8 %
// faster with 8 groups than with one, from 65 536 scenarios up the groups make no difference beyond the noise of 1.5 %.
// The groups' partial sums lie in a buffer allocated at create (admission_part_rows): a call never allocates.  A split therefore
// has scenarios x groups < 2 kAdmissionFill rows, and so has one forced with ONGYM_ADMISSION_GROUPS (read at create).
constexpr size_t kAdmissionFill = 131072;
static size_t admission_part_rows(const Params &P) {
    return std::min<size_t>(2 * kAdmissionFill, (size_t)P.batch * kMaxAdmissionActions * 16);
}

// Grid order of k_playout: the A * R wavefronts of a replica re-read its state, so either they are adjacent in
// dispatch order or the replicas are fastest, as in k_failure_impact.  Both are measured in profiles/r17_playout.txt.
constexpr int kPlayoutByReplica = 0;

// At the end of create, after every allocation of build(): the buffer of the groups' partial sums (so that no call allocates, and
// the state arrays lie where they lay without it)
static int admission_prepare(ongym_env *env) {
    Stage &st = env->stage[kStageAdmissionPart];
    const size_t bytes = admission_part_rows(env->P) * kAdmissionPart * sizeof(double);
    HIP_TRY(env, hipMalloc(&st.base, bytes));
    st.bytes = bytes;
    return 0;
}

// The measurement knobs of create, read from the environment once: the three of the tables and the lean kernels (CreateKnobs),
// and the two of the admission map and the playouts, which stay with the environment
static CreateKnobs read_knobs(ongym_env *env) {
    const auto flag = [](const char *name) { const char *v = std::getenv(name); return v && v[0] == '1'; };
    CreateKnobs k;
    k.force_generic = flag("ONGYM_FORCE_GENERIC");
    k.force_wide = flag("ONGYM_FORCE_WIDE");
    k.no_lwtab = flag("ONGYM_FAST_NO_LWTAB");
    const char *g = std::getenv("ONGYM_ADMISSION_GROUPS");
    env->admission_groups = g ? std::max(0, std::atoi(g)) : 0;
    const char *o = std::getenv("ONGYM_PLAYOUT_ORDER");
    env->playout_by_replica = o ? std::atoi(o) != 0 : kPlayoutByReplica;
    return k;
}

// ---- create: config_check and derive_tables (ongym_tables.hpp, no device needed), then the steps below in build()'s order.
// The device allocations and copies keep one fixed sequence: where the state arrays lie is part of what gets timed. ----
static_assert(kCfgMaxMods == kMaxMods && kCfgMaxLinks == kMaxLinks && kCfgMaxHops == kMaxHops, "ongym_tables.hpp checks other limits");
static_assert(kCfgPathRowsLong == kPathRowsLong && kCfgPathRowsShift == kPathRowsShift && kCfgPathRowsBits == kPathRowsBits &&
              kCfgPathRowsLanes == kPathRowsLanes && kCfgPathRowsFields * kPathRowsLanes == kWave,
              "ongym_tables.hpp packs the route rows otherwise than path_and unpacks them");

// the scalar fields of Params and the per-format tables
static void set_params(ongym_env *env, const ongym_config *c, const HostTables &T) {
    Params &P = env->P;
    const int M = c->n_mods;
    P.n_nodes = c->n_nodes; P.n_links = c->n_links; P.n_paths = c->n_paths; P.k_paths = c->k_paths; P.max_hops = c->max_hops;
    P.n_mods = M; P.n_slots = c->n_slots;
    P.n_mods_consider = (c->n_mods_consider <= 0 || c->n_mods_consider > M) ? M : c->n_mods_consider;   // qrmsa.pyx:313
    P.row_words = (c->n_slots + 63) / 64;
    P.ext_words = c->n_slots / 64 + 1;
    P.batch = c->batch; P.capacity = c->capacity; P.episode_length = c->episode_length; P.auto_reset = c->auto_reset;
    P.bit_rate_mode = c->bit_rate_mode; P.br_lo = c->bit_rate_lo; P.br_hi = c->bit_rate_hi;
    P.n_bit_rates = c->bit_rate_mode == 0 ? c->n_bit_rates : 1;
    P.req_mode = kReqNone;
    P.measure_disruptions = c->measure_disruptions ? 1 : 0;
    P.defragmentation = c->defragmentation ? 1 : 0;
    P.track_ids = (c->defragmentation || c->track_service_ids) ? 1 : 0;
    P.n_defrag_services = c->n_defrag_services;
    P.f0 = c->frequency_start; P.slot_bw = c->slot_bandwidth; P.channel_width = c->channel_width;
    P.nslots_width = T.nslots_width;
    P.mean_holding = c->mean_holding_time;
    P.mean_holding_f = (float)c->mean_holding_time;
    P.max_bit_rate = c->max_bit_rate;
    if (c->bit_rate_mode == 0) env->cfg_bit_rates.assign(c->bit_rates, c->bit_rates + c->n_bit_rates);
    P.uniform_alpha = T.uniform ? 1 : 0;
    P.rec32 = T.rec32 ? 1 : 0;
    P.alpha0_cl = T.cl[0];
    P.ase_shortcut = T.ase_shortcut ? 1 : 0;
    for (int m = 0; m < M; m++) { P.mod_se[m] = T.mod_se[m]; P.mod_thr[m] = T.mod_thr[m]; P.mod_phi53[m] = T.mod_phi53[m]; }
    P.tab_nmax = T.tab_nmax; P.tab_stride = T.tab_stride;
    P.lw_tab_off = T.lw_tab_off; P.lw_tab_bytes = T.lw_tab_bytes;
    env->path_pair_err = T.path_pair_err;
    env->admission_pair_err = T.admission_pair_err;
}

// upload of a whole vector
template <typename T>
static int upload(ongym_env *env, const std::vector<T> &v, const T **dst) { return upload(env, v.data(), v.size(), dst); }

// the pair table's two pitched layouts (the first with the link-weight table behind it: freed together), where they exist
static int upload_pair_layouts(ongym_env *env, const HostTables &T) {
    if (T.pair_tab2k.empty()) return 0;
    if (const int rc = upload(env, T.pair_tab2k, &env->P.pair_tab2k)) return rc;
    return upload(env, T.pair_tabp, &env->P.pair_tabp);
}

// Every table of the configuration and of HostTables, in the order create has always allocated them.  An optional table that
// is absent leaves its pointer null and allocates nothing.
static int upload_tables(ongym_env *env, const ongym_config *c, const HostTables &T) {
    Params &P = env->P;
    const size_t N = (size_t)c->n_nodes, NP = (size_t)c->n_paths;
    const bool discrete = c->bit_rate_mode == 0;
    const size_t n_rates = discrete ? (size_t)c->n_bit_rates : 1;
    const double one = 1.0, zero = 0.0;
    int rc;
    if (!T.pair_tab.empty() &&
        (rc = upload(env, reinterpret_cast<const double2 *>(T.pair_tab.data()), T.pair_tab.size() / 2, &P.pair_tab))) return rc;
    if ((rc = upload(env, T.nreq_tab, &P.nreq_tab))) return rc;
    if ((rc = upload(env, c->pair_paths, N * N * c->k_paths, &P.pair_paths))) return rc;
    if ((rc = upload(env, T.path_pair, &env->d_path_pair))) return rc;
    if ((rc = upload(env, c->path_hops, NP, &P.path_hops))) return rc;
    if ((rc = upload(env, c->path_links, NP * c->max_hops, &P.path_links))) return rc;
    if ((rc = upload(env, T.path_mask, &P.path_mask))) return rc;
    if ((rc = upload(env, T.path_ase, &P.path_ase))) return rc;
    if ((rc = upload(env, T.path_w1, &P.path_w1))) return rc;
    if ((rc = upload(env, T.self_asinh, &P.self_asinh))) return rc;
    if ((rc = upload(env, T.nli_coef, &P.nli_coef))) return rc;
    if ((rc = upload(env, T.req_coef, &P.req_coef))) return rc;
    if ((rc = upload(env, T.w1, &P.link_w1))) return rc;
    if ((rc = upload(env, T.w2, &P.link_w2))) return rc;
    if ((rc = upload(env, T.cl, &P.link_cl))) return rc;
    if ((rc = upload(env, T.selfc, &P.link_selfc))) return rc;
    if ((rc = upload(env, discrete ? c->bit_rates : &zero, n_rates, &P.bit_rates))) return rc;
    if ((rc = upload(env, discrete ? c->bit_rate_cum : &one, n_rates, &P.bit_rate_cum))) return rc;
    if ((rc = upload(env, c->node_cum, N, &P.node_cum))) return rc;
    if (c->path_len_norm && (rc = upload(env, c->path_len_norm, NP, &P.path_len_norm))) return rc;
    if ((rc = upload(env, T.plogp, &P.plogp))) return rc;
    return upload_pair_layouts(env, T);
}

// Lean kernels (ongym_fast.hpp): whether the configuration is eligible, as far as that needs no table on the device
static bool lean_eligible(const Params &P, const ongym_config *c, const CreateKnobs &knobs, const HostTables &T, size_t flds) {
    bool ok = T.uniform && P.ase_shortcut && !P.track_ids && !P.measure_disruptions && c->bit_rate_mode == 0 &&
              P.n_mods_consider == c->n_mods &&
              c->n_bit_rates <= 8 && c->n_links <= 32 + (int)kM64HiBits && c->n_nodes <= 64 && P.pair_tab2k != nullptr;
    if (knobs.force_generic) ok = false;
    if (ok) {
        for (int b = 0; b < c->n_bit_rates; b++) {
            const double r = c->bit_rates[b];
            if (!(r > 0) || r != std::floor(r) || r > 16777216.0) ok = false;   // integer-valued, exact as float32
        }
        if (T.max_n < 1 || T.max_n > 512 || T.max_n > P.tab_nmax) ok = false;
    }
    return ok && flds <= 160 * 1024;
}

// The M64 record keeps the link set (<= 32 + kM64HiBits bits) instead of the path id: it must identify the route.
// *ok = false, and nothing uploaded: two path ids with the same link set, the generic kernel stays.
static int upload_path_hash(ongym_env *env, const HostTables &T, bool *ok) {
    Params &P = env->P;
    const int NP = P.n_paths;
    int bits = 4, rc;
    while ((1 << bits) < 4 * NP) bits++;
    std::vector<uint64_t> keys((size_t)1 << bits, ~0ull);
    std::vector<int32_t> vals((size_t)1 << bits, -1);
    for (int p = 0; p < NP && *ok; p++) {
        const uint64_t key = T.path_mask[2 * p];
        uint32_t h = path_hash_slot(key, bits);
        while (keys[h] != ~0ull && keys[h] != key) h = (h + 1u) & ((1u << bits) - 1u);
        if (keys[h] == key) *ok = false;
        keys[h] = key; vals[h] = p;
    }
    if (!*ok) return 0;
    if ((rc = upload(env, keys, &P.path_hash_keys))) return rc;
    if ((rc = upload(env, vals, &P.path_hash_vals))) return rc;
    P.path_hash_bits = bits;
    return 0;
}

// Lean kernels: eligibility (env->fast_ok), the M64 path hash and the PathRec table
static int build_lean(ongym_env *env, const ongym_config *c, const CreateKnobs &knobs, const HostTables &T) {
    Params &P = env->P;
    const int NP = c->n_paths;
    const bool m64 = !P.rec32;
    const size_t flds = fast_lds_bytes(c->n_links, P.row_words, c->capacity, m64);
    bool ok = lean_eligible(P, c, knobs, T, flds);
    int rc;
    if (ok && m64 && (rc = upload_path_hash(env, T, &ok))) return rc;
    if (!ok) return 0;
    std::vector<PathRec> recs((size_t)NP);
    for (int p = 0; p < NP; p++) {
        PathRec &r = recs[(size_t)p];
        r.hops = (uint32_t)c->path_hops[p]; r.mask_lo = (uint32_t)T.path_mask[2 * p];
        r.mask_hi = (uint32_t)(T.path_mask[2 * p] >> 32);
        r.id = (uint32_t)p; r.ase = T.path_ase[(size_t)p]; r.w1 = T.path_w1[(size_t)p];
        // one mask word: mask_hi is 0 and no lean kernel reads `id` from the record (first fit knows the route it fetched,
        // the other policies take it from pair_paths), so the two dwords carry the route's weight-table multiplier and
        // block (see PathRec) and arrive with the same scalar load.  Kernels that sum over the links ignore both.
        if (!m64 && P.lw_tab_bytes) { r.mask_hi = T.lw_mult[(size_t)p]; r.id = T.lw_loc[(size_t)p]; }
    }
    const PathRec *d_recs = nullptr;
    if ((rc = upload(env, recs, &d_recs))) return rc;
    P.path_rec = d_recs;
    // first fit's copy: the same records with the route's links spelled out in dword 0 (path_rows_word, ongym_tables.hpp)
    for (int p = 0; p < NP; p++) recs[(size_t)p].hops = path_rows_word(c, p);
    if ((rc = upload(env, recs, &d_recs))) return rc;
    P.path_rec_ff = d_recs;
    env->fast_ok = true; env->fast_m64 = m64; env->fast_lds = flds;
    // every record the lean kernels ever see carries a slot count of the traffic table (records written by the other
    // entry points included: eligibility demands discrete bit rates): none above 32 -> the narrow build
    env->fast_wide = T.max_n > 32 || knobs.force_wide;
    return 0;
}

// every replica's DevEnv, and bitmaps that start "all free" so that queries before the first reset see an empty network
static int init_state(ongym_env *env, const ongym_config *c) {
    Params &P = env->P;
    const size_t B = (size_t)c->batch;
    std::vector<DevEnv> host(B);
    memset(host.data(), 0, B * sizeof(DevEnv));
    for (size_t r = 0; r < B; r++) {
        DevEnv &d = host[r];
        d.launch_power = c->replica_launch_power_w ? c->replica_launch_power_w[r] : c->launch_power_w;
        d.margin = c->replica_margin ? c->replica_margin[r] : c->margin;
        double load = c->replica_load ? c->replica_load[r] : c->load;
        d.mean_iat = 1 / (load / c->mean_holding_time);   // set_load, envs/qrmsa.pyx:1124-1132
        d.mean_iat_f = (float)d.mean_iat;
    }
    HIP_TRY(env, hipMemcpy(P.env, host.data(), B * sizeof(DevEnv), hipMemcpyHostToDevice));
    std::vector<uint64_t> row(P.row_words);
    for (int w = 0; w < P.row_words; w++) {
        const int b = std::min(c->n_slots - 64 * w, 64);
        row[w] = b >= 64 ? ~0ull : ((1ull << b) - 1ull);
    }
    std::vector<uint64_t> all(B * c->n_links * P.row_words);
    for (size_t i = 0; i < all.size(); i++) all[i] = row[i % P.row_words];
    HIP_TRY(env, hipMemcpy(P.occ, all.data(), all.size() * 8, hipMemcpyHostToDevice));
    return 0;
}

// The mutable state: the arrays and their initial contents
static int alloc_state(ongym_env *env, const ongym_config *c) {
    Params &P = env->P;
    const size_t B = (size_t)c->batch, E = (size_t)c->n_links;
    int rc;
    if ((rc = dev_alloc(env, B * E * P.row_words, &P.occ, true))) return rc;
    if ((rc = dev_alloc(env, B * c->capacity, &P.svc_a, true))) return rc;
    if ((rc = dev_alloc(env, B * c->capacity, &P.svc_b, true))) return rc;
    if ((rc = dev_alloc(env, B * c->capacity, &P.svc_r, true))) return rc;
    if (P.track_ids) {
        if ((rc = dev_alloc(env, B * c->capacity, &P.svc_q, true))) return rc;
        if ((rc = dev_alloc(env, B * c->capacity, &P.svc_o, true))) return rc;
        if ((rc = dev_alloc(env, B * ONGYM_MOVE_LOG, &P.move_log, true))) return rc;
        if ((rc = dev_alloc(env, B, &P.move_n, true))) return rc;
    }
    if ((rc = dev_alloc(env, B, &P.env, false))) return rc;
    if ((rc = init_state(env, c))) return rc;
    env->lds = lds_bytes(P);   // the launches raise their kernel's LDS limit above 64 KiB (launch_lds)
    if (env->lds > 160 * 1024) return fail_arg(env, "state does not fit the 160 KiB LDS: lower capacity", ONGYM_E_LIMIT);
    return 0;
}

// the lean units: LDS limits; a policy whose block does not fit the CU keeps the generic kernel
static void prepare_lean(ongym_env *env) {
    if (!env->fast_ok) return;
    for (const auto &u : kLeanUnits) {
        if (env->fast_ok && (env->fast_wide ? u.wide : u.narrow).prepare(env) == 0) env->lean_policies |= 1u << u.policy;
        else if (u.policy == ONGYM_POLICY_FIRST_FIT) env->fast_ok = false;
    }
    env->err.clear();
}

static int build(ongym_env *env, const ongym_config *c) {
    int rc;
    if ((rc = config_check(*c, env->err))) return rc;
    const CreateKnobs knobs = read_knobs(env);
    HostTables T;
    derive_tables(*c, knobs, kTabPitch, T);
    set_params(env, c, T);
    if ((rc = upload_tables(env, c, T))) return rc;
    if ((rc = build_lean(env, c, knobs, T))) return rc;
    if ((rc = alloc_state(env, c))) return rc;
    prepare_lean(env);
#ifdef ONGYM_STAMPS
    if ((rc = dev_alloc(env, 16, &env->P.dbg, true))) return rc;
#endif
    if ((rc = dev_alloc(env, 1, &env->d_P, false))) return rc;
    return push_params(env);
}

// ---- save / restore / fork of replica states (kernels: ongym_state.hpp) ----
// 64-bit FNV-1a over every ongym_config field a saved state depends on, with the tables' contents (not their addresses).
// Left out: batch, device, io_device, launch_power_w, margin, load and the replica_* arrays (they travel in the state or stay).
struct Fnv64 {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void *p, size_t n) {
        const unsigned char *c = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 1099511628211ull; }
    }
    template <class T> void val(T v) { bytes(&v, sizeof v); }
    template <class T> void tab(const T *p, size_t n) {
        val<uint64_t>(p ? (uint64_t)n : ~0ull);
        if (p && n) bytes(p, n * sizeof(T));
    }
};

static uint64_t state_fingerprint(const ongym_config *c) {
    Fnv64 f;
    const size_t N = (size_t)c->n_nodes, E = (size_t)c->n_links, NP = (size_t)c->n_paths, M = (size_t)c->n_mods;
    const int32_t ints[] = {c->struct_size, c->abi_version, c->n_nodes, c->n_links, c->n_paths, c->k_paths, c->max_hops,
                            c->n_mods, c->n_slots, c->capacity, c->episode_length, c->auto_reset, c->bit_rate_mode,
                            c->n_bit_rates, c->bit_rate_lo, c->bit_rate_hi, c->measure_disruptions, c->defragmentation,
                            c->n_defrag_services, c->track_service_ids, c->n_mods_consider};
    for (int32_t v : ints) f.val(v);
    const double dbls[] = {c->frequency_start, c->slot_bandwidth, c->channel_width, c->mean_holding_time, c->max_bit_rate,
                           c->nslots_channel_width};
    for (double v : dbls) f.val(v);
    f.tab(c->pair_paths, N * N * (size_t)c->k_paths);
    f.tab(c->path_hops, NP);
    f.tab(c->path_links, NP * (size_t)c->max_hops);
    f.tab(c->link_nspans, E); f.tab(c->link_span_km, E); f.tab(c->link_alpha, E); f.tab(c->link_nf, E);
    f.tab(c->mod_se, M); f.tab(c->mod_min_osnr, M);
    const bool discrete = c->bit_rate_mode == 0;
    f.tab(discrete ? c->bit_rates : nullptr, (size_t)c->n_bit_rates);
    f.tab(discrete ? c->bit_rate_cum : nullptr, (size_t)c->n_bit_rates);
    f.tab(c->node_cum, N);
    f.tab(c->path_len_norm, NP);
    return f.h;
}

static StateArrays state_arrays(const Params &P) {
    StateArrays a{};
    a.base[kSecOcc] = reinterpret_cast<unsigned char *>(P.occ);
    a.base[kSecSvcA] = reinterpret_cast<unsigned char *>(P.svc_a);
    a.base[kSecSvcB] = reinterpret_cast<unsigned char *>(P.svc_b);
    a.base[kSecSvcR] = reinterpret_cast<unsigned char *>(P.svc_r);
    a.base[kSecSvcQ] = reinterpret_cast<unsigned char *>(P.svc_q);
    a.base[kSecSvcO] = reinterpret_cast<unsigned char *>(P.svc_o);
    a.base[kSecMoveLog] = reinterpret_cast<unsigned char *>(P.move_log);
    a.base[kSecMoveN] = reinterpret_cast<unsigned char *>(P.move_n);
    a.base[kSecEnv] = reinterpret_cast<unsigned char *>(P.env);
    return a;
}

static void set_state_arrays(Params &P, void *const base[kStateSections]) {
    P.occ = static_cast<uint64_t *>(base[kSecOcc]);
    P.svc_a = static_cast<uint32_t *>(base[kSecSvcA]);
    P.svc_b = static_cast<uint32_t *>(base[kSecSvcB]);
    P.svc_r = static_cast<float *>(base[kSecSvcR]);
    P.svc_q = static_cast<uint32_t *>(base[kSecSvcQ]);
    P.svc_o = static_cast<double *>(base[kSecSvcO]);
    P.move_log = static_cast<ongym_move *>(base[kSecMoveLog]);
    P.move_n = static_cast<int32_t *>(base[kSecMoveN]);
    P.env = static_cast<DevEnv *>(base[kSecEnv]);
}

static StateLayout state_layout(const Params &P) {
    StateLayout L{};
    const int64_t C = P.capacity, ids = P.track_ids ? 1 : 0;
    const int64_t bytes[kStateSections] = {(int64_t)P.n_links * P.row_words * 8, C * 4, C * 4, C * 4, ids * C * 4, ids * C * 8,
                                           ids * ONGYM_MOVE_LOG * (int64_t)sizeof(ongym_move), ids * 4, (int64_t)sizeof(DevEnv)};
    int64_t off = 0;
    int32_t items = 0;
    for (int s = 0; s < kStateSections; s++) {
        L.bytes[s] = bytes[s];
        L.off[s] = off;
        off += (bytes[s] + 15) & ~(int64_t)15;
        L.shift[s] = s == kSecEnv ? 3 : bytes[s] % 16 == 0 ? 4 : bytes[s] % 8 == 0 ? 3 : 2;   // DevEnv: 8-byte words (kept words)
        L.prefix[s] = items;
        items += (int32_t)(bytes[s] >> L.shift[s]);
    }
    L.prefix[kStateSections] = items;
    L.block_bytes = off;
    return L;
}

static StateHeader state_header(const ongym_env *env, const StateLayout &L, int32_t count) {
    StateHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, "ONGYMST", 8);
    h.format = kStateFormat;
    h.header_bytes = (uint32_t)sizeof(StateHeader);
    h.fingerprint = env->state_fp;
    h.count = count;
    h.block_bytes = L.block_bytes;
    h.rec32 = env->P.rec32; h.track_ids = env->P.track_ids; h.row_words = env->P.row_words; h.n_links = env->P.n_links;
    h.capacity = env->P.capacity; h.devenv_bytes = (int32_t)sizeof(DevEnv); h.n_sections = kStateSections;
    h.trace_used = env->trace_used ? 1 : 0;
    h.req_mode = env->P.req_mode;
    for (int s = 0; s < kStateSections; s++) { h.sec_bytes[s] = L.bytes[s]; h.sec_off[s] = L.off[s]; }
    return h;
}

// DevEnv words (bit w = word w) the destination of a load or fork keeps: always the work counters total_*, plus the stream key
// (ONGYM_STATE_KEEP_STREAM) or the per-replica parameters (ONGYM_STATE_KEEP_PARAMS)
static void state_keep_mask(int32_t flags, uint64_t &lo, uint64_t &hi) {
    static_assert(offsetof(ongym_stats, total_active_sum) == offsetof(ongym_stats, total_steps) + 7 * 8, "total_* are 8 int64");
    static_assert(offsetof(DevEnv, margin) == 8 && offsetof(DevEnv, mean_iat) == 16 && offsetof(DevEnv, mean_iat_f) == 24,
                  "the parameters are the first four words of DevEnv");
    lo = hi = 0;
    auto set = [&](size_t off, size_t n) {
        for (size_t w = off / 8; w < (off + n + 7) / 8; w++) (w < 64 ? lo : hi) |= 1ull << (w & 63);
    };
    set(offsetof(DevEnv, st) + offsetof(ongym_stats, total_steps), 8 * 8);
    if (flags & ONGYM_STATE_KEEP_STREAM) set(offsetof(DevEnv, rng_key), 8);
    if (flags & ONGYM_STATE_KEEP_PARAMS) set(offsetof(DevEnv, launch_power), 28);
}

// count in [1, batch]; a NULL list means all replicas (count == batch); entries in [0, batch), distinct when `distinct`
static int check_state_list(ongym_env *env, int32_t count, const int32_t *replicas, bool distinct) {
    const int B = env->P.batch;
    if (count < 1 || count > B) return fail_arg(env, "state count must lie in [1, batch]");
    if (!replicas) return count == B ? 0 : fail_arg(env, "a NULL replica list means all replicas: count must equal batch");
    std::vector<char> seen(distinct ? (size_t)B : 0, 0);
    for (int32_t k = 0; k < count; k++) {
        const int32_t r = replicas[k];
        if (r < 0 || r >= B) return fail_arg(env, "replica list entry outside [0, batch)");
        if (distinct) {
            if (seen[(size_t)r]) return fail_arg(env, "a load list must not repeat a replica");
            seen[(size_t)r] = 1;
        }
    }
    return 0;
}

// the host list -> d_state_idx (stream-ordered: a launch of an earlier call that reads it has been issued before)
static int upload_state_list(ongym_env *env, int32_t count, const int32_t *list) {
    if (!env->d_state_idx) {
        int rc = dev_alloc(env, (size_t)env->P.batch, &env->d_state_idx, false);
        if (rc) return rc;
    }
    HIP_TRY(env, hipMemcpyAsync(env->d_state_idx, list, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, env->stream));
    return 0;
}

static int ensure_state_stage(ongym_env *env, size_t bytes) {
    if (env->state_stage_bytes >= bytes) return 0;
    if (env->d_state_stage) {
        HIP_TRY(env, hipStreamSynchronize(env->stream));
        (void)hipFree(env->d_state_stage);
        env->d_state_stage = nullptr;
        env->state_stage_bytes = 0;
    }
    HIP_TRY(env, hipMalloc(&env->d_state_stage, bytes));
    env->state_stage_bytes = bytes;
    return 0;
}

template <int MODE>
static int launch_state_copy(ongym_env *env, int blocks, const StateCopyArgs &a) {
    hipLaunchKernelGGL(k_state_copy<MODE>, dim3(blocks), dim3(kStateThreads), 0, env->stream, a);
    HIP_TRY(env, hipGetLastError());
    return 0;
}

extern "C" {

int32_t ongym_abi_version(void) { return ONGYM_ABI_VERSION; }

int32_t ongym_sizeof(int32_t what) {
    switch (what) {
        case 0: return (int32_t)sizeof(ongym_config);
        case 1: return (int32_t)sizeof(ongym_request);
        case 2: return (int32_t)sizeof(ongym_step_rec);
        case 3: return (int32_t)sizeof(ongym_service);
        case 4: return (int32_t)sizeof(ongym_stats);
        case 5: return (int32_t)sizeof(ongym_move);
        default: return -1;
    }
}

const char *ongym_last_error(ongym_env *env) { return env ? env->err.c_str() : g_create_error.c_str(); }

int ongym_create(const ongym_config *cfg, ongym_env **out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ONGYM_E_ARG; }
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(ongym_config) || cfg->abi_version != ONGYM_ABI_VERSION) {
        g_create_error = "ongym_config struct_size / abi_version mismatch";
        return ONGYM_E_ARG;
    }
    ongym_env *env = new (std::nothrow) ongym_env();
    if (!env) { g_create_error = "out of memory"; return ONGYM_E_ARG; }
    env->cfg = *cfg;
    int ndev = 0;
    hipError_t he = hipGetDeviceCount(&ndev);
    if (he != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
        g_create_error = "no usable HIP device (hipGetDeviceCount: " + std::string(hipGetErrorString(he)) + ")";
        delete env;
        return ONGYM_E_HIP;
    }
    int rc = 0;
    do {
        if (hipSetDevice(cfg->device) != hipSuccess) { env->err = "hipSetDevice failed"; rc = ONGYM_E_HIP; break; }
        if (hipStreamCreateWithFlags(&env->own_stream, hipStreamNonBlocking) != hipSuccess) { env->err = "hipStreamCreate failed"; rc = ONGYM_E_HIP; break; }
        env->stream = env->own_stream;
        if (hipEventCreate(&env->ev0) != hipSuccess || hipEventCreate(&env->ev1) != hipSuccess) { env->err = "hipEventCreate failed"; rc = ONGYM_E_HIP; break; }
        rc = build(env, cfg);
        if (!rc) rc = admission_prepare(env);
    } while (0);
    if (rc) {
        g_create_error = env->err;
        ongym_destroy(env);
        return rc;
    }
    env->state_fp = state_fingerprint(cfg);
    *out = env;
    return ONGYM_OK;
}

void ongym_destroy(ongym_env *env) {
    if (!env) return;
    (void)hipSetDevice(env->cfg.device);
    if (env->stream) (void)hipStreamSynchronize(env->stream);
    for (void *p : env->allocs) (void)hipFree(p);
    if (env->d_trace) (void)hipFree(env->d_trace);
    if (env->h_pinned) (void)hipHostFree(env->h_pinned);
    if (env->d_state_stage) (void)hipFree(env->d_state_stage);
    for (Stage &st : env->stage) if (st.base) (void)hipFree(st.base);
    if (env->ev0) (void)hipEventDestroy(env->ev0);
    if (env->ev1) (void)hipEventDestroy(env->ev1);
    if (env->own_stream) (void)hipStreamDestroy(env->own_stream);      // a caller's stream (ongym_set_stream) is the caller's
    delete env;
}

/* Resident workgroups (= replicas = wavefronts) per compute unit of the kernel that ongym_step_policy(first fit) launches,
 * as the HIP occupancy query reports it for this environment's LDS size. Diagnostic. */
int ongym_query_occupancy(ongym_env *env, int32_t *blocks_per_cu, int32_t *lds_bytes, int32_t *lean_kernel) {
    return ongym_query_occupancy_policy(env, ONGYM_POLICY_FIRST_FIT, blocks_per_cu, lds_bytes, lean_kernel);
}

int ongym_query_occupancy_policy(ongym_env *env, int32_t policy, int32_t *blocks_per_cu, int32_t *lds_bytes, int32_t *lean_kernel) {
    if (!env || !blocks_per_cu || !lds_bytes || !lean_kernel) return ONGYM_E_ARG;
    if (policy < ONGYM_POLICY_FIRST_FIT || policy >= ONGYM_POLICY_COUNT) return fail_arg(env, "unknown policy id");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    int nb = 0, lds = 0;
    const LeanFns *lean = lean_unit(env, policy);
    if (lean) {
        if (int rc = lean->occupancy(env, &nb, &lds)) return rc;
        *lds_bytes = lds;
    } else {
        // the generic kernel's state block (the policies with scratch ask for more at launch time)
        if (env->lds <= 8192) HIP_TRY(env, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_run<true, true, 5, 0>, 64, env->lds));
        else HIP_TRY(env, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_run<true, true, 4, 0>, 64, env->lds));
        *lds_bytes = (int32_t)env->lds;
    }
    *blocks_per_cu = nb;
    *lean_kernel = lean ? 1 : 0;
    return ONGYM_OK;
}

int ongym_query_link_weight_entry(ongym_env *env, int32_t path, uint32_t links, uint32_t out[4], double entry[2]) {
    if (!env || !out || !entry) return ONGYM_E_ARG;
    if (path < 0 || path >= env->P.n_paths) return fail_arg(env, "path out of range");
    out[0] = 0;
    if (!env->fast_ok || env->fast_m64 || !env->P.lw_tab_bytes) return ONGYM_OK;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    // the record and the entry as they lie in device memory, addressed as the kernels address them
    PathRec r;
    HIP_TRY(env, hipMemcpy(&r, static_cast<const PathRec *>(env->P.path_rec) + path, sizeof(r), hipMemcpyDeviceToHost));
    const uint32_t mult = r.mask_hi, loc = r.id, idx = lw_index(links, r.mask_lo, mult, loc);
    const size_t off = (size_t)(loc & ~31u) + (size_t)idx * 16;
    if (off < env->P.lw_tab_off || off + 16 > (size_t)env->P.lw_tab_off + env->P.lw_tab_bytes)
        return fail_arg(env, "weight-table entry outside the table");
    HIP_TRY(env, hipMemcpy(entry, reinterpret_cast<const char *>(env->P.pair_tab2k) + off, 16, hipMemcpyDeviceToHost));
    out[0] = 1; out[1] = mult; out[2] = idx; out[3] = 32u - (loc & 31u);
    return ONGYM_OK;
}

int ongym_query_path_rows(ongym_env *env, int32_t path, uint32_t *out) {
    if (!env || !out) return ONGYM_E_ARG;
    if (path < 0 || path >= env->P.n_paths) return fail_arg(env, "path out of range");
    if (!env->fast_ok) return fail_arg(env, "no lean kernel, no route-row table");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    HIP_TRY(env, hipMemcpy(out, static_cast<const PathRec *>(env->P.path_rec_ff) + path, sizeof(*out), hipMemcpyDeviceToHost));
    return ONGYM_OK;
}

int ongym_sync(ongym_env *env) {
    if (!env) return ONGYM_E_ARG;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    HIP_TRY(env, hipStreamSynchronize(env->stream));
    return ONGYM_OK;
}

int ongym_set_stream(ongym_env *env, void *hip_stream, int32_t use_own) {
    if (!env) return ONGYM_E_ARG;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    HIP_TRY(env, hipStreamSynchronize(env->stream));        // nothing of this environment is in flight on the old stream
    env->stream = use_own ? env->own_stream : static_cast<hipStream_t>(hip_stream);
    env->timed = false;                                     // the events were recorded on the old stream
    return ONGYM_OK;
}

double ongym_last_kernel_ms(ongym_env *env) {
    if (!env || !env->timed) return -1.0;
    if (hipEventSynchronize(env->ev1) != hipSuccess) return -1.0;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, env->ev0, env->ev1) != hipSuccess) return -1.0;
    return (double)ms;
}

int ongym_seed(ongym_env *env, uint64_t seed) { return ongym_seed_base(env, seed, 0); }

int ongym_seed_base(ongym_env *env, uint64_t seed, uint64_t replica_base) {
    if (!env) return ONGYM_E_ARG;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    env->P.req_mode = kReqRng;
    env->has_source = true;
    env->replica_base = replica_base;
    { int rc = push_params(env); if (rc) return rc; }
    int threads = 256, blocks = (env->P.batch + threads - 1) / threads;
    hipLaunchKernelGGL(k_seed, dim3(blocks), dim3(threads), 0, env->stream, env->P, seed, replica_base);
    HIP_TRY(env, hipGetLastError());
    return ONGYM_OK;
}

int ongym_set_requests(ongym_env *env, const ongym_request *reqs, int64_t n_per_replica) {
    if (!env || !reqs || n_per_replica <= 0) return env ? fail_arg(env, "bad trace") : ONGYM_E_ARG;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    HIP_TRY(env, hipStreamSynchronize(env->stream));
    size_t n = (size_t)env->P.batch * (size_t)n_per_replica;
    // validate node indices and times on the host when the trace is a host buffer (device traces are the caller's contract).
    // Nothing of the environment has changed when an entry is refused: the earlier request source stays installed.
    if (!env->cfg.io_device) {
        for (size_t i = 0; i < n; i++) {
            const ongym_request &q = reqs[i];
            if (q.source < 0 || q.source >= env->P.n_nodes || q.destination < 0 || q.destination >= env->P.n_nodes ||
                q.source == q.destination || !(q.bit_rate > 0))
                return fail_arg(env, "trace entry with invalid node pair / bit rate");
            // the sign bit of a stored release time is the 'disrupted' flag and the generic kernels compare fabsf of it, the lean
            // kernels the value itself: a clock below zero (-0.0 included) is one no two kernels agree on; NaN compares false
            // everywhere.  A holding time of +inf is legal: the service never leaves.
            if (!std::isfinite(q.arrival_time) || std::signbit(q.arrival_time))
                return fail_arg(env, "trace entry with an arrival time that is negative (sign bit set), infinite or NaN");
            if (std::isnan(q.holding_time) || std::signbit(q.holding_time))
                return fail_arg(env, "trace entry with a holding time that is negative (sign bit set) or NaN");
        }
        if (env->d_trace) { (void)hipFree(env->d_trace); env->d_trace = nullptr; }
        HIP_TRY(env, hipMalloc(&env->d_trace, n * sizeof(ongym_request)));
        HIP_TRY(env, hipMemcpy(env->d_trace, reqs, n * sizeof(ongym_request), hipMemcpyHostToDevice));
        env->P.trace = static_cast<const ongym_request *>(env->d_trace);
    } else {
        env->P.trace = reqs;
    }
    env->P.trace_n = n_per_replica;
    env->P.req_mode = kReqTrace;
    // the lean kernel replays a trace whose bit rates all come from the configured discrete table (it addresses per-request
    // constants by bit-rate index); anything else is the generic kernel's, for good (records may exceed the lean codec)
    env->trace_fast_ok = false;
    if (!env->cfg.io_device && env->fast_ok) {
        bool ok = true;
        for (size_t i = 0; i < n && ok; i++) {
            bool hit = false;
            for (int b = 0; b < env->P.n_bit_rates; b++) hit |= (float)env->cfg_bit_rates[(size_t)b] == reqs[i].bit_rate;
            ok = hit;
        }
        env->trace_fast_ok = ok;
    }
    if (!env->trace_fast_ok) env->trace_used = true;
    env->has_source = true;
    { int rc = push_params(env); if (rc) return rc; }
    int threads = 256, blocks = (env->P.batch + threads - 1) / threads;
    hipLaunchKernelGGL(k_rewind, dim3(blocks), dim3(threads), 0, env->stream, env->P);
    HIP_TRY(env, hipGetLastError());
    return ONGYM_OK;
}

// The two resets return without synchronising: they open a stage for the optional mask [batch] (a host mask is copied in on the
// stream, a NULL one reaches the kernel as NULL) and never close it.
int ongym_reset(ongym_env *env, const uint8_t *mask) {
    if (!env) return ONGYM_E_ARG;
    if (!env->has_source) return need_source(env);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    Span sp[] = {{mask, (size_t)env->P.batch, kIn}};
    if (int rc = stage_open(env, env->stage[kStageReset], sp)) return rc;
    return launch_lds(env, k_reset, dim3(env->P.batch), env->lds, env->d_P, sp[0].as<const uint8_t>());
}

int ongym_reset_episode_counters(ongym_env *env, const uint8_t *mask) {
    if (!env) return ONGYM_E_ARG;
    if (!env->P.track_ids) {
        env->err = "ongym_reset_episode_counters needs cfg.track_service_ids (service ids restart under running services, "
                   "and calculate_osnr skips interferers by service id)";
        return ONGYM_E_STATE;
    }
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    Span sp[] = {{mask, (size_t)env->P.batch, kIn}};
    if (int rc = stage_open(env, env->stage[kStageReset], sp)) return rc;
    int threads = 64, blocks = (env->P.batch + threads - 1) / threads;
    hipLaunchKernelGGL(k_reset_counters, dim3(blocks), dim3(threads), 0, env->stream, env->P, sp[0].as<const uint8_t>());
    HIP_TRY(env, hipGetLastError());
    return ONGYM_OK;
}

static int launch_run(ongym_env *env, int mode, int policy, int nsteps, const int32_t *actions, int32_t *act_out,
                      uint8_t *flag_out, ongym_step_rec *out) {
    // the lean kernels: same results, half the issued instructions (ongym_fast.hpp)
    const LeanFns *lean = mode == kModePolicyStep ? lean_unit(env, policy) : nullptr;
    return timed_launch(env, [&] {
        return lean ? lean->launch(env, nsteps, out) : with_run_kernel(env, policy, [&](auto kernel, size_t lds) {
            return launch_lds(env, kernel, dim3(env->P.batch), lds, env->d_P, mode, nsteps, actions, act_out, flag_out, out,
                              policy);
        });
    });
}

static int check_policy(ongym_env *env, int32_t policy) {
    if (policy < ONGYM_POLICY_FIRST_FIT || policy >= ONGYM_POLICY_COUNT) return fail_arg(env, "unknown policy id");
    if (policy >= ONGYM_POLICY_LOWEST_SPECTRUM && env->P.k_paths > 8)
        return fail_arg(env, "this policy supports at most 8 candidate routes", ONGYM_E_LIMIT);
    if (policy != ONGYM_POLICY_FIRST_FIT && env->P.n_mods_consider < env->P.n_mods)
        return fail_arg(env, "only the first-fit policy is fused for modulations_to_consider < n_mods", ONGYM_E_LIMIT);
    if (policy == ONGYM_POLICY_MSCL && (env->P.bit_rate_mode != 0 || env->P.n_bit_rates <= 0))
        return fail_arg(env, "the MSCL policy sums its capacity loss over the discrete bit rates: bit_rate_mode must be discrete", ONGYM_E_LIMIT);
    return 0;
}

int ongym_step_policy(ongym_env *env, int32_t policy, int32_t nsteps, ongym_step_rec *out) {
    if (!env) return ONGYM_E_ARG;
    int rc;
    if ((rc = check_policy(env, policy))) return rc;
    if (nsteps <= 0) return fail_arg(env, "nsteps must be positive");
    if (!env->has_source) return need_source(env);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    Span sp[] = {{out, (size_t)nsteps * env->P.batch * sizeof(ongym_step_rec), kOut}};
    if ((rc = stage_open(env, env->stage[kStageStep], sp))) return rc;
    rc = launch_run(env, kModePolicyStep, policy, nsteps, nullptr, nullptr, nullptr, sp[0].as<ongym_step_rec>());
    return rc || !out ? rc : stage_close(env, sp);     // without records nothing comes back: the call only launches
}

int ongym_step_actions(ongym_env *env, const int32_t *actions, ongym_step_rec *out) {
    if (!env || !actions) return env ? fail_arg(env, "null actions") : ONGYM_E_ARG;
    if (!env->has_source) return need_source(env);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)env->P.batch;
    Span sp[] = {{out, B * sizeof(ongym_step_rec), kOut}, {actions, B * sizeof(int32_t), kIn}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageStep], sp))) return rc;
    rc = launch_run(env, kModeActionStep, ONGYM_POLICY_FIRST_FIT, 1, sp[1].as<const int32_t>(), nullptr, nullptr,
                    sp[0].as<ongym_step_rec>());
    return rc ? rc : stage_close(env, sp);
}

int ongym_step_actions_bundle(ongym_env *env, const int32_t *actions, int32_t next_policy, ongym_step_rec *rec_out,
                              ongym_request *request_out, ongym_stats *stats_out, int32_t *next_actions, uint8_t *next_flags) {
    if (!env || !actions || !rec_out || !request_out || !stats_out) return env ? fail_arg(env, "null buffer") : ONGYM_E_ARG;
    if (env->cfg.io_device) return fail_arg(env, "ongym_step_actions_bundle returns host buffers: not with io_device", ONGYM_E_STATE);
    if (next_policy >= 0 && (!next_actions || !next_flags)) return fail_arg(env, "null next_actions / next_flags");
    if (!env->has_source) return need_source(env);
    int rc;
    if (next_policy >= 0 && (rc = check_policy(env, next_policy))) return rc;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)env->P.batch;
    // pinned staging: records | DevEnv (requests + statistics) | next actions | next flags | actions in
    const size_t o_rec = 0, o_env = o_rec + B * sizeof(ongym_step_rec), o_act = o_env + B * sizeof(DevEnv),
                 o_flag = o_act + B * sizeof(int32_t), o_in = o_flag + ((B + 15) & ~(size_t)15), total = o_in + B * sizeof(int32_t);
    if (env->h_pinned_bytes < total) {
        if (env->h_pinned) { (void)hipHostFree(env->h_pinned); env->h_pinned = nullptr; env->h_pinned_bytes = 0; }
        HIP_TRY(env, hipHostMalloc(&env->h_pinned, total, hipHostMallocDefault));
        env->h_pinned_bytes = total;
    }
    char *hp = static_cast<char *>(env->h_pinned);
    if (B <= 256) {
        // few replicas (the single-environment surface): the kernels read the actions from and write their results to the
        // pinned host buffer directly (it is device-accessible): launches and one synchronisation, no copy calls for them
        int32_t *h_act_in = reinterpret_cast<int32_t *>(hp + o_in);
        memcpy(h_act_in, actions, B * 4);
        if (next_policy >= 0)
            rc = launch_run(env, kModeActionThenPolicy, next_policy, 2, h_act_in, reinterpret_cast<int32_t *>(hp + o_act),
                            reinterpret_cast<uint8_t *>(hp + o_flag), reinterpret_cast<ongym_step_rec *>(hp + o_rec));
        else
            rc = launch_run(env, kModeActionStep, ONGYM_POLICY_FIRST_FIT, 1, h_act_in, nullptr, nullptr,
                            reinterpret_cast<ongym_step_rec *>(hp + o_rec));
        if (rc) return rc;
        HIP_TRY(env, hipMemcpyAsync(hp + o_env, env->P.env, B * sizeof(DevEnv), hipMemcpyDeviceToHost, env->stream));
        HIP_TRY(env, hipStreamSynchronize(env->stream));
    } else {
        // many replicas: device buffers from the step calls' stage; stage_close copies into the pinned buffer and synchronises
        const bool next = next_policy >= 0;
        Span sp[] = {{hp + o_rec, B * sizeof(ongym_step_rec), kOut}, {actions, B * sizeof(int32_t), kIn},
                     {next ? hp + o_act : nullptr, B * sizeof(int32_t), kOut}, {next ? hp + o_flag : nullptr, B, kOut}};
        if ((rc = stage_open(env, env->stage[kStageStep], sp))) return rc;
        if ((rc = launch_run(env, kModeActionStep, ONGYM_POLICY_FIRST_FIT, 1, sp[1].as<const int32_t>(), nullptr, nullptr,
                             sp[0].as<ongym_step_rec>()))) return rc;
        if (next && (rc = launch_run(env, kModePolicyOnly, next_policy, 1, nullptr, sp[2].as<int32_t>(), sp[3].as<uint8_t>(),
                                     nullptr))) return rc;
        HIP_TRY(env, hipMemcpyAsync(hp + o_env, env->P.env, B * sizeof(DevEnv), hipMemcpyDeviceToHost, env->stream));
        if ((rc = stage_close(env, sp))) return rc;
    }
    memcpy(rec_out, hp + o_rec, B * sizeof(ongym_step_rec));
    const DevEnv *de = reinterpret_cast<const DevEnv *>(hp + o_env);
    int flags = 0;
    for (size_t r = 0; r < B; r++) {
        stats_out[r] = de[r].st; flags |= de[r].st.flags;
        ongym_request &q = request_out[r];
        memset(&q, 0, sizeof(q));
        q.arrival_time = de[r].cur_at; q.holding_time = de[r].cur_ht; q.bit_rate = de[r].cur_br;
        q.source = (int16_t)de[r].cur_src; q.destination = (int16_t)de[r].cur_dst;
    }
    if (next_policy >= 0) { memcpy(next_actions, hp + o_act, B * 4); memcpy(next_flags, hp + o_flag, B); }
    if (flags & ONGYM_F_OVERFLOW) { env->err = "a replica overflowed its service table (raise capacity)"; return ONGYM_E_CAPACITY; }
    return ONGYM_OK;
}

int ongym_observe(ongym_env *env, float *obs, uint8_t *mask) {
    if (!env || !obs || !mask) return env ? fail_arg(env, "null obs/mask") : ONGYM_E_ARG;
    const Params &P = env->P;
    if (!P.path_len_norm || !(P.max_bit_rate > 0)) return fail_arg(env, "observation needs path_len_norm and max_bit_rate = max(bit_rates)");
    if (std::fabs(P.slot_bw - P.channel_width * 1e9) > 1e-6 * P.slot_bw) return fail_arg(env, "observation needs slot_bandwidth == channel_width*1e9");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t obs_dim = 3 + P.k_paths + (size_t)P.k_paths * P.n_mods_consider * 12;
    const size_t nact = (size_t)P.k_paths * P.n_mods_consider * P.n_slots + 1;
    const size_t B = (size_t)P.batch;
    Span sp[] = {{mask, B * nact, kOut}, {obs, B * obs_dim * sizeof(float), kOut}};               // staging: mask | obs
    int rc;
    if ((rc = stage_open(env, env->stage[kStageMask], sp))) return rc;
    HIP_TRY(env, hipMemsetAsync(sp[0].dev, 0, B * nact, env->stream));     // k_observe only sets the ones
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {
            return launch_lds(env, k_observe<UA, R32>, dim3(P.batch), obs_layout(P).total, env->d_P, sp[1].as<float>(),
                              sp[0].as<uint8_t>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_observe_blocks(ongym_env *env, int32_t blocks, float *obs, uint8_t *mask, int32_t *action_map) {
    if (!env) return ONGYM_E_ARG;
    if (!obs || !mask || !action_map) return fail_arg(env, "null obs/mask/action_map");
    if (blocks < 1 || blocks > kMaxBlocks) return fail_arg(env, "blocks must lie in [1, 16]");
    const Params &P = env->P;
    if (P.n_mods_consider < P.n_mods)
        return fail_arg(env, "the block action space has no format window: it needs modulations_to_consider == n_mods");
    if (!P.path_len_norm || !(P.max_bit_rate > 0)) return fail_arg(env, "block observation needs path_len_norm and max_bit_rate = max(bit_rates)");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, nout = (size_t)P.k_paths * blocks + 1;
    Span sp[] = {{obs, B * (size_t)blocks_obs_dim(P.k_paths, blocks) * sizeof(float), kOut},       // staging: obs | action_map | mask
                 {action_map, B * nout * sizeof(int32_t), kOut}, {mask, B * nout, kOut}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageBlocks], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {   // the step kernels' (UA, R32): the same QoT decisions
            return launch_lds(env, k_observe_blocks<UA, R32>, dim3(P.batch), blocks_lds_bytes(P), env->d_P, (int)blocks,
                              sp[0].as<float>(), sp[2].as<uint8_t>(), sp[1].as<int32_t>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_link_metrics(ongym_env *env, float *link_out, double *compactness, double *link_stats) {
    if (!env) return ONGYM_E_ARG;
    if (!link_out && !compactness && !link_stats) return fail_arg(env, "null link_out/compactness/link_stats: nothing to compute");
    const Params &P = env->P;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, E = (size_t)P.n_links;
    Span sp[] = {{link_stats, B * E * kLinkStats * sizeof(double), kIn | kOut},                    // staging: link_stats | compactness | link_out
                 {compactness, B * sizeof(double), kOut}, {link_out, B * E * kLinkMetrics * sizeof(float), kOut}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageMetrics], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto, auto R32) {     // the stored record codec
            return launch_lds(env, k_link_metrics<R32>, dim3(P.batch), metrics_lds_bytes(P), env->d_P, sp[2].as<float>(),
                              sp[1].as<double>(), sp[0].as<double>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_service_qot(ongym_env *env, double *svc_out, double *replica_out, float *link_out) {
    if (!env) return ONGYM_E_ARG;
    if (!svc_out && !replica_out && !link_out) return fail_arg(env, "null svc_out/replica_out/link_out: nothing to compute");
    const Params &P = env->P;
    const size_t lds = qot_lds_bytes(P);
    if (lds > 160 * 1024) return fail_arg(env, "the QoT kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch;
    Span sp[] = {{svc_out, B * P.capacity * kServiceQot * sizeof(double), kOut},                   // staging: svc_out | replica_out | link_out
                 {replica_out, B * kReplicaQot * sizeof(double), kOut}, {link_out, B * P.n_links * kLinkQot * sizeof(float), kOut}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageQot], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {     // attenuation and the stored record codec
            return launch_lds(env, k_service_qot<UA, R32>, dim3(P.batch), lds, env->d_P, sp[0].as<double>(), sp[1].as<double>(),
                              sp[2].as<float>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_action_impact(ongym_env *env, int32_t n_actions, const int32_t *actions, const double *svc_in, double *impact_out) {
    if (!env) return ONGYM_E_ARG;
    if (!actions || !impact_out) return fail_arg(env, "null actions/impact_out");
    if (n_actions < 1 || n_actions > kMaxImpactActions) return fail_arg(env, "n_actions must lie in [1, 256]");
    const Params &P = env->P;
    const size_t lds = impact_lds_bytes(P);
    if (lds > 160 * 1024) return fail_arg(env, "the impact kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, A = (size_t)n_actions;
    Span sp[] = {{impact_out, B * A * kActionImpact * sizeof(double), kOut},                       // staging: impact_out | svc_in | actions
                 {svc_in, B * P.capacity * kServiceQot * sizeof(double), kIn}, {actions, B * A * sizeof(int32_t), kIn}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageImpact], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {     // attenuation and the stored record codec
            return launch_lds(env, k_action_impact<UA, R32>, dim3(P.batch), lds, env->d_P, (int)n_actions,
                              sp[2].as<const int32_t>(), sp[1].as<const double>(), sp[0].as<double>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_failure_impact(ongym_env *env, int32_t n_fail, const int32_t *links, double *link_out, int32_t *svc_out) {
    if (!env) return ONGYM_E_ARG;
    if (!link_out) return fail_arg(env, "null link_out");
    const Params &P = env->P;
    if (n_fail < 1 || n_fail > P.n_links) return fail_arg(env, "n_fail must lie in [1, n_links]");
    if (!links && n_fail != P.n_links) return fail_arg(env, "null links: n_fail must be n_links");
    if (P.n_mods_consider < P.n_mods)
        return fail_arg(env, "restoration searches every format: it needs modulations_to_consider == n_mods");
    if (!env->path_pair_err.empty()) return fail_arg(env, env->path_pair_err.c_str());
    const size_t lds = failure_lds_bytes(P);
    if (lds > 160 * 1024) return fail_arg(env, "the failure kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, F = (size_t)n_fail;
    Span sp[] = {{link_out, B * F * kFailureImpact * sizeof(double), kOut},                        // staging: link_out | svc_out | links
                 {svc_out, B * F * P.capacity * sizeof(int32_t), kOut}, {links, B * F * sizeof(int32_t), kIn}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageFailure], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {     // attenuation and the stored record codec
            return launch_lds(env, k_failure_impact<UA, R32>, dim3(P.batch, n_fail), lds, env->d_P, (int)n_fail,
                              sp[2].as<const int32_t>(), env->d_path_pair, sp[0].as<double>(), sp[1].as<int32_t>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_failure_sets(ongym_env *env, int32_t n_sets, const uint64_t *sets, int32_t per_replica, double *set_out,
                       int32_t *svc_out) {
    if (!env) return ONGYM_E_ARG;
    if (!sets || !set_out) return fail_arg(env, "null sets/set_out");
    const Params &P = env->P;
    if (n_sets < 1 || n_sets > kMaxFailureSets) return fail_arg(env, "n_sets must lie in [1, 65535]");
    if (P.n_mods_consider < P.n_mods)
        return fail_arg(env, "restoration searches every format: it needs modulations_to_consider == n_mods");
    if (!env->path_pair_err.empty()) return fail_arg(env, env->path_pair_err.c_str());
    const size_t lds = failure_lds_bytes(P);
    if (lds > 160 * 1024) return fail_arg(env, "the failure kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, F = (size_t)n_sets, R = per_replica ? B : 1;
    Span sp[] = {{set_out, B * F * kFailureSets * sizeof(double), kOut},                           // staging: set_out | sets | svc_out
                 {sets, R * F * 2 * sizeof(uint64_t), kIn}, {svc_out, B * F * P.capacity * sizeof(int32_t), kOut}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageFailure], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {     // attenuation and the stored record codec
            return launch_lds(env, k_failure_sets<UA, R32>, dim3(P.batch, n_sets), lds, env->d_P, (int)n_sets,
                              sp[1].as<const uint64_t>(), (int)(per_replica != 0), env->d_path_pair, sp[0].as<double>(),
                              sp[2].as<int32_t>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

// The checks every call that restores victims makes before it launches (ongym_failure_sets' own)
static int cut_refusals(ongym_env *env) {
    const Params &P = env->P;
    if (P.n_mods_consider < P.n_mods)
        return fail_arg(env, "restoration searches every format: it needs modulations_to_consider == n_mods");
    if (!env->path_pair_err.empty()) return fail_arg(env, env->path_pair_err.c_str());
    return ONGYM_OK;
}

int ongym_cut_links(ongym_env *env, const uint64_t *sets, int32_t per_replica, int32_t flags, double *cut_out, int32_t *svc_out,
                    int32_t *index_out) {
    if (!env) return ONGYM_E_ARG;
    if (!sets) return fail_arg(env, "null sets");
    if (!cut_out) return fail_arg(env, "null cut_out");
    if (flags & ~ONGYM_CUT_NO_RESTORE) return fail_arg(env, "unknown flags: only ONGYM_CUT_NO_RESTORE is defined");
    if (int rc = cut_refusals(env)) return rc;
    const Params &P = env->P;
    const size_t lds = cut_lds_bytes(P);
    if (lds > 160 * 1024) return fail_arg(env, "the cut kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, R = per_replica ? B : 1;
    Span sp[] = {{cut_out, B * kCutLinks * sizeof(double), kOut}, {sets, R * 2 * sizeof(uint64_t), kIn},   // staging: cut_out | sets | svc_out | index_out
                 {svc_out, B * P.capacity * sizeof(int32_t), kOut}, {index_out, B * P.capacity * sizeof(int32_t), kOut}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageCut], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {     // attenuation and the stored record codec
            return launch_lds(env, k_cut_links<UA, R32>, dim3(P.batch), lds, env->d_P, sp[1].as<const uint64_t>(),
                              (int)(per_replica != 0), (int)((flags & ONGYM_CUT_NO_RESTORE) != 0), env->d_path_pair,
                              sp[0].as<double>(), sp[2].as<int32_t>(), sp[3].as<int32_t>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_repair_links(ongym_env *env, const uint64_t *sets, int32_t per_replica, int32_t *repaired_out) {
    if (!env) return ONGYM_E_ARG;
    if (!sets) return fail_arg(env, "null sets");
    const Params &P = env->P;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, R = per_replica ? B : 1;
    Span sp[] = {{sets, R * 2 * sizeof(uint64_t), kIn}, {repaired_out, B * sizeof(int32_t), kOut}};   // staging: sets | repaired_out
    int rc;
    if ((rc = stage_open(env, env->stage[kStageCut], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto, auto R32) {     // the stored record codec
            return launch_lds(env, k_repair_links<R32>, dim3(P.batch), 0, env->d_P, sp[0].as<const uint64_t>(),
                              (int)(per_replica != 0), sp[1].as<int32_t>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_failed_links(ongym_env *env, uint64_t *failed_out) {
    if (!env) return ONGYM_E_ARG;
    if (!failed_out) return fail_arg(env, "null failed_out");
    const Params &P = env->P;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    Span sp[] = {{failed_out, (size_t)P.batch * 2 * sizeof(uint64_t), kOut}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageCut], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto, auto R32) {     // the stored record codec
            return launch_lds(env, k_failed_links<R32>, dim3(P.batch), 0, env->d_P, sp[0].as<uint64_t>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

// The widest record a lean step kernel of this environment can carry: where one may run, it carries no slot count above its pair
// table's rows and, in the narrow build, above 32 (ongym_fast.hpp, "Eligibility"); otherwise any width up to S
static int lean_width_limit(const ongym_env *env) {
    const Params &P = env->P;
    const int max_slots = (env->fast_ok && !env->trace_used) ? std::min(P.tab_nmax, env->fast_wide ? 512 : 32) : P.n_slots;
    return std::min(max_slots, P.n_slots);
}

int ongym_spectrum_map(ongym_env *env, int16_t *owner_out, int32_t *rec_out, float *release_out, int32_t *audit_out) {
    if (!env) return ONGYM_E_ARG;
    if (!owner_out && !rec_out && !release_out && !audit_out)
        return fail_arg(env, "null owner_out/rec_out/release_out/audit_out: nothing to compute");
    const Params &P = env->P;
    if (owner_out && P.capacity > kSpectrumMaxOwners)
        return fail_arg(env, "owner_out holds record indices in an int16: it needs capacity <= 32766", ONGYM_E_LIMIT);
    const size_t lds = spectrum_lds_bytes(P, owner_out != nullptr);
    if (lds > 160 * 1024) return fail_arg(env, "the spectrum kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, C = (size_t)P.capacity;
    Span sp[] = {{owner_out, B * P.n_links * P.n_slots * sizeof(int16_t), kOut},                   // staging: owner_out | rec_out | release_out | audit_out
                 {rec_out, B * C * kSpectrumRec * sizeof(int32_t), kOut}, {release_out, B * C * sizeof(float), kOut},
                 {audit_out, B * kSpectrumAudit * sizeof(int32_t), kOut}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageSpectrum], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto, auto R32) {     // the stored record codec
            return launch_lds(env, k_spectrum_map<R32>, dim3(P.batch), lds, env->d_P, lean_width_limit(env), sp[0].as<int16_t>(),
                              sp[1].as<int32_t>(), sp[2].as<float>(), sp[3].as<int32_t>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_move_services(ongym_env *env, int32_t n_moves, const int32_t *moves, int32_t flags, double *move_out) {
    if (!env) return ONGYM_E_ARG;
    if (!moves || !move_out) return fail_arg(env, "null moves/move_out");
    if (n_moves < 1) return fail_arg(env, "n_moves must be at least 1");
    if (flags & ~ONGYM_MOVE_OWN_ROUTE) return fail_arg(env, "unknown flags: only ONGYM_MOVE_OWN_ROUTE is defined");
    if (int rc = cut_refusals(env)) return rc;
    const Params &P = env->P;
    const size_t lds = move_lds_bytes(P);
    if (lds > 160 * 1024) return fail_arg(env, "the move kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, N = (size_t)n_moves;
    Span sp[] = {{move_out, B * N * kMoveOut * sizeof(double), kOut}, {moves, B * N * 2 * sizeof(int32_t), kIn}};   // staging: move_out | moves
    int rc;
    if ((rc = stage_open(env, env->stage[kStageMove], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {     // attenuation and the stored record codec
            return launch_lds(env, k_move_services<UA, R32>, dim3(P.batch), lds, env->d_P, (int)n_moves,
                              sp[1].as<const int32_t>(), (int)((flags & ONGYM_MOVE_OWN_ROUTE) != 0), lean_width_limit(env),
                              env->d_path_pair,
                              sp[0].as<double>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

static int admission_groups(const ongym_env *env, size_t scenarios, int Q) {
    size_t g = 1;
    if (env->admission_groups > 0) g = (size_t)env->admission_groups;
    else while (g < 16 && scenarios * g < kAdmissionFill) g *= 2;
    g = std::min<size_t>(std::min<size_t>(g, 64), (size_t)Q);
    return (int)std::max<size_t>(1, std::min(g, admission_part_rows(env->P) / scenarios));
}

int ongym_admission_map(ongym_env *env, int32_t n_actions, const int32_t *actions, int32_t n_rates, const float *rates,
                        const double *weights, double *summary_out, int32_t *map_out, float *margin_out) {
    if (!env) return ONGYM_E_ARG;
    if (!summary_out) return fail_arg(env, "null summary_out");
    const Params &P = env->P;
    if (n_actions < 1 || n_actions > kMaxAdmissionActions) return fail_arg(env, "n_actions must lie in [1, 256]");
    if (!actions && n_actions != 1) return fail_arg(env, "null actions: n_actions must be 1");
    if (n_rates < 1 || n_rates > kMaxAdmissionRates) return fail_arg(env, "n_rates must lie in [1, 16]");
    AdmissionRates rv{};
    if (!rates) {
        if (P.bit_rate_mode != 0 || n_rates != P.n_bit_rates || (int)env->cfg_bit_rates.size() != n_rates)
            return fail_arg(env, "null rates: discrete bit rates and n_rates == n_bit_rates");
        for (int r = 0; r < n_rates; r++) rv.v[r] = (float)env->cfg_bit_rates[r];
    } else
        for (int r = 0; r < n_rates; r++) rv.v[r] = rates[r];
    for (int r = 0; r < n_rates; r++)
        if (!std::isfinite(rv.v[r]) || !(rv.v[r] > 0.0f)) return fail_arg(env, "every rate must be finite and positive");
    if (P.n_mods_consider < P.n_mods)
        return fail_arg(env, "the admission map searches every format: it needs modulations_to_consider == n_mods");
    if (!env->admission_pair_err.empty()) return fail_arg(env, env->admission_pair_err.c_str());
    const size_t lds = lds_bytes(P);
    if (lds > 160 * 1024) return fail_arg(env, "the admission kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, A = (size_t)n_actions, R = (size_t)n_rates, Q = (size_t)P.n_nodes * (P.n_nodes - 1) / 2;
    const int groups = admission_groups(env, B * A, (int)Q);
    Span sp[] = {{summary_out, B * A * kAdmissionMap * sizeof(double), kOut},          // staging: summary | map | margin | weights | actions
                 {map_out, B * A * Q * R * sizeof(int32_t), kOut}, {margin_out, B * A * Q * R * sizeof(float), kOut},
                 {weights, Q * R * sizeof(double), kIn}, {actions, B * A * sizeof(int32_t), kIn}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageAdmission], sp))) return rc;
    double *part = groups > 1 ? static_cast<double *>(env->stage[kStageAdmissionPart].base) : nullptr;   // allocated at create
    rc = timed_launch(env, [&]() -> int {
        const int lrc = with_layout(P, [&](auto UA, auto R32) {     // attenuation and the stored record codec
            return launch_lds(env, k_admission_map<UA, R32>, dim3(P.batch, n_actions, groups), lds, env->d_P, (int)n_actions,
                              sp[4].as<const int32_t>(), (int)n_rates, rv, sp[3].as<const double>(), groups, sp[0].as<double>(),
                              part, sp[1].as<int32_t>(), sp[2].as<float>());
        });
        if (lrc || groups == 1) return lrc;
        hipLaunchKernelGGL(k_admission_reduce, dim3((unsigned)((B * A + 255) / 256)), dim3(256), 0, env->stream, B * A, groups,
                           (const double *)part, sp[0].as<double>());
        HIP_TRY(env, hipGetLastError());
        return 0;
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_playout(ongym_env *env, int32_t n_actions, const int32_t *actions, int32_t horizon, int32_t policy, int32_t n_samples,
                  uint64_t seed, int32_t flags, double *playout_out) {
    if (!env) return ONGYM_E_ARG;
    if (!playout_out) return fail_arg(env, "null playout_out");
    const Params &P = env->P;
    if (n_actions < 1 || n_actions > kMaxPlayoutActions) return fail_arg(env, "n_actions must lie in [1, 256]");
    if (n_samples < 1 || n_samples > kMaxPlayoutSamples) return fail_arg(env, "n_samples must lie in [1, 64]");
    if (horizon < 1 || horizon > kMaxPlayoutHorizon) return fail_arg(env, "horizon must lie in [1, 4096]");
    if (n_actions * n_samples > kMaxPlayoutScenarios) return fail_arg(env, "n_actions * n_samples must not exceed 4096");
    if (!actions && n_actions != 1) return fail_arg(env, "null actions: n_actions must be 1");
    if (flags & ~ONGYM_PLAYOUT_OWN_STREAM) return fail_arg(env, "unknown flags");
    const bool own = (flags & ONGYM_PLAYOUT_OWN_STREAM) != 0;
    if (own && n_samples != 1) return fail_arg(env, "ONGYM_PLAYOUT_OWN_STREAM: the replica's own future is one future, n_samples must be 1");
    if (P.n_mods_consider < P.n_mods)
        return fail_arg(env, "the playout's policies search every format: it needs modulations_to_consider == n_mods");
    if (policy != ONGYM_POLICY_FIRST_FIT && policy != ONGYM_POLICY_LOAD_BALANCING)
        return fail_arg(env, "policy: the playout kernel is instantiated for first fit (0) and load balancing (1) only", ONGYM_E_LIMIT);
    if (P.track_ids)
        return fail_arg(env, "cfg.defragmentation / cfg.track_service_ids: their step writes the move log and the replica's "
                             "statistics in memory, a playout must not", ONGYM_E_LIMIT);
    if (!env->has_source) return need_source(env);
    if (P.req_mode == kReqTrace && !own)
        return fail_arg(env, "seed: the request source is a trace, which a playout continues only with ONGYM_PLAYOUT_OWN_STREAM",
                        ONGYM_E_STATE);
    const size_t lds = lds_bytes(P);
    if (lds > 160 * 1024) return fail_arg(env, "the playout kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)P.batch, A = (size_t)n_actions, R = (size_t)n_samples;
    Span sp[] = {{playout_out, B * A * R * kPlayout * sizeof(double), kOut}, {actions, B * A * sizeof(int32_t), kIn}};   // staging: playout_out | actions
    int rc;
    if ((rc = stage_open(env, env->stage[kStagePlayout], sp))) return rc;
    const int by_replica = env->playout_by_replica;
    const dim3 grid = by_replica ? dim3(P.batch, (unsigned)(A * R)) : dim3((unsigned)(B * A * R));
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {     // attenuation and the stored record codec
            return dispatch<int, ONGYM_POLICY_LOAD_BALANCING, ONGYM_POLICY_FIRST_FIT>(policy, [&](auto POL) {
                return launch_lds(env, k_playout<UA, R32, POL>, grid, lds, env->d_P, (int)n_actions, (int)n_samples, by_replica,
                                  sp[1].as<const int32_t>(), (int)horizon, seed, env->replica_base, (int)own, sp[0].as<double>());
            });
        });
    });
    return rc ? rc : stage_close(env, sp);
}

int ongym_sample_actions(ongym_env *env, const uint8_t *mask, uint64_t seed, uint64_t draw_index, int32_t *actions) {
    if (!env || !mask || !actions) return env ? fail_arg(env, "null mask/actions") : ONGYM_E_ARG;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const Params &P = env->P;
    const size_t nact = (size_t)P.k_paths * P.n_mods_consider * P.n_slots + 1, B = (size_t)P.batch;
    Span sp[] = {{mask, B * nact, kIn}, {actions, B * sizeof(int32_t), kOut}};                     // staging: mask | actions
    if (int rc = stage_open(env, env->stage[kStageMask], sp)) return rc;
    hipLaunchKernelGGL(k_sample_mask, dim3(P.batch), dim3(64), 0, env->stream, sp[0].as<const uint8_t>(), (long long)nact, seed,
                       env->replica_base, draw_index, sp[1].as<int32_t>());
    HIP_TRY(env, hipGetLastError());
    return stage_close(env, sp);
}

// Masked categorical action head (csrc/ongym_policy_head.hpp): one wavefront per row, kHeadWaves rows per workgroup.
static int head_check(ongym_env *env, const void *logits, int32_t dtype, const void *mask_or_bits, size_t mask_align) {
    if (!env->cfg.io_device) return fail_arg(env, "the masked categorical head takes device buffers: needs cfg.io_device = 1");
    if (!logits || !mask_or_bits) return fail_arg(env, "null logits / mask");
    if (dtype != ONGYM_DTYPE_F32 && dtype != ONGYM_DTYPE_BF16) return fail_arg(env, "dtype must be ONGYM_DTYPE_F32 or ONGYM_DTYPE_BF16");
    if ((uintptr_t)logits % 16) return fail_arg(env, "logits must be 16-byte aligned");
    if ((uintptr_t)mask_or_bits % mask_align) return fail_arg(env, "mask must be 8-byte aligned");
    return ONGYM_OK;
}

int ongym_masked_categorical_rows(ongym_env *env, int32_t rows, const void *logits, int32_t dtype, const void *mask,
                                  int32_t mask_format, int32_t mode, uint64_t seed, uint64_t draw_index, int32_t *actions,
                                  float *log_prob, float *entropy, float *row_stats, uint32_t *mask_bits) {
    if (!env) return ONGYM_E_ARG;
    if (mask_format != ONGYM_MASK_BYTES && mask_format != ONGYM_MASK_BITS) return fail_arg(env, "unknown mask format");
    { int rc = head_check(env, logits, dtype, mask, mask_format == ONGYM_MASK_BITS ? 4 : 8); if (rc) return rc; }
    if (!actions) return fail_arg(env, "null actions");
    if (mode < ONGYM_HEAD_SAMPLE || mode > ONGYM_HEAD_EVALUATE) return fail_arg(env, "unknown head mode");
    if (rows < 0) return fail_arg(env, "negative row count");
    if (mask_format == ONGYM_MASK_BITS && mask_bits) return fail_arg(env, "mask_bits out must be NULL when the mask is packed bits");
    const Params &P = env->P;
    const int nact = P.k_paths * P.n_mods_consider * P.n_slots + 1;
    const size_t lds = (size_t)kHeadWaves * ((nact + 31) / 32) * 4;
    if (lds > 64 * 1024) return fail_arg(env, "n_actions too large for the masked categorical head", ONGYM_E_LIMIT);
    if (rows == 0) return ONGYM_OK;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const dim3 grid((rows + kHeadWaves - 1) / kHeadWaves), block(64 * kHeadWaves);
    const size_t shm = mask_bits ? lds : 0;
    dispatch<int, ONGYM_MASK_BYTES, ONGYM_MASK_BITS>(mask_format, [&](auto MF) {
        dispatch<int, ONGYM_DTYPE_F32, ONGYM_DTYPE_BF16>(dtype, [&](auto DT) {
            dispatch<int, ONGYM_HEAD_SAMPLE, ONGYM_HEAD_ARGMAX, ONGYM_HEAD_EVALUATE>(mode, [&](auto MODE) {
                hipLaunchKernelGGL((k_head_fwd<DT, MODE, MF>), grid, block, shm, env->stream,
                                   static_cast<const typename HeadElem<DT>::T *>(logits),
                                   static_cast<const typename HeadMask<MF>::T *>(mask), rows, nact, seed, env->replica_base,
                                   draw_index, actions, log_prob, entropy, row_stats, mask_bits);
            });
        });
    });
    HIP_TRY(env, hipGetLastError());
    return ONGYM_OK;
}

int ongym_masked_categorical(ongym_env *env, const void *logits, int32_t dtype, const uint8_t *mask, int32_t mode,
                             uint64_t seed, uint64_t draw_index, int32_t *actions, float *log_prob, float *entropy,
                             float *row_stats, uint32_t *mask_bits) {
    if (!env) return ONGYM_E_ARG;
    return ongym_masked_categorical_rows(env, env->P.batch, logits, dtype, mask, ONGYM_MASK_BYTES, mode, seed, draw_index,
                                         actions, log_prob, entropy, row_stats, mask_bits);
}

int ongym_masked_categorical_backward_rows(ongym_env *env, int32_t rows, const void *logits, int32_t dtype,
                                           const uint32_t *mask_bits, const int32_t *actions, const float *row_stats,
                                           const float *entropy, const float *grad_log_prob, const float *grad_entropy,
                                           void *grad_logits) {
    if (!env) return ONGYM_E_ARG;
    { int rc = head_check(env, logits, dtype, mask_bits, 4); if (rc) return rc; }
    if (!actions || !row_stats || !entropy || !grad_logits) return fail_arg(env, "null actions / row_stats / entropy / grad_logits");
    if ((uintptr_t)grad_logits % 16) return fail_arg(env, "grad_logits must be 16-byte aligned");
    if (rows < 0) return fail_arg(env, "negative row count");
    if (rows == 0) return ONGYM_OK;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const Params &P = env->P;
    const int nact = P.k_paths * P.n_mods_consider * P.n_slots + 1;
    const dim3 grid((rows + kHeadWaves - 1) / kHeadWaves), block(64 * kHeadWaves);
    if (dtype == ONGYM_DTYPE_F32)
        hipLaunchKernelGGL((k_head_bwd<ONGYM_DTYPE_F32>), grid, block, 0, env->stream, static_cast<const float *>(logits),
                           mask_bits, rows, nact, actions, row_stats, entropy, grad_log_prob, grad_entropy, static_cast<float *>(grad_logits));
    else
        hipLaunchKernelGGL((k_head_bwd<ONGYM_DTYPE_BF16>), grid, block, 0, env->stream, static_cast<const uint16_t *>(logits),
                           mask_bits, rows, nact, actions, row_stats, entropy, grad_log_prob, grad_entropy, static_cast<uint16_t *>(grad_logits));
    HIP_TRY(env, hipGetLastError());
    return ONGYM_OK;
}

int ongym_masked_categorical_backward(ongym_env *env, const void *logits, int32_t dtype, const uint32_t *mask_bits,
                                      const int32_t *actions, const float *row_stats, const float *entropy,
                                      const float *grad_log_prob, const float *grad_entropy, void *grad_logits) {
    if (!env) return ONGYM_E_ARG;
    return ongym_masked_categorical_backward_rows(env, env->P.batch, logits, dtype, mask_bits, actions, row_stats, entropy,
                                                  grad_log_prob, grad_entropy, grad_logits);
}

// GAE over a rollout (csrc/ongym_gae.hpp)
static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int ongym_gae(ongym_env *env, int32_t steps, const ongym_step_rec *recs, const float *values, const float *last_values,
              float gamma, float gae_lambda, float *advantages, float *returns) {
    if (!env) return ONGYM_E_ARG;
    if (!env->cfg.io_device) return fail_arg(env, "ongym_gae takes device buffers: needs cfg.io_device = 1");
    if (steps < 1) return fail_arg(env, "steps must be >= 1");
    if (!recs || !values || !last_values || !advantages || !returns) return fail_arg(env, "null recs / values / last_values / outputs");
    if (!(gamma >= 0.f && gamma <= 1.f) || !(gae_lambda >= 0.f && gae_lambda <= 1.f))
        return fail_arg(env, "gamma and gae_lambda must lie in [0, 1]");
    if ((uintptr_t)recs % 8) return fail_arg(env, "recs must be 8-byte aligned");
    if ((uintptr_t)values % 4 || (uintptr_t)last_values % 4 || (uintptr_t)advantages % 4 || (uintptr_t)returns % 4)
        return fail_arg(env, "values / last_values / advantages / returns must be 4-byte aligned");
    const int B = env->P.batch;
    const size_t n = (size_t)steps * B, nf = n * sizeof(float);
    const struct { const void *p; size_t bytes; } in[] = {{recs, n * sizeof(ongym_step_rec)}, {values, nf}, {last_values, (size_t)B * 4},
                                                          {returns, nf}};
    for (const auto &r : in)
        if (ranges_overlap(advantages, nf, r.p, r.bytes)) return fail_arg(env, "advantages overlaps another buffer");
    for (int i = 0; i < 3; i++)
        if (ranges_overlap(returns, nf, in[i].p, in[i].bytes)) return fail_arg(env, "returns overlaps another buffer");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const int waves = std::min(kGaeWaves, (steps + kGaeChunk - 1) / kGaeChunk);
    hipLaunchKernelGGL(k_gae, dim3((B + 63) / 64), dim3(64 * waves), 0, env->stream, reinterpret_cast<const uint8_t *>(recs),
                       values, last_values, steps, B, waves, gamma, gamma * gae_lambda, advantages, returns);
    HIP_TRY(env, hipGetLastError());
    return ONGYM_OK;
}

int ongym_policy_actions(ongym_env *env, int32_t policy, int32_t *actions, uint8_t *flags) {
    if (!env || !actions) return env ? fail_arg(env, "null actions") : ONGYM_E_ARG;
    int rc;
    if ((rc = check_policy(env, policy))) return rc;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const size_t B = (size_t)env->P.batch;
    Span sp[] = {{actions, B * sizeof(int32_t), kOut}, {flags, B, kOut}};
    if ((rc = stage_open(env, env->stage[kStagePolicy], sp))) return rc;
    rc = launch_run(env, kModePolicyOnly, policy, 1, nullptr, sp[0].as<int32_t>(), sp[1].as<uint8_t>(), nullptr);
    return rc ? rc : stage_close(env, sp);
}

int ongym_score_actions(ongym_env *env, const double *weights, int32_t per_replica, int32_t *actions, double *best_out,
                        int32_t *count_out) {
    if (!env) return ONGYM_E_ARG;
    if (!actions || !weights) return fail_arg(env, "null actions/weights");
    const Params &P = env->P;
    if (P.n_mods_consider < P.n_mods)
        return fail_arg(env, "scoring walks every format: it needs modulations_to_consider == n_mods");
    const size_t lds = score_lds_bytes(P);
    if (lds > 160 * 1024) return fail_arg(env, "the scoring kernel's LDS block exceeds 160 KiB: lower capacity", ONGYM_E_LIMIT);
    const size_t B = (size_t)P.batch, nw = (per_replica ? B : 1) * kScoreFeatures;
    if (!env->cfg.io_device)
        for (size_t i = 0; i < nw; i++)
            if (!std::isfinite(weights[i])) return fail_arg(env, "weights must be finite");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    Span sp[] = {{actions, B * sizeof(int32_t), kOut}, {best_out, B * (1 + kScoreFeatures) * sizeof(double), kOut},   // staging:
                 {count_out, B * kScoreCounts * sizeof(int32_t), kOut}, {weights, nw * sizeof(double), kIn}};        // actions | best_out | count_out | weights
    int rc;
    if ((rc = stage_open(env, env->stage[kStageScore], sp))) return rc;
    rc = timed_launch(env, [&] {
        return with_layout(P, [&](auto UA, auto R32) {     // the step kernels' (UA, R32): the same QoT decisions
            return launch_lds(env, k_score_actions<UA, R32>, dim3(P.batch), lds, env->d_P, sp[3].as<const double>(),
                              (int)(per_replica != 0), sp[0].as<int32_t>(), sp[1].as<double>(), sp[2].as<int32_t>());
        });
    });
    return rc ? rc : stage_close(env, sp);
}

// One plugin-API query: range checks, k_query, the results back behind one synchronisation.  sp = the int32 row that goes in,
// the int32 results, the service records, the request; a query leaves empty what it does not use.  The results are host buffers
// under io_device too, so the query stage is always used.
enum { kSpanRow, kSpanInt, kSpanSvc, kSpanReq, kQuerySpans };
static int query(ongym_env *env, int what, int replica, int path, int slot, int n, Span (&sp)[kQuerySpans]) {
    if (replica < 0 || replica >= env->P.batch) return fail_arg(env, "replica out of range");
    if ((what == kQAvailable || what == kQPathFree) && (path < 0 || path >= env->P.n_paths)) return fail_arg(env, "path id out of range");
    if (what == kQPathFree && (slot < 0 || n <= 0 || slot >= env->P.n_slots || n > 1023)) return fail_arg(env, "slot / nslots out of range");
    if (what == kQCandidates && (path <= 0 || path > 1023 || n <= 0 || n > 1023)) return fail_arg(env, "total_slots / nslots out of range");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    int rc;
    if ((rc = stage_open(env, env->stage[kStageQuery], sp, true))) return rc;
    rc = with_layout(env->P, [&](auto UA, auto R32) {
        return launch_lds(env, k_query<UA, R32>, dim3(1), env->lds, env->d_P, what, replica, path, slot, n,
                          sp[kSpanRow].as<const int32_t>(), sp[kSpanInt].as<int32_t>(), sp[kSpanSvc].as<ongym_service>(),
                          sp[kSpanReq].as<ongym_request>());
    });
    return rc ? rc : stage_close(env, sp, true);
}

int ongym_query_available(ongym_env *env, int32_t replica, int32_t path_id, int32_t *out) {
    if (!env || !out) return ONGYM_E_ARG;
    Span sp[kQuerySpans] = {{}, {out, (size_t)env->P.n_slots * sizeof(int32_t), kOut}};
    return query(env, kQAvailable, replica, path_id, 0, 0, sp);
}

int ongym_query_gsnr(ongym_env *env, int32_t replica, int32_t path_id, int32_t slot, int32_t nslots, double out[3]) {
    if (!env || !out) return ONGYM_E_ARG;
    const int32_t cand[3] = {path_id, slot, nslots};        // calculate_osnr(env, candidate), core/osnr.pyx:21-142
    return ongym_query_gsnr_many(env, replica, 1, cand, out);
}

int ongym_query_gsnr_many(ongym_env *env, int32_t replica, int32_t count, const int32_t *cands, double *out) {
    if (!env || (count > 0 && (!cands || !out))) return ONGYM_E_ARG;
    if (count < 0) return fail_arg(env, "negative candidate count");
    if (count == 0) return ONGYM_OK;
    if (replica < 0 || replica >= env->P.batch) return fail_arg(env, "replica out of range");
    for (int32_t i = 0; i < count; i++) {    // every operand is checked on the host before the launch
        const int32_t path = cands[3 * i], slot = cands[3 * i + 1], n = cands[3 * i + 2];
        if (path < 0 || path >= env->P.n_paths) return fail_arg(env, "path id out of range");
        if (slot < 0 || n <= 0 || slot + n > env->P.n_slots) return fail_arg(env, "slot range out of the grid");
    }
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    Span sp[] = {{cands, (size_t)count * 3 * sizeof(int32_t), kIn}, {out, (size_t)count * 3 * sizeof(double), kOut}};
    int rc;
    if ((rc = stage_open(env, env->stage[kStageQuery], sp, true))) return rc;
    rc = with_layout(env->P, [&](auto UA, auto R32) {
        return launch_lds(env, k_query_gsnr_many<UA, R32>, dim3(count), env->lds, env->d_P, replica, count,
                          sp[0].as<const int32_t>(), sp[1].as<double>());
    });
    return rc ? rc : stage_close(env, sp, true);
}

int ongym_query_candidates(ongym_env *env, const int32_t *row, int32_t total_slots, int32_t nslots,
                           int32_t *starts_out, int32_t *count) {
    if (!env || !row || !starts_out || !count) return ONGYM_E_ARG;
    if (total_slots <= 0 || total_slots > 1023) return fail_arg(env, "total_slots out of range");
    std::vector<int32_t> flags((size_t)total_slots);
    Span sp[kQuerySpans] = {{row, flags.size() * sizeof(int32_t), kIn}, {flags.data(), flags.size() * sizeof(int32_t), kOut}};
    if (int rc = query(env, kQCandidates, 0, total_slots, 0, nslots, sp)) return rc;
    int32_t k = 0;
    for (int32_t s = 0; s < total_slots; s++) if (flags[s]) starts_out[k++] = s;   // flag -> list, no arithmetic
    *count = k;
    return ONGYM_OK;
}

int ongym_query_path_free(ongym_env *env, int32_t replica, int32_t path_id, int32_t slot, int32_t nslots, int32_t *out) {
    if (!env || !out) return ONGYM_E_ARG;
    Span sp[kQuerySpans] = {{}, {out, sizeof(int32_t), kOut}};
    return query(env, kQPathFree, replica, path_id, slot, nslots, sp);
}

int ongym_query_moves(ongym_env *env, int32_t replica, ongym_move *out, int32_t *count) {
    if (!env || !out || !count) return ONGYM_E_ARG;
    if (replica < 0 || replica >= env->P.batch) return fail_arg(env, "replica out of range");
    *count = 0;
    if (!env->P.defragmentation) return ONGYM_OK;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    HIP_TRY(env, hipStreamSynchronize(env->stream));
    int32_t n = 0;
    HIP_TRY(env, hipMemcpy(&n, env->P.move_n + replica, sizeof(n), hipMemcpyDeviceToHost));
    const int32_t kept = n < ONGYM_MOVE_LOG ? n : ONGYM_MOVE_LOG;
    if (kept > 0)
        HIP_TRY(env, hipMemcpy(out, env->P.move_log + (size_t)replica * ONGYM_MOVE_LOG, (size_t)kept * sizeof(ongym_move),
                               hipMemcpyDeviceToHost));
    *count = n;
    return ONGYM_OK;
}

int ongym_query_grid(ongym_env *env, int32_t replica, int32_t *out) {
    if (!env || !out) return ONGYM_E_ARG;
    Span sp[kQuerySpans] = {{}, {out, (size_t)env->P.n_links * env->P.n_slots * sizeof(int32_t), kOut}};
    return query(env, kQGrid, replica, 0, 0, 0, sp);
}

// Count and records come back in one copy behind one synchronisation: all `capacity` records, of which the first *n reach `out`
int ongym_query_services(ongym_env *env, int32_t replica, ongym_service *out, int32_t *n) {
    if (!env || !out || !n) return ONGYM_E_ARG;
    std::vector<ongym_service> recs((size_t)env->P.capacity);
    Span sp[kQuerySpans] = {{}, {n, sizeof(int32_t), kOut}, {recs.data(), recs.size() * sizeof(ongym_service), kOut}};
    if (int rc = query(env, kQServices, replica, 0, 0, 0, sp)) return rc;
    memcpy(out, recs.data(), (size_t)*n * sizeof(ongym_service));
    return ONGYM_OK;
}

int ongym_query_request(ongym_env *env, int32_t replica, ongym_request *out) {
    if (!env || !out) return ONGYM_E_ARG;
    Span sp[kQuerySpans] = {{}, {}, {}, {out, sizeof(ongym_request), kOut}};
    return query(env, kQRequest, replica, 0, 0, 0, sp);
}

int ongym_stats_get(ongym_env *env, ongym_stats *out) {
    if (!env || !out) return ONGYM_E_ARG;
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    HIP_TRY(env, hipStreamSynchronize(env->stream));
    std::vector<DevEnv> host((size_t)env->P.batch);
    HIP_TRY(env, hipMemcpy(host.data(), env->P.env, host.size() * sizeof(DevEnv), hipMemcpyDeviceToHost));
    int flags = 0;
    for (size_t r = 0; r < host.size(); r++) { out[r] = host[r].st; flags |= host[r].st.flags; }
    if (flags & ONGYM_F_OVERFLOW) { env->err = "a replica overflowed its service table (raise capacity)"; return ONGYM_E_CAPACITY; }
    return ONGYM_OK;
}

// ---- save / restore / fork of replica states ----
int ongym_state_size(ongym_env *env, int32_t count, int64_t *bytes) {
    if (!env || !bytes) return env ? fail_arg(env, "null bytes") : ONGYM_E_ARG;
    if (count < 1 || count > env->P.batch) return fail_arg(env, "state count must lie in [1, batch]");
    *bytes = (int64_t)sizeof(StateHeader) + (int64_t)count * state_layout(env->P).block_bytes;
    return ONGYM_OK;
}

int ongym_state_save(ongym_env *env, int32_t count, const int32_t *replicas, void *out) {
    if (!env || !out) return env ? fail_arg(env, "null state buffer") : ONGYM_E_ARG;
    if (int rc = check_state_list(env, count, replicas, false)) return rc;
    if (env->cfg.io_device && (uintptr_t)out % 16) return fail_arg(env, "a device state buffer must be 16-byte aligned");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const StateLayout L = state_layout(env->P);
    const size_t total = sizeof(StateHeader) + (size_t)count * (size_t)L.block_bytes;
    unsigned char *blob = static_cast<unsigned char *>(out);
    if (!env->cfg.io_device) {
        if (int rc = ensure_state_stage(env, total)) return rc;
        blob = static_cast<unsigned char *>(env->d_state_stage);
    }
    if (replicas)
        if (int rc = upload_state_list(env, count, replicas)) return rc;
    StateCopyArgs a{};
    a.L = L;
    a.cur = state_arrays(env->P);
    a.blob = blob + sizeof(StateHeader);
    a.hdr_out = blob;
    a.list = replicas ? env->d_state_idx : nullptr;
    a.batch = env->P.batch;
    a.hdr = state_header(env, L, count);
    if (int rc = launch_state_copy<kCopyPack>(env, count, a)) return rc;
    if (!env->cfg.io_device) {
        HIP_TRY(env, hipMemcpyAsync(out, blob, total, hipMemcpyDeviceToHost, env->stream));
        HIP_TRY(env, hipStreamSynchronize(env->stream));
    }
    return ONGYM_OK;
}

int ongym_state_load(ongym_env *env, int32_t count, const int32_t *replicas, const void *in, int32_t flags) {
    if (!env || !in) return env ? fail_arg(env, "null state buffer") : ONGYM_E_ARG;
    if (flags & ~(ONGYM_STATE_KEEP_STREAM | ONGYM_STATE_KEEP_PARAMS)) return fail_arg(env, "unknown ONGYM_STATE_* flag");
    if (int rc = check_state_list(env, count, replicas, true)) return rc;
    if (env->cfg.io_device && (uintptr_t)in % 16) return fail_arg(env, "a device state buffer must be 16-byte aligned");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    StateHeader h;
    if (env->cfg.io_device) {   // one small device-to-host copy: waits for the stream
        HIP_TRY(env, hipMemcpyAsync(&h, in, sizeof h, hipMemcpyDeviceToHost, env->stream));
        HIP_TRY(env, hipStreamSynchronize(env->stream));
    } else {
        memcpy(&h, in, sizeof h);
    }
    const StateLayout L = state_layout(env->P);
    const StateHeader want = state_header(env, L, count);
    if (memcmp(h.magic, want.magic, sizeof h.magic) || h.format != want.format || h.header_bytes != want.header_bytes)
        return fail_arg(env, "not a state blob of this library (bad magic, format or header size)");
    if (h.fingerprint != want.fingerprint)
        return fail_arg(env, "state blob was saved by an environment with another configuration (fingerprint mismatch: "
                             "topology, tables, slots, capacity or traffic differ)");
    if (h.rec32 != want.rec32 || h.track_ids != want.track_ids || h.row_words != want.row_words || h.n_links != want.n_links ||
        h.capacity != want.capacity || h.devenv_bytes != want.devenv_bytes || h.n_sections != want.n_sections ||
        h.block_bytes != want.block_bytes || memcmp(h.sec_bytes, want.sec_bytes, sizeof h.sec_bytes) ||
        memcmp(h.sec_off, want.sec_off, sizeof h.sec_off))
        return fail_arg(env, "state blob layout differs from this build's (record codec, id tracking, row words, capacity or "
                             "sizeof(DevEnv))");
    if (h.count != count) return fail_arg(env, "state blob holds another number of replicas than count");
    // a destination without a request source adopts the device generator when every replica comes from one (the blob carries
    // the stream keys and counters); anything else needs ongym_seed / ongym_set_requests BEFORE the load (both rewind counters)
    const bool adopt_rng = !env->has_source && h.req_mode == kReqRng && count == env->P.batch;
    if (!env->has_source && !adopt_rng)
        return fail_arg(env, "no request source: call ongym_seed or ongym_set_requests before ongym_state_load (a load of all "
                             "replicas from a device-generator environment sets it)", ONGYM_E_STATE);
    if (adopt_rng && (flags & ONGYM_STATE_KEEP_STREAM))
        return fail_arg(env, "ONGYM_STATE_KEEP_STREAM needs a request source on the destination", ONGYM_E_STATE);
    const unsigned char *blob = static_cast<const unsigned char *>(in);
    if (!env->cfg.io_device) {
        const size_t total = sizeof(StateHeader) + (size_t)count * (size_t)L.block_bytes;
        if (int rc = ensure_state_stage(env, total)) return rc;
        HIP_TRY(env, hipMemcpyAsync(env->d_state_stage, in, total, hipMemcpyHostToDevice, env->stream));
        HIP_TRY(env, hipStreamSynchronize(env->stream));
        blob = static_cast<const unsigned char *>(env->d_state_stage);
    }
    if (replicas)
        if (int rc = upload_state_list(env, count, replicas)) return rc;
    StateCopyArgs a{};
    a.L = L;
    a.cur = state_arrays(env->P);
    a.blob = const_cast<unsigned char *>(blob) + sizeof(StateHeader);
    a.list = replicas ? env->d_state_idx : nullptr;
    a.batch = env->P.batch;
    state_keep_mask(flags, a.keep_lo, a.keep_hi);
    // records of a trace the lean kernels cannot replay may exceed the lean codec (slot counts past its tables, bit rates
    // outside the configured table): the destination keeps the generic kernels from now on, as ongym_set_requests does
    if (h.trace_used) env->trace_used = true;
    if (adopt_rng) {
        env->P.req_mode = kReqRng;
        env->has_source = true;
        if (int rc = push_params(env)) return rc;
    }
    return launch_state_copy<kCopyUnpack>(env, count, a);
}

int ongym_fork(ongym_env *env, const int32_t *src, int32_t flags) {
    if (!env || !src) return env ? fail_arg(env, "null src") : ONGYM_E_ARG;
    if (flags & ~(ONGYM_STATE_KEEP_STREAM | ONGYM_STATE_KEEP_PARAMS)) return fail_arg(env, "unknown ONGYM_STATE_* flag");
    const int B = env->P.batch;
    if (!env->cfg.io_device)
        for (int j = 0; j < B; j++)
            if (src[j] >= B) return fail_arg(env, "fork source entry >= batch");
    HIP_TRY(env, hipSetDevice(env->cfg.device));
    const StateLayout L = state_layout(env->P);
    if (!env->state_alt[kSecEnv]) {   // the second set of state arrays, once: all sections or none
        void *p[kStateSections] = {};
        for (int s = 0; s < kStateSections; s++) {
            if (!L.bytes[s]) continue;
            const hipError_t e = hipMalloc(&p[s], (size_t)B * (size_t)L.bytes[s]);
            if (e != hipSuccess) {
                for (int q = 0; q < s; q++) if (p[q]) (void)hipFree(p[q]);
                env->err = std::string("hipMalloc of the fork's state arrays: ") + hipGetErrorString(e);
                return ONGYM_E_HIP;
            }
        }
        for (int s = 0; s < kStateSections; s++)
            if (p[s]) { env->allocs.push_back(p[s]); env->state_alt[s] = p[s]; }
    }
    if (!env->cfg.io_device)
        if (int rc = upload_state_list(env, B, src)) return rc;
    StateCopyArgs a{};
    a.L = L;
    a.cur = state_arrays(env->P);
    for (int s = 0; s < kStateSections; s++) a.alt.base[s] = static_cast<unsigned char *>(env->state_alt[s]);
    a.list = env->cfg.io_device ? src : env->d_state_idx;
    a.batch = B;
    state_keep_mask(flags, a.keep_lo, a.keep_hi);
    if (int rc = launch_state_copy<kCopyGather>(env, B, a)) return rc;
    // every replica now lives in the other set: swap the sets (the kernels and queries read the arrays through Params)
    void *old[kStateSections];
    for (int s = 0; s < kStateSections; s++) old[s] = a.cur.base[s];
    set_state_arrays(env->P, env->state_alt);
    for (int s = 0; s < kStateSections; s++) env->state_alt[s] = old[s];
    return push_params(env);
}

#ifdef ONGYM_STAMPS
// diagnostic build only: per-phase shader-cycle sums (not part of the ABI)
int ongym_debug_stamps(ongym_env *env, unsigned long long *out16) {
    HIP_TRY(env, hipStreamSynchronize(env->stream));
    HIP_TRY(env, hipMemcpy(out16, env->P.dbg, 16 * 8, hipMemcpyDeviceToHost));
    HIP_TRY(env, hipMemset(env->P.dbg, 0, 16 * 8));
    return 0;
}
#endif

}  // extern "C"
