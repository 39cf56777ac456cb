// ongym_host.hpp — host-side state of one environment, shared by the translation units of libongym_hip.so
// (ongym_hip.hip: generic kernels + C ABI; ongym_fast.hip: the lean policy kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "ongym_device.hpp"

using ongym::Params;

// Device staging of a call with host buffers: the call's arrays side by side, grown on demand and never shrunk (stage_open,
// ongym_hip.hip).  One slot per family of calls, and no slot shared between calls whose buffers could be in flight together:
struct Stage { void *base; size_t bytes; };
enum {
    kStageBlocks, kStageMetrics, kStageQot, kStageImpact,   // ongym_observe_blocks, _link_metrics, _service_qot, _action_impact
    kStageFailure,  // ongym_failure_impact: link_out | svc_out | links; ongym_failure_sets: set_out | sets | svc_out
    kStageAdmission,      // ongym_admission_map: summary | map | margin | weights | actions
    kStageAdmissionPart,  // ... and its groups' partial sums (device only, allocated at create and never grown)
    kStagePlayout,  // ongym_playout: playout_out | actions
    kStageCut,      // ongym_cut_links: cut_out | sets | svc_out | index_out; ongym_repair_links: sets | repaired_out; ongym_failed_links
    kStageStep,     // ongym_step_policy, _step_actions, _step_actions_bundle (B > 256): records | actions | next actions | flags
    kStagePolicy,   // ongym_policy_actions: actions | flags
    kStageMask,     // ongym_observe (mask | obs) and ongym_sample_actions (mask | actions): ONE buffer for the action mask
    kStageReset,    // ongym_reset, _reset_episode_counters: the mask; these two return without synchronising
    kStageQuery,    // the ongym_query_* calls: used with io_device too (query results are always host buffers)
    kStageMove,     // ongym_move_services: move_out | moves
    kStageSpectrum, // ongym_spectrum_map: owner_out | rec_out | release_out | audit_out
    kStageScore,    // ongym_score_actions: actions | best_out | count_out | weights
    kStages
};

struct ongym_env {
    ongym_config cfg{};
    Params P{};
    Params *d_P = nullptr;          // device copy read by the kernels (scalar loads); refreshed by push_params
    hipStream_t stream = nullptr;   // the stream every call runs on: own_stream, or the caller's (ongym_set_stream)
    hipStream_t own_stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    size_t lds = 0;
    std::vector<void *> allocs;
    std::string err;
    void *d_trace = nullptr;        // owned copy of a host trace
    Stage stage[kStages] = {};      // device staging of the calls that take host buffers (stage_open, ongym_hip.hip)
    void *h_pinned = nullptr; size_t h_pinned_bytes = 0;     // pinned staging of ongym_step_actions_bundle
    bool has_source = false;
    uint64_t replica_base = 0;      // global index of this environment's first replica (ongym_seed_base)
    std::vector<double> cfg_bit_rates;     // host copy of the discrete bit rates
    bool fast_ok = false;           // the configuration is eligible for k_fast (decided in build_lean(), ongym_hip.hip)
    bool fast_m64 = false;
    bool fast_wide = true;          // some slot count of the traffic table exceeds 32: the general (`w`) lean kernels run
    uint32_t lean_policies = 0;     // bit p: policy p's lean unit prepared at create (its LDS block fits the CU)
    bool trace_used = false;        // a trace the lean kernel cannot replay was installed: its records may not fit the lean codec
    bool trace_fast_ok = false;     // the installed (host) trace only carries bit rates of the configured table
    size_t fast_lds = 0;
    // save / restore / fork of replica states (ongym_state.hpp)
    uint64_t state_fp = 0;          // fingerprint of the configuration (computed at create from the tables' contents)
    void *state_alt[9] = {};        // ongym_fork: the second set of state arrays (lazily allocated; swapped with Params' set)
    int32_t *d_state_idx = nullptr; // [batch] replica list of a save / load, or a host fork list
    void *d_state_stage = nullptr; size_t state_stage_bytes = 0;   // device copy of a host blob
    // ongym_failure_impact (ongym_failure.hpp): route -> node pair (the lowest src * n_nodes + dst whose pair_paths list holds
    // it; -1: in no list), built at create; a message instead when two pairs disagree about a route's list
    const int32_t *d_path_pair = nullptr;
    std::string path_pair_err;
    // ongym_admission_map (ongym_admission.hpp): a message when a node pair lists different routes in its two directions
    std::string admission_pair_err;
    int admission_groups = 0;       // ONGYM_ADMISSION_GROUPS at create: wavefront groups per scenario instead of the rule's (0: the rule)
    // ongym_playout (ongym_playout.hpp): ONGYM_PLAYOUT_ORDER at create, a measurement knob: 1 = grid with the replicas fastest,
    // 0 = a replica's scenarios adjacent, unset = the default
    int playout_by_replica = 0;
};

#define HIP_TRY(env, expr)                                                                               \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess) {                                                                          \
            (env)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                              \
            return ONGYM_E_HIP;                                                                          \
        }                                                                                                \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is set on the CURRENT device's function object: keep, per (device, kernel), the
// largest request ever made (an environment with a smaller LDS block must not lower the limit under one created earlier)
// and only ever raise it.  Defined in ongym_hip.hip; serialised by a mutex (environments may be created from several threads).
hipError_t raise_lds_limit(int device, const void *kernel, size_t bytes);

// ongym_fast.hip, two units per policy id p: the lean kernels k_fast<..., p> — LDS limit, launch, occupancy query.  The `w`
// units are the general build (slot counts up to 512); the plain ones assume every slot count of the configuration is <= 32
// (ongym_env::fast_wide == false: one-step run-AND shifts, two-word marks, no wide-release path: +6 % on NSFNET-320).
namespace ongym {
#define ONGYM_FAST_DECL(p)                                                            \
    int fast_prepare_p##p(ongym_env *env);                                            \
    int fast_launch_p##p(ongym_env *env, int nsteps, ongym_step_rec *d_out);          \
    int fast_occupancy_p##p(ongym_env *env, int *blocks_per_cu, int *lds_bytes);
ONGYM_FAST_DECL(0) ONGYM_FAST_DECL(1) ONGYM_FAST_DECL(2) ONGYM_FAST_DECL(10)
ONGYM_FAST_DECL(0w) ONGYM_FAST_DECL(1w) ONGYM_FAST_DECL(2w) ONGYM_FAST_DECL(10w)
#undef ONGYM_FAST_DECL
}
