/*
 * ongym.h — C ABI of the MI355X-native batched QRMSA environment (libongym_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of LEA-UFPA/optical-networking-gym: the per-request loop of
 * optical_networking_gym/envs/qrmsa.pyx (first-fit policy + step + traffic/departure bookkeeping) with the GN model of
 * optical_networking_gym/core/osnr.pyx.  The reference has no C interface of its own (its Cython modules only export
 * the CPython module init), so each entry point below names the reference Python/Cython interface it replaces.
 * Plain pointers and sizes only; no torch / numpy types.  Host code stays Python (ctypes), see INTEGRATION.md.
 *
 * Ownership : the library owns all device state; callers own every buffer they pass in.  Input tables given to
 *             ongym_create are copied.  Output buffers are host pointers, or device pointers when cfg.io_device = 1
 *             (e.g. torch.Tensor.data_ptr() of a PyTorch-ROCm tensor on the same device).
 * Errors    : every call returns 0 on success, <0 on error (ONGYM_E_*); ongym_last_error() gives text. Nothing throws.
 *             The reference's ValueError on a QoT-infeasible action (qrmsa.pyx:925-929) is the per-replica
 *             ONGYM_F_QOT_ERROR flag of ongym_step_rec.flags (the Python shim re-raises it in single-env mode).
 * Threading : one ongym_env = one HIP device + one HIP stream; not thread-safe; launches are asynchronous on that
 *             stream, results are complete after ongym_sync() (calls that copy to host buffers sync themselves).
 * Staging   : a call that takes host buffers lays its arrays out in a device buffer of its call family (grown on demand,
 *             kept until ongym_destroy), copies the inputs in, launches, copies the outputs back and synchronises once.
 *             A NULL optional array takes no room.  With cfg.io_device the kernels get the caller's pointers instead.
 * Multi-GPU : one process per GPU, one ongym_env each; replicas are independent so there is no data-path collective.
 */
#ifndef ONGYM_H
#define ONGYM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ONGYM_ABI_VERSION 4

enum {
    ONGYM_OK = 0,
    ONGYM_E_ARG = -1,      /* bad argument / inconsistent tables */
    ONGYM_E_HIP = -2,      /* HIP runtime error (no device, launch failure, ...) */
    ONGYM_E_STATE = -3,    /* call not valid in the current state (e.g. no request source set) */
    ONGYM_E_CAPACITY = -4, /* a replica overflowed its service table (cfg.capacity too small) */
    ONGYM_E_LIMIT = -5     /* configuration exceeds a compile-time limit of the kernels */
};

/* policies fused on device; replaces optical_networking_gym/heuristics/heuristics.py:923-966 */
enum {
    ONGYM_POLICY_FIRST_FIT = 0,      /* heuristic_shortest_available_path_first_fit_best_modulation, heuristics.py:923-966 */
    ONGYM_POLICY_LOAD_BALANCING = 1, /* load_balancing_best_modulation, heuristics.py:547-627 (graph_load.py heuristic 4) */
    ONGYM_POLICY_HIGHEST_SNR = 2,    /* heuristic_highest_snr, heuristics.py:272-328 (graph_load.py heuristic 2) */
    /* the cheaper remaining policies of heuristics.py, one shared kernel instantiation (graph_launch_power.py 2,3,6,7,9): */
    ONGYM_POLICY_LOWEST_SPECTRUM = 3, /* shortest_available_path_lowest_spectrum_best_modulation, :431-490 */
    ONGYM_POLICY_LB_FIRST_FIT = 4,    /* heuristic_load_balancing_first_fit, :202-269 */
    ONGYM_POLICY_BEST_MOD_LB = 5,     /* best_modulation_load_balancing, :491-545 */
    ONGYM_POLICY_MSCL_SIMPLIFIED = 6, /* heuristic_mscl_simplified, :765-839 */
    ONGYM_POLICY_MSCL_SEQUENTIAL = 7, /* heuristic_mscl_sequential_simplified, :841-921 */
    ONGYM_POLICY_PSR = 8,             /* heuristic_psr with its default coefficients, :1019-1119 */
    ONGYM_POLICY_EXACT_FIT = 9,       /* heuristic_exact_fit, :1121-1227 (asks for no guard slot: the step may answer
                                         with the occupied-slots penalty, retry = 1) */
    /* the two policies that score every candidate (one more instantiation, csrc/ongym_scored.hpp): */
    ONGYM_POLICY_LOWEST_FRAGMENTATION = 10, /* heuristic_lowest_fragmentation, :330-414 (its request is sized slots + 1; if the
                                               step's own GSNR check at `slots` then fails - the reference raises ValueError,
                                               qrmsa.pyx:925-929 - the fused loop rejects the request with
                                               ONGYM_F_QOT_ERROR | ONGYM_F_BLOCKED_OSNR and goes on) */
    ONGYM_POLICY_MSCL = 11,                 /* heuristic_mscl, :647-749 (discrete bit rates only: the loss is summed over them) */
    ONGYM_POLICY_COUNT = 12
};

/* ongym_step_rec.flags */
enum {
    ONGYM_F_BLOCKED_RESOURCES = 1, /* 2nd element of the heuristic's return tuple, heuristics.py:966 */
    ONGYM_F_BLOCKED_OSNR = 2,      /* 3rd element */
    ONGYM_F_QOT_ERROR = 4,         /* action decoded to free slots whose GSNR < threshold+margin: qrmsa.pyx:925-929 */
    ONGYM_F_OVERFLOW = 8,          /* service table full: request was rejected artificially, results invalid */
    ONGYM_F_NO_REQUEST = 16        /* replay trace exhausted: step was a no-op */
};

/*
 * Static description of the network + traffic.  Replaces the arguments of QRMSAEnv.__init__ (qrmsa.pyx:206-237) and
 * the data that optical_networking_gym/topology.pyx:244-369 (get_topology) attaches to the graph, flattened:
 *   pair_paths[(src*n_nodes+dst)*k_paths + k] = path id or -1      (k_shortest_paths[src,dst][k], qrmsa.pyx:277)
 *   path_links[p*max_hops + h], h < path_hops[p]                    (Path.links, topology.pyx:72-95; link "index")
 *   link_*[e]                                                       (Link.spans: all spans of a link are equal,
 *                                                                    topology.pyx:288-299; alpha in 1/m, nf linear,
 *                                                                    Span, topology.pyx:11-34)
 *   mod_se / mod_min_osnr [m]                                       (Modulation, topology.pyx:53-70), m ascending
 */
typedef struct ongym_config {
    int32_t struct_size; /* = sizeof(ongym_config) */
    int32_t abi_version; /* = ONGYM_ABI_VERSION */
    int32_t n_nodes, n_links, n_paths, k_paths, max_hops, n_mods, n_slots;
    int32_t batch;          /* number of independent replicas B */
    int32_t capacity;       /* max simultaneously running services per replica (multiple of 64) */
    int32_t episode_length; /* qrmsa.pyx:210; an episode is episode_length-1 steps */
    int32_t auto_reset;     /* 1: a replica that terminates is reset inside the same launch (graph_load.py:157-158) */
    int32_t bit_rate_mode;  /* 0 = "discrete" (bit_rates/bit_rate_cum), 1 = "continuous" (randint(lo,hi)) */
    int32_t n_bit_rates;
    int32_t bit_rate_lo, bit_rate_hi;
    int32_t device;         /* HIP device ordinal */
    int32_t io_device;      /* 1: in/out buffers of step/set_requests calls are device pointers */
    int32_t measure_disruptions; /* qrmsa.pyx:224, 937-952: after every accept re-evaluate the GSNR of the services that share a
                                    link with the new one and count those that fall below their modulation's threshold */
    int32_t defragmentation;     /* qrmsa.pyx:233, 1117-1119: after a departure, try to move running services to lower slots */
    int32_t n_defrag_services;   /* qrmsa.pyx:234: 0 = after EVERY departure, no limit on moves; N > 0 = only when the
                                    episode's request count is a multiple of N, at most N moves */
    double frequency_start;       /* Hz,  qrmsa.pyx:221 */
    double slot_bandwidth;        /* Hz,  qrmsa.pyx:222 */
    double channel_width;         /* GHz, qrmsa.pyx:228 (get_number_slots, qrmsa.pyx:1198-1205) */
    double launch_power_w;        /* 10**((dBm-30)/10), qrmsa.pyx:288 */
    double margin;                /* dB, qrmsa.pyx:223 */
    double load;                  /* Erlang, qrmsa.pyx:211 */
    double mean_holding_time;     /* s, qrmsa.pyx:212 */
    const int32_t *pair_paths;    /* [n_nodes*n_nodes*k_paths] */
    const int32_t *path_hops;     /* [n_paths] */
    const int32_t *path_links;    /* [n_paths*max_hops] */
    const int32_t *link_nspans;   /* [n_links] */
    const double *link_span_km;   /* [n_links] */
    const double *link_alpha;     /* [n_links] 1/m */
    const double *link_nf;        /* [n_links] linear */
    const int32_t *mod_se;        /* [n_mods] spectral efficiency (1..6) */
    const double *mod_min_osnr;   /* [n_mods] dB */
    const double *bit_rates;      /* [n_bit_rates] Gb/s */
    const double *bit_rate_cum;   /* [n_bit_rates] cumulative probabilities, last = 1 */
    const double *node_cum;       /* [n_nodes] cumulative node request probabilities, last = 1 (qrmsa.pyx:278-286) */
    /* optional per-replica overrides (NULL = use the scalar above): the JOCN sweeps over launch power / load / margin
     * (graph_launch_power.py, graph_load.py, graph_margin.py) become a batch dimension */
    const double *replica_launch_power_w; /* [batch] */
    const double *replica_load;           /* [batch] */
    const double *replica_margin;         /* [batch] */
    /* observation() only (qrmsa.pyx:583-781): route lengths normalised by the min/max LINK length (:692-705) */
    const double *path_len_norm;          /* [n_paths] or NULL (ongym_observe then fails) */
    double max_bit_rate;                  /* max(bit_rates), qrmsa.pyx:679 */
    /* 1: keep Service.service_id (qrmsa.pyx:1092) per running service, as cfg.defragmentation does.  calculate_osnr skips
     * the running services whose id equals the evaluated service's (core/osnr.pyx:65, "quirk Q12"); ids are unique inside
     * an episode, so this only shows after ongym_reset_episode_counters restarted them under services that keep running.
     * Needed by ongym_reset_episode_counters; selects the id-tracking (slower) kernels. */
    int32_t track_service_ids;
    /* modulations_to_consider (qrmsa.pyx:313): 0 or >= n_mods = all of them.  Below n_mods the action space shrinks to
     * k_paths * n_mods_consider * n_slots + 1 and addresses the n_mods_consider formats at and below max_modulation_idx
     * (action codec qrmsa.pyx:801-834, heuristics.py:36-54); ongym_observe then first finds max_modulation_idx like
     * get_max_modulation_index (qrmsa.pyx:543-581) and reports that window (:712-717). */
    int32_t n_mods_consider;
    /* Width that get_number_slots divides by (qrmsa.pyx:1198-1205), in the unit of channel_width; 0 = channel_width itself.
     * The reference's `bands` argument (qrmsa.pyx:417-425; passed by graph_launch_power.py:102) makes get_number_slots use the
     * C band's width in Hz - every service then needs ONE slot (quirk Q9) - while observation() and step() keep computing
     * frequencies with channel_width (qrmsa.pyx:606-610, 678): the two widths are separate fields here. */
    double nslots_channel_width;
} ongym_config;

/* One service request; replaces the fields drawn in QRMSAEnv._next_service (qrmsa.pyx:1079-1101). */
typedef struct ongym_request {
    float arrival_time; /* absolute, already rounded to float32 like the reference's `cdef float at` */
    float holding_time;
    float bit_rate;
    int16_t source;     /* node index */
    int16_t destination;
} ongym_request;

/* Per-replica result of one step; replaces the (obs, reward, terminated, truncated, info) tuple of QRMSAEnv.step
 * (qrmsa.pyx:838-1065) for gen_observation=False, plus what the heuristic returned. 56 bytes. */
typedef struct ongym_step_rec {
    int32_t action;      /* action index applied (p*M*S + (max_mod-m)*S + slot, reject = k*M*S; heuristics.py:36-54) */
    int16_t route;       /* info["chosen_path_index"], -1 on reject */
    int16_t modulation;  /* absolute modulation index, -1 on reject */
    int16_t slot;        /* info["chosen_slot"], -1 on reject */
    int16_t nslots;
    uint8_t accepted;
    uint8_t terminated;
    uint8_t retry;       /* 1: slots were not free, request stays current (qrmsa.pyx:886-897) */
    uint8_t flags;       /* ONGYM_F_* */
    int32_t active;      /* running services after the step (len(topology.graph["running_services"])) */
    double osnr, ase, nli; /* dB, of the accepted service (info["osnr"]); 0 on reject */
    double reward;
} ongym_step_rec;

/* A running service as seen by the compatibility view (Service, qrmsa.pyx:29-53). */
typedef struct ongym_service {
    int32_t path_id;
    int16_t slot, nslots;
    int16_t modulation;
    int16_t reserved;   /* 1: member of disrupted_services_list (measure_disruptions) */
    float release_time; /* float32(arrival+holding), the heap key after rounding (qrmsa.pyx:1114-1115,1329) */
    int32_t service_id; /* Service.service_id (qrmsa.pyx:1092); kept only when cfg.defragmentation, else -1 */
    int32_t pad_;
    double osnr;        /* Service.OSNR as last written (provisioning or defragment(), qrmsa.pyx:1630); only when
                           cfg.defragmentation, else 0 */
} ongym_service;

/* One reallocation done by defragment() (qrmsa.pyx:1590-1635) during the LAST step of a replica: what the compatibility
 * view needs to update the moved Service object (initial_slot, center_frequency, OSNR, ASE, NLI). */
#define ONGYM_MOVE_LOG 64
typedef struct ongym_move {
    int32_t service_id;
    int32_t slot;        /* new initial_slot */
    double osnr, ase, nli; /* dB, as rewritten by defragment() */
} ongym_move;

/* Counters behind the info dict (qrmsa.pyx:996-1060) and the JOCN per-episode CSV row (graph_load.py:169-186). */
typedef struct ongym_stats {
    int64_t services_processed, services_accepted;                 /* never reset (quirk Q3) */
    int64_t episode_services_processed, episode_services_accepted; /* current episode */
    double bit_rate_requested, bit_rate_provisioned;               /* reset by reset(), qrmsa.pyx:466-467 */
    double episode_bit_rate_requested, episode_bit_rate_provisioned;
    int64_t rejected;                                              /* bl_reject of the current episode */
    int64_t episode_modulation_hist[8];
    double episode_osnr_sum;                                       /* sum of Service.OSNR over the episode's services */
    int64_t episodes_completed;
    int64_t disrupted_services, episode_disrupted_services;       /* qrmsa.pyx:948-952 (both zeroed by reset()) */
    /* defragment() (qrmsa.pyx:1545-1639): counters of the current episode, their value when the last step built its info
     * dict (i.e. before that step's _next_service ran, :1008-1009) */
    int64_t episode_defrag_cycles, episode_service_reallocations;
    int64_t step_defrag_cycles, step_service_reallocations;
    /* totals over all completed steps since create (for throughput accounting and the RCCL stats reduction) */
    int64_t total_steps, total_accepted, total_gn_evals, total_interferer_terms;
    int64_t total_paths_tried, total_path_hops; /* candidate paths whose slot rows were read, and their hops */
    int64_t total_gn_shortcuts;                 /* GN evaluations decided by the ASE-only bound (device only) */
    int64_t total_active_sum;                   /* sum over steps of the running-service count after the step */
    double current_time;
    int32_t active, flags;
    int32_t max_modulation_idx; /* QRMSAEnv.max_modulation_idx: n_mods-1 after reset (qrmsa.pyx:437), set by observation()'s
                                   get_max_modulation_index (:543-581, 680); the action codec is relative to it */
    int32_t reserved0_;
    /* snapshot taken at the last terminal step (what graph_load.py writes per episode). Kept LAST: the kernels hold only
     * the fields above in LDS and write these straight to memory. */
    int64_t last_episode_processed, last_episode_accepted, last_rejected;
    double last_service_blocking_rate, last_episode_service_blocking_rate;
    double last_bit_rate_blocking_rate, last_episode_bit_rate_blocking_rate;
    int64_t last_modulation_hist[8];
    double last_mean_gsnr;
    int64_t last_episode_disrupted;
    int64_t last_episode_defrag_cycles, last_episode_service_reallocations;   /* :1008-1009 at the terminal step */
} ongym_stats;

typedef struct ongym_env ongym_env;

/* QRMSAEnv.__init__ (qrmsa.pyx:206-425) for B replicas; does NOT generate the first request: call
 * ongym_seed or ongym_set_requests, then ongym_reset. */
int ongym_create(const ongym_config *cfg, ongym_env **out);
void ongym_destroy(ongym_env *env);

/* Request source A — device generator: replica r draws from the counter-based stream (seed, r) defined in
 * ongym_traffic.h.  Stands in for `self.rng = random.Random()` (qrmsa.pyx:241; unseeded in the reference, quirk Q2). */
int ongym_seed(ongym_env *env, uint64_t seed);
/* The same with a replica offset: local replica r draws stream (seed, replica_base + r).  A batch sharded over several
 * environments / GPUs (shard k owning the global replicas [base_k, base_k + batch_k)) then simulates exactly the
 * replicas of the unsharded batch — the fan-out of graph_load.py:361-363 (one simulation per Pool task) with
 * reproducible streams.  ongym_seed(env, seed) == ongym_seed_base(env, seed, 0). */
int ongym_seed_base(ongym_env *env, uint64_t seed, uint64_t replica_base);
/* Request source B — trace replay: reqs[r*n_per_replica + i] is the i-th request replica r will draw.
 * Used for parity against captured reference traces (each _next_service call consumes one entry).
 * Times: every arrival_time is finite with a clear sign bit (so not -0.0 either), every holding_time is not NaN and has a
 * clear sign bit; a holding_time of +inf is legal (the service never leaves).  Arrival times need not be monotone: when the
 * clock steps back nothing leaves.  A service leaves when float32(arrival + holding) <= float32(clock), and the sign bit of
 * a stored release time is the 'disrupted' flag of measure_disruptions, so the step kernels do not agree on a clock below
 * zero, and no comparison holds with a NaN.  A host trace (io_device = 0) is checked: an entry outside this contract, or
 * with an invalid node pair or bit rate, returns ONGYM_E_ARG and leaves the earlier request source installed.  A device
 * trace (io_device = 1) is not read by the host: the same contract is the caller's to keep. */
int ongym_set_requests(ongym_env *env, const ongym_request *reqs, int64_t n_per_replica);

/* QRMSAEnv.reset (qrmsa.pyx:427-504) on the replicas with mask[r] != 0 (NULL = all).  The mask is read on the stream (a
 * host mask is copied at the call) and the call returns without synchronising; so does ongym_reset_episode_counters. */
int ongym_reset(ongym_env *env, const uint8_t *mask);

/* QRMSAEnv.reset(options={"only_episode_counters": True}) (qrmsa.pyx:427-464) on the replicas with mask[r] != 0 (NULL =
 * all): episode counters and histograms to zero, and — like the reference's `self._events = []` — the departure heap is
 * dropped, so the services running at that moment never leave.  Grid, running services, totals, clock and the current
 * request stay; no request is drawn.  Needs cfg.track_service_ids (ONGYM_E_STATE otherwise): service ids restart at 0 under
 * services that keep running, and calculate_osnr identifies "self" by service id (core/osnr.pyx:65). */
int ongym_reset_episode_counters(ongym_env *env, const uint8_t *mask);

/* nsteps iterations of `action,_,_ = heuristic(env); env.step(action)` (graph_load.py:161-163) fused on device.
 * out: [nsteps][batch] records or NULL. */
int ongym_step_policy(ongym_env *env, int32_t policy, int32_t nsteps, ongym_step_rec *out);
/* QRMSAEnv.step(action) (qrmsa.pyx:838-1065) with caller-supplied actions[batch]. out: [batch] or NULL. */
int ongym_step_actions(ongym_env *env, const int32_t *actions, ongym_step_rec *out);
/* The loop body of the reference's drivers (graph_load.py:157-164: `action = heuristic(env); env.step(action)`) for callers that
 * hold ONE environment and need every result on the host: ongym_step_actions(actions), then - on the same stream, with no host
 * round trip in between - fused policy `next_policy` evaluated on the NEW current request (as ongym_policy_actions; a negative
 * id skips it), and step records [batch], the new requests [batch], the statistics [batch] and the next actions / flags [batch]
 * come back together behind ONE synchronisation (host buffers only; next_actions / next_flags may be NULL when next_policy < 0). */
int ongym_step_actions_bundle(ongym_env *env, const int32_t *actions, int32_t next_policy, ongym_step_rec *rec_out,
                              ongym_request *request_out, ongym_stats *stats_out, int32_t *next_actions, uint8_t *next_flags);
/* The heuristic alone, without stepping: actions[batch], flags[batch] (ONGYM_F_BLOCKED_*) (heuristics.py:923-966). */
int ongym_policy_actions(ongym_env *env, int32_t policy, int32_t *actions, uint8_t *flags);

/* QRMSAEnv.observation() (qrmsa.pyx:583-781, gen_observation=True) for the CURRENT request of every replica:
 * obs  float32 [batch][1 + 2 + k_paths + k_paths*Mc*12]  (bit rate, src, dst, k route lengths, 12 features per (path,
 *      modulation) pair incl. the normalised GSNR of calculate_osnr_observation, core/osnr.pyx:259-369)
 * mask uint8   [batch][k_paths*Mc*n_slots + 1]            (info['mask'], last entry = reject = 1)
 * Mc = cfg.n_mods_consider.  For Mc < n_mods the call first sets ongym_stats.max_modulation_idx like
 * get_max_modulation_index (qrmsa.pyx:543-581) and describes the Mc formats at and below it.
 * Needs slot_bandwidth == channel_width*1e9 (the reference's observation mixes the two, core/osnr.pyx:259-369). With per-link
 * attenuation the interferer field is evaluated term by term (no pair table): same results, about ten times slower. */
int ongym_observe(ongym_env *env, float *obs, uint8_t *mask);

/* Block action space (DeepRMSA / optical-rl-gym; the reference's `blocks_to_consider` and get_available_blocks,
 * qrmsa.pyx:231, 242, 1515-1531) for the CURRENT request of every replica, J = blocks in [1, 16], K = k_paths, M = n_mods:
 * the fitting blocks of route k for n slots are the maximal free runs [a, a+L) of its row (the AND of its links' free bits),
 * in increasing a, that hold a candidate of _get_candidates (qrmsa.pyx:515-541): L >= n for a run that ends at n_slots,
 * L >= n + 1 (guard slot) otherwise.  Blocks(k, m) are the first J of them for n = get_number_slots(request, m).  Block
 * action (k, j) decodes best format first, as first fit does (heuristics.py:923-966): the first m (M-1 down to 0) with a
 * block Blocks(k, m)[j] = (a, L) whose calculate_osnr at (route k, slot a, n) passes minimum_osnr[m] + margin; none: invalid.
 * So block action (k, 0) is first fit restricted to route k.
 * obs        float32 [batch][3 + 3K + 6KJ]: ongym_observe's first 3 + K entries (bit rate, src, dst, K route lengths), then per
 *            route its free-slot count / S and longest free run / S (-1: no such route), then per (k, j), route-major: valid,
 *            a/S, L/S, n/S, (m+1)/M, (GSNR_dB - minimum_osnr[m] - margin)/10 (an invalid entry: 0, then five -1)
 * mask       uint8   [batch][KJ + 1]: entry k*J + j = valid; the last entry (reject) is always 1
 * action_map int32   [batch][KJ + 1]: the full action index k*M*S + (M-1-m)*S + a of every valid entry (get_action_index
 *            with max_modulation_idx = M-1), the reject action K*M*S elsewhere: ongym_step_actions takes it as it is
 * Read-only: no replica state, statistic or counter changes.  The QoT decisions are the step's own (same GN code, same n(m)), so
 * a valid entry is always accepted.  A replica without a current request gets zeros in the first 3 + K entries and nothing
 * valid.  Needs path_len_norm and max_bit_rate (not slot_bandwidth == channel_width*1e9: the GN model is the step's); refuses
 * n_mods_consider < n_mods (no format window) with ONGYM_E_ARG.  Buffers: host buffers, or device buffers with cfg.io_device
 * (then the call only launches on the environment's stream and nothing synchronises). */
enum { ONGYM_MAX_BLOCKS = 16 };   /* J at most */
int ongym_observe_blocks(ongym_env *env, int32_t blocks, float *obs, uint8_t *mask, int32_t *action_map);

/* Spectrum fragmentation of every link of every replica (utils.pyx:61-107; qrmsa.pyx:1150-1186, 1353-1480), E = n_links in
 * table order (link e = topology[u][v]["index"]), S = n_slots.  A free run is a maximal run of free slots of link e's row, a
 * used run a maximal run of used slots; nothing at or above S counts.
 * link_out    float32 [batch][E][8], computed in double and rounded once: F = free slots, free runs, Lmax = longest free run
 *             (0: none), used runs, occupied span (one past the last used slot minus the first; 0: none), external
 *             fragmentation 1 - Lmax/F (0 if F = 0), entropy -sum (L/S) ln(L/S) over the free runs L, rss sqrt(sum L^2) / sum L
 *             (0 if F = 0).  The metrics of the utils functions on FREE runs, as their text says they measure: the reference's
 *             heuristic_lowest_fragmentation hands them rows where 1 means free, so there they count used runs instead
 *             (entry 3 is the per-link term of fragmentation_route_cuts as the reference computes it).
 * compactness float64 [batch]: _get_network_compactness, (occupied / slot_hops) * (E / inner_free_blocks) summed over the links
 *             with more than one used run (occupied = their spans, inner_free_blocks = free runs inside them; slot_hops = sum
 *             of nslots * hops over the running services); 1.0 when no link has a free run inside its span.
 * link_stats  float64 [batch][E][4] in/out (utilization, external_fragmentation, compactness, last_update), owned by the caller
 *             and zeroed by it before the first call: _update_link_stats of every link at the replica's current_time, with the
 *             reference's arithmetic and quirks (max_empty = 0 unless two or more free runs that are not exactly the first and
 *             the last; the fragmentation divisor is the used-slot count, so an idle link gives NaN; the compactness divisor
 *             counts used runs; utilization is not updated at current_time 0 but the other two are still divided by it).
 *             NaN and negative values are kept.
 * Any pointer may be NULL, not all three (ONGYM_E_ARG).  Read-only: no replica state, statistic or counter changes.  Buffers:
 * host buffers (staged through a device buffer; the call synchronises), or device buffers with cfg.io_device (then the call
 * only launches on the environment's stream and nothing synchronises). */
enum { ONGYM_N_LINK_METRICS = 8, ONGYM_N_LINK_STATS = 4 };   /* entries per link of link_out, link_stats */
int ongym_link_metrics(ongym_env *env, float *link_out, double *compactness, double *link_stats);

/* Current quality of transmission of every running lightpath of every replica (core/osnr.pyx:21-142), C = capacity, E = n_links
 * in table order.  Record i is the i-th record of the replica, in the order ongym_query_services returns them.  Each running
 * service is evaluated at its own path, slot and slot count against every other running service of the replica, at the
 * replica's current launch power; itself is skipped, and with id tracking every running service with its service_id too
 * (quirk Q12, core/osnr.pyx:65), as measure_disruptions and defragmentation evaluate running services.  Any attenuation.
 * svc_out     float64 [batch][C][4]: GSNR, ASE, NLI (dB) and the margin GSNR - mod_min_osnr[modulation] of record i < active;
 *             NaN for the records at and beyond active.
 * replica_out float64 [batch][6]: running services; services below minimum_osnr (no margin: measure_disruptions' test,
 *             qrmsa.pyx:947); services below minimum_osnr + margin (the replica's margin: those the step's QoT check would
 *             refuse now); the lowest margin (NaN if nothing runs); the mean GSNR in dB (NaN if nothing runs); the record index of
 *             the lowest margin (the lowest index on a tie, -1 if nothing runs).  Both "below" tests compare in the linear domain
 *             with the dB fallback band of the step's QoT check, so they decide as the step decides.
 * link_out    float32 [batch][E][3]: running lightpaths that cross the link, their lowest margin (NaN if none), how many of
 *             them are below minimum_osnr.
 * Any pointer may be NULL, not all three (ONGYM_E_ARG).  Read-only: no replica state, statistic, counter (total_gn_evals
 * included), disrupted flag or random-number position changes.  Buffers: host buffers (staged through a device buffer grown on
 * demand; the call synchronises), or device buffers with cfg.io_device (then the call only launches on the environment's
 * stream and nothing synchronises).  ongym_last_kernel_ms times the kernel. */
enum { ONGYM_N_SERVICE_QOT = 4, ONGYM_N_REPLICA_QOT = 6, ONGYM_N_LINK_QOT = 3 };   /* entries per row of svc_out, replica_out, link_out */
int ongym_service_qot(ongym_env *env, double *svc_out, double *replica_out, float *link_out);

/* What each candidate action would do to the lightpaths that are running, before it is taken (A = n_actions, C = capacity).
 * actions [batch][A] are full step action indices (a row of ongym_observe_blocks' action_map, ongym_policy_actions' output
 * with A = 1, or any list), 1 <= A <= 256.  Each is decoded exactly as ongym_step_actions decodes it for the replica's current
 * request (route, format, start slot, the slot count of the step's own per-request table).  The candidate is that lightpath at
 * the replica's current launch power; its victims are the running records that share at least one link with its route (with id
 * tracking, records with the current request's service_id are not: quirk Q12).  Per victim, "before" is its current linear
 * ASE + NLI exactly as ongym_service_qot reports it, and "after" adds the candidate as one more interferer on every shared
 * link (the GN model is additive in the interferers, core/osnr.pyx:64-93): calculate_osnr(victim) inside
 * measure_disruptions right after the provisioning and before any departure (envs/qrmsa.pyx:937-953).  The candidate's own
 * QoT is not evaluated (the action mask says so already).
 * impact_out float64 [batch][A][8]:
 *   0 status                0 evaluated; 1 skipped (index < 0, the reject action or beyond it, or no current request);
 *                           2 spectrum not free (the step's is_path_free fails, or no such route / format / slot count)
 *   1 affected              number of victims
 *   2 below_minimum_after   victims with GSNR_after < minimum_osnr of their format (the test of qrmsa.pyx:947)
 *   3 newly_below_minimum   of those, the ones not below before
 *   4 newly_below_margin    victims below minimum_osnr + the replica's margin after and not before
 *   5 lowest_margin_after   min over the victims of GSNR_after - minimum_osnr (dB)
 *   6 largest_drop          max over the victims of GSNR_before - GSNR_after (dB)
 *   7 lowest_margin_record  record index of column 5 (the lowest index on a tie; the order of ongym_query_services)
 *   Status 1 or 2: columns 1-7 are NaN.  Status 0 without a victim: columns 1-4 are 0, 5 and 6 NaN, 7 is -1.  Every "below"
 *   decision compares linear 1/GSNR inside the 1e-9 dB-fallback band of the step's QoT check and of ongym_service_qot.
 * svc_in      NULL, or the svc_out (float64 [batch][C][4], dB) of an ongym_service_qot call on the SAME state: "before" is then
 *             10^(-ASE/10) + 10^(-NLI/10) of it and the kernel evaluates no baseline of its own.
 * Read-only: no replica state, statistic, counter (total_gn_evals included), disrupted flag or random-number position changes.
 * Buffers: host buffers (staged through a device buffer grown on demand; the call synchronises), or device buffers with
 * cfg.io_device (then the call only launches on the environment's stream and nothing synchronises).  ongym_last_kernel_ms
 * times the kernel. */
enum { ONGYM_N_ACTION_IMPACT = 8, ONGYM_MAX_IMPACT_ACTIONS = 256 };   /* impact_out entries per row; A at most */
int ongym_action_impact(ongym_env *env, int32_t n_actions, const int32_t *actions, const double *svc_in, double *impact_out);

/* What happens when a fibre is cut: per replica and per failed link of a list, the running lightpaths that go down with the
 * link and how many of them first fit restores through the spectrum that is left, at acceptable QoT (F = n_fail, E = n_links,
 * C = capacity, K = k_paths, M = n_mods, S = n_slots).  links int32 [batch][F], 1 <= F <= E, link indices in table order;
 * NULL (only with F = E): column f fails link f.  Every (replica, column) is ONE independent single-link failure on the
 * replica's current state; duplicates are allowed, an index < 0 or >= E is skipped (status 1).
 * Scenario (failed link e):
 *   victims      the running records whose route contains e, in ascending record index (the order of ongym_query_services)
 *   release      all victims leave at once, each as a departure of the step releases it (_release_path, qrmsa.pyx:1332-1350:
 *                [slot, slot + n + 1) clamped at S on every link of its route); they interfere with nobody any more
 *   restoration  one victim after the other in record order.  A victim of format m and n slots is a request of capacity
 *                n * se[m] (the record keeps no bit rate: "at least the capacity it had"); under format m' it needs
 *                n' = ceil(n * se[m] / se[m']) slots, a format with n' > S is unusable.  The search is first fit's
 *                (heuristics.py:923-966) over the routes k = 0..K-1 of the victim's node pair that do not contain e, formats
 *                m' = M-1 down to 0, the lowest start of _get_candidates(row, n', S) only, the step's GN model over everything
 *                running in the scenario at that moment (the survivors and the victims restored so far at their new places;
 *                the replica's launch power; with id tracking, records with the victim's service_id left out, quirk Q12) and
 *                the step's admission test against minimum_osnr[m'] + the replica's margin.  The first (k, m', a) that passes
 *                is provisioned as the step provisions ([a, a + n') plus the guard slot unless it ends at S) and joins the
 *                running set: later victims see its spectrum and its interference.  A victim without one is lost.
 *   node pair    of a route: the pair with the lowest src * n_nodes + dst whose pair_paths list holds it.  If two pairs that
 *                hold a route list different routes, the call refuses (ONGYM_E_ARG) rather than guess.
 * link_out float64 [batch][F][10]:
 *   0 status              0 evaluated; 1 skipped
 *   1 victims             count
 *   2 victim_capacity     sum of n * se[m] over the victims (x channel_width: Gb/s, an upper bound)
 *   3 restored            count
 *   4 restored_capacity   sum of n * se[m] (the original's) over the restored
 *   5 lost_no_spectrum    lost, and no eligible (route, format) had a valid start (no eligible route included)
 *   6 lost_qot            lost, and at least one start was evaluated and refused
 *   7 extra_hops          sum over the restored of hops(new route) - hops(old route)
 *   8 extra_slot_hops     sum over the restored of n' hops(new) - n hops(old)
 *   9 lowest_margin       min over the restored of GSNR - minimum_osnr[m'] - margin when it was restored (dB); NaN if none
 *   Status 1: columns 1-9 are NaN.  Column 1 = columns 3 + 5 + 6.
 * svc_out     NULL, or int32 [batch][F][C] (LARGE: 4 F C bytes per replica, 2.6 GB for 65 536 replicas of NSFNET at C = 448 and
 *             F = E = 22; ask for it on small batches or short link lists): per record -1 if it is no victim (or at and beyond the
 *             running count), the reject action K M S if it is lost, else the action index k M S + (M-1-m') S + a of its
 *             restoration.
 * Refused (ONGYM_E_ARG): F out of range, NULL links with F != E, NULL link_out, n_mods_consider < n_mods (no format window, as
 * ongym_observe_blocks).
 * Read-only: no replica state, statistic, counter (total_gn_evals included), disrupted flag, move log or random-number
 * position changes.  Buffers: host buffers (staged through a device buffer grown on demand; the call synchronises), or device
 * buffers with cfg.io_device (then the call only launches on the environment's stream and nothing synchronises).
 * ongym_last_kernel_ms times the kernel. */
enum { ONGYM_N_FAILURE_IMPACT = 10 };   /* link_out entries per row */
int ongym_failure_impact(ongym_env *env, int32_t n_fail, const int32_t *links, double *link_out, int32_t *svc_out);

/* What happens when several links go down at once - two fibres, a node (all its links), a shared-risk link group (the fibres
 * of one duct): ongym_failure_impact with a SET of failed links per scenario (F = n_sets, E = n_links, C = capacity).  None
 * of these follows from single-link answers: a victim of link A must also avoid link B, the victims of A and B compete for the
 * same left-over spectrum one after the other, and a lightpath that crosses both is one victim.
 * sets uint64 [R][F][2], 1 <= F <= 65 535; R = batch with per_replica != 0, otherwise R = 1: one list shared by all replicas.
 * Bit e & 63 of word e >> 6 fails link e (the bit order of the library's path masks).  Every (replica, column) is ONE
 * independent scenario on the replica's current state; duplicates are allowed; the empty set and a set with a bit at an
 * index >= E are skipped (status 1).
 * Scenario: that of ongym_failure_impact with "contains e" read as "contains a failed link".  The victims are the running
 * records whose route contains ANY failed link, each counted once, in ascending record index; all leave at once; restoration
 * goes one victim after the other in record order over the routes k = 0..K-1 of the victim's node pair that contain NO
 * failed link, formats from M-1 down, the lowest start only, the same capacity rule n' = ceil(n se[m] / se[m']), the same ASE
 * bound, GN model (over what runs in the scenario at that moment, quirk Q12 under id tracking) and admission test; a
 * restoration is provisioned and appended as the step does it.
 * set_out float64 [batch][F][12]:
 *   0-9  the columns of ongym_failure_impact's link_out, same names and meaning (5 lost_no_spectrum still includes "no eligible
 *        route")
 *   10 lost_no_route       the part of column 5 whose node pair has no route left at all (every route of the pair, or the pair
 *                          itself, is gone): where the lightpaths that end at a failed node are counted
 *   11 failed_links        number of links in the set
 *   Status 1: columns 1-11 are NaN.  Column 1 = columns 3 + 5 + 6, column 10 <= column 5.
 * svc_out     NULL, or int32 [batch][F][C], encoded as ongym_failure_impact's (4 F C bytes per replica: for small batches or
 *             short lists).
 * Refused (ONGYM_E_ARG): F out of range, NULL sets, NULL set_out, n_mods_consider < n_mods, pair lists that disagree on a
 * route's node pair; ONGYM_E_LIMIT: the LDS block exceeds the limit (as ongym_failure_impact).
 * Read-only: no replica state, statistic, counter (total_gn_evals included), disrupted flag, move log or random-number
 * position changes.  Buffers: host buffers (staged through a device buffer grown on demand; the call synchronises), or device
 * buffers with cfg.io_device (then the call only launches on the environment's stream and nothing synchronises; sets must be
 * 8-byte aligned).  ongym_last_kernel_ms times the kernel. */
enum { ONGYM_N_FAILURE_SETS = 12, ONGYM_MAX_FAILURE_SETS = 65535 };   /* set_out entries per row; F at most */
int ongym_failure_sets(ongym_env *env, int32_t n_sets, const uint64_t *sets, int32_t per_replica, double *set_out,
                       int32_t *svc_out);

/* Link failures on LIVE replicas: cut a set of links per replica, let traffic continue on the degraded network, return the
 * fibre later (E = n_links, S = n_slots, C = capacity).  ongym_failure_impact and ongym_failure_sets answer "what if" on a
 * private copy; these three calls change the replica's own state.
 * A failed link is a full row that no record crosses.  Nothing new is stored: link e is FAILED exactly when row e of the
 *   bitmap has no free slot in [0, S) and no running record's route contains e.  (A healthy full link has records on it, a
 *   healthy link without records is entirely free: the bitmap is the union of the records' provisioned ranges.)  Every step
 *   kernel, policy, observation and mask therefore sees the link as full and places nothing on it, and no release touches
 *   the row, because releases walk a record's own route.
 * Cut (per replica, one set): 1. every running record whose route contains a failed link (a victim) leaves, all at once;
 *   2. the victims are restored one after the other in record order by first fit over the routes that contain no failed
 *   link, exactly as in ongym_failure_sets' scenario; 3. bits [0, S) of every failed row are cleared; 4. the state is stored.
 *   Survivors keep their order, release time, id and Service.OSNR and are compacted; a restored victim is appended in victim
 *   order with its own release time, id and disrupted flag; under id tracking its Service.OSNR becomes the restoration's GSNR
 *   and episode_osnr_sum moves by new - old (what defragmentation does to a moved service).  A lost victim leaves as a
 *   departure leaves: nothing is subtracted.  No statistic other than `active` (and, with ids, episode_osnr_sum) changes,
 *   total_* included; the pending request, the clock, the stream position and the move log stay.
 *   With ONGYM_CUT_NO_RESTORE step 2 is skipped and every victim is dropped.
 *   Cutting an already failed link finds no victim and changes nothing.  A replica whose set is empty or has a bit at an
 *   index >= E is left byte for byte as it was (status 1).
 * Consequences: state save, load and fork carry failures with the bitmap.  ongym_link_metrics reports a failed link as fully
 *   used.  The read-only analyses (action impact, failure impact and sets, admission map, playout) treat a failed link as a
 *   full one: a route through it is "a route without spectrum", not "no route".  ongym_reset and the in-launch auto reset
 *   rebuild the spectrum as the reference's reset does and so RETURN EVERY FIBRE: a caller who wants a failure to outlast an
 *   episode cuts again after `terminated`.  An observation or mask taken before a cut is stale after it.
 * sets      uint64 [batch][2] with per_replica != 0, otherwise [2] shared by all replicas; bit order of ongym_failure_sets.
 * cut_out   float64 [batch][13]: columns 0-11 are ongym_failure_sets' set_out columns, same names, meaning and status rule;
 *             12 dropped   victims whose restoration was not attempted: 0 without the flag; with it the victims, and
 *                          columns 3-8 and 10 are 0
 *           Column 1 = columns 3 + 5 + 6 + 12.  Status 1: columns 1-12 are NaN.
 * svc_out   NULL, or int32 [batch][C] in PRE-cut record order, encoded as ongym_failure_sets' svc_out; a dropped victim gets
 *           the reject action.
 * index_out NULL, or int32 [batch][C]: the POST-cut record index of every pre-cut record (survivors compacted in order, the
 *           restored appended in victim order); -1 for a lost or dropped record and at and beyond the running count.
 * Refused (ONGYM_E_ARG): NULL sets, NULL cut_out, unknown flags, n_mods_consider < n_mods, pair lists that disagree on a
 * route's node pair; ONGYM_E_LIMIT: the LDS block (the state block + 14 C bytes, 26 C with id tracking) exceeds 160 KiB.
 * Buffers: host buffers (staged; the call synchronises), or device buffers with cfg.io_device (the call only launches on the
 * environment's stream and nothing synchronises; sets must be 8-byte aligned).  ongym_last_kernel_ms times the kernel. */
enum { ONGYM_N_CUT_LINKS = 13 };   /* cut_out entries per replica */
enum { ONGYM_CUT_NO_RESTORE = 1 };
int ongym_cut_links(ongym_env *env, const uint64_t *sets, int32_t per_replica, int32_t flags,
                    double *cut_out, int32_t *svc_out, int32_t *index_out);

/* Returns fibre: of the links in the replica's set, those that are failed by the rule above get bits [0, S) of their rows set
 * again; the others (healthy links, indices >= E) are ignored.  Only the changed rows are written; records, statistics and the
 * request state stay.  sets as ongym_cut_links'.  repaired_out: NULL, or int32 [batch], the links returned.  Refused
 * (ONGYM_E_ARG): NULL sets.  Buffers and timing as ongym_cut_links'. */
int ongym_repair_links(ongym_env *env, const uint64_t *sets, int32_t per_replica, int32_t *repaired_out);

/* The failed links of every replica by the rule above: failed_out uint64 [batch][2], bit e & 63 of word e >> 6 for link e.
 * Read-only.  Refused (ONGYM_E_ARG): NULL failed_out.  Buffers and timing as ongym_cut_links'. */
int ongym_failed_links(ongym_env *env, uint64_t *failed_out);

/* The spectrum map of every replica: who holds every slot, the running records of all replicas, and an audit of the rule that
 * every call which changes a replica keeps: the used cells of the bitmap are exactly the disjoint union of the running records'
 * provisioned ranges (E = n_links in table order, S = n_slots, C = capacity, P = n_paths, M = n_mods).
 * Records   A = the replica's `active` clamped to [0, C].  Record i < A, in ongym_query_services' order, is decoded from the
 *           stored words.  It is well-formed iff 0 <= path < P, n >= 1, slot + n <= S, format < M and, under the 32-bit-mask
 *           record codec (E <= 32, P <= 512), its mask word is the low word of its route's link mask.
 * Claims    a well-formed record claims, on every link of its route, its signal cells [slot, slot + n) and the guard cell
 *           slot + n if slot + n < S.  A malformed record claims nothing.
 * Failed    a link whose row has no free slot in [0, S) and that no well-formed record's route contains (ongym_failed_links).
 * Width     the widest record ongym_move_services may write on this environment (its "Width" above).
 * owner_out   int16 [batch][E][S], 2 E S bytes per replica (NSFNET, S = 320, batch 65 536: 0.9 GB): v >= 0 a signal cell of
 *             record v; -1 free in the bitmap and unclaimed; -32767 <= v <= -2 the guard cell of record -2 - v; -32768 used in
 *             the bitmap and unclaimed (a failed link's cells, or an orphan).  A cell with several claimants shows the claim of
 *             the lowest record index; a claimed cell shows its claim whatever the bitmap says.  Needs C <= 32766
 *             (ONGYM_E_LIMIT otherwise; the other three outputs take any capacity).
 * rec_out     int32 [batch][C][6]: path_id, slot, nslots, modulation, service_id (-1 unless ids are kept), flags (bit 0: in
 *             the disrupted list, the sign of the stored release time; bit 1: malformed).  Rows at and beyond A: all -1.
 * release_out float32 [batch][C]: the release time without its sign; NaN at and beyond A.  For well-formed records rec_out and
 *             release_out equal ongym_query_services field for field.
 * audit_out   int32 [batch][10]:
 *             0 violations          bit 0: `active` outside [0, C]; bits 1-5: columns 2, 3, 4, 5, 6 non-zero
 *             1 records             A
 *             2 malformed           records that are not well-formed
 *             3 overlap_cells       cells with two or more claimants
 *             4 claimed_free_cells  cells with a claimant whose bitmap bit says free
 *             5 orphan_cells        used, unclaimed cells on links that are not failed
 *             6 over_width          well-formed records with n above the width limit
 *             7 failed_links        their count (information)
 *             8 claimed_cells       cells with at least one claimant (information)
 *             9 used_cells          used bits in [0, S) over all links (information)
 *             With violations = 0, column 9 = column 8 + S x column 7.
 * Not audited, deliberately: release times, service ids (quirk Q12 allows duplicates), statistics and the pending request.
 * Defined on any state ongym_state_load accepts: no record field and no `active` is used as an index before its range check.
 * Any pointer may be NULL, not all four (ONGYM_E_ARG).  Read-only: no replica state, statistic, counter, disrupted flag, move
 * log or stream position changes.  ONGYM_E_LIMIT: the LDS block (24 bytes per row word; with owner_out 4 S + 8 C more)
 * exceeds 160 KiB.  Buffers: host buffers (staged through a device buffer grown on demand; the call synchronises once), or
 * device buffers with cfg.io_device (then the call only launches on the environment's stream and nothing synchronises).
 * ongym_last_kernel_ms times the kernel. */
enum { ONGYM_N_SPECTRUM_AUDIT_COLUMNS = 10, ONGYM_N_SPECTRUM_RECORD_COLUMNS = 6 };   /* entries per row of audit_out, rec_out */
enum { ONGYM_SPECTRUM_DISRUPTED = 1, ONGYM_SPECTRUM_MALFORMED = 2 };                  /* the bits of rec_out's flags column */
/* owner_out: free and unclaimed; the guard cell of record i reads ONGYM_OWNER_GUARD_BASE - i; used and unclaimed; C at most */
enum { ONGYM_OWNER_FREE = -1, ONGYM_OWNER_GUARD_BASE = -2, ONGYM_OWNER_UNOWNED = -32768, ONGYM_MAX_OWNER_CAPACITY = 32766 };
int ongym_spectrum_map(ongym_env *env, int16_t *owner_out, int32_t *rec_out, float *release_out, int32_t *audit_out);

/* Moves running lightpaths on LIVE replicas: a chosen record is placed again, at a chosen action or where first fit puts it
 * (K = k_paths, M = n_mods, S = n_slots, C = capacity, N = n_moves).  A move is a restoration of ongym_cut_links with one victim
 * and no failed link, written back to the victim's own record index.
 * moves     int32 [batch][N][2] = (record, target).  A replica applies its moves in order; each sees the state the previous left.
 *   record  an index in [0, active), or ONGYM_MOVE_TOP: the running record that no move of this call has attempted yet
 *           (explicit ones included, whatever their outcome) and whose last slot, slot + n - 1, is highest; ties go to the
 *           lowest index.  Indices are stable: a moved record keeps its index, its release time with its sign (the disrupted
 *           flag) and its id, and no other record changes place, so an index read from the records before the call holds
 *           during and after it.
 *   target  a step action k M S + (M - 1 - m) S + start on the route list of the record's own node pair (the route's pair as
 *           the restorations find it), or ONGYM_MOVE_FIRST_FIT.  The service keeps its capacity n mod_se[m]; under format m' it
 *           takes ceil(n mod_se[m] / mod_se[m']) slots, the restorations' rule.
 *   Width   a move writes no record wider than the lean step kernels of the environment can carry, because traffic goes on
 *           after it: where a lean kernel may run (an eligible configuration whose traffic so far fits the lean tables), the
 *           limit is the widest slot count of the traffic table (the rows of the pair table), 32 in the narrow build;
 *           otherwise it is S.  A format under which the service would take more slots is "no spectrum" (status 3) for an
 *           explicit target and is passed over by ONGYM_MOVE_FIRST_FIT.
 * One move: 1. the record's own range counts as free (n + 1 slots, clamped at S) and the record is no interferer, nor, with id
 *   tracking, are its namesakes; 2. an explicit target must be one of `_get_candidates`' starts for the new slot count on the
 *   target route in that state (n' free slots and the guard slot unless the range ends at S), so a failed link is never chosen
 *   and a target that overlaps the old range is fine; 3. the target must pass the step's admission test with the replica's margin
 *   (the exact ASE lower bound where first fit uses it, then the GN model); 4. ONGYM_MOVE_FIRST_FIT is first fit's search - routes
 *   in order, formats best first, the lowest start - over the pair's routes, with ONGYM_MOVE_OWN_ROUTE over the record's own
 *   route only; 5. a result equal to the present placement changes nothing; 6. on success the old range is released, the new one
 *   provisioned with its guard slot, the record words rewritten in place, and under id tracking Service.OSNR becomes the new
 *   GSNR and episode_osnr_sum moves by new - old; 7. on any failure the replica is exactly as before that move.
 *   No statistic other than episode_osnr_sum (with ids) changes, total_* included; the pending request, the clock, the stream
 *   position and the move log stay.  A replica none of whose moves succeeds is left byte for byte as it was.
 * move_out  float64 [batch][N][6]:
 *             0 status           0 moved; 1 invalid: record out of [0, active), no record left for ONGYM_MOVE_TOP, action out of
 *                                [0, K M S), or the pair has no route k; 2 unchanged: the target is the present placement;
 *                                3 no spectrum: n' above the width limit, the start is no candidate start, or first fit found no
 *                                start anywhere;
 *                                4 refused on QoT
 *             1 record           the resolved index, -1 if none
 *             2 old_action       the present placement in the encoding above, with the record's k on its pair's list (-1 with
 *                                column 1)
 *             3 new_action       the placement after the move: column 2 unless moved
 *             4 margin           GSNR - threshold - margin of the new placement in dB, NaN unless moved
 *             5 slot_hops_delta  n' hops' - n hops, 0 unless moved
 * Refused (ONGYM_E_ARG): NULL moves, NULL move_out, n_moves < 1, unknown flags, n_mods_consider < n_mods, pair lists that
 * disagree on a route's node pair; ONGYM_E_LIMIT: the LDS block (the state block + C / 8 bytes) exceeds 160 KiB.
 * Buffers: host buffers (staged; the call synchronises), or device buffers with cfg.io_device (the call only launches on the
 * environment's stream and nothing synchronises).  ongym_last_kernel_ms times the kernel. */
enum { ONGYM_N_MOVE_COLUMNS = 6 };   /* move_out entries per row */
enum { ONGYM_MOVE_TOP = -1 };        /* record selector */
enum { ONGYM_MOVE_FIRST_FIT = -1 };  /* target selector */
enum { ONGYM_MOVE_OWN_ROUTE = 1 };   /* flag */
int ongym_move_services(ongym_env *env, int32_t n_moves, const int32_t *moves, int32_t flags, double *move_out);

/* What the network could still carry right now: per replica and per candidate action of a list, first fit's admission decision
 * for EVERY request the traffic model can draw - every unordered node pair and every bit rate of a list - on the replica's
 * current state (N = n_nodes, K = k_paths, M = n_mods, S = n_slots, C = capacity, Q = N (N - 1) / 2, A = n_actions, R = n_rates).
 * Cells      node pairs are the unordered pairs s < d in lexicographic order, q = 0..Q-1; the routes of pair q are
 *            pair_paths[(s N + d) K + k].  Both directions of a pair must list the same routes (checked at create: the create
 *            succeeds, this call refuses with ONGYM_E_ARG and names the pair).  rates float [R], 1 <= R <= 16, Gb/s, shared by
 *            all replicas, ALWAYS a host array (it travels with the launch, also with cfg.io_device); NULL with
 *            n_rates == n_bit_rates: the configuration's discrete bit rates (refused in continuous mode or with another
 *            n_rates).  Rate r needs (int)ceil((double)r / (mod_se[m] * nslots_width)) slots under format m, the step's own
 *            expression (for the configured rates: nreq_tab); a format with n < 1 or n > S is unusable.
 * Scenarios  actions int32 [batch][A], 1 <= A <= 256; NULL (only with A = 1): the state as it is.  Every (replica, a) is ONE
 *            independent scenario on the replica's current state; the action is decoded for the replica's current request as
 *            ongym_action_impact decodes it.  Status:
 *   0  the action decodes and its slots are free: the candidate is provisioned as the step provisions ([a, a + n) plus the
 *      guard slot unless it ends at S) and appended as a running record at `active` (with id tracking: with the current
 *      request's id); then the map is taken.  As in ongym_action_impact the candidate's own QoT is not evaluated.
 *   1  NULL, an index < 0, the reject action or beyond it, or no current request: nothing is applied, the row is the map of the
 *      state as it is (one call yields the baseline and the candidates)
 *   2  spectrum not free, or no such route / format / slot count (ongym_action_impact's status 2): summary columns 1-7 NaN, map
 *      entries -1, margins NaN
 *   3  the running count is already C: as status 2 (a candidate that is also not free has status 2)
 * A cell (q, r) of a scenario is first fit's decision (heuristics.py:923-966) for a request of rate r between the pair: routes
 * k = 0..K-1 (stop at -1), formats M-1 down to 0, only the lowest start of _get_candidates(row, n, S), the step's GN model over
 * everything running in the scenario at the replica's launch power, the step's admission test against minimum_osnr[m] + the
 * replica's margin, the exact ASE lower bound where first fit uses it.  A probe has no service id: nobody is left out of its
 * interferers (quirk Q12 concerns requests that carry an id).  No probe is provisioned: cells do not see each other.  Outcome:
 * admitted with (k, m, a); blocked for spectrum (no (route, format) had a valid start); blocked on QoT (at least one start was
 * evaluated, by bound or GN sum, and refused: the rule of lost_qot in ongym_failure_impact).
 * summary_out float64 [batch][A][8]:
 *   0 status
 *   1 admitted              cells
 *   2 blocked_no_spectrum   cells
 *   3 blocked_qot           cells                                  (columns 1 + 2 + 3 = Q R)
 *   4 blocking_probability  sum of w[q][r] over the blocked cells
 *   5 bit_rate_blocking     sum of w rate over the blocked cells / sum of w rate over all cells
 *   6 lowest_margin         min over the admitted cells of GSNR - minimum_osnr[m] - margin (dB); NaN if none is admitted
 *   7 detoured              admitted cells with k > 0
 * weights     float64 [Q][R], or NULL: uniform 1 / (Q R).  The sums run in a fixed order, pair-major, without floating-point
 *             atomics: the same state and inputs give the same bytes on every call.
 * map_out     NULL, or int32 [batch][A][Q][R] (LARGE: 4 A Q R bytes per replica, 3.9 GB for 65 536 replicas of NSFNET with four
 *             rates and A = 41; ask for it on small batches or short action lists): k M S + (M-1-m) S + a of an admitted cell,
 *             K M S blocked for spectrum, K M S + 1 blocked on QoT.
 * margin_out  NULL, or float32 [batch][A][Q][R]: the admitted cell's margin (column 6's quantity), NaN otherwise.
 * Refused (ONGYM_E_ARG): A or R out of range, NULL actions with A != 1, NULL summary_out, a non-finite or non-positive rate,
 * n_mods_consider < n_mods (no format window, as ongym_observe_blocks), asymmetric pair lists.
 * Read-only: no replica state, statistic, counter (total_gn_evals included), disrupted flag, move log or random-number
 * position changes.  Buffers (all but rates): host buffers (staged through a device buffer grown on demand; the call
 * synchronises), or device buffers with cfg.io_device (then the call only launches on the environment's stream and nothing
 * synchronises).  ongym_last_kernel_ms times the kernel(s).
 * Launch geometry: small batches split a scenario's pairs over several wavefronts and add their partial sums in a fixed order
 * (a buffer for them is allocated at create; the call itself never allocates).  ONGYM_ADMISSION_GROUPS=<g> in the environment at
 * create forces g wavefronts per scenario: a measurement and test knob, not for production (the split changes the order of the
 * sums of columns 4 and 5, i.e. their last bits, and nothing else). */
/* summary_out entries per row; A and R at most */
enum { ONGYM_N_ADMISSION_MAP = 8, ONGYM_MAX_ADMISSION_ACTIONS = 256, ONGYM_MAX_ADMISSION_RATES = 16 };
int ongym_admission_map(ongym_env *env, int32_t n_actions, const int32_t *actions, int32_t n_rates, const float *rates,
                        const double *weights, double *summary_out, int32_t *map_out, float *margin_out);

/* Playouts: per replica, per candidate action of a list and per sample, the candidate applied to the pending request and then
 * `horizon` requests decided by a policy, on a private copy of the replica - the leaf evaluation of a tree search, the rollout
 * algorithm of policy improvement, an n-step baseline (A = n_actions, H = horizon, R = n_samples, C = capacity).
 * Every (replica b, action a, sample r) is ONE independent scenario on the replica's current state.  By definition it is what
 * these calls would do to a copy of the replica:
 *   1. the stream is replaced as ongym_seed_base with seed + r and the environment's replica_base replaces it: the key becomes
 *      the stream key of (seed + r, replica_base + b) (include/ongym_traffic.h), the request counter 0.  The pending request, the
 *      clock and everything else stay.  With ONGYM_PLAYOUT_OWN_STREAM in `flags` the replica's own source continues from its
 *      own position instead - its device generator or its trace, i.e. the true future; R must then be 1, `seed` is ignored.
 *   2. the candidate is applied as ongym_step_actions applies actions[b][a] (same decoding, same GN evaluation, same
 *      bookkeeping).  An index < 0, or actions == NULL (only with A = 1): `policy` decides the pending request as well.
 *   3. H iterations of ongym_step_policy with `policy` follow.
 * The A candidates of a replica see the same future for the same r (common random numbers).  The scenario ends early after a
 * step whose record would have terminated = 1, with or without cfg.auto_reset - a playout never crosses an episode boundary -
 * and when the source has no further request (trace exhausted).
 * playout_out float64 [batch][A][R][8]:
 *   0 status              0 the action was applied (accepted, or the reject action: a real choice, the future proceeds)
 *                         1 the policy decided the pending request
 *                         2 the step would answer "retry" (slots not free, no such route or format)
 *                         3 the step would flag a QoT error
 *                         4 the replica has no pending request
 *                         status >= 2: columns 1-7 are NaN, nothing is played
 *   1 first_accepted      `accepted` of the first step's record (0 for a reject, capacity overflow included)
 *   2 steps               policy iterations that ran after the first step (<= H)
 *   3 accepted            iterations among them whose record has accepted = 1
 *   4 blocked             the others (columns 3 + 4 = column 2)
 *   5 bit_rate_accepted   sum of the accepted requests' bit rates over those iterations, Gb/s, added in step order
 *   6 bit_rate_requested  sum over the requests those iterations decided (the request the last iteration drew is not decided
 *                         and does not count)
 *   7 active_end          `active` of the last record that ran
 * Refused with ONGYM_E_ARG: A outside 1..256, R outside 1..64, H outside 1..4096, A R > 4096, NULL actions with A != 1, NULL
 * playout_out, unknown flags, ONGYM_PLAYOUT_OWN_STREAM with R != 1, n_mods_consider < n_mods.  With ONGYM_E_LIMIT: a policy
 * other than first fit (0) or load balancing (1) (the kernel is instantiated for these two), cfg.defragmentation or
 * cfg.track_service_ids (their step writes the move log and statistics in memory).  With ONGYM_E_STATE: no request source; a
 * trace source without ONGYM_PLAYOUT_OWN_STREAM.
 * Read-only: no replica state, statistic, work counter, random-number position or disrupted flag changes.  Buffers: host
 * buffers (staged through a device buffer grown on demand; the call synchronises), or device buffers with cfg.io_device (then
 * the call only launches on the environment's stream and nothing synchronises).  ongym_last_kernel_ms times the kernel. */
/* playout_out entries per row; A, R, A R and H at most */
enum { ONGYM_N_PLAYOUT = 8, ONGYM_MAX_PLAYOUT_ACTIONS = 256, ONGYM_MAX_PLAYOUT_SAMPLES = 64, ONGYM_MAX_PLAYOUT_SCENARIOS = 4096,
       ONGYM_MAX_PLAYOUT_HORIZON = 4096 };
enum { ONGYM_PLAYOUT_OWN_STREAM = 1 };
int ongym_playout(ongym_env *env, int32_t n_actions, const int32_t *actions, int32_t horizon, int32_t policy,
                  int32_t n_samples, uint64_t seed, int32_t flags, double *playout_out);

/* One uniformly random VALID action per replica from an action mask [batch][k_paths*Mc*n_slots + 1] (as ongym_observe
 * writes it): what gymnasium's `action_space.sample(mask=info["mask"])` does on the reference's Discrete action space
 * (qrmsa.pyx:319-321; wrappers/qrmsa_gym.py:74-75 hands the mask out) - the masked random policy that exercises the
 * observation path.  Deterministic in (seed, draw_index, global replica index); the stream is this library's counter-based
 * generator (include/ongym_traffic.h), not NumPy's.  The reject action is always valid, so a choice always exists.
 * mask / actions: host buffers, or device buffers with cfg.io_device (then nothing synchronises). */
int ongym_sample_actions(ongym_env *env, const uint8_t *mask, uint64_t seed, uint64_t draw_index, int32_t *actions);

/* Masked categorical action head: the action distribution of the reference's masked PPO training
 * (examples/ONDM_2025/train_multi_masked_ppo.py: sb3-contrib MaskablePPO, whose MaskableCategorical is a Categorical over
 * logits with the masked entries filled with -1e8) over the env's action mask, evaluated on device in ONE pass per row.
 * Semantics are the exact masked distribution (what the -1e8 fill approximates): masked entries do not exist, whatever their
 * logit holds (NaN and +-inf included); p = softmax over the valid entries, entropy = -sum_valid p log p.
 *   logits  [batch][n_actions] of type `dtype` (ONGYM_DTYPE_*), 16-byte aligned base; n_actions = k_paths*Mc*n_slots + 1
 *   mask    uint8 [batch][n_actions] as the observation call writes it (nonzero = valid), 8-byte aligned base
 *   mode    ONGYM_HEAD_SAMPLE: draw from the masked softmax (MaskableCategorical.sample): Gumbel-max, per-entry uniforms of the
 *             counter-based generator of ongym_traffic.h, one stream per (seed, global replica = replica_base + r,
 *             draw_index) countered by entry, in a domain of its own (not the uniform sampler's stream);
 *           ONGYM_HEAD_ARGMAX: the first valid entry with the largest logit (MaskableCategorical.mode(), deterministic=True);
 *           ONGYM_HEAD_EVALUATE: log-prob and entropy of the GIVEN actions (MaskablePPO's evaluate_actions); actions are read.
 * Outputs per row: actions (written in the first two modes), log_prob, entropy, row_stats float [batch][2] (the largest
 * valid logit m and log sum_valid e^(x-m), kept for the backward call; log_prob = (x_a - m) - log sum, so it does not depend
 * on a common offset of the row), mask_bits uint32 [batch][ceil(n_actions/32)] (bit j of row r = mask[r][j] != 0, padding
 * bits 0); every output but actions may be NULL.  Rows where only the reject entry is valid give (reject, 0, 0); rows with no
 * valid entry (a caller error) give the reject action and NaN log_prob / entropy / row_stats; in evaluate mode an action
 * outside the mask gets log_prob = -inf.
 * Non-finite logits in VALID entries: -inf means probability 0 (as torch's Categorical): every output is bit for bit the one
 * of the same call with that entry masked (its evaluate log_prob is -inf, its gradient 0); a row whose valid entries are all
 * -inf is a row with no valid entry.  NaN or +inf poisons its row: log_prob and entropy are NaN (in every mode), the sampled
 * or argmax action is still an entry of the mask, and other rows are not affected.
 * Device pointers only: both calls fail with ONGYM_E_ARG unless cfg.io_device = 1.  Launched on the env's current stream
 * (ongym_set_stream), nothing synchronises. */
enum { ONGYM_DTYPE_F32 = 0, ONGYM_DTYPE_BF16 = 1 };
enum { ONGYM_HEAD_SAMPLE = 0, ONGYM_HEAD_ARGMAX = 1, ONGYM_HEAD_EVALUATE = 2 };
int ongym_masked_categorical(ongym_env *env, const void *logits, int32_t dtype, const uint8_t *mask, int32_t mode,
                             uint64_t seed, uint64_t draw_index, int32_t *actions, float *log_prob, float *entropy,
                             float *row_stats, uint32_t *mask_bits);
/* Gradient of  sum_r g_lp[r] log_prob[r] + g_H[r] entropy[r]  with respect to the logits of the forward call above, from the
 * saved mask bits, actions, row_stats and entropy (not the caller's mask, which the next observation overwrites):
 * grad_logits[r][j] = valid ? g_lp (delta_{j,a} - p_j) - g_H p_j (log p_j + H) : 0, written in the logits' dtype (a valid
 * entry with a logit of -inf counts as masked: 0; p log p = 0 where p = 0).  g_lp / g_H (float [batch]) may be NULL (zero).  Same pointer, alignment and stream rules. */
int ongym_masked_categorical_backward(ongym_env *env, const void *logits, int32_t dtype, const uint32_t *mask_bits,
                                      const int32_t *actions, const float *row_stats, const float *entropy,
                                      const float *grad_log_prob, const float *grad_entropy, void *grad_logits);

/* The head on ANY number of rows (a PPO minibatch gathered from a rollout), with the mask given as bytes or packed bits.
 * Semantics are those of the pair above with `rows` (>= 0; 0 launches nothing) in place of cfg.batch: logits, mask, outputs
 * and grad_logits have `rows` rows, and in sample mode row r draws from the stream of global replica replica_base + r.  For
 * rows == cfg.batch and ONGYM_MASK_BYTES the outputs are bit for bit those of ongym_masked_categorical.
 *   mask_format  ONGYM_MASK_BYTES: mask is uint8 [rows][n_actions], 8-byte aligned (as above);
 *                ONGYM_MASK_BITS:  mask is uint32 [rows][ceil(n_actions/32)], 4-byte aligned, in the layout the forward writes
 *                to mask_bits (bit j of row r = entry j; padding bits are ignored); mask_bits out must then be NULL.
 * A rollout keeps the 8x smaller bits of every step (mask_bits out of the sampling call) and evaluates minibatches from them. */
enum { ONGYM_MASK_BYTES = 0, ONGYM_MASK_BITS = 1 };
int ongym_masked_categorical_rows(ongym_env *env, int32_t rows, const void *logits, int32_t dtype,
                                  const void *mask, int32_t mask_format, int32_t mode, uint64_t seed,
                                  uint64_t draw_index, int32_t *actions, float *log_prob, float *entropy,
                                  float *row_stats, uint32_t *mask_bits);
int ongym_masked_categorical_backward_rows(ongym_env *env, int32_t rows, const void *logits, int32_t dtype,
                                           const uint32_t *mask_bits, const int32_t *actions, const float *row_stats,
                                           const float *entropy, const float *grad_log_prob,
                                           const float *grad_entropy, void *grad_logits);

/* Generalised advantage estimation over a rollout (SB3's RolloutBuffer.compute_returns_and_advantage, as MaskablePPO runs it),
 * the episode ends taken from the step records:
 *   recs         ongym_step_rec [steps][batch]: `steps` calls of ongym_step_actions writing consecutive slices, 8-byte aligned
 *   values       float [steps][batch]: the value estimate of each step's observation
 *   last_values  float [batch]: the value of the observation after the last step
 * For t = steps-1 .. 0 (A = 0 before the first iteration):
 *   nnt   = 1 - recs[t][b].terminated
 *   vnext = t == steps-1 ? last_values[b] : values[t+1][b]
 *   delta = (float)recs[t][b].reward + gamma * vnext * nnt - values[t][b]
 *   A     = delta + gamma * gae_lambda * nnt * A;   advantages[t][b] = A;  returns[t][b] = A + values[t][b]
 * f32 arithmetic, in any summation order; NaN / inf as the sequential recurrence (0 * NaN = NaN: a NaN crosses a termination).
 * Device buffers only (cfg.io_device = 1), f32 buffers 4-byte aligned; outputs must not overlap each other or an input.
 * ONGYM_E_ARG also for steps < 1 and gamma or gae_lambda outside [0, 1].  On the env's stream, nothing synchronises. */
int ongym_gae(ongym_env *env, int32_t steps, const ongym_step_rec *recs, const float *values,
              const float *last_values, float gamma, float gae_lambda, float *advantages, float *returns);

/* Plugin-API queries on one replica (host buffers always, staged with cfg.io_device too; each synchronises once): */
/* QRMSAEnv.get_available_slots(path) (qrmsa.pyx:1482-1512): out[n_slots], 1 = free on every link of the path */
int ongym_query_available(ongym_env *env, int32_t replica, int32_t path_id, int32_t *out);
/* calculate_osnr(env, service) (core/osnr.pyx:21-142) for a candidate (path, slot, nslots): out = gsnr, ase, nli dB
 * (ongym_query_gsnr_many with one candidate) */
int ongym_query_gsnr(ongym_env *env, int32_t replica, int32_t path_id, int32_t slot, int32_t nslots, double out[3]);
/* The same for `count` candidates of one replica in ONE launch (one wavefront per candidate) — what a plugin heuristic
 * that scores every feasible start needs (heuristics.py:272-328, 330-416, 647-749): cands int32 [count][3] =
 * {path_id, slot, nslots}; out double [count][3] = {gsnr, ase, nli} dB.  Host buffers. */
int ongym_query_gsnr_many(ongym_env *env, int32_t replica, int32_t count, const int32_t *cands, double *out);
/* QRMSAEnv._get_candidates(available_slots, n, total_slots) (qrmsa.pyx:515-541) on an ARBITRARY row (1 = free):
 * starts_out[total_slots] receives the feasible start slots in ascending order, *count their number.
 * total_slots <= 1023. State-independent (no replica argument). */
int ongym_query_candidates(ongym_env *env, const int32_t *row, int32_t total_slots, int32_t nslots,
                           int32_t *starts_out, int32_t *count);
/* QRMSAEnv.is_path_free(path, initial_slot, number_slots) (qrmsa.pyx:1248-1264): *out = 1 if free */
int ongym_query_path_free(ongym_env *env, int32_t replica, int32_t path_id, int32_t slot, int32_t nslots,
                          int32_t *out);
/* The reallocations defragment() made while the last step of `replica` processed its departures, in order:
 * out[min(*count, ONGYM_MOVE_LOG)]; *count is the total (entries beyond ONGYM_MOVE_LOG are not kept). */
int ongym_query_moves(ongym_env *env, int32_t replica, ongym_move *out, int32_t *count);
/* topology.graph["available_slots"] (qrmsa.pyx:306-309): out[n_links*n_slots] */
int ongym_query_grid(ongym_env *env, int32_t replica, int32_t *out);
/* topology.graph["running_services"]: out[capacity], *n = count */
int ongym_query_services(ongym_env *env, int32_t replica, ongym_service *out, int32_t *n);
/* QRMSAEnv.current_service */
int ongym_query_request(ongym_env *env, int32_t replica, ongym_request *out);

/* per-replica counters: out[batch] (host buffer) */
int ongym_stats_get(ongym_env *env, ongym_stats *out);

/* Save, restore and fork replica states.  A replica's state is everything that decides its future:
 *   its slot bitmap; its service records (with ids, OSNR and the last step's move log where cfg.defragmentation or
 *   cfg.track_service_ids keeps them); the clock and the pending request (cur_*, have_request); the request counter and the
 *   stream key; the per-replica parameters (launch power, margin, mean inter-arrival time); the running-OSNR accumulators;
 *   and every ongym_stats field (max_modulation_idx, which the action codec is relative to, and the terminal-step snapshot
 *   included) EXCEPT the work counters total_steps .. total_active_sum: they count work done in THIS environment, so they
 *   stay with the destination replica and keep counting.
 * Flags of a load or fork:
 *   ONGYM_STATE_KEEP_STREAM  the destination keeps its own stream key.  The pending request, the clock and the request counter
 *                            still come from the source (release times are absolute), so the requests after the pending one
 *                            are drawn from the destination's stream at the source's counter: independent futures of one state.
 *   ONGYM_STATE_KEEP_PARAMS  the destination keeps its launch power, margin and load (mean inter-arrival time): one loaded
 *                            network forked into a power or load sweep.
 * Trace sources (ongym_set_requests): the cursor travels, the rows do not; each replica goes on reading its own row.
 * Request source of the destination: ongym_seed and ongym_set_requests rewind every replica's counter, so they come BEFORE a
 * load.  A destination without a source takes the device generator when the load covers all its replicas and the blob comes
 * from a device-generator environment (the keys and counters travel); any other load into it fails with ONGYM_E_STATE.
 * A blob saved by an environment that replayed a trace the lean kernels cannot run (bit rates outside the configured table,
 * or a device trace) carries that fact: the destination then runs the generic kernels from the load on, as the source did.
 * Python-side counters (such as the draw counter of the action head's helper) are not device state.
 *
 * The blob (out / in): a device pointer when cfg.io_device = 1 (16-byte aligned, e.g. a torch uint8 tensor), a host pointer
 * otherwise; ongym_state_size bytes: a 256-byte header (magic, format version, configuration fingerprint, layout facts: record
 * codec, id tracking, row words, links, capacity, sizeof of the per-replica block, section sizes and offsets, count), then
 * `count` replica blocks, each section 16-byte aligned.  A blob loads into any environment whose ongym_config agrees on every
 * field but batch, device, io_device, launch_power_w, margin, load and the replica_* arrays (the tables are compared by
 * content); anything else is refused with ONGYM_E_ARG and an ongym_last_error text.
 * replicas: host int32 [count] (NULL = all `batch` replicas in order, count must then equal batch), entries in [0, batch); a
 * load list must not repeat an entry.  count lies in [1, batch].  Everything is checked before any launch.
 * Streams: save and load run on the env's stream.  Load reads the header on the host first: for a device blob that is one
 * small device-to-host copy, which waits for the stream.  Calls with host blobs synchronise. */
enum { ONGYM_STATE_KEEP_STREAM = 1, ONGYM_STATE_KEEP_PARAMS = 2 };
int ongym_state_size(ongym_env *env, int32_t count, int64_t *bytes);      /* header + count replica blocks */
int ongym_state_save(ongym_env *env, int32_t count, const int32_t *replicas, void *out);
int ongym_state_load(ongym_env *env, int32_t count, const int32_t *replicas, const void *in, int32_t flags);
/* The in-loop gather: replica j takes the PRE-fork state of replica src[j], whatever the overlap (permutations, cycles,
 * one replica into all).  src[j] < 0, src[j] == j or src[j] >= batch leaves replica j unchanged.  src int32 [batch] follows
 * cfg.io_device: a device list is read on the env's stream and nothing synchronises (its entries cannot be checked); a host
 * list with an entry >= batch is refused with ONGYM_E_ARG before any launch.  Runs in one pass into a second set of state
 * arrays (allocated on the first fork: twice the state memory from then on), which then becomes the environment's. */
int ongym_fork(ongym_env *env, const int32_t *src, int32_t flags);

/* Diagnostic: resident workgroups (one wavefront = one replica each) per compute unit of the kernel that
 * ongym_step_policy(ONGYM_POLICY_FIRST_FIT) launches on this environment, its dynamic LDS bytes per replica, and whether it
 * is the lean kernel (1) or the generic one (0). */
int ongym_query_occupancy(ongym_env *env, int32_t *blocks_per_cu, int32_t *lds_bytes, int32_t *lean_kernel);
/* The same for the kernel ongym_step_policy(policy) launches.  Lean kernels (csrc/ongym_fast.hpp) exist for first fit, load
 * balancing, highest SNR and lowest fragmentation - the four heuristics the reference benchmark selects among
 * (examples/JOCN_Benchmark_2024/graph_load.py:116-125). */
int ongym_query_occupancy_policy(ongym_env *env, int32_t policy, int32_t *blocks_per_cu, int32_t *lds_bytes, int32_t *lean_kernel);
/* Diagnostic, read-only: what a lean kernel fetches from the shared-link weight table (csrc/ongym_lwtab.hpp) for route `path`
 * and an interferer whose link mask is `links` (bit l = link l; links that are not on the route do not matter).
 * out[0] = 1 when the environment has a table (links fit one mask word, every route got a multiplier, ONGYM_FAST_NO_LWTAB
 * was not 1 at create), else 0 and nothing else is written.  out[1] = the route's multiplier, out[2] = the index the kernel
 * computes, out[3] = the number of index bits W; entry[0..1] = (sum w1, sum w2) as read back from device memory at the address
 * the kernel would use.  ONGYM_E_ARG: path outside 0..n_paths-1 or a NULL pointer. */
int ongym_query_link_weight_entry(ongym_env *env, int32_t path, uint32_t links, uint32_t out[4], double entry[2]);
/* Diagnostic, read-only: dword 0 of route `path` in first fit's copy of the route records, as read back from device memory
 * (csrc/ongym_tables.hpp, path_rows_word).  Bits 0..7 = the hop count; four fields 6 bits apart from bit 8 (link ids < 32: five bits each
 * count) = the route's links in path_links order, the first link repeated behind the last hop; bit 31 (the spare bit of the
 * last field) = the route takes the link loop (more than four
 * hops, n_slots >= 512 or n_links > 32), its fields are then 0.  ONGYM_E_ARG: path outside 0..n_paths-1, a NULL pointer or an
 * environment without lean kernels. */
int ongym_query_path_rows(ongym_env *env, int32_t path, uint32_t *out);
int ongym_sync(ongym_env *env);
/* Run every later call of this environment on the CALLER's HIP stream (a hipStream_t passed as void *, e.g. PyTorch-ROCm's
 * torch.cuda.current_stream().cuda_stream) instead of the environment's own: the environment's launches are then ordered with
 * the caller's kernels on that stream and an RL loop (observe -> policy network -> step) needs no host synchronisation
 * between them.  use_own != 0 returns to the environment's own stream (hip_stream is then ignored); with use_own == 0 a NULL
 * hip_stream is HIP's default (null) stream, which is what PyTorch's default current stream is.  The call first drains the
 * stream used so far.  The caller keeps ownership of its stream and must keep it alive while it is set.  (The reference's
 * counterpart is the implicit ordering of a single Python thread: wrappers/qrmsa_gym.py:45-59.) */
int ongym_set_stream(ongym_env *env, void *hip_stream, int32_t use_own);
/* Device time (ms, HIP events on the env's stream) of the most recent step launch; <0 if none. */
double ongym_last_kernel_ms(ongym_env *env);
const char *ongym_last_error(ongym_env *env);
/* sizes the host side needs to allocate buffers / check the build */
int32_t ongym_abi_version(void);
int32_t ongym_sizeof(int32_t what); /* 0 config, 1 request, 2 step_rec, 3 service, 4 stats, 5 move */

/* The weighted candidate-scoring policy, weights per replica: the call, its features and its rules */
#include "ongym_score.h"

#ifdef __cplusplus
}
#endif
#endif /* ONGYM_H */
