"""ctypes mirror of include/ongym.h and the loader of libongym_hip.so.

There is no CPU fallback: if the HIP library is missing or fails to load, `load_library()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from ._tables import StaticTables, cumulative, modulation_arrays

ABI_VERSION = 4
PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.join(os.path.dirname(PKG_DIR), "csrc")
HIP_LIB_PATH = os.path.join(CSRC_DIR, "libongym_hip.so")

OK, E_ARG, E_HIP, E_STATE, E_CAPACITY, E_LIMIT = 0, -1, -2, -3, -4, -5   # return codes (ONGYM_OK, ONGYM_E_*)
POLICY_FIRST_FIT = 0
POLICY_LOAD_BALANCING = 1
POLICY_HIGHEST_SNR = 2
POLICY_LOWEST_SPECTRUM, POLICY_LB_FIRST_FIT, POLICY_BEST_MOD_LB = 3, 4, 5
POLICY_MSCL_SIMPLIFIED, POLICY_MSCL_SEQUENTIAL, POLICY_PSR, POLICY_EXACT_FIT = 6, 7, 8, 9
POLICY_LOWEST_FRAGMENTATION, POLICY_MSCL, POLICY_COUNT = 10, 11, 12
F_BLOCKED_RESOURCES, F_BLOCKED_OSNR, F_QOT_ERROR, F_OVERFLOW, F_NO_REQUEST = 1, 2, 4, 8, 16
DTYPE_F32, DTYPE_BF16 = 0, 1                                # ongym_masked_categorical logits dtypes
HEAD_SAMPLE, HEAD_ARGMAX, HEAD_EVALUATE = 0, 1, 2           # ... and modes
MASK_BYTES, MASK_BITS = 0, 1                                # ongym_masked_categorical_rows mask formats
STATE_KEEP_STREAM, STATE_KEEP_PARAMS = 1, 2                # ongym_state_load / ongym_fork flags
MAX_BLOCKS = 16                                             # ongym_observe_blocks: blocks per route
LINK_METRICS = ("free_slots", "free_blocks", "largest_free_block", "used_blocks", "occupied_span", "external_fragmentation",
                "entropy", "rss")                           # ongym_link_metrics: link_out features per link, in order
LINK_STATS = ("utilization", "external_fragmentation", "compactness", "last_update")   # ... and link_stats entries
SERVICE_QOT = ("gsnr", "ase", "nli", "margin")               # ongym_service_qot: svc_out entries per record (dB), in order
REPLICA_QOT = ("running", "below_minimum", "below_margin", "lowest_margin", "mean_gsnr", "lowest_margin_index")   # replica_out
LINK_QOT = ("lightpaths", "lowest_margin", "below_minimum")  # ... and link_out entries per link
ACTION_IMPACT = ("status", "affected", "below_minimum_after", "newly_below_minimum", "newly_below_margin", "lowest_margin_after",
                 "largest_drop", "lowest_margin_record")     # ongym_action_impact: impact_out entries per (replica, action)
MAX_IMPACT_ACTIONS = 256                                    # ... and the longest action list per replica
FAILURE_IMPACT = ("status", "victims", "victim_capacity", "restored", "restored_capacity", "lost_no_spectrum", "lost_qot",
                  "extra_hops", "extra_slot_hops", "lowest_margin")   # ongym_failure_impact: link_out entries per (replica, link)
FAILURE_SETS = FAILURE_IMPACT + ("lost_no_route", "failed_links")     # ongym_failure_sets: set_out entries per (replica, link set)
MAX_FAILURE_SETS = 65535                                              # link sets per replica in one call
CUT_LINKS = FAILURE_SETS + ("dropped",)                               # ongym_cut_links: cut_out entries per replica
CUT_NO_RESTORE = 1                                                    # ... its flag: every victim is dropped, none restored
MOVE_TOP, MOVE_FIRST_FIT, MOVE_OWN_ROUTE = -1, -1, 1                   # ongym_move_services: record selector, target selector, flag
MOVE_COLUMNS = ("status", "record", "old_action", "new_action", "margin", "slot_hops_delta")   # ... move_out entries per (replica, move)
SPECTRUM_AUDIT_COLUMNS = ("violations", "records", "malformed", "overlap_cells", "claimed_free_cells", "orphan_cells", "over_width",
                          "failed_links", "claimed_cells", "used_cells")   # ongym_spectrum_map: audit_out entries per replica
SPECTRUM_RECORD_COLUMNS = ("path_id", "slot", "nslots", "modulation", "service_id", "flags")   # ... rec_out entries per record
SPECTRUM_DISRUPTED, SPECTRUM_MALFORMED = 1, 2                # ... the bits of its flags column
OWNER_FREE, OWNER_GUARD_BASE, OWNER_UNOWNED = -1, -2, -32768  # ... owner_out: free; guard cell of record i = -2 - i; used, unclaimed
MAX_OWNER_CAPACITY = 32766                                  # ... owner_out needs capacity <= this
ADMISSION_MAP = ("status", "admitted", "blocked_no_spectrum", "blocked_qot", "blocking_probability", "bit_rate_blocking",
                 "lowest_margin", "detoured")                # ongym_admission_map: summary_out entries per (replica, action)
MAX_ADMISSION_ACTIONS, MAX_ADMISSION_RATES = 256, 16        # ... and the longest action and rate lists
PLAYOUT = ("status", "first_accepted", "steps", "accepted", "blocked", "bit_rate_accepted", "bit_rate_requested",
           "active_end")                                    # ongym_playout: playout_out entries per (replica, action, sample)
PLAYOUT_OWN_STREAM = 1                                      # ... its flag: the replica's own source continues
MAX_PLAYOUT_ACTIONS, MAX_PLAYOUT_SAMPLES, MAX_PLAYOUT_SCENARIOS, MAX_PLAYOUT_HORIZON = 256, 64, 4096, 4096   # ... its limits (A, R, A R, H)
# ongym_score_actions (include/ongym_score.h): the features x0..x9 of a candidate placement, in the order of the weights
SCORE_FEATURES = ("route", "hops", "format_rank", "slots", "slot_hops", "start", "load", "touch", "gsnr", "margin")
SCORE_COUNT_COLUMNS = ("with_spectrum", "feasible", "flags")   # ... and count_out entries per replica


def score_weights(**named) -> np.ndarray:
    """float64 [len(SCORE_FEATURES)]: the weight vector with the named features' weights, zero elsewhere"""
    w = np.zeros(len(SCORE_FEATURES))
    for name, value in named.items():
        w[SCORE_FEATURES.index(name)] = float(value)
    return w


def first_feasible_weights(n_mods: int, n_slots: int) -> np.ndarray:
    """The weights whose score is the step's action index k M S + format_rank S + start: the lowest feasible action wins"""
    return score_weights(route=int(n_mods) * int(n_slots), format_rank=int(n_slots), start=1)


# Weight vectors by name.  first_feasible depends on the configuration: its entry is the helper, called with (n_mods, n_slots).
SCORE_PRESETS = {
    "first_feasible": first_feasible_weights,
    "highest_snr": score_weights(gsnr=-1),
    "lowest_margin": score_weights(margin=1),
    # fewest slot-hops; among equals the shorter-listed route, then the lower start (both far below one slot-hop: k < 2^7, s < 2^10)
    "least_slot_hops": score_weights(slot_hops=1, route=2.0 ** -8, start=2.0 ** -20),
}


def score_preset(name: str, n_mods: int, n_slots: int) -> np.ndarray:
    """A copy of the weight vector SCORE_PRESETS[name] for a configuration with n_mods formats and n_slots slots"""
    w = SCORE_PRESETS[name]
    return w(n_mods, n_slots) if callable(w) else w.copy()

_i32p, _f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)


class OngymConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("abi_version", C.c_int32),
        ("n_nodes", C.c_int32), ("n_links", C.c_int32), ("n_paths", C.c_int32), ("k_paths", C.c_int32),
        ("max_hops", C.c_int32), ("n_mods", C.c_int32), ("n_slots", C.c_int32),
        ("batch", C.c_int32), ("capacity", C.c_int32), ("episode_length", C.c_int32), ("auto_reset", C.c_int32),
        ("bit_rate_mode", C.c_int32), ("n_bit_rates", C.c_int32), ("bit_rate_lo", C.c_int32),
        ("bit_rate_hi", C.c_int32), ("device", C.c_int32), ("io_device", C.c_int32), ("measure_disruptions", C.c_int32),
        ("defragmentation", C.c_int32), ("n_defrag_services", C.c_int32),
        ("frequency_start", C.c_double), ("slot_bandwidth", C.c_double), ("channel_width", C.c_double),
        ("launch_power_w", C.c_double), ("margin", C.c_double), ("load", C.c_double),
        ("mean_holding_time", C.c_double),
        ("pair_paths", _i32p), ("path_hops", _i32p), ("path_links", _i32p), ("link_nspans", _i32p),
        ("link_span_km", _f64p), ("link_alpha", _f64p), ("link_nf", _f64p),
        ("mod_se", _i32p), ("mod_min_osnr", _f64p), ("bit_rates", _f64p), ("bit_rate_cum", _f64p),
        ("node_cum", _f64p),
        ("replica_launch_power_w", _f64p), ("replica_load", _f64p), ("replica_margin", _f64p),
        ("path_len_norm", _f64p), ("max_bit_rate", C.c_double),
        ("track_service_ids", C.c_int32), ("n_mods_consider", C.c_int32),
        ("nslots_channel_width", C.c_double),
    ]


REQUEST_DTYPE = np.dtype([("arrival_time", "<f4"), ("holding_time", "<f4"), ("bit_rate", "<f4"),
                          ("source", "<i2"), ("destination", "<i2")])
STEP_DTYPE = np.dtype([("action", "<i4"), ("route", "<i2"), ("modulation", "<i2"), ("slot", "<i2"),
                       ("nslots", "<i2"), ("accepted", "u1"), ("terminated", "u1"), ("retry", "u1"),
                       ("flags", "u1"), ("active", "<i4"), ("osnr", "<f8"), ("ase", "<f8"), ("nli", "<f8"),
                       ("reward", "<f8")], align=True)
SERVICE_DTYPE = np.dtype([("path_id", "<i4"), ("slot", "<i2"), ("nslots", "<i2"), ("modulation", "<i2"),
                          ("reserved", "<i2"), ("release_time", "<f4"), ("service_id", "<i4"), ("pad_", "<i4"),
                          ("osnr", "<f8")], align=True)
MOVE_LOG = 64
MOVE_DTYPE = np.dtype([("service_id", "<i4"), ("slot", "<i4"), ("osnr", "<f8"), ("ase", "<f8"), ("nli", "<f8")], align=True)
STATS_DTYPE = np.dtype([
    ("services_processed", "<i8"), ("services_accepted", "<i8"),
    ("episode_services_processed", "<i8"), ("episode_services_accepted", "<i8"),
    ("bit_rate_requested", "<f8"), ("bit_rate_provisioned", "<f8"),
    ("episode_bit_rate_requested", "<f8"), ("episode_bit_rate_provisioned", "<f8"),
    ("rejected", "<i8"), ("episode_modulation_hist", "<i8", (8,)), ("episode_osnr_sum", "<f8"),
    ("episodes_completed", "<i8"), ("disrupted_services", "<i8"), ("episode_disrupted_services", "<i8"),
    ("episode_defrag_cycles", "<i8"), ("episode_service_reallocations", "<i8"),
    ("step_defrag_cycles", "<i8"), ("step_service_reallocations", "<i8"),
    ("total_steps", "<i8"), ("total_accepted", "<i8"), ("total_gn_evals", "<i8"),
    ("total_interferer_terms", "<i8"), ("total_paths_tried", "<i8"), ("total_path_hops", "<i8"),
    ("total_gn_shortcuts", "<i8"), ("total_active_sum", "<i8"), ("current_time", "<f8"), ("active", "<i4"), ("flags", "<i4"),
    ("max_modulation_idx", "<i4"), ("reserved0_", "<i4"),
    # terminal-step snapshot (kept last, see include/ongym.h)
    ("last_episode_processed", "<i8"), ("last_episode_accepted", "<i8"), ("last_rejected", "<i8"),
    ("last_service_blocking_rate", "<f8"), ("last_episode_service_blocking_rate", "<f8"),
    ("last_bit_rate_blocking_rate", "<f8"), ("last_episode_bit_rate_blocking_rate", "<f8"),
    ("last_modulation_hist", "<i8", (8,)), ("last_mean_gsnr", "<f8"), ("last_episode_disrupted", "<i8"),
    ("last_episode_defrag_cycles", "<i8"), ("last_episode_service_reallocations", "<i8")], align=True)


class ConfigHolder:
    """An `OngymConfig` plus the numpy arrays its pointers refer to (kept alive here)."""

    def __init__(self, tables: StaticTables, *, modulations: Sequence, num_spectrum_resources: int = 320,
                 batch: int = 1, capacity: int = 1024, episode_length: int = 1000, auto_reset: bool = False,
                 load: float = 10.0, mean_service_holding_time: float = 10800.0,
                 bit_rate_selection: str = "continuous", bit_rates: Sequence[float] = (10, 40, 100),
                 bit_rate_probabilities: Optional[Sequence[float]] = None,
                 node_request_probabilities: Optional[Sequence[float]] = None,
                 bit_rate_lower_bound: float = 25.0, bit_rate_higher_bound: float = 100.0,
                 launch_power_dbm: float = 0.0, frequency_start: float = 3e8 / 1565e-9,
                 frequency_slot_bandwidth: float = 12.5e9, margin: float = 0.0, channel_width: float = 12.5,
                 nslots_channel_width: float = 0.0,
                 device: int = 0, io_device: bool = False, measure_disruptions: bool = False,
                 defragmentation: bool = False, n_defrag_services: int = 0,
                 replica_launch_power_dbm: Optional[Sequence[float]] = None,
                 replica_load: Optional[Sequence[float]] = None,
                 replica_margin: Optional[Sequence[float]] = None, track_service_ids: bool = False,
                 modulations_to_consider: Optional[int] = None):
        if capacity % 64 or capacity <= 0:
            raise ValueError("capacity must be a positive multiple of 64")
        if load <= 0 or mean_service_holding_time <= 0:
            raise ValueError("Both load and mean_service_holding_time must be positive values.")
        self.tables = tables
        t = tables
        mod_se, mod_thr = modulation_arrays(modulations)
        keep = self._keep = {}

        def i32(name, a):
            keep[name] = np.ascontiguousarray(a, np.int32)
            return keep[name].ctypes.data_as(_i32p)

        def f64(name, a):
            keep[name] = np.ascontiguousarray(a, np.float64)
            return keep[name].ctypes.data_as(_f64p)

        c = self.struct = OngymConfig()
        c.struct_size = C.sizeof(OngymConfig)
        c.abi_version = ABI_VERSION
        c.n_nodes, c.n_links, c.n_paths, c.k_paths = t.n_nodes, t.n_links, t.n_paths, t.k_paths
        c.max_hops, c.n_mods, c.n_slots = t.max_hops, len(mod_se), int(num_spectrum_resources)
        c.batch, c.capacity, c.episode_length, c.auto_reset = int(batch), int(capacity), int(episode_length), int(auto_reset)
        if bit_rate_selection == "discrete":
            c.bit_rate_mode = 0
            rates = np.asarray(bit_rates, np.float64)
            cum = cumulative(bit_rate_probabilities, len(rates))
        elif bit_rate_selection == "continuous":
            c.bit_rate_mode = 1
            rates = np.asarray([0.0])
            cum = np.asarray([1.0])
        else:
            raise ValueError("bit_rate_selection must be 'continuous' or 'discrete'")
        c.n_bit_rates = len(rates)
        c.bit_rate_lo, c.bit_rate_hi = int(bit_rate_lower_bound), int(bit_rate_higher_bound)  # qrmsa.pyx:250-254
        c.device, c.io_device = int(device), int(bool(io_device))
        c.measure_disruptions = int(bool(measure_disruptions))
        c.defragmentation, c.n_defrag_services = int(bool(defragmentation)), int(n_defrag_services)
        c.track_service_ids = int(bool(track_service_ids))
        mtc = len(mod_se) if modulations_to_consider is None else min(int(modulations_to_consider), len(mod_se))   # qrmsa.pyx:313
        if mtc < 1:
            raise ValueError("modulations_to_consider must be >= 1")
        c.n_mods_consider = mtc
        c.frequency_start, c.slot_bandwidth = float(frequency_start), float(frequency_slot_bandwidth)
        c.channel_width = float(channel_width)
        c.nslots_channel_width = float(nslots_channel_width)      # `bands`: the C band's width in Hz (quirk Q9); 0 = channel_width
        c.launch_power_w = 10 ** ((float(launch_power_dbm) - 30) / 10)  # qrmsa.pyx:288
        c.margin, c.load, c.mean_holding_time = float(margin), float(load), float(mean_service_holding_time)
        c.pair_paths = i32("pair_paths", t.pair_paths)
        c.path_hops = i32("path_hops", t.path_hops)
        c.path_links = i32("path_links", t.path_links)
        c.link_nspans = i32("link_nspans", t.link_nspans)
        c.link_span_km = f64("link_span_km", t.link_span_km)
        c.link_alpha = f64("link_alpha", t.link_alpha)
        c.link_nf = f64("link_nf", t.link_nf)
        c.mod_se = i32("mod_se", mod_se)
        c.mod_min_osnr = f64("mod_min_osnr", mod_thr)
        c.bit_rates = f64("bit_rates", rates)
        c.bit_rate_cum = f64("bit_rate_cum", cum)
        c.node_cum = f64("node_cum", cumulative(node_request_probabilities, t.n_nodes))
        if replica_launch_power_dbm is not None:
            c.replica_launch_power_w = f64("rlp", [10 ** ((float(x) - 30) / 10) for x in replica_launch_power_dbm])
        if replica_load is not None:
            c.replica_load = f64("rload", replica_load)
        if replica_margin is not None:
            c.replica_margin = f64("rmargin", replica_margin)
        # observation(): route lengths normalised by min/max LINK length (qrmsa.pyx:692-705), max(bit_rates) (:679)
        lo, hi = float(np.min(t.link_length)), float(np.max(t.link_length))
        c.path_len_norm = f64("path_len_norm", [(x - lo) / (hi - lo) if hi != lo else 0.0 for x in t.path_length])
        # observation() normalises by max(self.bit_rates) whatever the selection mode (qrmsa.pyx:679, 688): in "continuous"
        # mode that is the max of the (otherwise unused) bit_rates tuple
        c.max_bit_rate = float(np.max(np.asarray(bit_rates, np.float64))) if len(bit_rates) else 0.0
        for name in ("rlp", "rload", "rmargin"):
            if name in keep and len(keep[name]) != batch:
                raise ValueError("per-replica override arrays must have `batch` entries")
        self.mod_se, self.mod_thr = mod_se, mod_thr
        self.bit_rates = rates

    @property
    def reject_action(self) -> int:
        c = self.struct
        return c.k_paths * c.n_mods_consider * c.n_slots


# ongym_sizeof(what), what = 0..5: the struct and the size this module lays it out with
STRUCT_SIZES = (("ongym_config", C.sizeof(OngymConfig)), ("ongym_request", REQUEST_DTYPE.itemsize),
                ("ongym_step_rec", STEP_DTYPE.itemsize), ("ongym_service", SERVICE_DTYPE.itemsize),
                ("ongym_stats", STATS_DTYPE.itemsize), ("ongym_move", MOVE_DTYPE.itemsize))

# The prototypes of include/ongym.h in the header's order, name -> (restype, argtypes): a new entry point is its prototype
# there and one row here (tests/test_abi_mirror_host.py holds the two together).  Pointers are c_void_p, because callers pass
# arr.ctypes.data, None and c_void_p, except the three that are passed by reference.
_i32, _u32, _i64, _u64, _f32, _f64, _vp = C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_void_p
SIGNATURES = {
    "ongym_create": (_i32, (C.POINTER(OngymConfig), C.POINTER(_vp))),
    "ongym_destroy": (None, (_vp,)),
    "ongym_seed": (_i32, (_vp, _u64)),
    "ongym_seed_base": (_i32, (_vp, _u64, _u64)),
    "ongym_set_requests": (_i32, (_vp, _vp, _i64)),
    "ongym_reset": (_i32, (_vp, _vp)),
    "ongym_reset_episode_counters": (_i32, (_vp, _vp)),
    "ongym_step_policy": (_i32, (_vp, _i32, _i32, _vp)),
    "ongym_step_actions": (_i32, (_vp, _vp, _vp)),
    "ongym_step_actions_bundle": (_i32, (_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp)),
    "ongym_policy_actions": (_i32, (_vp, _i32, _vp, _vp)),
    "ongym_observe": (_i32, (_vp, _vp, _vp)),
    "ongym_observe_blocks": (_i32, (_vp, _i32, _vp, _vp, _vp)),
    "ongym_link_metrics": (_i32, (_vp, _vp, _vp, _vp)),
    "ongym_service_qot": (_i32, (_vp, _vp, _vp, _vp)),
    "ongym_action_impact": (_i32, (_vp, _i32, _vp, _vp, _vp)),
    "ongym_failure_impact": (_i32, (_vp, _i32, _vp, _vp, _vp)),
    "ongym_failure_sets": (_i32, (_vp, _i32, _vp, _i32, _vp, _vp)),
    "ongym_cut_links": (_i32, (_vp, _vp, _i32, _i32, _vp, _vp, _vp)),
    "ongym_repair_links": (_i32, (_vp, _vp, _i32, _vp)),
    "ongym_failed_links": (_i32, (_vp, _vp)),
    "ongym_spectrum_map": (_i32, (_vp, _vp, _vp, _vp, _vp)),
    "ongym_move_services": (_i32, (_vp, _i32, _vp, _i32, _vp)),
    "ongym_admission_map": (_i32, (_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp)),
    "ongym_playout": (_i32, (_vp, _i32, _vp, _i32, _i32, _i32, _u64, _i32, _vp)),
    "ongym_sample_actions": (_i32, (_vp, _vp, _u64, _u64, _vp)),
    "ongym_masked_categorical": (_i32, (_vp, _vp, _i32, _vp, _i32, _u64, _u64, _vp, _vp, _vp, _vp, _vp)),
    "ongym_masked_categorical_backward": (_i32, (_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "ongym_masked_categorical_rows": (_i32, (_vp, _i32, _vp, _i32, _vp, _i32, _i32, _u64, _u64, _vp, _vp, _vp, _vp, _vp)),
    "ongym_masked_categorical_backward_rows": (_i32, (_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "ongym_gae": (_i32, (_vp, _i32, _vp, _vp, _vp, _f32, _f32, _vp, _vp)),
    "ongym_query_available": (_i32, (_vp, _i32, _i32, _vp)),
    "ongym_query_gsnr": (_i32, (_vp, _i32, _i32, _i32, _i32, _vp)),
    "ongym_query_gsnr_many": (_i32, (_vp, _i32, _i32, _vp, _vp)),
    "ongym_query_candidates": (_i32, (_vp, _vp, _i32, _i32, _vp, _vp)),
    "ongym_query_path_free": (_i32, (_vp, _i32, _i32, _i32, _i32, _vp)),
    "ongym_query_moves": (_i32, (_vp, _i32, _vp, _vp)),
    "ongym_query_grid": (_i32, (_vp, _i32, _vp)),
    "ongym_query_services": (_i32, (_vp, _i32, _vp, _vp)),
    "ongym_query_request": (_i32, (_vp, _i32, _vp)),
    "ongym_stats_get": (_i32, (_vp, _vp)),
    "ongym_state_size": (_i32, (_vp, _i32, C.POINTER(_i64))),
    "ongym_state_save": (_i32, (_vp, _i32, _vp, _vp)),
    "ongym_state_load": (_i32, (_vp, _i32, _vp, _vp, _i32)),
    "ongym_fork": (_i32, (_vp, _vp, _i32)),
    "ongym_query_occupancy": (_i32, (_vp, _vp, _vp, _vp)),
    "ongym_query_occupancy_policy": (_i32, (_vp, _i32, _vp, _vp, _vp)),
    "ongym_query_link_weight_entry": (_i32, (_vp, _i32, _u32, _vp, _vp)),
    "ongym_query_path_rows": (_i32, (_vp, _i32, _vp)),
    "ongym_sync": (_i32, (_vp,)),
    "ongym_set_stream": (_i32, (_vp, _vp, _i32)),
    "ongym_last_kernel_ms": (_f64, (_vp,)),
    "ongym_last_error": (C.c_char_p, (_vp,)),
    "ongym_abi_version": (_i32, ()),
    "ongym_sizeof": (_i32, (_i32,)),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
# An older build of the library named by ONGYM_HIP_LIB (tools/ab_bench.py, tools/time_action_impact.py --fork-loop, the
# diag_stamps tools) may lack these; calling one then fails with ctypes' AttributeError.  Any other missing name fails the load.
ABSENT_FROM_OLDER_BUILDS = (
    "ongym_step_actions_bundle", "ongym_action_impact", "ongym_failure_impact", "ongym_failure_sets", "ongym_cut_links",
    "ongym_repair_links", "ongym_failed_links", "ongym_move_services", "ongym_spectrum_map", "ongym_admission_map",
    "ongym_playout", "ongym_sample_actions", "ongym_query_link_weight_entry", "ongym_query_path_rows", "ongym_set_stream")

# The prototype of include/ongym_score.h (ongym.h includes it behind its own declarations), held to that header by
# tests/test_score_host.py.  The in-tree library must export it; an older build named by ONGYM_HIP_LIB may lack it.
SCORE_SIGNATURES = {
    "ongym_score_actions": (_i32, (_vp, _vp, _i32, _vp, _vp, _vp)),
}

_LIB = None


def _declare(lib):
    for name, (restype, argtypes) in SCORE_SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        elif not os.environ.get("ONGYM_HIP_LIB"):
            raise RuntimeError(f"{lib._name} does not export {name}")
    for name, (restype, argtypes) in SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        elif name == "ongym_query_occupancy_policy" and os.environ.get("ONGYM_HIP_LIB"):
            # an older experiment build named by ONGYM_HIP_LIB (tools/ab_bench.py): first fit only
            lib.ongym_query_occupancy_policy = lambda h, policy, nb, lds, lean: lib.ongym_query_occupancy(h, nb, lds, lean)
        elif name not in ABSENT_FROM_OLDER_BUILDS:
            raise RuntimeError(f"{lib._name} does not export {name}")


def load_library(path: Optional[str] = None):
    """dlopen libongym_hip.so (built in-tree by __graft_entry__.build()). Raises if it is missing: there is no
    fallback implementation."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    path = path or os.environ.get("ONGYM_HIP_LIB") or HIP_LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build the HIP extension first "
                           f"(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    lib = C.CDLL(path)
    _declare(lib)
    if lib.ongym_abi_version() != ABI_VERSION:
        raise RuntimeError("libongym_hip.so ABI version mismatch")
    for what, (struct, expect) in enumerate(STRUCT_SIZES):
        got = lib.ongym_sizeof(what)
        if got != expect:
            raise RuntimeError(f"struct size mismatch for {struct}: library {got}, python {expect}")
    _LIB = lib
    return lib
