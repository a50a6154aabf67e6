"""ctypes binding of the C ABI declared in include/hyperball.h.

The shared library is built in-tree (stract_amd/lib/libhyperball.so) by
`__graft_entry__.build()` / `make -C stract_amd/csrc`.  There is no Python or CPU
fallback: if the library is missing, or no gfx950 device is present, calls raise.
"""
import ctypes
import os

# OpenMP worker threads of the host-side pieces (store writer, column reader, the synthetic-graph and oracle support
# libraries) must SLEEP when a parallel region ends, not spin: a box that shows 256 hardware threads under a 16-CPU
# container quota otherwise has hundreds of spinning workers competing with the one thread that drives the GPU - measured:
# ~100 ms lost in the first HIP wait after every parallel region (profiles/r04d_ingest_append_trace.txt).  libgomp reads the
# variable when it is loaded, i.e. before the libraries below are.
os.environ.setdefault("OMP_WAIT_POLICY", "passive")

import numpy as np  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HB_LIB_PATH") or os.path.join(_HERE, "lib", "libhyperball.so")  # HB_LIB_PATH: debug / interpreter builds
# The EXPERIMENTS build (stract_amd/csrc/hb_experiments.h: A/B switches of rejected kernel forms, test hooks; `make exp`): the product
# library refuses those switches, so a Context that asks for one is served by this build.  Tests and measurement tools only.
LIB_EXP_PATH = os.environ.get("HB_LIB_PATH") or os.path.join(_HERE, "lib", "libhyperball_exp.so")

HB_OK = 0
HB_ERR_INVALID, HB_ERR_NO_DEVICE, HB_ERR_HIP, HB_ERR_NOMEM, HB_ERR_RCCL, HB_ERR_LIMIT, HB_ERR_IO = -1, -2, -3, -4, -5, -6, -7
HB_STORE_F64, HB_STORE_U64 = 0, 1
HB_COLL_U8, HB_COLL_U32, HB_COLL_U64, HB_COLL_F64 = 0, 1, 2, 3
HB_COLL_MAX, HB_COLL_SUM = 0, 1
HB_SKIPPED_REL_MASK = 0x6FED00

HB_FLAG_NO_FRONTIER = 0x01
HB_FLAG_NO_REORDER = 0x02
HB_FLAG_UNFUSED = 0x04
HB_FLAG_PASS_STATS = 0x08
HB_FLAG_NO_XCD_MAP = 0x20
HB_FLAG_NO_RCCL = 0x40
HB_FLAG_RCCL_SELF = 0x80
HB_FLAG_NO_SPARSE = 0x100
HB_FLAG_DEST_PARTITION = 0x200
HB_FLAG_HOST_INGEST = 0x400
HB_FLAG_HOST_PLAN = 0x800
HB_FLAG_CHANGED_ONLY = 0x1000
HB_FLAG_REFERENCE_TAIL = 0x2000
HB_FLAG_NO_INIT_PASS = 0x4000
HB_FLAG_ALL_RELS = 0x8000
HB_FLAG_LIVE_FIRST = 0x10000
HB_FLAG_NO_LIVE_FIRST = 0x20000
HB_FLAG_NO_SATURATION = 0x40000
HB_FLAG_NO_EARLY_EXIT = 0x80000      # dense passes gather every source of a row (A/B and test switch of DESIGN.md section 39)
HB_FLAG_FORCE_EARLY_EXIT = 0x100000  # ... test for the early exit from pass 1 on, whatever is saturated (tests)
HB_FLAG_PACKED_WIRE = 0x200000      # whole counters travel as 48-byte rows, 6 bits per register
HB_SAMPLE_MAX_LEVELS = 16

# switches of the experiments build in hb_options.tune[1] (stract_amd/csrc/hb_experiments.h describes each)
HB_X_TILE_EPILOGUE = 0x100
HB_X_SEED_3LAUNCH = 0x800
HB_X_NO_EDGE_OVERLAP = 0x1000
HB_X_BITMAP_SLOTWISE = 0x2000
HB_X_NO_STAGED_RESULTS = 0x4000
HB_X_SNAPSHOT_EVERY_PASS = 0x8000
HB_X_SHORT_FINAL_LIST = 0x10000
HB_X_ONE_SNAPSHOT = 0x20000
HB_X_NO_TAIL_PIPELINE = 0x100000
HB_X_TAIL_KERNEL = 0x200000
HB_X_TAIL_KERNEL_ANY = 0x400000
HB_X_FULL_INIT = 0x800000
HB_X_WIRE_64B = 0x1000000
HB_X_SCATTER_TRANSPOSE = 0x2000000
HB_X_SWEEP_ROUNDS = 0x4000000
HB_X_GENERIC_LEVEL1 = 0x8000000
HB_X_PROBE_NO_SIZE = 0x10000000
HB_X_SIM_SMALL_PIECES = 0x20000000

# numpy views of the plain-data structs
U128 = np.dtype([("lo", "<u8"), ("hi", "<u8")])
EDGE = np.dtype([("from", U128), ("to", U128), ("rel_flags", "<u8")])
assert U128.itemsize == 16 and EDGE.itemsize == 40


# int all_to_all(void *user, const void *send, void *recv, uint64_t bytes_per_rank, void *stream) - hb_set_all_to_all
ALL_TO_ALL_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p)


class HbOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("chunk", ctypes.c_uint32),
        ("max_passes", ctypes.c_uint32),
        ("rank", ctypes.c_int32),
        ("world_size", ctypes.c_int32),
        ("rccl_id", ctypes.c_uint8 * 128),
        ("tune", ctypes.c_uint32 * 8),
    ]


class _Stats(ctypes.Structure):
    """a stats struct whose dict form is its plain fields"""

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class HbStats(_Stats):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("m_input", ctypes.c_uint64),
        ("m_unique", ctypes.c_uint64),
        ("m_eff", ctypes.c_uint64),
        ("passes", ctypes.c_uint64),
        ("results", ctypes.c_uint64),
        ("ms_ingest", ctypes.c_double),
        ("ms_plan", ctypes.c_double),
        ("ms_h2d", ctypes.c_double),
        ("ms_loop", ctypes.c_double),
        ("ms_loop_gpu", ctypes.c_double),
        ("ms_collective", ctypes.c_double),
        ("ms_d2h", ctypes.c_double),
        ("work_rows", ctypes.c_uint64),
        ("virtual_rows", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("virtual_edges", ctypes.c_uint64),
        ("levels", ctypes.c_uint64),
        ("level1_edges", ctypes.c_uint64),
        ("level1_rows", ctypes.c_uint64),
        ("direct_edges", ctypes.c_uint64),
        ("rows_with_in_edges", ctypes.c_uint64),
        ("wire_bytes", ctypes.c_uint64),
        ("ingest_peak_bytes", ctypes.c_uint64),
        ("pool_peak_bytes", ctypes.c_uint64),
        ("result_stages", ctypes.c_uint64),
        ("result_list", ctypes.c_uint64),
        ("pipelined_passes", ctypes.c_uint64),
        ("tail_kernel_passes", ctypes.c_uint64),
    ]


class HbPassStats(ctypes.Structure):
    _fields_ = [
        ("pass_", ctypes.c_uint64),
        ("changed", ctypes.c_uint64),
        ("active_edges", ctypes.c_uint64),
        ("touched", ctypes.c_uint64),
        ("mode", ctypes.c_uint32),
        ("ms_gpu", ctypes.c_float),
        ("ms_main", ctypes.c_float),
        ("ms_collective", ctypes.c_float),
        ("ms_level1", ctypes.c_float),
        ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["pass"] = d.pop("pass_")
        return d


class HbSampleOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("max_dist", ctypes.c_uint32),
        ("seed", ctypes.c_uint64),
        ("samples", ctypes.c_uint64),
        ("num_nodes", ctypes.c_uint64),
        ("epsilon", ctypes.c_double),
        ("sources", ctypes.c_void_p),
        ("source_count", ctypes.c_uint64),
    ]


class HbSampleStats(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("levels", ctypes.c_uint32),
        ("k_req", ctypes.c_uint64),
        ("sources", ctypes.c_uint64),
        ("batches", ctypes.c_uint64),
        ("results", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("level_changed", ctypes.c_uint64 * HB_SAMPLE_MAX_LEVELS),
        ("level_modes", ctypes.c_uint32 * HB_SAMPLE_MAX_LEVELS),
        ("level_ms", ctypes.c_double * HB_SAMPLE_MAX_LEVELS),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k in ("level_changed", "level_modes", "level_ms"):
            d[k] = list(d[k])[:self.levels]
        return d


HB_DIST_REVERSED = 0x1
HB_DIST_WITH_MAX = 0x2
HB_DIST_TOP_DOWN_ONLY = 0x4
HB_DIST_BOTTOM_UP_ONLY = 0x8
HB_DIST_UNREACHED = 255


class HbDistanceOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("max_dist", ctypes.c_uint32),
        ("sources", ctypes.c_void_p),
        ("source_count", ctypes.c_uint64),
    ]


class HbDistanceStats(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("levels", ctypes.c_uint32),
        ("max_distance", ctypes.c_uint32),
        ("reached", ctypes.c_uint64),
        ("unknown_sources", ctypes.c_uint64),
        ("edges_inspected", ctypes.c_uint64),
        ("frontier", ctypes.c_uint64 * 256),
        ("step", ctypes.c_uint8 * 256),
        ("ms_total", ctypes.c_double),
        ("ms_levels", ctypes.c_double),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k in ("frontier", "step"):
            d[k] = list(d[k])[:self.levels + 1]  # [0] = the sources, [d] = level d
        return d


HB_BC_RAW = 0x1
HB_BC_DENSE_ONLY = 0x2
HB_BC_SPARSE_ONLY = 0x4


class HbBetweennessOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("sources", ctypes.c_void_p),
        ("source_count", ctypes.c_uint64),
    ]


class HbBetweennessStats(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("max_dist", ctypes.c_uint32),
        ("sources", ctypes.c_uint64),
        ("unknown_sources", ctypes.c_uint64),
        ("batches", ctypes.c_uint64),
        ("results", ctypes.c_uint64),
        ("levels_forward", ctypes.c_uint64),
        ("levels_backward", ctypes.c_uint64),
        ("levels_mode", ctypes.c_uint64 * 3),
        ("edges_gathered", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("ms_forward", ctypes.c_double),
        ("ms_backward", ctypes.c_double),
        ("ms_mode", ctypes.c_double * 3),
        ("ms_dense_max", ctypes.c_double),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k in ("levels_mode", "ms_mode"):  # per mode: dense, bitmap, sweep
            d[k] = list(d[k])
        return d


HB_SIM_NORMALIZED = 0x1
HB_SIM_DENSE_ONLY = 0x2
HB_SIM_SPARSE_ONLY = 0x4
HB_SIM_SELF_SCORE = 0x8
HB_SIM_TOP_SKIP_ANCHORS = 0x1


class HbSimilarityOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("liked", ctypes.c_void_p),
        ("liked_count", ctypes.c_uint64),
        ("disliked", ctypes.c_void_p),
        ("disliked_count", ctypes.c_uint64),
        ("self_score", ctypes.c_double),
        ("limit", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class HbSimilarityStats(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("liked", ctypes.c_uint64),
        ("disliked", ctypes.c_uint64),
        ("unknown", ctypes.c_uint64),
        ("batches", ctypes.c_uint64),
        ("rows_nonzero", ctypes.c_uint64),
        ("levels_mode", ctypes.c_uint64 * 3),
        ("edges_gathered", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("ms_bloom", ctypes.c_double),
        ("ms_count", ctypes.c_double),
        ("ms_score", ctypes.c_double),
        ("ms_mode", ctypes.c_double * 3),
        ("listed_rows", ctypes.c_uint64),
        ("list_entries", ctypes.c_uint64),
        ("ms_lists", ctypes.c_double),
        ("ms_list_count", ctypes.c_double),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k in ("levels_mode", "ms_mode"):  # per mode: dense, bitmap, sweep
            d[k] = list(d[k])
        return d


HB_SEED_FROM_IMAGE = 0x1


class HbNearestSeedOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("discount_factor", ctypes.c_double),
        ("rounds", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("orig_ids", ctypes.c_void_p),
        ("orig_vals", ctypes.c_void_p),
        ("orig_count", ctypes.c_uint64),
        ("key_ids", ctypes.c_void_p),
        ("keys", ctypes.c_void_p),
        ("key_count", ctypes.c_uint64),
    ]


class HbNearestSeedStats(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("rounds_run", ctypes.c_uint32),
        ("with_original", ctypes.c_uint64),
        ("filled", ctypes.c_uint64 * 16),
        ("unknown_orig", ctypes.c_uint64),
        ("unknown_keys", ctypes.c_uint64),
        ("no_seed", ctypes.c_uint64),
        ("seed_without_value", ctypes.c_uint64),
        ("results", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("ms_seed", ctypes.c_double),
        ("ms_fill", ctypes.c_double),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["filled"] = list(d["filled"])  # per round; the 16th entry holds every later round
        return d


HB_LINKS_KEYS_FROM_RANKS = 0x1
HB_LINKS_KEEP_SELF = 0x1
HB_LINKS_SPREAD_ORDS = 0x2
HB_LINKS_NO_SHORTCUT = 0x4


class HbSimilarOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("nodes", ctypes.c_void_p),
        ("node_count", ctypes.c_uint64),
        ("limit", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class HbSimilarStats(_Stats):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("apply", ctypes.c_uint32),
    ] + [(k, ctypes.c_uint64) for k in ("liked_distinct", "unknown", "nb", "forward_entries", "distinct_targets", "count_bound", "taken", "candidates",
                                        "pairs_gated", "pairs_intersected", "written", "device_bytes")] + [
        (k, ctypes.c_double) for k in ("ms_total", "ms_in", "ms_forward", "ms_count", "ms_bitvec", "ms_score", "ms_gpu_lists", "ms_gpu_score")]


HB_SCORE_SMALL_PIECES = 0x100


class HbScoreRequest(ctypes.Structure):
    _fields_ = [
        ("liked", ctypes.c_void_p),
        ("liked_count", ctypes.c_uint64),
        ("disliked", ctypes.c_void_p),
        ("disliked_count", ctypes.c_uint64),
        ("nodes", ctypes.c_void_p),
        ("node_count", ctypes.c_uint64),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("self_score", ctypes.c_double),
    ]


class HbScoreOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("requests", ctypes.POINTER(HbScoreRequest)),
        ("request_count", ctypes.c_uint64),
        ("limit", ctypes.c_uint32),
        ("slots_per_batch", ctypes.c_uint32),
    ]


class HbScoreStats(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ] + [(k, ctypes.c_uint64) for k in ("requests", "anchors", "nodes", "unknown_anchors", "unknown_nodes", "distinct", "pairs", "pairs_self", "pairs_empty",
                                        "pairs_gated", "pairs_intersected", "pieces", "device_bytes")] + [
        (k, ctypes.c_double) for k in ("ms_total", "ms_lists", "ms_bitvec", "ms_pairs", "ms_finish")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class HbLinksKeyOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("key_ids", ctypes.c_void_p),
        ("keys", ctypes.c_void_p),
        ("key_count", ctypes.c_uint64),
    ]


class HbLinksKeyStats(_Stats):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("listed", ctypes.c_uint64),
        ("unknown_keys", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("ms_order", ctypes.c_double),
    ]


class HbLinksOptions(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("nodes", ctypes.c_void_p),
        ("node_count", ctypes.c_uint64),
        ("limit", ctypes.c_uint32),
        ("slots_per_batch", ctypes.c_uint32),
    ]


class HbLinksStats(_Stats):
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("queries", ctypes.c_uint64),
        ("unknown", ctypes.c_uint64),
        ("distinct", ctypes.c_uint64),
        ("batches", ctypes.c_uint64),
        ("entries", ctypes.c_uint64),
        ("rows_walked", ctypes.c_uint64),
        ("edges_gathered", ctypes.c_uint64),
        ("selected", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("ms_expand", ctypes.c_double),
        ("ms_select", ctypes.c_double),
        ("ms_emit", ctypes.c_double),
    ]


# every symbol include/hyperball.h declares: (name, restype, argtypes)
_P = ctypes.c_void_p
_U64 = ctypes.c_uint64
_SIGNATURES = [
    ("hb_abi_version", ctypes.c_int, []),
    ("hb_release_cached_memory", ctypes.c_int, [ctypes.c_void_p]),
    ("hb_create", ctypes.c_int, [ctypes.POINTER(HbOptions), ctypes.POINTER(_P)]),
    ("hb_destroy", None, [_P]),
    ("hb_last_error", ctypes.c_char_p, [_P]),
    ("hb_load_edges", ctypes.c_int, [_P, _P, _U64, _P, _U64]),
    ("hb_append_edges", ctypes.c_int, [_P, _P, _U64]),
    ("hb_finalize", ctypes.c_int, [_P, _P, _U64]),
    ("hb_discard_appended", ctypes.c_int, [_P]),
    ("hb_load_tail_edges", ctypes.c_int, [_P, _P, _U64]),
    ("hb_append_tail_edges", ctypes.c_int, [_P, _P, _U64]),
    ("hb_tail_segment_end", ctypes.c_int, [_P]),
    ("hb_debug_set_ingest_limits", ctypes.c_int, [_P, _U64, _U64, _U64]),
    ("hb_set_collectives", ctypes.c_int, [_P, _P]),
    ("hb_set_all_to_all", ctypes.c_int, [_P, _P]),
    ("hb_debug_staged_copy", ctypes.c_int, [_P, _P, _U64, ctypes.c_int, _P]),
    ("hb_pinned_alloc", ctypes.c_int, [_U64, ctypes.POINTER(ctypes.c_void_p)]),
    ("hb_pinned_free", None, [ctypes.c_void_p]),
    ("hb_debug_h2d_rate", ctypes.c_int, [_P, _P, _U64, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    ("hb_debug_tail_index", ctypes.c_int, [_U64, _P, _P, _U64, _P, _U64, _P, _P, _U64, ctypes.POINTER(ctypes.c_uint64)]),
    ("hb_load_dense", ctypes.c_int, [_P, _P, _U64, _P, _P, _U64]),
    ("hb_run", ctypes.c_int, [_P, ctypes.POINTER(HbStats)]),
    ("hb_begin", ctypes.c_int, [_P]),
    ("hb_step", ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int)]),
    ("hb_finish", ctypes.c_int, [_P]),
    ("hb_get_stats", ctypes.c_int, [_P, ctypes.POINTER(HbStats)]),
    ("hb_get_pass_stats", ctypes.c_int, [_P, _U64, ctypes.POINTER(HbPassStats)]),
    ("hb_result_count", ctypes.c_int, [_P, ctypes.POINTER(_U64)]),
    ("hb_result_copy", ctypes.c_int, [_P, _P, _P, _U64]),
    ("hb_result_ranks", ctypes.c_int, [_P, _P, _U64]),
    ("hb_result_top", ctypes.c_int, [_P, _U64, _P, _P, ctypes.POINTER(ctypes.c_uint64)]),
    ("hb_rccl_unique_id", ctypes.c_int, [_P]),
    ("hb_device_count", ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ("hb_device_name", ctypes.c_int, [_P, ctypes.c_char_p, _U64]),
    ("hb_device_synchronize", ctypes.c_int, [_P]),
    ("hb_debug_copy_registers", ctypes.c_int, [_P, _P]),
    ("hb_debug_copy_kahan", ctypes.c_int, [_P, _P, _P]),
    ("hb_debug_copy_sizes", ctypes.c_int, [_P, _P]),
    ("hb_debug_hll_size", ctypes.c_int, [_P, _P, _U64, _P]),
    ("hb_debug_state_hash", ctypes.c_int, [_P, _P]),
    ("hb_debug_copy_graph", ctypes.c_int, [_P, _P, _P, _P]),
    ("hb_debug_copy_plan", ctypes.c_int, [_P, _P, _P, _P, _P, _P]),
    ("hb_debug_exchange", ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int]),
    ("hb_debug_wire6", ctypes.c_int, [_P, _P, _U64, ctypes.c_uint32, _P, _P, _P]),
    ("hb_step_local", ctypes.c_int, [_P]),
    ("hb_step_finish", ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int)]),
    ("hb_host_ingest", ctypes.c_int, [_P, _U64, _P, _U64, ctypes.POINTER(_U64), ctypes.POINTER(_U64),
                                      ctypes.POINTER(_U64), _P, _P, _P]),
    ("hb_host_plan", ctypes.c_int, [_U64, _P, _P, ctypes.c_uint32, ctypes.c_uint32, _P, _P, _P, _P, _P, _P]),
    ("hb_host_plan_live", ctypes.c_int, [_U64, _P, _P, ctypes.c_uint32, ctypes.c_uint32, _P, _P]),
    ("hb_debug_plan_live", ctypes.c_int, [_P, _P]),
    ("hb_debug_saturation", ctypes.c_int, [_P, _P, _P, _P, _P]),
]
# include/hb_webgraph.h
_SIGNATURES += [
    ("hbw_open", ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(_P)]),
    ("hbw_close", None, [_P]),
    ("hbw_last_error", ctypes.c_char_p, [_P]),
    ("hbw_num_segments", ctypes.c_int, [_P, ctypes.POINTER(_U64)]),
    ("hbw_segment_info", ctypes.c_int, [_P, _U64, ctypes.c_char_p, ctypes.POINTER(_U64)]),
    ("hbw_total_rows", ctypes.c_int, [_P, ctypes.POINTER(_U64)]),
    ("hbw_read_host_edges", ctypes.c_int, [_P, _U64, _U64, _P]),
    ("hbw_read_page_edges", ctypes.c_int, [_P, _U64, _U64, _P]),
    ("hb_load_webgraph", ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_uint32]),
    ("hbw_debug_sstable", ctypes.c_int, [_P, _U64, ctypes.c_int, _P, _U64, _P, _U64, ctypes.POINTER(_U64)]),
    ("hbw_debug_crc32", ctypes.c_uint32, [_P, _U64]),
]
# include/hb_ampc.h
_SIGNATURES += [
    ("hbu_create", ctypes.c_int, [ctypes.c_int32, _U64, ctypes.POINTER(_P)]),
    ("hbu_destroy", None, [_P]),
    ("hbu_last_error", ctypes.c_char_p, [_P]),
    ("hbu_len", ctypes.c_int, [_P, ctypes.POINTER(_U64)]),
    ("hbu_batch_set", ctypes.c_int, [_P, _P, _P, _U64]),
    ("hbu_batch_get", ctypes.c_int, [_P, _P, _U64, _P, _P]),
    ("hbu_batch_upsert", ctypes.c_int, [_P, _P, _P, _U64, _P]),
    ("hbu_create_kind", ctypes.c_int, [ctypes.c_int32, _U64, ctypes.c_uint32, ctypes.POINTER(_P)]),
    ("hbu_kind", ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    ("hbu_batch_set_values", ctypes.c_int, [_P, _P, _P, _U64]),
    ("hbu_batch_get_values", ctypes.c_int, [_P, _P, _U64, _P, _P]),
    ("hbu_batch_upsert_values", ctypes.c_int, [_P, ctypes.c_uint32, _P, _P, _U64, _P]),
    ("hbu_wave_group_length", ctypes.c_uint32, []),
    ("hbu_clone", ctypes.c_int, [_P, ctypes.POINTER(_P)]),
    ("hbu_update_centralities", ctypes.c_int, [_P, _P, _P, _P, _P, _U64, _U64, ctypes.POINTER(_U64)]),
    ("hbu_update_counters", ctypes.c_int, [_P, _P, _P, _P, _U64, _P]),
    ("hbu_update_distances", ctypes.c_int, [_P, _P, _P, _P, _U64, _P, _P, ctypes.POINTER(_U64)]),
    ("hbu_graph_create", ctypes.c_int, [ctypes.c_int32, _P, _U64, _P, _P, _U64, _U64, ctypes.POINTER(_P)]),
    ("hbu_graph_len", ctypes.c_int, [_P, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("hbu_graph_destroy", None, [_P]),
    ("hbu_bloom_num_bits", _U64, [_U64, ctypes.c_double]),
    ("hbu_filter_create", ctypes.c_int, [ctypes.c_int32, ctypes.c_uint32, _U64, ctypes.POINTER(_P)]),
    ("hbu_filter_destroy", None, [_P]),
    ("hbu_filter_clear", ctypes.c_int, [_P]),
    ("hbu_filter_fill", ctypes.c_int, [_P]),
    ("hbu_filter_insert", ctypes.c_int, [_P, _P, _U64]),
    ("hbu_filter_contains", ctypes.c_int, [_P, _P, _U64, _P]),
    ("hbu_filter_union", ctypes.c_int, [_P, _P]),
    ("hbu_filter_count", ctypes.c_int, [_P, ctypes.POINTER(_U64)]),
    ("hbu_filter_export_bits", ctypes.c_int, [_P, _P]),
    ("hbu_filter_import_bits", ctypes.c_int, [_P, _P]),
    ("hbu_filter_export_ids", ctypes.c_int, [_P, _P, _U64, ctypes.POINTER(_U64)]),
    ("hbu_setup_counters", ctypes.c_int, [_P, _P, _P, _P]),
    ("hbu_round_counters", ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("hbu_round_distances", ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("hbu_round_centralities", ctypes.c_int, [_P, _P, _P, _P, _P, _P, _U64, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("hbu_export", ctypes.c_int, [_P, _P, _P, _U64, ctypes.POINTER(_U64)]),
    ("hbu_fold_harmonic", ctypes.c_int, [_P, _P, ctypes.c_double, ctypes.c_uint32, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("hbu_graph_node_sketch", ctypes.c_int, [_P, _P]),
    ("hbu_fold_harmonic_lanes", ctypes.c_int, [_P, _P, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("hbu_round_lane_distances", ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("hbu_finish_centralities", ctypes.c_int, [_P, ctypes.c_double, _P, _P, _P, _U64, ctypes.POINTER(_U64)]),
    ("hbu_top_centralities", ctypes.c_int, [_P, ctypes.c_double, _U64, _P, _P, ctypes.POINTER(_U64)]),
    ("hbu_store_centralities", ctypes.c_int, [_P, ctypes.c_double, ctypes.c_char_p, ctypes.c_char_p, _U64]),
]
# include/hb_store.h
_SIGNATURES += [
    ("hb_store_write", ctypes.c_int, [ctypes.c_char_p, _P, _P, ctypes.c_int, _U64, ctypes.c_char_p, ctypes.c_size_t]),
    ("hb_store_harmonic", ctypes.c_int, [ctypes.c_char_p, _P, _P, _P, _U64, ctypes.c_char_p, ctypes.c_size_t]),
    ("hb_store_harmonic_results", ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_char_p, _U64]),
]
# include/hyperball.h: sampled harmonic centrality (ApproxHarmonic)
_SIGNATURES += [
    ("hb_sampled_harmonic", ctypes.c_int, [_P, ctypes.POINTER(HbSampleOptions), ctypes.POINTER(HbSampleStats)]),
    ("hb_sample_sources", ctypes.c_int, [_P, _U64, _U64, _P, ctypes.POINTER(_U64)]),
    ("hb_debug_sample_histogram", ctypes.c_int, [_P, _P]),
]
# include/hyperball.h: exact shortest-path distances (ShortestPaths)
_SIGNATURES += [
    ("hb_distances", ctypes.c_int, [_P, ctypes.POINTER(HbDistanceOptions), ctypes.POINTER(HbDistanceStats)]),
    ("hb_distance_count", ctypes.c_int, [_P, ctypes.POINTER(_U64)]),
    ("hb_distance_copy", ctypes.c_int, [_P, _P, _P, _U64]),
    ("hb_distance_all", ctypes.c_int, [_P, _P, _U64]),
]
# include/hyperball.h: exact betweenness centrality (Betweenness)
_SIGNATURES += [
    ("hb_betweenness", ctypes.c_int, [_P, ctypes.POINTER(HbBetweennessOptions), ctypes.POINTER(HbBetweennessStats)]),
    ("hb_betweenness_count", ctypes.c_int, [_P, ctypes.POINTER(_U64)]),
    ("hb_betweenness_copy", ctypes.c_int, [_P, _P, _P, _U64]),
    ("hb_betweenness_all", ctypes.c_int, [_P, _P, _U64]),
    ("hb_debug_copy_betweenness_batch", ctypes.c_int, [_P, _P, _P, _P]),
]
# include/hyperball.h: inbound similarity (Scorer over BitVec)
_SIGNATURES += [
    ("hb_inbound_similarity", ctypes.c_int, [_P, ctypes.POINTER(HbSimilarityOptions), ctypes.POINTER(HbSimilarityStats)]),
    ("hb_similarity_all", ctypes.c_int, [_P, _P, _U64]),
    ("hb_similarity_lookup", ctypes.c_int, [_P, _P, _U64, _P]),
    ("hb_similarity_top", ctypes.c_int, [_P, _U64, ctypes.c_uint32, _P, _P, ctypes.POINTER(_U64)]),
    ("hb_debug_copy_similarity_batch", ctypes.c_int, [_P, _P, _P, _P]),
]
# include/hyperball.h: nearest-seed centrality (HarmonicNearestSeed)
_SIGNATURES += [
    ("hb_nearest_seed", ctypes.c_int, [_P, ctypes.POINTER(HbNearestSeedOptions), ctypes.POINTER(HbNearestSeedStats)]),
    ("hb_nearest_seed_count", ctypes.c_int, [_P, ctypes.POINTER(_U64)]),
    ("hb_nearest_seed_copy", ctypes.c_int, [_P, _P, _P, _U64]),
    ("hb_nearest_seed_all", ctypes.c_int, [_P, _P, _U64]),
    ("hb_nearest_seed_top", ctypes.c_int, [_P, _U64, _P, _P, ctypes.POINTER(_U64)]),
    ("hb_nearest_seed_seeds", ctypes.c_int, [_P, _P, _P, _U64]),
    # include/hyperball.h: limited, rank-ordered host backlinks (HostBacklinksQuery .. Limit(L))
    ("hb_links_set_keys", ctypes.c_int, [_P, ctypes.POINTER(HbLinksKeyOptions), ctypes.POINTER(HbLinksKeyStats)]),
    ("hb_backlinks", ctypes.c_int, [_P, ctypes.POINTER(HbLinksOptions), ctypes.POINTER(HbLinksStats)]),
    ("hb_forwardlinks", ctypes.c_int, [_P, ctypes.POINTER(HbLinksOptions), ctypes.POINTER(HbLinksStats)]),
    ("hb_links_count", ctypes.c_int, [_P, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("hb_links_copy", ctypes.c_int, [_P, _P, _P, _P, _P, _U64]),
    # include/hyperball.h: similar hosts (scored_nodes of SimilarHostsFinder)
    ("hb_similar_hosts", ctypes.c_int, [_P, ctypes.POINTER(HbSimilarOptions), ctypes.POINTER(HbSimilarStats)]),
    ("hb_similar_count", ctypes.c_int, [_P, ctypes.POINTER(_U64)]),
    ("hb_similar_copy", ctypes.c_int, [_P, _P, _P, _U64]),
    ("hb_similar_candidates", ctypes.c_int, [_P, _P, _P, _U64, ctypes.POINTER(_U64)]),
    # include/hyperball.h: scoring result hosts (Scorer::score per search)
    ("hb_score_hosts", ctypes.c_int, [_P, ctypes.POINTER(HbScoreOptions), ctypes.POINTER(HbScoreStats)]),
    ("hb_score_count", ctypes.c_int, [_P, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    ("hb_score_copy", ctypes.c_int, [_P, _P, _P, _U64]),
]
SYMBOLS = [s[0] for s in _SIGNATURES]

_lib = None
_lib_exp = None


def needs_experiments_build(tune):
    """hb_options.tune values that only the experiments build understands (hb_experiments.h): tune[1] above its low byte, tune[7]."""
    tune = tuple(tune)
    return (len(tune) > 1 and (int(tune[1]) & ~0xFF) != 0) or (len(tune) > 7 and int(tune[7]) != 0)


class HyperballError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hyperball error %d: %s" % (code, msg))
        self.code = code


def _open(path):
    if not os.path.exists(path):
        raise HyperballError(HB_ERR_INVALID,
                             "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "or `make -C stract_amd/csrc` (there is no CPU fallback)" % path)
    lib = ctypes.CDLL(path)
    if hasattr(lib, "hb_simt_interpreter") and os.environ.get("HB_ALLOW_SIMT_INTERPRETER") != "1":
        # tests/simt builds the library's sources against a host interpreter of the device code: test infrastructure for
        # kernel LOGIC, never a way to compute.  Only tests/test_simt.py sets the variable (for its own child process).
        raise HyperballError(HB_ERR_NO_DEVICE, "%s is the SIMT-interpreter test build, not the gfx950 library: refused "
                             "(there is no CPU fallback)" % path)
    for name, res, args in _SIGNATURES:
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    return lib


def load(experiments=False):
    """Load libhyperball.so (once).  Raises if it has not been built.  experiments=True: the experiments build (see LIB_EXP_PATH)."""
    global _lib, _lib_exp
    if experiments and LIB_EXP_PATH != LIB_PATH:
        if _lib_exp is None:
            _lib_exp = _open(LIB_EXP_PATH)
        return _lib_exp
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


def device_count():
    n = ctypes.c_int(0)
    load().hb_device_count(ctypes.byref(n))
    return n.value


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class PinnedRecords:
    """A page-locked batch buffer of `count` SmallEdge records (hb_pinned_alloc = hipHostMalloc in the runtime the LIBRARY
    runs on): `.array` is a numpy view of it.  Pinned batches reach hb_append_edges at the full rate of the host link."""

    def __init__(self, count, dtype=None):
        self.dtype = np.dtype(EDGE if dtype is None else dtype)
        self.count = int(count)
        self._p = ctypes.c_void_p()
        nbytes = max(self.count, 1) * self.dtype.itemsize
        rc = load().hb_pinned_alloc(nbytes, ctypes.byref(self._p))
        if rc != HB_OK or not self._p.value:
            raise HyperballError(rc, "hb_pinned_alloc(%d bytes) failed" % nbytes)
        buf = (ctypes.c_uint8 * nbytes).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=self.count)

    def close(self):
        if self._p is not None and self._p.value:
            self.array = None
            load().hb_pinned_free(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def store_write(path, ids, values):
    """One speedy_kv database directory (include/hb_store.h): ids = U128 array, values = float64 (Db<NodeID, f64>) or
    uint64 (Db<NodeID, u64>) array of the same length.  Host only."""
    ids = np.ascontiguousarray(ids, dtype=U128)
    values = np.ascontiguousarray(values)
    if values.dtype == np.float64:
        kind = HB_STORE_F64
    elif values.dtype == np.uint64:
        kind = HB_STORE_U64
    else:
        raise TypeError("values must be float64 or uint64, not %s" % values.dtype)
    if len(ids) != len(values):
        raise ValueError("ids and values differ in length")
    err = ctypes.create_string_buffer(512)
    rc = load().hb_store_write(os.fsencode(path), _ptr(ids), _ptr(values), kind, len(ids), err, len(err))
    if rc != HB_OK:
        raise HyperballError(rc, err.value.decode(errors="replace"))


def store_harmonic(output, ids, centralities, ranks):
    """`<output>/harmonic` + `<output>/harmonic_rank`: what store_harmonic (centrality/mod.rs:72-114) leaves on disk."""
    ids = np.ascontiguousarray(ids, dtype=U128)
    centralities = np.ascontiguousarray(centralities, dtype=np.float64)
    ranks = np.ascontiguousarray(ranks, dtype=np.uint64)
    if not (len(ids) == len(centralities) == len(ranks)):
        raise ValueError("ids, centralities and ranks differ in length")
    err = ctypes.create_string_buffer(512)
    rc = load().hb_store_harmonic(os.fsencode(output), _ptr(ids), _ptr(centralities), _ptr(ranks), len(ids), err, len(err))
    if rc != HB_OK:
        raise HyperballError(rc, err.value.decode(errors="replace"))


class Context:
    """Thin owner of an hb_ctx*; methods map 1:1 onto the C entry points."""

    def __init__(self, device=-1, flags=0, chunk=0, max_passes=0, rank=0, world_size=1, rccl_id=None, tune=()):
        self.lib = load(experiments=needs_experiments_build(tune))
        opt = HbOptions()
        opt.struct_size = ctypes.sizeof(HbOptions)
        opt.device = device
        opt.flags = flags
        opt.chunk = chunk
        opt.max_passes = max_passes
        opt.rank = rank
        opt.world_size = world_size
        if rccl_id is not None:
            ctypes.memmove(opt.rccl_id, bytes(rccl_id), 128)
        for i, v in enumerate(tune):
            opt.tune[i] = int(v)
        h = ctypes.c_void_p()
        rc = self.lib.hb_create(ctypes.byref(opt), ctypes.byref(h))
        if rc != HB_OK:
            raise HyperballError(rc, (self.lib.hb_last_error(None) or b"").decode())
        self.h = h
        self._keep = []

    # -- plumbing
    def _check(self, rc):
        if rc != HB_OK:
            raise HyperballError(rc, (self.lib.hb_last_error(self.h) or b"").decode())

    def _call(self, fn, opt, stats_cls):
        """an operator: both struct_size fields, the call, the check; the stats as a dict"""
        opt.struct_size = ctypes.sizeof(opt)
        st = stats_cls()
        st.struct_size = ctypes.sizeof(st)
        self._check(fn(self.h, ctypes.byref(opt), ctypes.byref(st)))
        return st.as_dict()

    @staticmethod
    def _u128_arg(a, empty_len):
        """a list of node ids as a contiguous U128 array; an empty (or absent) one as `empty_len` zeroed entries to point at"""
        return np.ascontiguousarray(a, dtype=U128) if a is not None and len(a) else np.zeros(empty_len, dtype=U128)

    def _count(self, fn):
        k = ctypes.c_uint64(0)
        self._check(fn(self.h, ctypes.byref(k)))
        return k.value

    def _pairs(self, count_fn, copy_fn, dtype):
        """a compacted result: (ids U128, values `dtype`), as many as count_fn says"""
        k = self._count(count_fn)
        ids = np.zeros(k, dtype=U128)
        vals = np.zeros(k, dtype=dtype)
        self._check(copy_fn(self.h, _ptr(ids), _ptr(vals), k))
        return ids, vals

    def _per_node(self, fn, dtype, fill):
        """one value per node, ascending NodeID; `fill` = what a node without a value keeps"""
        out = np.full(self.n(), fill, dtype=dtype)
        self._check(fn(self.h, _ptr(out), len(out)))
        return out

    def _top(self, fn, k, *extra):
        """the first k entries of a ranking: (ids, float64 values), as many as the library wrote"""
        k = int(k)
        ids = np.zeros(k, dtype=U128)
        vals = np.zeros(k, dtype=np.float64)
        w = ctypes.c_uint64(0)
        self._check(fn(self.h, k, *extra, _ptr(ids), _ptr(vals), ctypes.byref(w)))
        return ids[:w.value], vals[:w.value]

    def close(self):
        if getattr(self, "h", None):
            self.lib.hb_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- input
    def load_edges(self, edges, node_ids=None):
        edges = np.ascontiguousarray(edges, dtype=EDGE)
        n = 0
        if node_ids is not None:
            node_ids = np.ascontiguousarray(node_ids, dtype=U128)
            n = len(node_ids)
        self._check(self.lib.hb_load_edges(self.h, _ptr(node_ids), n, _ptr(edges), len(edges)))

    def append_edges(self, edges):
        edges = np.ascontiguousarray(edges, dtype=EDGE)
        self._check(self.lib.hb_append_edges(self.h, _ptr(edges), len(edges)))

    def load_tail_edges(self, records):
        """HB_FLAG_REFERENCE_TAIL: the page-level records update_changed_counters follows (harmonic.rs:82-92)."""
        records = np.ascontiguousarray(records, dtype=EDGE)
        self._check(self.lib.hb_load_tail_edges(self.h, _ptr(records) if len(records) else None, len(records)))

    def append_tail_edges(self, records):
        records = np.ascontiguousarray(records, dtype=EDGE)
        self._check(self.lib.hb_append_tail_edges(self.h, _ptr(records) if len(records) else None, len(records)))

    def h2d_rate(self, host_array, reps=3):
        """GB/s at which this host buffer reaches the device through the library's stream (hb_debug_h2d_rate)."""
        g = ctypes.c_double(0.0)
        self._check(self.lib.hb_debug_h2d_rate(self.h, _ptr(host_array), host_array.nbytes, reps, ctypes.byref(g)))
        return g.value

    def set_ingest_limits(self, max_records=0, max_device_bytes=0, chunk_records=0):
        """Test hook (hb_debug_set_ingest_limits): reach the device ingest's refusal / spill / multi-chunk paths with small inputs."""
        self._check(self.lib.hb_debug_set_ingest_limits(self.h, max_records, max_device_bytes, chunk_records))

    def tail_segment_end(self):
        """The tail records appended since the last call were one whole segment of the store (doc order)."""
        self._check(self.lib.hb_tail_segment_end(self.h))

    def finalize(self, node_ids=None):
        n = 0
        if node_ids is not None:
            node_ids = np.ascontiguousarray(node_ids, dtype=U128)
            n = len(node_ids)
        self._check(self.lib.hb_finalize(self.h, _ptr(node_ids), n))

    def load_dense(self, sorted_ids, row_ptr, src):
        sorted_ids = np.ascontiguousarray(sorted_ids, dtype=U128)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        src = np.ascontiguousarray(src, dtype=np.uint32)
        assert len(row_ptr) == len(sorted_ids) + 1
        self._check(self.lib.hb_load_dense(self.h, _ptr(sorted_ids), len(sorted_ids), _ptr(row_ptr), _ptr(src), len(src)))

    # -- compute
    def run(self):
        st = HbStats()
        self._check(self.lib.hb_run(self.h, ctypes.byref(st)))
        return st.as_dict()

    def begin(self):
        self._check(self.lib.hb_begin(self.h))

    def step(self):
        has = ctypes.c_int(0)
        self._check(self.lib.hb_step(self.h, ctypes.byref(has)))
        return bool(has.value)

    def step_local(self):
        self._check(self.lib.hb_step_local(self.h))

    def step_finish(self):
        has = ctypes.c_int(0)
        self._check(self.lib.hb_step_finish(self.h, ctypes.byref(has)))
        return bool(has.value)

    @staticmethod
    def exchange(ctxs, phase=0):
        """Emulated collective between logical ranks on one device (hb_debug_exchange)."""
        arr = (ctypes.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        ctxs[0]._check(ctxs[0].lib.hb_debug_exchange(arr, len(ctxs), phase))

    def set_all_to_all(self, callback):
        """hb_set_all_to_all: `callback` is a ctypes function pointer (ALL_TO_ALL_FN) the caller keeps alive, or None."""
        self._check(self.lib.hb_set_all_to_all(self.h, ctypes.cast(callback, ctypes.c_void_p) if callback is not None else None))

    def wire6(self, rows=None, pieces=1, count=None):
        """hb_debug_wire6: the three kernels of HB_FLAG_PACKED_WIRE on `rows` (pieces x count x 64 uint8, or pieces * count rows of 64):
        pack, register-wise maximum over the pieces in packed form, unpack.  Returns (packed_max count x 48, rows_out count x 64,
        (ms_pack, ms_max, ms_unpack)).  rows=None: every piece is the context's resident counters (`count` rows of them, after
        begin()); nothing is uploaded or downloaded and both arrays are None."""
        ms = (ctypes.c_float * 3)()
        if rows is None:
            self._check(self.lib.hb_debug_wire6(self.h, None, int(count), int(pieces), None, None, ms))
            return None, None, tuple(ms)
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 64)
        assert len(rows) % pieces == 0
        count = len(rows) // pieces
        packed = np.zeros((count, 48), dtype=np.uint8)
        out = np.zeros((count, 64), dtype=np.uint8)
        self._check(self.lib.hb_debug_wire6(self.h, _ptr(rows), count, int(pieces), _ptr(packed), _ptr(out), ms))
        return packed, out, tuple(ms)

    def finish(self):
        self._check(self.lib.hb_finish(self.h))

    def stats(self):
        st = HbStats()
        self._check(self.lib.hb_get_stats(self.h, ctypes.byref(st)))
        return st.as_dict()

    def pass_stats(self):
        out = []
        t = 0
        while True:
            ps = HbPassStats()
            if self.lib.hb_get_pass_stats(self.h, t, ctypes.byref(ps)) != HB_OK:
                break
            out.append(ps.as_dict())
            t += 1
        return out

    def synchronize(self):
        self._check(self.lib.hb_device_synchronize(self.h))

    def device_name(self):
        buf = ctypes.create_string_buffer(64)
        self._check(self.lib.hb_device_name(self.h, buf, 64))
        return buf.value.decode()

    # -- sampled harmonic centrality (ApproxHarmonic::build, approx_harmonic.rs:40-89)
    def sampled_harmonic(self, seed=0, samples=0, num_nodes=0, max_dist=0, epsilon=0.0, sources=None):
        """hb_sampled_harmonic: the results (results / ranks / top / store_harmonic) become the sampled values; returns hb_sample_stats.
        sources: U128 array of node ids (None = the seeded sampler)."""
        o = HbSampleOptions()
        o.max_dist, o.seed, o.samples, o.num_nodes, o.epsilon = int(max_dist), int(seed), int(samples), int(num_nodes), float(epsilon)
        if sources is not None:
            # (an empty list stays a list: the library refuses sources with source_count == 0 instead of sampling)
            count = len(sources)
            sources = self._u128_arg(sources, 1)
            o.sources = sources.ctypes.data
            o.source_count = count
        self._sample_levels = 0
        st = self._call(self.lib.hb_sampled_harmonic, o, HbSampleStats)
        self._sample_levels = st["levels"]
        return st

    def sample_sources(self, seed, k):
        """hb_sample_sources: the sorted node ids the seeded sampler picks for (seed, k)."""
        w = ctypes.c_uint64(0)
        self._check(self.lib.hb_sample_sources(self.h, int(seed), int(k), None, ctypes.byref(w)))
        out = np.zeros(w.value, dtype=U128)
        self._check(self.lib.hb_sample_sources(self.h, int(seed), int(k), _ptr(out), ctypes.byref(w)))
        return out[:w.value]

    def sample_histogram(self):
        """c_d per node of the last sampled run: (n, D) uint16, ascending NodeID, D = max_dist + 1 of that run."""
        levels = getattr(self, "_sample_levels", 0)
        if not levels:
            raise HyperballError(HB_ERR_INVALID, "no sampled result (call sampled_harmonic first)")
        out = np.zeros((self.n(), int(levels)), dtype=np.uint16)
        self._check(self.lib.hb_debug_sample_histogram(self.h, _ptr(out)))
        return out

    # -- exact shortest-path distances (ShortestPaths, shortest_path.rs:26-227)
    _DIST_MODES = {None: 0, "auto": 0, "top_down": HB_DIST_TOP_DOWN_ONLY, "bottom_up": HB_DIST_BOTTOM_UP_ONLY}

    def _distances(self, sources, reversed, max_dist, mode, flags):
        o = HbDistanceOptions()
        o.flags = int(flags) | (HB_DIST_REVERSED if reversed else 0) | self._DIST_MODES[mode]
        if max_dist is not None:
            o.flags |= HB_DIST_WITH_MAX
            o.max_dist = int(max_dist)
        count = len(sources)
        sources = self._u128_arg(sources, 1)
        o.sources = sources.ctypes.data
        o.source_count = count
        return self._call(self.lib.hb_distances, o, HbDistanceStats)

    def distance_count(self):
        return self._count(self.lib.hb_distance_count)

    def distance_copy(self):
        """The reached nodes of the last distances() call: (ids ascending, dist uint8)."""
        return self._pairs(self.lib.hb_distance_count, self.lib.hb_distance_copy, np.uint8)

    def distance_all(self):
        """One byte per node of the last distances() call, ascending NodeID; HB_DIST_UNREACHED = no distance."""
        return self._per_node(self.lib.hb_distance_all, np.uint8, HB_DIST_UNREACHED)

    def distances(self, sources, reversed=False, max_dist=None, mode=None, flags=0):
        """hb_distances from `sources` (U128 array of node ids): (ids, dist, stats) - the reached nodes in ascending NodeID order with
        their distances (dijkstra_multi's map).  reversed: distances TO the sources; max_dist: None = run to exhaustion, else the
        *_with_max methods' bound (nodes up to max_dist + 1 are reported); mode: None / "top_down" / "bottom_up" (forced step, same result)."""
        st = self._distances(sources, reversed, max_dist, mode, flags)
        ids, dist = self.distance_copy()
        return ids, dist, st

    def distances_all(self, sources, reversed=False, max_dist=None, mode=None, flags=0):
        """The same call; the result as one byte per node (ascending NodeID, 255 = unreached): (dist, stats)."""
        st = self._distances(sources, reversed, max_dist, mode, flags)
        return self.distance_all(), st

    # -- exact betweenness centrality (Betweenness, centrality/betweenness.rs:29-172)
    _BC_MODES = {None: 0, "auto": 0, "dense": HB_BC_DENSE_ONLY, "sparse": HB_BC_SPARSE_ONLY}

    def _betweenness(self, sources, raw, mode, flags=0):
        o = HbBetweennessOptions()
        o.flags = int(flags) | (HB_BC_RAW if raw else 0) | self._BC_MODES[mode]
        if sources is not None:
            count = len(sources)
            sources = self._u128_arg(sources, 1)
            o.sources = sources.ctypes.data
            o.source_count = count
        return self._call(self.lib.hb_betweenness, o, HbBetweennessStats)

    def betweenness_count(self):
        return self._count(self.lib.hb_betweenness_count)

    def betweenness_copy(self):
        """The results of the last betweenness() call: (ids ascending, values float64)."""
        return self._pairs(self.lib.hb_betweenness_count, self.lib.hb_betweenness_copy, np.float64)

    def betweenness_all(self):
        """One float64 per node of the last betweenness() call, ascending NodeID; -1.0 = no result."""
        return self._per_node(self.lib.hb_betweenness_all, np.float64, -1.0)

    def betweenness(self, sources=None, raw=False, mode=None, flags=0):
        """hb_betweenness from `sources` (U128 array of node ids; None = every node of a graph of at most 100 000): (ids, vals, stats) -
        the sources and every node one of them reaches, ascending NodeID, with sum / (S (S - 1)) (raw: the sum itself); mode: None /
        "dense" / "sparse" (forced kind of forward level)."""
        st = self._betweenness(sources, raw, mode, flags)
        ids, vals = self.betweenness_copy()
        return ids, vals, st

    def debug_betweenness_batch(self):
        """dist (n, 8) uint8, sigma (n, 8) uint64, delta (n, 8) float64 of the LAST batch of the last betweenness() call, ascending NodeID;
        lane = position of the source within the batch."""
        n = self.n()
        dist = np.full((n, 8), 255, dtype=np.uint8)
        sigma = np.zeros((n, 8), dtype=np.uint64)
        delta = np.zeros((n, 8), dtype=np.float64)
        self._check(self.lib.hb_debug_copy_betweenness_batch(self.h, _ptr(dist), _ptr(sigma), _ptr(delta)))
        return dist, sigma, delta

    # -- inbound similarity (Scorer, ranking/inbound_similarity.rs:61-138)
    _SIM_MODES = {None: 0, "auto": 0, "dense": HB_SIM_DENSE_ONLY, "sparse": HB_SIM_SPARSE_ONLY}

    def inbound_similarity(self, liked=(), disliked=(), normalized=False, self_score=None, mode=None, flags=0, limit=0):
        """hb_inbound_similarity: scores every node against `liked` / `disliked` (U128 arrays of node ids, duplicates and unknown ids
        allowed); returns the stats.  mode: None / "dense" / "sparse" (forced kind of count level).  limit: 0 = whole in-lists,
        1 .. 1024 = every BitVec from the `limit` best backlinks under the current key set (links_set_keys); the reference uses 512."""
        o = HbSimilarityOptions()
        o.limit = int(limit)
        o.flags = int(flags) | (HB_SIM_NORMALIZED if normalized else 0) | self._SIM_MODES[mode]
        if self_score is not None:
            o.flags |= HB_SIM_SELF_SCORE
            o.self_score = float(self_score)
        liked, disliked = self._u128_arg(liked, 0), self._u128_arg(disliked, 0)
        if len(liked):
            o.liked = liked.ctypes.data
            o.liked_count = len(liked)
        if len(disliked):
            o.disliked = disliked.ctypes.data
            o.disliked_count = len(disliked)
        return self._call(self.lib.hb_inbound_similarity, o, HbSimilarityStats)

    def similarity_all(self):
        """One float64 per node of the last inbound_similarity() call, ascending NodeID."""
        return self._per_node(self.lib.hb_similarity_all, np.float64, 0)

    def similarity_lookup(self, ids):
        """Scorer::score of the given hosts (U128 array); an id that is no node gets the score of an empty BitVec."""
        ids = np.ascontiguousarray(ids, dtype=U128)
        out = np.zeros(len(ids), dtype=np.float64)
        self._check(self.lib.hb_similarity_lookup(self.h, _ptr(ids) if len(ids) else None, len(ids), _ptr(out) if len(ids) else None))
        return out

    def similarity_top(self, k, skip_anchors=False):
        """The k best nodes of the last inbound_similarity() call: (ids, scores), score descending, ties by NodeID descending."""
        return self._top(self.lib.hb_similarity_top, k, HB_SIM_TOP_SKIP_ANCHORS if skip_anchors else 0)

    def debug_similarity_batch(self):
        """counts (n, 16) uint32 of the LAST batch of the last inbound_similarity() call, and the per-graph bloom masks (n) uint64 and
        in-degrees (n) uint32, ascending NodeID; after a limited call: those of the cut lists."""
        n = self.n()
        counts = np.zeros((n, 16), dtype=np.uint32)
        bloom = np.zeros(n, dtype=np.uint64)
        length = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.hb_debug_copy_similarity_batch(self.h, _ptr(counts), _ptr(bloom), _ptr(length)))
        return counts, bloom, length

    # -- nearest-seed centrality (HarmonicNearestSeed, entrypoint/centrality.rs:126-201)
    def nearest_seed(self, orig_ids=None, orig_vals=None, key_ids=None, keys=None, discount_factor=0.5, rounds=0, from_image=False, flags=0):
        """hb_nearest_seed: every node without an original value takes discount_factor x the value of its seed (the in-neighbour with
        the smallest (key, NodeID)); returns the stats.  orig_ids / orig_vals: the original centralities (U128 / float64 arrays), or
        from_image=True for the context's live result; key_ids / keys: the order keys (U128 / uint64), unlisted nodes have 2^64 - 1."""
        o = HbNearestSeedOptions()
        o.flags = int(flags) | (HB_SEED_FROM_IMAGE if from_image else 0)
        o.discount_factor = float(discount_factor)
        o.rounds = int(rounds)
        if orig_ids is not None and len(orig_ids):
            orig_ids = np.ascontiguousarray(orig_ids, dtype=U128)
            orig_vals = np.ascontiguousarray(orig_vals, dtype=np.float64)
            if len(orig_ids) != len(orig_vals):
                raise ValueError("orig_ids and orig_vals differ in length")
            o.orig_ids, o.orig_vals, o.orig_count = orig_ids.ctypes.data, orig_vals.ctypes.data, len(orig_ids)
        if key_ids is not None and len(key_ids):
            key_ids = np.ascontiguousarray(key_ids, dtype=U128)
            keys = np.ascontiguousarray(keys, dtype=np.uint64)
            if len(key_ids) != len(keys):
                raise ValueError("key_ids and keys differ in length")
            o.key_ids, o.keys, o.key_count = key_ids.ctypes.data, keys.ctypes.data, len(key_ids)
        return self._call(self.lib.hb_nearest_seed, o, HbNearestSeedStats)

    def nearest_seed_count(self):
        return self._count(self.lib.hb_nearest_seed_count)

    def nearest_seed_copy(self):
        """The results of the last nearest_seed() call: (ids ascending, values float64)."""
        return self._pairs(self.lib.hb_nearest_seed_count, self.lib.hb_nearest_seed_copy, np.float64)

    def nearest_seed_all(self):
        """One float64 per node of the last nearest_seed() call, ascending NodeID; -1.0 = no result."""
        return self._per_node(self.lib.hb_nearest_seed_all, np.float64, -1.0)

    def nearest_seed_top(self, k):
        """The k best results of the last nearest_seed() call: (ids, values), value descending, ties by NodeID ASCENDING."""
        return self._top(self.lib.hb_nearest_seed_top, k)

    def nearest_seed_seeds(self):
        """seed(v) of every node of the last nearest_seed() call, ascending NodeID: (ids U128, has_seed bool)."""
        n = self.n()
        seed = np.zeros(n, dtype=U128)
        has = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.hb_nearest_seed_seeds(self.h, _ptr(seed), _ptr(has), n))
        return seed, has.astype(bool)

    # -- limited, rank-ordered host backlinks (HostBacklinksQuery .. Limit(L), webgraph/query/backlink.rs:230-360)
    def links_set_keys(self, key_ids=None, keys=None, from_ranks=False, flags=0):
        """hb_links_set_keys: the order keys of the backlink lists (U128 / uint64 arrays; unlisted nodes have 2^64 - 1), or
        from_ranks=True for the harmonic ranks of the context's live result; builds the dense order on the device.  Returns the stats."""
        o = HbLinksKeyOptions()
        o.flags = int(flags) | (HB_LINKS_KEYS_FROM_RANKS if from_ranks else 0)
        if key_ids is not None and len(key_ids):
            key_ids = np.ascontiguousarray(key_ids, dtype=U128)
            keys = np.ascontiguousarray(keys, dtype=np.uint64)
            if len(key_ids) != len(keys):
                raise ValueError("key_ids and keys differ in length")
            o.key_ids, o.keys, o.key_count = key_ids.ctypes.data, keys.ctypes.data, len(key_ids)
        return self._call(self.lib.hb_links_set_keys, o, HbLinksKeyStats)

    def backlinks(self, nodes, limit, flags=0, slots_per_batch=0):
        """hb_backlinks: the first `limit` in-neighbours of every node of `nodes` (U128 array) in the order (key, NodeID); returns the
        stats, links_copy() the lists."""
        return self._links_query(self.lib.hb_backlinks, nodes, limit, flags, slots_per_batch)

    def forwardlinks(self, nodes, limit, flags=0, slots_per_batch=0):
        """hb_forwardlinks (HostForwardlinksQuery .. Limit(L), webgraph/query/forwardlink.rs:183-330): the first `limit` out-neighbours
        of every node of `nodes` (U128 array) in the order (key, NodeID); returns the stats, links_copy() the lists."""
        return self._links_query(self.lib.hb_forwardlinks, nodes, limit, flags, slots_per_batch)

    def _links_query(self, call, nodes, limit, flags, slots_per_batch):
        o = HbLinksOptions()
        o.flags = int(flags)
        nodes = np.ascontiguousarray(nodes, dtype=U128)
        if len(nodes):
            o.nodes, o.node_count = nodes.ctypes.data, len(nodes)
        o.limit = int(limit)
        o.slots_per_batch = int(slots_per_batch)
        return self._call(call, o, HbLinksStats)

    def links_count(self):
        """(queries, entries) of the last backlinks() / forwardlinks() call"""
        q, e = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.lib.hb_links_count(self.h, ctypes.byref(q), ctypes.byref(e)))
        return q.value, e.value

    def links_copy(self, ids=True, keys=True):
        """The lists of the last backlinks() / forwardlinks() call: (offsets uint64 [queries + 1], ids U128, keys uint64, degrees uint64); query i's list
        is ids[offsets[i]:offsets[i + 1]], in (key, NodeID) order.  ids=False / keys=False leaves that array on the device (None)."""
        q, e = self.links_count()
        offsets = np.zeros(q + 1, dtype=np.uint64)
        degrees = np.zeros(q, dtype=np.uint64)
        out_ids = np.zeros(e, dtype=U128) if ids else None
        out_keys = np.zeros(e, dtype=np.uint64) if keys else None
        self._check(self.lib.hb_links_copy(self.h, _ptr(offsets), _ptr(degrees), _ptr(out_ids) if ids else None, _ptr(out_keys) if keys else None, e))
        return offsets, out_ids, out_keys, degrees

    # -- similar hosts (scored_nodes of SimilarHostsFinder::find_similar_hosts, similar_hosts.rs:54-272)
    def similar_hosts(self, nodes, limit, flags=0):
        """hb_similar_hosts: the `limit` hosts most similar to the liked hosts `nodes` (U128 array, caller order; duplicates and unknown
        ids count); returns the stats, similar_copy() the list, similar_candidates() the co-citation pre-selection."""
        o = HbSimilarOptions()
        o.flags = int(flags)
        nodes = np.ascontiguousarray(nodes, dtype=U128)
        if len(nodes):
            o.nodes, o.node_count = nodes.ctypes.data, len(nodes)
        o.limit = int(limit)
        return self._call(self.lib.hb_similar_hosts, o, HbSimilarStats)

    def similar_copy(self):
        """(ids U128, scores float64) of the last similar_hosts() call, best first"""
        return self._pairs(self.lib.hb_similar_count, self.lib.hb_similar_copy, np.float64)

    def similar_candidates(self):
        """(ids U128, counts uint64): the pre-selection of the last similar_hosts() call after the liked hosts were dropped, in its order"""
        w = ctypes.c_uint64(0)
        self._check(self.lib.hb_similar_candidates(self.h, None, None, 0, ctypes.byref(w)))
        ids = np.zeros(w.value, dtype=U128)
        counts = np.zeros(w.value, dtype=np.uint64)
        self._check(self.lib.hb_similar_candidates(self.h, _ptr(ids), _ptr(counts), w.value, ctypes.byref(w)))
        return ids, counts

    # -- scoring result hosts (Scorer::score per search, ranking/pipeline/scorers/inbound_similarity.rs:38-54)
    def score_hosts(self, requests, limit=512, flags=0, slots_per_batch=0, small_pieces=False):
        """hb_score_hosts: every request is a dict with `nodes` (the result hosts, U128 array, scored in this order) and optionally
        `liked`, `disliked` (U128 arrays; duplicates and unknown ids count), `normalized`, `self_score`.  limit: 1 .. 1024 backlinks
        per BitVec under the current key set (the reference: 512).  Returns the stats; score_copy() the scores."""
        keep = []  # (the arrays the request structs point into)

        def arr(a):
            a = self._u128_arg(a, 0)
            keep.append(a)
            return (a.ctypes.data if len(a) else None), len(a)

        reqs = (HbScoreRequest * max(len(requests), 1))()
        for q, r in zip(reqs, requests):
            q.liked, q.liked_count = arr(r.get("liked"))
            q.disliked, q.disliked_count = arr(r.get("disliked"))
            q.nodes, q.node_count = arr(r.get("nodes"))
            q.flags = HB_SIM_NORMALIZED if r.get("normalized") else 0
            if r.get("self_score") is not None:
                q.flags |= HB_SIM_SELF_SCORE
                q.self_score = float(r["self_score"])
        o = HbScoreOptions()
        o.flags = int(flags) | (HB_SCORE_SMALL_PIECES if small_pieces else 0)
        if len(requests):
            o.requests, o.request_count = reqs, len(requests)
        o.limit = int(limit)
        o.slots_per_batch = int(slots_per_batch)
        return self._call(self.lib.hb_score_hosts, o, HbScoreStats)

    def score_copy(self):
        """The scores of the last score_hosts() call: one float64 array per request, in request order, one value per node entry"""
        r, k = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.lib.hb_score_count(self.h, ctypes.byref(r), ctypes.byref(k)))
        offsets = np.zeros(r.value + 1, dtype=np.uint64)
        scores = np.zeros(k.value, dtype=np.float64)
        self._check(self.lib.hb_score_copy(self.h, _ptr(offsets), _ptr(scores), k.value))
        return [scores[int(offsets[i]):int(offsets[i + 1])].copy() for i in range(r.value)]

    # -- results
    def results(self):
        return self._pairs(self.lib.hb_result_count, self.lib.hb_result_copy, np.float64)

    def ranks(self):
        """harmonic_rank of every result (store_harmonic order), aligned with results()."""
        out = np.zeros(self._count(self.lib.hb_result_count), dtype=np.uint64)
        self._check(self.lib.hb_result_ranks(self.h, _ptr(out), len(out)))
        return out

    def store_harmonic(self, output):
        """store_harmonic (centrality/mod.rs:72-114) from the results this context holds; key order sorted on the device."""
        err = ctypes.create_string_buffer(512)
        rc = self.lib.hb_store_harmonic_results(self.h, os.fsencode(output), err, len(err))
        if rc != HB_OK:
            raise HyperballError(rc, err.value.decode(errors="replace"))

    def top(self, k):
        """top_nodes(TopNodes::Top(k)) (centrality/mod.rs:33-52): (ids, vals), largest centrality first."""
        return self._top(self.lib.hb_result_top, min(int(k), self._count(self.lib.hb_result_count)))

    # -- debug exports
    def n(self):
        return self.stats()["n"]

    def registers(self):
        out = np.zeros((self.n(), 64), dtype=np.uint8)
        self._check(self.lib.hb_debug_copy_registers(self.h, _ptr(out)))
        return out

    def kahan(self):
        n = self.n()
        s = np.zeros(n, dtype=np.float64)
        e = np.zeros(n, dtype=np.float64)
        self._check(self.lib.hb_debug_copy_kahan(self.h, _ptr(s), _ptr(e)))
        return s, e

    def sizes(self):
        out = np.zeros(self.n(), dtype=np.uint64)
        self._check(self.lib.hb_debug_copy_sizes(self.h, _ptr(out)))
        return out

    def state_hash(self):
        """(registers checksum, Kahan checksum) of the current state (hb_debug_state_hash)."""
        out = np.zeros(2, dtype=np.uint64)
        self._check(self.lib.hb_debug_state_hash(self.h, _ptr(out)))
        return int(out[0]), int(out[1])

    def hll_size(self, regs):
        regs = np.ascontiguousarray(regs, dtype=np.uint8).reshape(-1, 64)
        out = np.zeros(len(regs), dtype=np.uint64)
        self._check(self.lib.hb_debug_hll_size(self.h, _ptr(regs), len(regs), _ptr(out)))
        return out

    def plan(self):
        """The device work layout as it lies in HBM (hb_debug_copy_plan), same dict as host_plan()."""
        sizes = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.hb_debug_copy_plan(self.h, _ptr(sizes), None, None, None, None))
        n_pad, nv, slen, levels = (int(x) for x in sizes)
        order = np.zeros(n_pad, dtype=np.uint32)
        prp = np.zeros(n_pad + nv + 1, dtype=np.uint64)
        psrc = np.zeros(slen, dtype=np.uint32)
        lb = np.zeros(levels + 1, dtype=np.uint64)
        self._check(self.lib.hb_debug_copy_plan(self.h, _ptr(sizes), _ptr(order), _ptr(prp), _ptr(psrc), _ptr(lb)))
        return dict(order=order, row_ptr=prp, src=psrc, level_begin=lb, n_pad=n_pad, nv=nv)

    def plan_live(self):
        """(live-first order in use, n_live, n_live_pad) of the loaded graph's layout (hb_debug_plan_live)."""
        out = np.zeros(3, dtype=np.uint64)
        self._check(self.lib.hb_debug_plan_live(self.h, _ptr(out)))
        return bool(out[0]), int(out[1]), int(out[2])

    def saturation(self):
        """(skipping in use, U[64], node bits[n] in input order, hub-chunk bits[nv] in plan order) of the run in progress
        (hb_debug_saturation); (False, None, None, None) for a context that does not skip saturated rows."""
        info = np.zeros(5, dtype=np.uint64)
        self._check(self.lib.hb_debug_saturation(self.h, _ptr(info), None, None, None))
        if not info[0]:
            return False, None, None, None
        u = np.zeros(64, dtype=np.uint8)
        node = np.zeros(int(info[1]), dtype=np.uint8)
        virt = np.zeros(int(info[2]), dtype=np.uint8)
        self._check(self.lib.hb_debug_saturation(self.h, _ptr(info), _ptr(u), _ptr(node), _ptr(virt)))
        return True, u, node.astype(bool), virt.astype(bool)

    def early_exit(self):
        """(the last dense pass ran the early-exit instances, work rows of that pass that left their gather loop early)
        (hb_debug_saturation)"""
        info = np.zeros(5, dtype=np.uint64)
        self._check(self.lib.hb_debug_saturation(self.h, _ptr(info), None, None, None))
        return bool(info[4]), int(info[3])

    def graph(self):
        st = self.stats()
        ids = np.zeros(st["n"], dtype=U128)
        row_ptr = np.zeros(st["n"] + 1, dtype=np.uint64)
        src = np.zeros(st["m_eff"], dtype=np.uint32)
        self._check(self.lib.hb_debug_copy_graph(self.h, _ptr(ids), _ptr(row_ptr), _ptr(src)))
        return ids, row_ptr, src


def rccl_unique_id():
    buf = (ctypes.c_uint8 * 128)()
    rc = load().hb_rccl_unique_id(buf)
    if rc != HB_OK:
        raise HyperballError(rc, (load().hb_last_error(None) or b"").decode())
    return bytes(buf)


def host_ingest(edges, node_ids=None):
    """Host-only: the reference's node/edge-set semantics (no device needed).
    Returns (ids, row_ptr, src, m_unique)."""
    lib = load()
    edges = np.ascontiguousarray(edges, dtype=EDGE)
    nn = 0
    if node_ids is not None:
        node_ids = np.ascontiguousarray(node_ids, dtype=U128)
        nn = len(node_ids)
    n, mu, me = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib.hb_host_ingest(_ptr(node_ids), nn, _ptr(edges), len(edges), ctypes.byref(n), ctypes.byref(mu),
                            ctypes.byref(me), None, None, None)
    if rc != HB_OK:
        raise HyperballError(rc, (lib.hb_last_error(None) or b"").decode())
    ids = np.zeros(n.value, dtype=U128)
    row_ptr = np.zeros(n.value + 1, dtype=np.uint64)
    src = np.zeros(me.value, dtype=np.uint32)
    rc = lib.hb_host_ingest(_ptr(node_ids), nn, _ptr(edges), len(edges), ctypes.byref(n), ctypes.byref(mu),
                            ctypes.byref(me), _ptr(ids), _ptr(row_ptr), _ptr(src))
    if rc != HB_OK:
        raise HyperballError(rc, (lib.hb_last_error(None) or b"").decode())
    return ids, row_ptr, src, mu.value


def host_plan(row_ptr, src, flags=0, chunk=0, tune=()):
    """Host-only: the device work layout (order, plan_row_ptr, plan_src, level_begin, n_pad)."""
    lib = load()
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    src = np.ascontiguousarray(src, dtype=np.uint32)
    n = len(row_ptr) - 1
    sizes = np.zeros(4, dtype=np.uint64)
    tn = np.zeros(8, dtype=np.uint32)
    tn[:len(tune)] = tune
    rc = lib.hb_host_plan(n, _ptr(row_ptr), _ptr(src), flags, chunk, _ptr(tn), _ptr(sizes), None, None, None, None)
    if rc != HB_OK:
        raise HyperballError(rc, (lib.hb_last_error(None) or b"").decode())
    n_pad, nv, slen, levels = (int(x) for x in sizes)
    order = np.zeros(n_pad, dtype=np.uint32)
    prp = np.zeros(n_pad + nv + 1, dtype=np.uint64)
    psrc = np.zeros(slen, dtype=np.uint32)
    lb = np.zeros(levels + 1, dtype=np.uint64)
    rc = lib.hb_host_plan(n, _ptr(row_ptr), _ptr(src), flags, chunk, _ptr(tn), _ptr(sizes), _ptr(order), _ptr(prp),
                          _ptr(psrc), _ptr(lb))
    if rc != HB_OK:
        raise HyperballError(rc, (lib.hb_last_error(None) or b"").decode())
    world = int(tn[7]) if tn[7] > 1 else 1
    if world == 1:
        order = order[:n]  # no padding rows inside: a permutation of the sids
    live = host_plan_live(row_ptr, src, flags, chunk, tune)
    return dict(order=order, row_ptr=prp, src=psrc, level_begin=lb, n_pad=n_pad, nv=nv, slice=n_pad // world,
                live_first=live[0], n_live=live[1], n_live_pad=live[2])


def host_plan_live(row_ptr, src, flags=0, chunk=0, tune=()):
    """Host-only: (live-first order in use, n_live, n_live_pad) of the host planner's layout, as Context.plan_live() gives them."""
    lib = load()
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    src = np.ascontiguousarray(src, dtype=np.uint32)
    tn = np.zeros(8, dtype=np.uint32)
    tn[:len(tune)] = tune
    live = np.zeros(3, dtype=np.uint64)
    rc = lib.hb_host_plan_live(len(row_ptr) - 1, _ptr(row_ptr), _ptr(src), flags, chunk, _ptr(tn), _ptr(live))
    if rc != HB_OK:
        raise HyperballError(rc, (lib.hb_last_error(None) or b"").decode())
    return bool(live[0]), int(live[1]), int(live[2])
