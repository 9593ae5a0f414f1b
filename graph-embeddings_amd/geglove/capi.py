"""ctypes declarations for libgeglove.so -- one entry per symbol of include/geglove.h.

No torch types cross this boundary: plain pointers and sizes only.  Loading the library
does not touch the GPU; every computing entry point fails with GE_ERR_HIP when no gfx950
device is present (there is no CPU fallback in the product).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libgeglove.so")

GE_OK, GE_ERR_ARG, GE_ERR_OOM, GE_ERR_HIP, GE_ERR_STATE, GE_ERR_OVERFLOW = 0, -1, -2, -3, -4, -5
GE_COST_GLOVE, GE_COST_PGLOVE = 0, 1
GE_OPT_ADAGRAD, GE_OPT_ADAM, GE_OPT_AMSGRAD = 0, 1, 2
GE_NORM_NONE, GE_NORM_UNITY, GE_NORM_COUNTS = 0, 1, 2
GE_MODE_HOGWILD, GE_MODE_DETERMINISTIC, GE_MODE_STRATIFIED = 0, 1, 2
GE_ARITH_JAVA, GE_ARITH_FP32 = 0, 1
GE_SHUFFLE_JAVA, GE_SHUFFLE_DEVICE, GE_SHUFFLE_NONE = 0, 1, 2
GE_HOT_AUTO, GE_HOT_NONE, GE_HOT_ALL = 0, 1, 2
GE_DTYPE_F32, GE_DTYPE_BF16 = 0, 1
GE_LAYOUT_FIXED_CUTS, GE_LAYOUT_PLAIN_LONG_ROWS, GE_LAYOUT_SEPARATE_TABLES, GE_LAYOUT_PACKED_RECORDS, GE_LAYOUT_FIRST_PLACEMENT = 1, 2, 4, 8, 16
GE_LAYOUT_HUB_TILES, GE_LAYOUT_NO_HUB_TILES = 32, 64
GE_LAYOUT_HUB_PANELS, GE_LAYOUT_NO_HUB_PANELS = 128, 256
GE_LAYOUT_DEEP_PANELS, GE_LAYOUT_NO_DEEP_PANELS = 512, 1024
GE_LAYOUT_DEEP_WALK, GE_LAYOUT_NO_DEEP_WALK = 2048, 4096
(GE_STATE_FOCUS, GE_STATE_CONTEXT, GE_STATE_FBIAS, GE_STATE_CBIAS, GE_STATE_GSQ_FOCUS,
 GE_STATE_GSQ_CONTEXT, GE_STATE_GSQ_FBIAS, GE_STATE_GSQ_CBIAS, GE_STATE_M2_FOCUS, GE_STATE_M2_CONTEXT,
 GE_STATE_M2_FBIAS, GE_STATE_M2_CBIAS) = range(12)
STATE_NAMES = ("focus", "context", "fbias", "cbias", "gsq_focus", "gsq_context", "gsq_fbias", "gsq_cbias")
M2_NAMES = ("m2_focus", "m2_context", "m2_fbias", "m2_cbias")
ALL_STATE_NAMES = STATE_NAMES + M2_NAMES

# every symbol include/geglove.h declares (tests check the library exports all of them)
SYMBOLS = (
    "ge_glove_cfg_default", "ge_glove_create", "ge_glove_epoch", "ge_glove_extract_f32",
    "ge_glove_extract_f64", "ge_glove_get_state", "ge_glove_set_state", "ge_glove_device_ptr",
    "ge_glove_epoch_order", "ge_glove_get_perm", "ge_glove_rng_state", "ge_glove_last_kernel_ms", "ge_glove_get_info", "ge_glove_tile_info", "ge_glove_panel_info", "ge_glove_destroy",
    "ge_bca_build", "ge_coo_get", "ge_coo_destroy", "ge_exchange_turn_bf16", "ge_glove_context_layout",
    "ge_local_group_create", "ge_local_group_destroy", "ge_local_group_abort", "ge_rccl_unique_id", "ge_rccl_selftest", "ge_sync_cfg_size", "ge_sync_create", "ge_sync_begin", "ge_sync_finish", "ge_sync_turn", "ge_sync_sync",
    "ge_sync_epoch", "ge_sync_hub_rows", "ge_sync_hub_exchange", "ge_sync_hub_exchange_live", "ge_sync_live_rows", "ge_sync_hub_plan", "ge_sync_replicate", "ge_sync_allreduce_f64", "ge_sync_destroy",
    "ge_sim_cfg_default", "ge_sim_cfg_size", "ge_sim_pattern_supported", "ge_similarity_pairs", "ge_sim_pairs_get", "ge_sim_pairs_destroy", "ge_copy_bandwidth", "ge_last_error", "ge_version", "ge_glove_cfg_size", "ge_glove_info_size", "ge_bca_cfg_size", "ge_device_count",
    "ge_pca_cfg_default", "ge_pca_cfg_size", "ge_pca_fit", "ge_glove_pca_fit", "ge_pca_from_moments", "ge_pca_get", "ge_pca_transform",
    "ge_glove_pca_transform", "ge_pca_last_kernel_ms", "ge_pca_destroy",
    "ge_nn_cfg_default", "ge_nn_cfg_size", "ge_nn_create", "ge_glove_nn_create", "ge_nn_query_rows", "ge_nn_query_vectors", "ge_nn_get",
    "ge_nn_last_kernel_ms", "ge_nn_destroy",
    "ge_synth_cfg_default", "ge_synth_cfg_size", "ge_synth_coo", "ge_coo_device", "ge_coo_synth_stats", "ge_glove_create_coo",
    "ge_glove_eval_create", "ge_glove_eval_run", "ge_eval_last_kernel_ms", "ge_eval_get", "ge_eval_destroy", "ge_holdout_mask",
    "ge_glove_set_arith", "ge_glove_get_arith",
    "ge_glove_rank_create", "ge_glove_rank_run", "ge_rank_last_kernel_ms", "ge_rank_last_phase_ms", "ge_rank_get", "ge_rank_summary_size", "ge_rank_destroy",
    "ge_kmeans_cfg_default", "ge_kmeans_cfg_size", "ge_kmeans_create", "ge_glove_kmeans_create", "ge_kmeans_set_centroids", "ge_kmeans_step",
    "ge_kmeans_run", "ge_kmeans_get", "ge_kmeans_last_kernel_ms", "ge_kmeans_destroy",
    "ge_glove_predict_create", "ge_glove_predict_run", "ge_predict_last_kernel_ms", "ge_predict_get", "ge_predict_destroy",
    "ge_fold_cfg_default", "ge_fold_cfg_size", "ge_glove_fold_create", "ge_glove_fold_run", "ge_fold_last_kernel_ms", "ge_fold_get",
    "ge_fold_destroy", "ge_foldin_mask",
    "ge_ivf_cfg_default", "ge_ivf_cfg_size", "ge_ivf_create", "ge_glove_ivf_create", "ge_ivf_query_rows", "ge_ivf_query_vectors", "ge_ivf_get",
    "ge_ivf_last_kernel_ms", "ge_ivf_destroy",
    "ge_classify_cfg_default", "ge_classify_cfg_size", "ge_classify_create", "ge_glove_classify_create", "ge_classify_set_weights",
    "ge_classify_eval", "ge_classify_run", "ge_classify_predict", "ge_classify_score", "ge_classify_get", "ge_classify_last_kernel_ms",
    "ge_classify_destroy",
    "ge_match_cfg_default", "ge_match_cfg_size", "ge_match_summary_size", "ge_match_create", "ge_glove_match_create", "ge_match_run",
    "ge_match_get", "ge_match_last_kernel_ms", "ge_match_destroy",
    "ge_align_cfg_default", "ge_align_cfg_size", "ge_align_summary_size", "ge_align_create", "ge_glove_align_create", "ge_align_run",
    "ge_align_get", "ge_align_last_kernel_ms", "ge_align_destroy",
)
GE_FOLD_FOCUS, GE_FOLD_CONTEXT = 0, 1
FOLD_SIDES = {"focus": GE_FOLD_FOCUS, "context": GE_FOLD_CONTEXT}
FOLD_SHUFFLES = {"none": GE_SHUFFLE_NONE, "device": GE_SHUFFLE_DEVICE, "java": GE_SHUFFLE_JAVA}
GE_NN_COSINE, GE_NN_DOT = 0, 1
NN_METRICS = {"cosine": GE_NN_COSINE, "dot": GE_NN_DOT}
GE_KM_COSINE, GE_KM_EUCLID = 0, 1
KM_METRICS = {"cosine": GE_KM_COSINE, "euclid": GE_KM_EUCLID}
GE_KM_INIT_KEY = 0x4B4D45414E53
GE_CLS_COSINE, GE_CLS_RAW = 0, 1
CLS_NORMALIZE = {"cosine": GE_CLS_COSINE, "none": GE_CLS_RAW}
GE_CLS_STOP_NONE, GE_CLS_STOP_GRADIENT, GE_CLS_STOP_MAXITER, GE_CLS_STOP_LINESEARCH = 0, 1, 2, 3
CLS_STOPS = ("none", "gradient", "maxiter", "linesearch")


class GloveCfg(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("dim", C.c_int32), ("nnz", C.c_int64),
                ("cost", C.c_int32), ("opt", C.c_int32), ("learning_rate", C.c_float),
                ("xmax", C.c_double), ("seed", C.c_int64), ("threads", C.c_int32),
                ("mode", C.c_int32), ("shuffle", C.c_int32), ("device", C.c_int32),
                ("stream", C.c_void_p), ("row_begin", C.c_int32), ("row_end", C.c_int32),
                ("hot_columns", C.c_int32), ("workers", C.c_int32), ("emb_dtype", C.c_int32),
                ("hot_theta", C.c_float), ("stale_budget", C.c_float), ("flush_every", C.c_int32),
                ("blocks_per_cu", C.c_int32), ("layout_flags", C.c_int32), ("strata", C.c_int32)]


class GloveInfo(C.Structure):
    _fields_ = [("group_width", C.c_int32), ("vector_width", C.c_int32), ("chunks_per_lane", C.c_int32),
                ("blocks", C.c_int32), ("groups_in_flight", C.c_int32), ("hot_columns", C.c_int32),
                ("hot_nonzeros", C.c_int64), ("hot_threshold", C.c_int64), ("chunks", C.c_int64), ("hub_chunks", C.c_int64),
                ("long_rows", C.c_int64), ("shared_chunks", C.c_int64), ("flush_min", C.c_int32), ("row_stride", C.c_int32),
                ("runs", C.c_int64), ("schedule_bytes", C.c_int64), ("placements", C.c_int32), ("placement_best_ms", C.c_float),
                ("placement_worst_ms", C.c_float), ("reserved_", C.c_int32), ("strata", C.c_int32), ("strata_path", C.c_int64)]


class Csr(C.Structure):
    _fields_ = [("num_vertices", C.c_int32), ("ptr", C.POINTER(C.c_int64)),
                ("idx", C.POINTER(C.c_int32)), ("weight", C.POINTER(C.c_float))]


class BcaCfg(C.Structure):
    _fields_ = [("alpha", C.c_double), ("epsilon", C.c_double), ("directed", C.c_int32),
                ("normalize", C.c_int32), ("device", C.c_int32), ("row_begin", C.c_int32),
                ("row_end", C.c_int32), ("table_slots", C.c_int64), ("pool_entries", C.c_int64)]


class SimCfg(C.Structure):
    _fields_ = [("method", C.c_int32), ("threshold", C.c_double), ("ngram", C.c_int32), ("smooth", C.c_double),
                ("distance", C.c_double), ("time", C.c_int32), ("pattern", C.c_char_p), ("upper_triangle", C.c_int32),
                ("device", C.c_int32), ("job_begin", C.c_int32), ("job_end", C.c_int32)]


class Strings(C.Structure):
    _fields_ = [("count", C.c_int32), ("offset", C.POINTER(C.c_int64)), ("units", C.POINTER(C.c_uint16))]


class ContextLayout(C.Structure):
    _fields_ = [("table", C.c_void_p), ("dtype", C.c_int32), ("hub_rows", C.c_void_p), ("hub_index", C.c_void_p),
                ("n_hub", C.c_int32), ("vocab_size", C.c_int32), ("dim", C.c_int32), ("row_stride", C.c_int32), ("accum", C.c_void_p),
                ("accum_stride", C.c_int32), ("bias", C.c_void_p), ("bias_stride", C.c_int32), ("accum_bias", C.c_void_p),
                ("accum_bias_stride", C.c_int32)]


TRANSPORT_START = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p))
TRANSPORT_WAIT = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p)
TRANSPORT_BCAST = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32)


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("start", TRANSPORT_START), ("wait", TRANSPORT_WAIT), ("broadcast", TRANSPORT_BCAST)]


class SyncCfg(C.Structure):
    _fields_ = [("world", C.c_int32), ("rank", C.c_int32), ("wire", C.c_int32), ("accum_every", C.c_int32),
                ("transport", C.POINTER(Transport)), ("rccl_id", C.c_void_p), ("local_group", C.c_void_p)]


class PcaCfg(C.Structure):
    _fields_ = [("variance", C.c_double), ("max_components", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p)]


class NnCfg(C.Structure):
    _fields_ = [("metric", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p)]


class KmeansCfg(C.Structure):
    _fields_ = [("metric", C.c_int32), ("k", C.c_int32), ("seed", C.c_uint64), ("device", C.c_int32), ("stream", C.c_void_p)]


class ClassifyCfg(C.Structure):
    _fields_ = [("normalize", C.c_int32), ("classes", C.c_int32), ("l2", C.c_double), ("tolerance", C.c_double), ("device", C.c_int32),
                ("stream", C.c_void_p)]


class ClassifySummary(C.Structure):
    _fields_ = [("count", C.c_int64), ("correct", C.c_int64), ("accuracy", C.c_double), ("macro_f1", C.c_double),
                ("tp", C.POINTER(C.c_int64)), ("fp", C.POINTER(C.c_int64)), ("fn", C.POINTER(C.c_int64))]


class IvfCfg(C.Structure):
    _fields_ = [("metric", C.c_int32), ("lists", C.c_int32), ("train_iterations", C.c_int32), ("seed", C.c_uint64),
                ("centroids", C.POINTER(C.c_float)), ("device", C.c_int32), ("stream", C.c_void_p)]


class MatchCfg(C.Structure):
    _fields_ = [("metric", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p)]


class MatchSummary(C.Structure):
    _fields_ = [("pairs", C.c_int64), ("components", C.c_int64), ("groups", C.c_int64), ("grouped_rows", C.c_int64), ("largest", C.c_int64)]


class AlignCfg(C.Structure):
    _fields_ = [("metric", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p)]


class AlignSummary(C.Structure):
    _fields_ = [("candidates", C.c_int64), ("assigned", C.c_int64), ("mutual", C.c_int64), ("sources_with_candidates", C.c_int64),
                ("targets_with_candidates", C.c_int64), ("ambiguous_sources", C.c_int64)]


class SynthCfg(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("row_begin", C.c_int32), ("row_end", C.c_int32), ("nnz", C.c_int64),
                ("seed", C.c_uint64), ("device", C.c_int32), ("stream", C.c_void_p)]


class RankSummary(C.Structure):
    _fields_ = [("n", C.c_int64), ("mrr", C.c_double), ("mean_rank", C.c_double), ("hits1", C.c_int64), ("hits10", C.c_int64),
                ("hits100", C.c_int64)]


class FoldCfg(C.Structure):
    _fields_ = [("side", C.c_int32), ("epochs", C.c_int32), ("shuffle", C.c_int32), ("learning_rate", C.c_float), ("seed", C.c_int64)]


class GeError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("geglove error %d: %s" % (status, message))
        self.status = status


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7) and its
    libraries ask for it by file name, so they load it even when /opt/rocm's copy is already in the process -- and
    the second runtime then sees no GPU ("No HIP GPUs are available").  The other order is fine: libgeglove.so asks
    for the SONAME and takes whichever copy is loaded.  So when torch is installed (the multi-GPU path and some
    tests use it in the same process) its copy is mapped first, without importing torch."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(path):
        C.CDLL(path, mode=C.RTLD_GLOBAL)


def lib():
    """Loads libgeglove.so; raises (loudly) when the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libgeglove.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C graph-embeddings_amd/csrc`" % LIB_PATH)
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    i32p, i64p, f32p, f64p = (C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_double))
    vp = C.c_void_p
    L.ge_glove_cfg_default.argtypes = [C.POINTER(GloveCfg)]; L.ge_glove_cfg_default.restype = None
    L.ge_glove_create.argtypes = [C.POINTER(GloveCfg), i32p, i32p, f32p, C.POINTER(vp)]
    L.ge_glove_epoch.argtypes = [vp, C.c_int32, f64p]
    L.ge_glove_extract_f32.argtypes = [vp, f32p]
    L.ge_glove_extract_f64.argtypes = [vp, f64p]
    L.ge_glove_get_state.argtypes = [vp, C.c_int32, f32p, C.c_int64]
    L.ge_glove_set_state.argtypes = [vp, C.c_int32, f32p, C.c_int64]
    L.ge_glove_device_ptr.argtypes = [vp, C.c_int32, C.POINTER(vp), i64p]
    L.ge_glove_epoch_order.argtypes = [vp, C.c_int32, i32p, C.c_int64]
    L.ge_glove_get_perm.argtypes = [vp, i32p, C.c_int64]
    L.ge_glove_rng_state.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.ge_glove_last_kernel_ms.argtypes = [vp, f32p, i32p]
    L.ge_glove_get_info.argtypes = [vp, C.POINTER(GloveInfo)]
    L.ge_glove_tile_info.argtypes = [vp, C.POINTER(C.c_int64)]
    L.ge_glove_panel_info.argtypes = [vp, C.POINTER(C.c_int64)]
    L.ge_glove_set_arith.argtypes = [vp, C.c_int32]
    L.ge_glove_get_arith.argtypes = [vp, i32p]
    L.ge_glove_destroy.argtypes = [vp]; L.ge_glove_destroy.restype = None
    L.ge_bca_build.argtypes = [C.POINTER(Csr), C.POINTER(Csr), C.POINTER(BcaCfg), C.POINTER(vp)]
    L.ge_coo_get.argtypes = [vp, i64p, C.POINTER(i32p), C.POINTER(i32p), C.POINTER(f32p), C.POINTER(i64p), f64p]
    L.ge_coo_destroy.argtypes = [vp]; L.ge_coo_destroy.restype = None
    L.ge_sim_cfg_default.argtypes = [C.POINTER(SimCfg)]; L.ge_sim_cfg_default.restype = None
    L.ge_sim_pattern_supported.argtypes = [C.c_char_p]; L.ge_sim_pattern_supported.restype = C.c_int32
    L.ge_similarity_pairs.argtypes = [C.POINTER(Strings), i32p, i32p, C.c_int32, i32p, i32p, C.c_int32, C.POINTER(SimCfg), C.POINTER(vp)]
    L.ge_sim_pairs_get.argtypes = [vp, i64p, C.POINTER(i32p), C.POINTER(i32p), C.POINTER(f32p)]
    L.ge_sim_pairs_destroy.argtypes = [vp]; L.ge_sim_pairs_destroy.restype = None
    L.ge_glove_context_layout.argtypes = [vp, C.POINTER(ContextLayout)]
    L.ge_exchange_turn_bf16.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, C.c_uint32, vp]
    L.ge_rccl_unique_id.argtypes = [vp]
    L.ge_local_group_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.ge_local_group_destroy.argtypes = [vp]; L.ge_local_group_destroy.restype = None
    L.ge_local_group_abort.argtypes = [vp]; L.ge_local_group_abort.restype = None
    L.ge_rccl_selftest.argtypes = [C.c_int32]
    L.ge_sync_cfg_size.argtypes = []; L.ge_sync_cfg_size.restype = C.c_int32
    L.ge_sync_create.argtypes = [vp, C.POINTER(SyncCfg), C.POINTER(vp)]
    L.ge_sync_begin.argtypes = [vp, C.c_int32]
    for nm in ("ge_sync_finish", "ge_sync_turn", "ge_sync_sync"):
        getattr(L, nm).argtypes = [vp]
    L.ge_sync_epoch.argtypes = [vp, C.c_int32, C.c_int32, f64p]
    L.ge_sync_hub_rows.argtypes = [vp, i32p, C.c_int32, i32p]
    L.ge_sync_hub_exchange.argtypes = [vp]
    L.ge_sync_hub_exchange_live.argtypes = [vp]
    L.ge_sync_live_rows.argtypes = [vp, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]
    L.ge_sync_hub_plan.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ge_sync_replicate.argtypes = [vp, C.c_int32]
    L.ge_sync_allreduce_f64.argtypes = [vp, f64p, C.c_int32, C.c_int32]
    L.ge_sync_destroy.argtypes = [vp]; L.ge_sync_destroy.restype = None
    if L.ge_sync_cfg_size() != C.sizeof(SyncCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_sync_cfg is %d bytes there, %d here)"
                          % (L.ge_sync_cfg_size(), C.sizeof(SyncCfg)))
    L.ge_copy_bandwidth.argtypes = [C.c_int32, C.c_int64, C.c_int32, f64p]
    L.ge_last_error.argtypes = []; L.ge_last_error.restype = C.c_char_p
    L.ge_version.argtypes = []; L.ge_version.restype = C.c_char_p
    L.ge_device_count.argtypes = []; L.ge_device_count.restype = C.c_int32
    L.ge_glove_cfg_size.argtypes = []; L.ge_glove_cfg_size.restype = C.c_int32
    L.ge_sim_cfg_size.argtypes = []; L.ge_sim_cfg_size.restype = C.c_int32
    L.ge_bca_cfg_size.argtypes = []; L.ge_bca_cfg_size.restype = C.c_int32
    L.ge_glove_info_size.argtypes = []; L.ge_glove_info_size.restype = C.c_int32
    if L.ge_bca_cfg_size() != C.sizeof(BcaCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_bca_cfg is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_bca_cfg_size(), C.sizeof(BcaCfg)))
    if L.ge_sim_cfg_size() != C.sizeof(SimCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_sim_cfg is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_sim_cfg_size(), C.sizeof(SimCfg)))
    if L.ge_glove_cfg_size() != C.sizeof(GloveCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_glove_cfg is %d bytes there, "
                          "%d here): rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_glove_cfg_size(), C.sizeof(GloveCfg)))
    if L.ge_glove_info_size() != C.sizeof(GloveInfo):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_glove_info is %d bytes there, "
                          "%d here): rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_glove_info_size(), C.sizeof(GloveInfo)))
    _declare_pca(L)
    _declare_nn(L)
    _declare_synth(L)
    _declare_eval(L)
    _declare_rank(L)
    _declare_kmeans(L)
    _declare_predict(L)
    _declare_fold(L)
    _declare_ivf(L)
    _declare_classify(L)
    _declare_match(L)
    _declare_align(L)
    for name in SYMBOLS:
        f = getattr(L, name)
        if f.restype is C.c_int:      # default restype -> ge_status
            f.restype = C.c_int32
    _lib = L
    return L


def _declare_pca(L):
    """The PCA section of include/geglove.h."""
    vp, f32p, f64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.ge_pca_cfg_default.argtypes = [C.POINTER(PcaCfg)]; L.ge_pca_cfg_default.restype = None
    L.ge_pca_cfg_size.argtypes = []; L.ge_pca_cfg_size.restype = C.c_int32
    if L.ge_pca_cfg_size() != C.sizeof(PcaCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_pca_cfg is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_pca_cfg_size(), C.sizeof(PcaCfg)))
    L.ge_pca_fit.argtypes = [f32p, C.c_int64, C.c_int32, C.POINTER(PcaCfg), C.POINTER(vp)]
    L.ge_glove_pca_fit.argtypes = [vp, C.POINTER(PcaCfg), C.POINTER(vp)]
    L.ge_pca_from_moments.argtypes = [f64p, f64p, C.c_int32, C.c_int64, C.POINTER(PcaCfg), C.POINTER(vp)]
    L.ge_pca_get.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(f64p), C.POINTER(f64p),
                             C.POINTER(f64p), C.POINTER(f64p)]
    L.ge_pca_transform.argtypes = [vp, f32p, C.c_int64, f32p]
    L.ge_glove_pca_transform.argtypes = [vp, vp, f32p]
    L.ge_pca_last_kernel_ms.argtypes = [vp, f32p, f32p]
    L.ge_pca_destroy.argtypes = [vp]; L.ge_pca_destroy.restype = None


class Pca:
    """A ge_pca model: Pca.fit(rows) / Pca.fit_glove(handle) / Pca.from_moments(mean, cov, n_rows), then the tables of
    ge_pca_get as numpy arrays (copies) and transform(rows) / transform_glove(handle)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _cfg(variance, max_components, device):
        cfg = PcaCfg(); lib().ge_pca_cfg_default(C.byref(cfg))
        cfg.variance, cfg.max_components, cfg.device = variance, max_components, device
        return cfg

    @classmethod
    def fit(cls, rows, variance=0.95, max_components=0, device=0):
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        h = C.c_void_p()
        check(lib().ge_pca_fit(rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], rows.shape[1],
                               C.byref(cls._cfg(variance, max_components, device)), C.byref(h)))
        return cls(h)

    @classmethod
    def fit_glove(cls, glove_handle, variance=0.95, max_components=0):
        h = C.c_void_p()
        check(lib().ge_glove_pca_fit(glove_handle, C.byref(cls._cfg(variance, max_components, 0)), C.byref(h)))
        return cls(h)

    @classmethod
    def from_moments(cls, mean, cov, n_rows, variance=0.95, max_components=0, device=0):
        import numpy as np
        mean = np.ascontiguousarray(mean, dtype=np.float64); cov = np.ascontiguousarray(cov, dtype=np.float64)
        f64p = C.POINTER(C.c_double)
        h = C.c_void_p()
        check(lib().ge_pca_from_moments(mean.ctypes.data_as(f64p), cov.ctypes.data_as(f64p), mean.shape[0], n_rows,
                                        C.byref(cls._cfg(variance, max_components, device)), C.byref(h)))
        return cls(h)

    def get(self):
        """(dim, k, n_rows, mean[dim], cov[dim, dim], eigenvalues[dim], components[dim, dim]); column c of components is the
        unit eigenvector of the c-th largest eigenvalue."""
        import numpy as np
        f64p = C.POINTER(C.c_double)
        dim, k, n = C.c_int32(), C.c_int32(), C.c_int64()
        mean, cov, eig, comp = f64p(), f64p(), f64p(), f64p()
        check(lib().ge_pca_get(self._h, C.byref(dim), C.byref(k), C.byref(n), C.byref(mean), C.byref(cov), C.byref(eig), C.byref(comp)))
        D = dim.value
        arr = lambda p, shape: np.ctypeslib.as_array(p, shape=shape).copy()
        return D, k.value, n.value, arr(mean, (D,)), arr(cov, (D, D)), arr(eig, (D,)), arr(comp, (D, D))

    @property
    def k(self):
        return self.get()[1]

    def transform(self, rows):
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        out = np.empty((rows.shape[0], self.k), dtype=np.float32)
        check(lib().ge_pca_transform(self._h, rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def transform_glove(self, glove_handle, vocab_size):
        import numpy as np
        out = np.empty((vocab_size, self.k), dtype=np.float32)
        check(lib().ge_glove_pca_transform(self._h, glove_handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def kernel_ms(self):
        fit, tr = C.c_float(), C.c_float()
        check(lib().ge_pca_last_kernel_ms(self._h, C.byref(fit), C.byref(tr)))
        return fit.value, tr.value

    def close(self):
        if self._h:
            lib().ge_pca_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _declare_nn(L):
    """The nearest-neighbour section of include/geglove.h."""
    vp, i32p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    L.ge_nn_cfg_default.argtypes = [C.POINTER(NnCfg)]; L.ge_nn_cfg_default.restype = None
    L.ge_nn_cfg_size.argtypes = []; L.ge_nn_cfg_size.restype = C.c_int32
    if L.ge_nn_cfg_size() != C.sizeof(NnCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_nn_cfg is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_nn_cfg_size(), C.sizeof(NnCfg)))
    L.ge_nn_create.argtypes = [f32p, C.c_int64, C.c_int32, i32p, C.c_int64, C.POINTER(NnCfg), C.POINTER(vp)]
    L.ge_glove_nn_create.argtypes = [vp, i32p, C.c_int64, C.POINTER(NnCfg), C.POINTER(vp)]
    L.ge_nn_query_rows.argtypes = [vp, i32p, C.c_int64, C.c_int32, C.c_int32, i32p, f32p]
    L.ge_nn_query_vectors.argtypes = [vp, f32p, C.c_int64, C.c_int32, i32p, f32p]
    L.ge_nn_get.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ge_nn_last_kernel_ms.argtypes = [vp, f32p, f32p]
    L.ge_nn_destroy.argtypes = [vp]; L.ge_nn_destroy.restype = None


class Neighbors:
    """A ge_nn index: Neighbors.create(rows) / Neighbors.create_glove(handle), then query_rows(ids, k) / query_vectors(vectors, k),
    each returning (int32[nq, k] original row ids, float32[nq, k] scores), best first."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _cfg(metric, device):
        cfg = NnCfg(); lib().ge_nn_cfg_default(C.byref(cfg))
        cfg.metric, cfg.device = NN_METRICS.get(metric, metric), device
        return cfg

    @staticmethod
    def _subset(subset):
        import numpy as np
        if subset is None:
            return None, None, 0
        subset = np.ascontiguousarray(subset, dtype=np.int32)
        return subset, subset.ctypes.data_as(C.POINTER(C.c_int32)), subset.shape[0]

    @classmethod
    def create(cls, rows, subset=None, metric="cosine", device=0):
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        keep, sub, n_sub = cls._subset(subset)
        h = C.c_void_p()
        check(lib().ge_nn_create(rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], rows.shape[1], sub, n_sub,
                                 C.byref(cls._cfg(metric, device)), C.byref(h)))
        return cls(h)

    @classmethod
    def create_glove(cls, glove_handle, subset=None, metric="cosine"):
        keep, sub, n_sub = cls._subset(subset)
        h = C.c_void_p()
        check(lib().ge_glove_nn_create(glove_handle, sub, n_sub, C.byref(cls._cfg(metric, 0)), C.byref(h)))
        return cls(h)

    def get(self):
        """(n_indexed, dim, metric)"""
        n, dim, metric = C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().ge_nn_get(self._h, C.byref(n), C.byref(dim), C.byref(metric)))
        return n.value, dim.value, metric.value

    @staticmethod
    def _out(nq, k):
        import numpy as np
        idx = np.empty((nq, k), dtype=np.int32); score = np.empty((nq, k), dtype=np.float32)
        return idx, score, idx.ctypes.data_as(C.POINTER(C.c_int32)), score.ctypes.data_as(C.POINTER(C.c_float))

    def query_rows(self, query_ids, k, exclude_self=False):
        """query_ids: None (every indexed row, in order) or row ids that are members of the index."""
        import numpy as np
        if query_ids is None:
            ids, nq = None, self.get()[0]
        else:
            keep = np.ascontiguousarray(query_ids, dtype=np.int32)
            ids, nq = keep.ctypes.data_as(C.POINTER(C.c_int32)), keep.shape[0]
        idx, score, pi, ps = self._out(nq, k)
        check(lib().ge_nn_query_rows(self._h, ids, nq, k, 1 if exclude_self else 0, pi, ps))
        return idx, score

    def query_vectors(self, vectors, k):
        import numpy as np
        vectors = np.ascontiguousarray(vectors, dtype=np.float32)
        idx, score, pi, ps = self._out(vectors.shape[0], k)
        check(lib().ge_nn_query_vectors(self._h, vectors.ctypes.data_as(C.POINTER(C.c_float)), vectors.shape[0], k, pi, ps))
        return idx, score

    def kernel_ms(self):
        prep, query = C.c_float(), C.c_float()
        check(lib().ge_nn_last_kernel_ms(self._h, C.byref(prep), C.byref(query)))
        return prep.value, query.value

    def close(self):
        if self._h:
            lib().ge_nn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _declare_synth(L):
    """The generator section of include/geglove.h."""
    vp, i32p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    L.ge_synth_cfg_default.argtypes = [C.POINTER(SynthCfg)]; L.ge_synth_cfg_default.restype = None
    L.ge_synth_cfg_size.argtypes = []; L.ge_synth_cfg_size.restype = C.c_int32
    if L.ge_synth_cfg_size() != C.sizeof(SynthCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_synth_cfg is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_synth_cfg_size(), C.sizeof(SynthCfg)))
    L.ge_synth_coo.argtypes = [C.POINTER(SynthCfg), C.POINTER(vp)]
    L.ge_coo_device.argtypes = [vp, i32p, C.POINTER(i32p), C.POINTER(i32p), C.POINTER(f32p)]
    L.ge_coo_synth_stats.argtypes = [vp, C.POINTER(C.c_int64), f32p, C.POINTER(C.c_int64)]
    L.ge_glove_create_coo.argtypes = [C.POINTER(GloveCfg), vp, C.POINTER(vp)]


class Coo:
    """A ge_coo handle (here: the device-resident result of synth_coo)."""

    def __init__(self, handle, vocab_size):
        self._h = handle
        self.vocab_size = vocab_size

    @property
    def handle(self):
        return self._h

    def get(self):
        """(I, J, X, row_ptr, max): numpy copies of the host views (a device-resident result comes down on the first call)."""
        import numpy as np
        i32p, f32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
        n, mx = C.c_int64(), C.c_double()
        pI, pJ, pX, pR = i32p(), i32p(), f32p(), i64p()
        check(lib().ge_coo_get(self._h, C.byref(n), C.byref(pI), C.byref(pJ), C.byref(pX), C.byref(pR), C.byref(mx)))
        arr = lambda p, m, dt: np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, dt)
        return (arr(pI, n.value, np.int32), arr(pJ, n.value, np.int32), arr(pX, n.value, np.float32),
                arr(pR, self.vocab_size + 1, np.int64), mx.value)

    @property
    def nnz(self):
        n = C.c_int64()
        check(lib().ge_coo_get(self._h, C.byref(n), None, None, None, None, None))
        return n.value

    def device_views(self):
        """(device, dI, dJ, dX): the device ordinal (-1: host-resident) and the raw device addresses (None then)."""
        dev = C.c_int32()
        pI, pJ, pX = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_float)()
        check(lib().ge_coo_device(self._h, C.byref(dev), C.byref(pI), C.byref(pJ), C.byref(pX)))
        addr = lambda p: C.cast(p, C.c_void_p).value
        return dev.value, addr(pI), addr(pJ), addr(pX)

    def stats(self):
        """(draws, kernel_ms, peak_bytes) of the generator"""
        draws, ms, peak = C.c_int64(), C.c_float(), C.c_int64()
        check(lib().ge_coo_synth_stats(self._h, C.byref(draws), C.byref(ms), C.byref(peak)))
        return draws.value, ms.value, peak.value

    def close(self):
        if self._h:
            lib().ge_coo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth_coo(V, nnz, rows=None, seed=0xC0FFEE, device=0):
    """ge_synth_coo: the synthetic matrix of include/geglove.h's recipe, generated on `device`.  rows = (row_begin, row_end) of a
    shard, None = all rows.  Returns a Coo."""
    cfg = SynthCfg(); lib().ge_synth_cfg_default(C.byref(cfg))
    cfg.vocab_size, cfg.nnz, cfg.seed, cfg.device = V, nnz, seed & 0xFFFFFFFFFFFFFFFF, device
    if rows is not None:
        cfg.row_begin, cfg.row_end = rows
    h = C.c_void_p()
    check(lib().ge_synth_coo(C.byref(cfg), C.byref(h)))
    return Coo(h, V)


def _declare_eval(L):
    """The held-out evaluation section of include/geglove.h."""
    vp, i32p, f32p, f64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.ge_glove_eval_create.argtypes = [vp, i32p, i32p, f32p, C.c_int64, C.POINTER(vp)]
    L.ge_glove_eval_run.argtypes = [vp, f32p, f64p, f64p]
    L.ge_eval_last_kernel_ms.argtypes = [vp, f32p]
    L.ge_eval_get.argtypes = [vp, C.POINTER(C.c_int64), i32p]
    L.ge_eval_destroy.argtypes = [vp]; L.ge_eval_destroy.restype = None
    L.ge_holdout_mask.argtypes = [C.c_uint64, C.c_int64, C.c_double, C.POINTER(C.c_uint8)]


class Evaluation:
    """A ge_eval set on a trainer handle: Evaluation(glove_handle, I, J, X), then run() after any epoch.  Close it before the
    trainer handle goes."""

    def __init__(self, glove_handle, I, J, X):
        import numpy as np
        I = np.ascontiguousarray(I, dtype=np.int32); J = np.ascontiguousarray(J, dtype=np.int32)
        X = np.ascontiguousarray(X, dtype=np.float32)
        if not (I.shape == J.shape == X.shape and I.ndim == 1):
            raise ValueError("I, J, X must be one-dimensional arrays of one length")
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        h = C.c_void_p()
        check(lib().ge_glove_eval_create(glove_handle, I.ctypes.data_as(i32p), J.ctypes.data_as(i32p), X.ctypes.data_as(f32p),
                                         I.shape[0], C.byref(h)))
        self._h = h
        self.n = I.shape[0]

    def run(self, residual=True, term=True):
        """(residual float32[n] or None, term float64[n] or None, cost_sum), the arrays in the caller's order."""
        import numpy as np
        res = np.empty(self.n, dtype=np.float32) if residual else None
        trm = np.empty(self.n, dtype=np.float64) if term else None
        total = C.c_double()
        check(lib().ge_glove_eval_run(self._h, res.ctypes.data_as(C.POINTER(C.c_float)) if residual else None,
                                      trm.ctypes.data_as(C.POINTER(C.c_double)) if term else None, C.byref(total)))
        return res, trm, total.value

    def kernel_ms(self):
        ms = C.c_float()
        check(lib().ge_eval_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def reordered(self):
        """True when creation sorted the set by focus row (it did not arrive so)."""
        flag = C.c_int32()
        check(lib().ge_eval_get(self._h, None, C.byref(flag)))
        return bool(flag.value)

    def close(self):
        if self._h:
            lib().ge_eval_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def holdout_mask(seed, n, fraction):
    """ge_holdout_mask: uint8[n], 1 where nonzero k is held out (a function of seed, k and fraction alone; no device)."""
    import numpy as np
    mask = np.empty(n, dtype=np.uint8)
    check(lib().ge_holdout_mask(int(seed) & 0xFFFFFFFFFFFFFFFF, n, float(fraction), mask.ctypes.data_as(C.POINTER(C.c_uint8))))
    return mask


def _declare_rank(L):
    """The ranking section of include/geglove.h."""
    vp, i32p, i64p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    L.ge_rank_summary_size.argtypes = []; L.ge_rank_summary_size.restype = C.c_int32
    if L.ge_rank_summary_size() != C.sizeof(RankSummary):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_rank_summary is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_rank_summary_size(), C.sizeof(RankSummary)))
    L.ge_glove_rank_create.argtypes = [vp, i32p, i32p, C.c_int64, i64p, i32p, C.POINTER(vp)]
    L.ge_glove_rank_run.argtypes = [vp, i32p, f32p, C.POINTER(RankSummary)]
    L.ge_rank_last_kernel_ms.argtypes = [vp, f32p]
    L.ge_rank_last_phase_ms.argtypes = [vp, f32p, f32p, f32p]
    L.ge_rank_get.argtypes = [vp, i64p, i64p, i32p, i32p]
    L.ge_rank_destroy.argtypes = [vp]; L.ge_rank_destroy.restype = None


class Ranking:
    """A ge_rank set on a trainer handle: Ranking(glove_handle, I, J, filter_ptr, filter_idx), then run() after any epoch.  The
    filter lists are CSR-shaped (filter_ptr int64[n + 1] into filter_idx, ids of a list strictly ascending); both None = no
    filter.  Close it before the trainer handle goes."""

    def __init__(self, glove_handle, I, J, filter_ptr=None, filter_idx=None):
        import numpy as np
        I = np.ascontiguousarray(I, dtype=np.int32); J = np.ascontiguousarray(J, dtype=np.int32)
        if not (I.shape == J.shape and I.ndim == 1):
            raise ValueError("I, J must be one-dimensional arrays of one length")
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        pp = pi = None
        if filter_ptr is not None:
            fp = np.ascontiguousarray(filter_ptr, dtype=np.int64)
            fi = np.ascontiguousarray(filter_idx if filter_idx is not None else [], dtype=np.int32)
            if fp.shape != (I.shape[0] + 1,) or fi.ndim != 1 or (fp.size and fp[-1] != fi.shape[0]):
                raise ValueError("filter_ptr must hold n + 1 offsets, the last one the length of filter_idx")
            pp, pi = fp.ctypes.data_as(i64p), fi.ctypes.data_as(i32p)
        h = C.c_void_p()
        check(lib().ge_glove_rank_create(glove_handle, I.ctypes.data_as(i32p), J.ctypes.data_as(i32p), I.shape[0], pp, pi, C.byref(h)))
        self._h = h
        self.n = I.shape[0]

    def run(self, rank=True, score=True):
        """(rank int32[n] or None, score float32[n] or None, summary dict), the arrays in the caller's order."""
        import numpy as np
        rk = np.empty(self.n, dtype=np.int32) if rank else None
        sc = np.empty(self.n, dtype=np.float32) if score else None
        s = RankSummary()
        check(lib().ge_glove_rank_run(self._h, rk.ctypes.data_as(C.POINTER(C.c_int32)) if rank else None,
                                      sc.ctypes.data_as(C.POINTER(C.c_float)) if score else None, C.byref(s)))
        return rk, sc, {name: getattr(s, name) for name, _ in RankSummary._fields_}

    def kernel_ms(self):
        ms = C.c_float()
        check(lib().ge_rank_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def phase_ms(self):
        """(staging, target and filter scores, dense count) of the last run, device milliseconds."""
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        check(lib().ge_rank_last_phase_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def get(self):
        """{n, candidates, dim, ranges}: ranges = the candidate ranges of the last run's grid (0 before the first run)."""
        n, m, d, r = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().ge_rank_get(self._h, C.byref(n), C.byref(m), C.byref(d), C.byref(r)))
        return {"n": n.value, "candidates": m.value, "dim": d.value, "ranges": r.value}

    def close(self):
        if self._h:
            lib().ge_rank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _declare_predict(L):
    """The prediction section of include/geglove.h."""
    vp, i32p, i64p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    L.ge_glove_predict_create.argtypes = [vp, i32p, C.c_int64, i64p, i32p, i32p, C.c_int64, C.c_int32, C.POINTER(vp)]
    L.ge_glove_predict_run.argtypes = [vp, C.c_int32, i32p, f32p, i32p]
    L.ge_predict_last_kernel_ms.argtypes = [vp, f32p, f32p, f32p]
    L.ge_predict_get.argtypes = [vp, i64p, i64p, i32p, i32p]
    L.ge_predict_destroy.argtypes = [vp]; L.ge_predict_destroy.restype = None


class Prediction:
    """A ge_predict set on a trainer handle: Prediction(glove_handle, I, filters, subset, exclude_self), then run(K) after any
    epoch.  filters: None or (filter_ptr int64[n + 1], filter_idx), CSR-shaped with the ids of a list strictly ascending;
    subset: None (all columns) or strictly ascending candidate column ids.  Close it before the trainer handle goes."""

    def __init__(self, glove_handle, I, filters=None, subset=None, exclude_self=False):
        import numpy as np
        I = np.ascontiguousarray(I, dtype=np.int32)
        if I.ndim != 1:
            raise ValueError("I must be a one-dimensional array")
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        pp = pi = ps = None
        if filters is not None:
            fp = np.ascontiguousarray(filters[0], dtype=np.int64)
            fi = np.ascontiguousarray(filters[1] if filters[1] is not None else [], dtype=np.int32)
            if fp.shape != (I.shape[0] + 1,) or fi.ndim != 1 or (fp.size and fp[-1] != fi.shape[0]):
                raise ValueError("filter_ptr must hold n + 1 offsets, the last one the length of filter_idx")
            pp, pi = fp.ctypes.data_as(i64p), fi.ctypes.data_as(i32p)
        n_sub = 0
        if subset is not None:
            sub = np.ascontiguousarray(subset, dtype=np.int32)
            if sub.ndim != 1:
                raise ValueError("subset must be a one-dimensional array")
            ps, n_sub = sub.ctypes.data_as(i32p), sub.shape[0]
        h = C.c_void_p()
        check(lib().ge_glove_predict_create(glove_handle, I.ctypes.data_as(i32p), I.shape[0], pp, pi, ps, n_sub, 1 if exclude_self else 0,
                                            C.byref(h)))
        self._h = h
        self.n = I.shape[0]

    def run(self, K):
        """(index int32[n, K], score float32[n, K], count int32[n]): the K best candidates of every query in order, short lists
        filled with (-1, -inf)."""
        import numpy as np
        K = int(K)
        shape = (self.n, K if 1 <= K <= 128 else 0)            # a K outside the limits is the library's to refuse
        index = np.empty(shape, dtype=np.int32)
        score = np.empty(shape, dtype=np.float32)
        count = np.empty(self.n, dtype=np.int32)
        check(lib().ge_glove_predict_run(self._h, K, index.ctypes.data_as(C.POINTER(C.c_int32)), score.ctypes.data_as(C.POINTER(C.c_float)),
                                         count.ctypes.data_as(C.POINTER(C.c_int32))))
        return index, score, count

    def kernel_ms(self):
        """(staging, score and select, merge) of the last run, device milliseconds."""
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        check(lib().ge_predict_last_kernel_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def info(self):
        """{n, candidates, dim, ranges}: ranges = the candidate ranges of the last run's grid (0 before the first run)."""
        n, m, d, r = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().ge_predict_get(self._h, C.byref(n), C.byref(m), C.byref(d), C.byref(r)))
        return {"n": n.value, "candidates": m.value, "dim": d.value, "ranges": r.value}

    def close(self):
        if self._h:
            lib().ge_predict_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _declare_fold(L):
    """The fold-in section of include/geglove.h."""
    vp, i32p, i64p, f32p, f64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.ge_fold_cfg_default.argtypes = [C.POINTER(FoldCfg)]; L.ge_fold_cfg_default.restype = None
    L.ge_fold_cfg_size.argtypes = []; L.ge_fold_cfg_size.restype = C.c_int32
    if L.ge_fold_cfg_size() != C.sizeof(FoldCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_fold_cfg is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_fold_cfg_size(), C.sizeof(FoldCfg)))
    L.ge_glove_fold_create.argtypes = [vp, i64p, i32p, f32p, C.c_int64, C.POINTER(FoldCfg), C.POINTER(vp)]
    L.ge_glove_fold_run.argtypes = [vp, f32p, f32p, f32p, f32p, f32p, f64p]
    L.ge_fold_last_kernel_ms.argtypes = [vp, f32p]
    L.ge_fold_get.argtypes = [vp, i64p, i64p, i32p, i64p]
    L.ge_fold_destroy.argtypes = [vp]; L.ge_fold_destroy.restype = None
    L.ge_foldin_mask.argtypes = [C.c_uint64, C.c_int64, C.c_double, C.POINTER(C.c_uint8)]


class Folding:
    """A ge_fold set on a trainer handle: Folding(glove_handle, row_ptr, idx, X, side, epochs, shuffle, lr, seed), then run() after
    any epoch.  Row r holds the entries [row_ptr[r], row_ptr[r + 1]) of (idx, X): ids of the frozen side (columns for side "focus",
    focus rows for side "context").  lr 0 = the handle's.  Close it before the trainer handle goes."""

    def __init__(self, glove_handle, row_ptr, idx, X, side="focus", epochs=10, shuffle="device", lr=0.0, seed=0):
        import numpy as np
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        idx = np.ascontiguousarray(idx, dtype=np.int32); X = np.ascontiguousarray(X, dtype=np.float32)
        if row_ptr.ndim != 1 or row_ptr.shape[0] < 1 or not (idx.shape == X.shape and idx.ndim == 1):
            raise ValueError("row_ptr must hold n_rows + 1 offsets; idx, X must be one-dimensional arrays of one length")
        if int(row_ptr[-1]) != idx.shape[0]:
            raise ValueError("the last offset of row_ptr must be the length of idx")
        cfg = FoldCfg()
        lib().ge_fold_cfg_default(C.byref(cfg))
        cfg.side = FOLD_SIDES[side] if isinstance(side, str) else int(side)
        cfg.shuffle = FOLD_SHUFFLES[shuffle] if isinstance(shuffle, str) else int(shuffle)
        cfg.epochs, cfg.learning_rate, cfg.seed = int(epochs), float(lr), int(seed)
        # an array of length 0 has no address worth passing: the library only requires the pointers to be non-null
        pad = lambda a: a if a.shape[0] else np.zeros(1, a.dtype)
        h = C.c_void_p()
        check(lib().ge_glove_fold_create(glove_handle, row_ptr.ctypes.data_as(C.POINTER(C.c_int64)), pad(idx).ctypes.data_as(C.POINTER(C.c_int32)),
                                         pad(X).ctypes.data_as(C.POINTER(C.c_float)), row_ptr.shape[0] - 1, C.byref(cfg), C.byref(h)))
        self._h = h
        self.n_rows, self.epochs = row_ptr.shape[0] - 1, int(epochs)
        self.dim = self.info["dim"]

    def run(self, init_rows=None, init_bias=None):
        """(rows float32[n_rows, dim], bias float32[n_rows], cost float32[n_rows, E], history float64[E])."""
        import numpy as np
        f32p = C.POINTER(C.c_float)
        ir = ib = None
        if init_rows is not None:
            ir = np.ascontiguousarray(init_rows, dtype=np.float32)
            if ir.shape != (self.n_rows, self.dim):
                raise ValueError("init_rows must be [n_rows, dim]")
        if init_bias is not None:
            ib = np.ascontiguousarray(init_bias, dtype=np.float32)
            if ib.shape != (self.n_rows,):
                raise ValueError("init_bias must be [n_rows]")
        rows = np.empty((self.n_rows, self.dim), dtype=np.float32)
        bias = np.empty(self.n_rows, dtype=np.float32)
        cost = np.empty((self.n_rows, self.epochs), dtype=np.float32)
        history = np.empty(self.epochs, dtype=np.float64)
        check(lib().ge_glove_fold_run(self._h, None if ir is None else ir.ctypes.data_as(f32p), None if ib is None else ib.ctypes.data_as(f32p),
                                      rows.ctypes.data_as(f32p), bias.ctypes.data_as(f32p), cost.ctypes.data_as(f32p),
                                      history.ctypes.data_as(C.POINTER(C.c_double))))
        return rows, bias, cost, history

    @property
    def kernel_ms(self):
        ms = C.c_float()
        check(lib().ge_fold_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    @property
    def info(self):
        """{n_rows, nnz, dim, path}: path = E * the longest row, the sequential updates that bound a run from below."""
        n, z, d, p = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
        check(lib().ge_fold_get(self._h, C.byref(n), C.byref(z), C.byref(d), C.byref(p)))
        return {"n_rows": n.value, "nnz": z.value, "dim": d.value, "path": p.value}

    def close(self):
        if self._h:
            lib().ge_fold_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def foldin_mask(seed, n, fraction):
    """ge_foldin_mask: uint8[n], 1 where vertex v is late (a function of seed, v and fraction alone; no device)."""
    import numpy as np
    mask = np.empty(n, dtype=np.uint8)
    check(lib().ge_foldin_mask(int(seed) & 0xFFFFFFFFFFFFFFFF, n, float(fraction), mask.ctypes.data_as(C.POINTER(C.c_uint8))))
    return mask


def _declare_kmeans(L):
    """The clustering section of include/geglove.h."""
    vp, i32p, i64p, f32p, f64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.ge_kmeans_cfg_default.argtypes = [C.POINTER(KmeansCfg)]; L.ge_kmeans_cfg_default.restype = None
    L.ge_kmeans_cfg_size.argtypes = []; L.ge_kmeans_cfg_size.restype = C.c_int32
    if L.ge_kmeans_cfg_size() != C.sizeof(KmeansCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_kmeans_cfg is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_kmeans_cfg_size(), C.sizeof(KmeansCfg)))
    L.ge_kmeans_create.argtypes = [f32p, C.c_int64, C.c_int32, i32p, C.c_int64, C.POINTER(KmeansCfg), C.POINTER(vp)]
    L.ge_glove_kmeans_create.argtypes = [vp, i32p, C.c_int64, C.POINTER(KmeansCfg), C.POINTER(vp)]
    L.ge_kmeans_set_centroids.argtypes = [vp, f32p]
    L.ge_kmeans_step.argtypes = [vp, i64p, f64p]
    L.ge_kmeans_run.argtypes = [vp, C.c_int32, i32p, i32p]
    L.ge_kmeans_get.argtypes = [vp, i64p, i32p, i32p, i32p, f32p, f32p, i32p, i32p, i32p, f64p, f64p]
    L.ge_kmeans_last_kernel_ms.argtypes = [vp, f32p, f32p]
    L.ge_kmeans_destroy.argtypes = [vp]; L.ge_kmeans_destroy.restype = None


class Clustering:
    """A ge_kmeans handle: Clustering.create(rows, k) / Clustering.create_glove(handle, k), optionally set_centroids(values), then
    step() -> (changed, objective) or run(max_iter) -> (steps run, converged); labels, best, centroids and sizes read the state."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _cfg(k, metric, seed, device):
        cfg = KmeansCfg(); lib().ge_kmeans_cfg_default(C.byref(cfg))
        cfg.metric, cfg.k, cfg.seed, cfg.device = KM_METRICS.get(metric, metric), k, seed & (2 ** 64 - 1), device
        return cfg

    @classmethod
    def create(cls, rows, k, subset=None, metric="cosine", seed=0, device=0):
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        keep, sub, n_sub = Neighbors._subset(subset)
        h = C.c_void_p()
        check(lib().ge_kmeans_create(rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], rows.shape[1], sub, n_sub,
                                     C.byref(cls._cfg(k, metric, seed, device)), C.byref(h)))
        return cls(h)

    @classmethod
    def create_glove(cls, glove_handle, k, subset=None, metric="cosine", seed=0):
        keep, sub, n_sub = Neighbors._subset(subset)
        h = C.c_void_p()
        check(lib().ge_glove_kmeans_create(glove_handle, sub, n_sub, C.byref(cls._cfg(k, metric, seed, 0)), C.byref(h)))
        return cls(h)

    def get(self):
        """dict: n, dim, k, steps, converged, objective (of the last step), sum_sq"""
        n, dim, k, steps, conv = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        obj, sq = C.c_double(), C.c_double()
        check(lib().ge_kmeans_get(self._h, C.byref(n), C.byref(dim), C.byref(k), None, None, None, None, C.byref(steps), C.byref(conv),
                                  C.byref(obj), C.byref(sq)))
        return {"n": n.value, "dim": dim.value, "k": k.value, "steps": steps.value, "converged": bool(conv.value),
                "objective": obj.value, "sum_sq": sq.value}

    def set_centroids(self, centroids):
        import numpy as np
        g = self.get()
        centroids = np.ascontiguousarray(centroids, dtype=np.float32)
        if centroids.shape != (g["k"], g["dim"]):
            raise ValueError("centroids must be %d x %d, got %r" % (g["k"], g["dim"], centroids.shape))
        check(lib().ge_kmeans_set_centroids(self._h, centroids.ctypes.data_as(C.POINTER(C.c_float))))

    def step(self):
        """One assign and one update: (changed, objective of the assign)."""
        changed, obj = C.c_int64(), C.c_double()
        check(lib().ge_kmeans_step(self._h, C.byref(changed), C.byref(obj)))
        return changed.value, obj.value

    def run(self, max_iter=50):
        """Steps until no label changes or max_iter steps have run: (steps run, converged)."""
        steps, conv = C.c_int32(), C.c_int32()
        check(lib().ge_kmeans_run(self._h, max_iter, C.byref(steps), C.byref(conv)))
        return steps.value, bool(conv.value)

    def _read(self, slot, shape, dtype, ctype):
        import numpy as np
        out = np.empty(shape, dtype=dtype)
        args = [None] * 11
        args[slot] = out.ctypes.data_as(C.POINTER(ctype))
        check(lib().ge_kmeans_get(self._h, *args))
        return out

    @property
    def labels(self):
        import numpy as np
        return self._read(3, (self.get()["n"],), np.int32, C.c_int32)

    @property
    def best(self):
        import numpy as np
        return self._read(4, (self.get()["n"],), np.float32, C.c_float)

    @property
    def centroids(self):
        import numpy as np
        g = self.get()
        return self._read(5, (g["k"], g["dim"]), np.float32, C.c_float)

    @property
    def sizes(self):
        import numpy as np
        return self._read(6, (self.get()["k"],), np.int32, C.c_int32)

    @property
    def kernel_ms(self):
        """(assign, update) device milliseconds of the last step"""
        a, u = C.c_float(), C.c_float()
        check(lib().ge_kmeans_last_kernel_ms(self._h, C.byref(a), C.byref(u)))
        return a.value, u.value

    def close(self):
        if self._h:
            lib().ge_kmeans_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _declare_ivf(L):
    """The inverted-file section of include/geglove.h."""
    vp, i32p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    L.ge_ivf_cfg_default.argtypes = [C.POINTER(IvfCfg)]; L.ge_ivf_cfg_default.restype = None
    L.ge_ivf_cfg_size.argtypes = []; L.ge_ivf_cfg_size.restype = C.c_int32
    if L.ge_ivf_cfg_size() != C.sizeof(IvfCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_ivf_cfg is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_ivf_cfg_size(), C.sizeof(IvfCfg)))
    L.ge_ivf_create.argtypes = [f32p, C.c_int64, C.c_int32, i32p, C.c_int64, C.POINTER(IvfCfg), C.POINTER(vp)]
    L.ge_glove_ivf_create.argtypes = [vp, i32p, C.c_int64, C.POINTER(IvfCfg), C.POINTER(vp)]
    L.ge_ivf_query_rows.argtypes = [vp, i32p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, i32p, f32p, i32p, i32p]
    L.ge_ivf_query_vectors.argtypes = [vp, f32p, C.c_int64, C.c_int32, C.c_int32, i32p, f32p, i32p, i32p]
    L.ge_ivf_get.argtypes = [vp, C.POINTER(C.c_int64), i32p, i32p, i32p, i32p, f32p, i32p, i32p]
    L.ge_ivf_last_kernel_ms.argtypes = [vp, f32p, f32p, f32p, f32p]
    L.ge_ivf_destroy.argtypes = [vp]; L.ge_ivf_destroy.restype = None


class IvfNeighbors:
    """A ge_ivf index: IvfNeighbors.create(rows, lists) / IvfNeighbors.create_glove(handle, lists), then query_rows(ids, k, nprobe) /
    query_vectors(vectors, k, nprobe), each returning (int32[nq, k] original row ids, float32[nq, k] scores, int32[nq] counts,
    int32[nq] candidates looked at), best first; slots past a count hold (-1, -inf)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _cfg(lists, train_iterations, seed, centroids, dim, metric, device):
        import numpy as np
        cfg = IvfCfg(); lib().ge_ivf_cfg_default(C.byref(cfg))
        cfg.metric, cfg.lists, cfg.seed, cfg.device = NN_METRICS.get(metric, metric), lists, seed & (2 ** 64 - 1), device
        if train_iterations is not None:
            cfg.train_iterations = train_iterations
        keep = None
        if centroids is not None:
            keep = np.ascontiguousarray(centroids, dtype=np.float32)
            if dim is not None and keep.shape != (lists, dim):
                raise ValueError("centroids must be %d x %d, got %r" % (lists, dim, keep.shape))
            cfg.centroids = keep.ctypes.data_as(C.POINTER(C.c_float))
        return cfg, keep

    @classmethod
    def create(cls, rows, lists, subset=None, train_iterations=None, seed=0, centroids=None, metric="cosine", device=0):
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        keep, sub, n_sub = Neighbors._subset(subset)
        cfg, cen = cls._cfg(lists, train_iterations, seed, centroids, rows.shape[1], metric, device)
        h = C.c_void_p()
        check(lib().ge_ivf_create(rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], rows.shape[1], sub, n_sub, C.byref(cfg), C.byref(h)))
        return cls(h)

    @classmethod
    def create_glove(cls, glove_handle, lists, subset=None, train_iterations=None, seed=0, centroids=None, metric="cosine"):
        keep, sub, n_sub = Neighbors._subset(subset)
        cfg, cen = cls._cfg(lists, train_iterations, seed, centroids, None, metric, 0)
        h = C.c_void_p()
        check(lib().ge_glove_ivf_create(glove_handle, sub, n_sub, C.byref(cfg), C.byref(h)))
        return cls(h)

    def get(self):
        """dict: n, dim, lists, train_steps, converged"""
        n, dim, lists, steps, conv = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().ge_ivf_get(self._h, C.byref(n), C.byref(dim), C.byref(lists), None, None, None, C.byref(steps), C.byref(conv)))
        return {"n": n.value, "dim": dim.value, "lists": lists.value, "train_steps": steps.value, "converged": bool(conv.value)}

    def _read(self, slot, shape, dtype, ctype):
        import numpy as np
        out = np.empty(shape, dtype=dtype)
        args = [None] * 8
        args[slot] = out.ctypes.data_as(C.POINTER(ctype))
        check(lib().ge_ivf_get(self._h, *args))
        return out

    @property
    def labels(self):
        import numpy as np
        return self._read(3, (self.get()["n"],), np.int32, C.c_int32)

    @property
    def sizes(self):
        import numpy as np
        return self._read(4, (self.get()["lists"],), np.int32, C.c_int32)

    @property
    def centroids(self):
        import numpy as np
        g = self.get()
        return self._read(5, (g["lists"], g["dim"]), np.float32, C.c_float)

    @staticmethod
    def _out(nq, k):
        import numpy as np
        i32p = C.POINTER(C.c_int32)
        idx = np.empty((nq, k), dtype=np.int32); score = np.empty((nq, k), dtype=np.float32)
        count = np.empty(nq, dtype=np.int32); cand = np.empty(nq, dtype=np.int32)
        return (idx, score, count, cand), (idx.ctypes.data_as(i32p), score.ctypes.data_as(C.POINTER(C.c_float)), count.ctypes.data_as(i32p),
                                            cand.ctypes.data_as(i32p))

    def query_rows(self, query_ids, k, nprobe, exclude_self=False):
        """query_ids: None (every indexed row, in order) or row ids that are members of the index."""
        import numpy as np
        if query_ids is None:
            ids, nq = None, self.get()["n"]
        else:
            keep = np.ascontiguousarray(query_ids, dtype=np.int32)
            ids, nq = keep.ctypes.data_as(C.POINTER(C.c_int32)), keep.shape[0]
        out, ptrs = self._out(nq, k)
        check(lib().ge_ivf_query_rows(self._h, ids, nq, k, nprobe, 1 if exclude_self else 0, *ptrs))
        return out

    def query_vectors(self, vectors, k, nprobe):
        import numpy as np
        vectors = np.ascontiguousarray(vectors, dtype=np.float32)
        out, ptrs = self._out(vectors.shape[0], k)
        check(lib().ge_ivf_query_vectors(self._h, vectors.ctypes.data_as(C.POINTER(C.c_float)), vectors.shape[0], k, nprobe, *ptrs))
        return out

    def kernel_ms(self):
        """(build, probe, scan, merge) device milliseconds: of creation, and of the last query call"""
        v = [C.c_float() for _ in range(4)]
        check(lib().ge_ivf_last_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def close(self):
        if self._h:
            lib().ge_ivf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _declare_match(L):
    """The matching section of include/geglove.h."""
    vp, i32p, f32p, i64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    L.ge_match_cfg_default.argtypes = [C.POINTER(MatchCfg)]; L.ge_match_cfg_default.restype = None
    L.ge_match_cfg_size.argtypes = []; L.ge_match_cfg_size.restype = C.c_int32
    L.ge_match_summary_size.argtypes = []; L.ge_match_summary_size.restype = C.c_int32
    if L.ge_match_cfg_size() != C.sizeof(MatchCfg) or L.ge_match_summary_size() != C.sizeof(MatchSummary):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_match_cfg is %d bytes there, %d here; "
                          "ge_match_summary %d there, %d here): rebuild with `make -C graph-embeddings_amd/csrc`"
                          % (L.ge_match_cfg_size(), C.sizeof(MatchCfg), L.ge_match_summary_size(), C.sizeof(MatchSummary)))
    L.ge_match_create.argtypes = [f32p, C.c_int64, C.c_int32, i32p, C.c_int64, C.POINTER(MatchCfg), C.POINTER(vp)]
    L.ge_glove_match_create.argtypes = [vp, i32p, C.c_int64, C.POINTER(MatchCfg), C.POINTER(vp)]
    L.ge_match_run.argtypes = [vp, C.c_float, C.c_int64]
    L.ge_match_get.argtypes = [vp, i64p, i64p, C.POINTER(i32p), C.POINTER(i32p), C.POINTER(f32p), C.POINTER(i32p), C.POINTER(MatchSummary)]
    L.ge_match_last_kernel_ms.argtypes = [vp, f32p, f32p, f32p, f32p]
    L.ge_match_destroy.argtypes = [vp]; L.ge_match_destroy.restype = None


class Matching:
    """A ge_match index: Matching.from_rows(rows) / Matching.from_glove(handle), then run(threshold, max_pairs) ->
    (int32[m] a, int32[m] b, float32[m] score, int32[n] label, summary dict): every pair a < b of original row ids whose score
    reaches the threshold, in ascending (a, b), and per indexed position the smallest row id of its connected component.
    More than max_pairs pairs: GeError with status GE_ERR_OVERFLOW; found() then gives the exact number."""

    def __init__(self, handle, stream=None):
        self._h = handle
        self._stream = stream

    @staticmethod
    def _cfg(metric, device, stream):
        cfg = MatchCfg(); lib().ge_match_cfg_default(C.byref(cfg))
        cfg.metric, cfg.device, cfg.stream = NN_METRICS.get(metric, metric), device, stream
        return cfg

    @classmethod
    def from_rows(cls, rows, subset=None, metric="cosine", device=0, stream=None):
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        keep, sub, n_sub = Neighbors._subset(subset)
        h = C.c_void_p()
        check(lib().ge_match_create(rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], rows.shape[1], sub, n_sub,
                                    C.byref(cls._cfg(metric, device, stream)), C.byref(h)))
        return cls(h, stream)

    @classmethod
    def from_glove(cls, glove_handle, subset=None, metric="cosine", stream=None):
        keep, sub, n_sub = Neighbors._subset(subset)
        h = C.c_void_p()
        check(lib().ge_glove_match_create(glove_handle, sub, n_sub, C.byref(cls._cfg(metric, 0, stream)), C.byref(h)))
        return cls(h, stream)

    def found(self):
        """The qualifying pairs of the last run, also after an overflow."""
        n = C.c_int64()
        check(lib().ge_match_get(self._h, None, C.byref(n), None, None, None, None, None))
        return n.value

    def run(self, threshold, max_pairs=1 << 24):
        import numpy as np
        check(lib().ge_match_run(self._h, threshold, max_pairs))
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        n, a, b, score, label, summary = C.c_int64(), i32p(), i32p(), f32p(), i32p(), MatchSummary()
        check(lib().ge_match_get(self._h, C.byref(n), None, C.byref(a), C.byref(b), C.byref(score), C.byref(label), C.byref(summary)))
        m = summary.pairs

        def copy(ptr, count, dtype):          # the views are the handle's: copy them out
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count else np.empty(0, dtype)

        return (copy(a, m, np.int32), copy(b, m, np.int32), copy(score, m, np.float32), copy(label, n.value, np.int32),
                {k: getattr(summary, k) for k, _ in MatchSummary._fields_})

    def kernel_ms(self):
        """(prepare, join, sort, components) device milliseconds: of creation, and of the last run"""
        v = [C.c_float() for _ in range(4)]
        check(lib().ge_match_last_kernel_ms(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def close(self):
        if self._h:
            lib().ge_match_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check(status):
    if status != GE_OK:
        raise GeError(status, lib().ge_last_error().decode(errors="replace"))


def _declare_classify(L):
    """The classification section of include/geglove.h."""
    vp, i32p, i64p, f32p, f64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_double)
    u8p = C.POINTER(C.c_uint8)
    L.ge_classify_cfg_default.argtypes = [C.POINTER(ClassifyCfg)]; L.ge_classify_cfg_default.restype = None
    L.ge_classify_cfg_size.argtypes = []; L.ge_classify_cfg_size.restype = C.c_int32
    if L.ge_classify_cfg_size() != C.sizeof(ClassifyCfg):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_classify_cfg is %d bytes there, %d here): "
                          "rebuild with `make -C graph-embeddings_amd/csrc`" % (L.ge_classify_cfg_size(), C.sizeof(ClassifyCfg)))
    L.ge_classify_create.argtypes = [f32p, C.c_int64, C.c_int32, i32p, C.c_int64, i32p, u8p, C.POINTER(ClassifyCfg), C.POINTER(vp)]
    L.ge_glove_classify_create.argtypes = [vp, i32p, C.c_int64, i32p, u8p, C.POINTER(ClassifyCfg), C.POINTER(vp)]
    L.ge_classify_set_weights.argtypes = [vp, f32p]
    L.ge_classify_eval.argtypes = [vp, f64p, f64p]
    L.ge_classify_run.argtypes = [vp, C.c_int32, i32p, i32p]
    L.ge_classify_predict.argtypes = [vp, i32p, f32p]
    L.ge_classify_score.argtypes = [vp, u8p, C.POINTER(ClassifySummary), i64p]
    L.ge_classify_get.argtypes = [vp, i64p, i32p, i32p, i64p, f32p, i32p, i32p, f64p, i64p]
    L.ge_classify_last_kernel_ms.argtypes = [vp, f32p, f32p, f32p]
    L.ge_classify_destroy.argtypes = [vp]; L.ge_classify_destroy.restype = None


class Classifier:
    """A ge_classifier handle: Classifier.create(rows, labels, classes) / Classifier.create_glove(handle, labels, classes),
    optionally set_weights(values), then eval() -> (loss, gradient), run(max_iter) -> (iterations run, stop), predict() ->
    (labels, probabilities) and score(mask) -> dict."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _cfg(classes, normalize, l2, tolerance, device):
        cfg = ClassifyCfg(); lib().ge_classify_cfg_default(C.byref(cfg))
        cfg.normalize, cfg.classes, cfg.device = CLS_NORMALIZE.get(normalize, normalize), classes, device
        if l2 is not None:
            cfg.l2 = l2
        if tolerance is not None:
            cfg.tolerance = tolerance
        return cfg

    @staticmethod
    def _marks(labels, train):
        import numpy as np
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        keep = [labels]
        tp = None
        if train is not None:
            train = np.ascontiguousarray(train, dtype=np.uint8)
            if train.shape != labels.shape:
                raise ValueError("train must have one entry per label")
            keep.append(train)
            tp = train.ctypes.data_as(C.POINTER(C.c_uint8))
        return keep, labels.ctypes.data_as(C.POINTER(C.c_int32)), tp

    @classmethod
    def create(cls, rows, labels, classes, train=None, subset=None, normalize="cosine", l2=None, tolerance=None, device=0):
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        keep, sub, n_sub = Neighbors._subset(subset)
        n = n_sub if sub is not None else rows.shape[0]
        marks, lp, tp = cls._marks(labels, train)
        if marks[0].shape != (n,):
            raise ValueError("labels must have one entry per indexed row (%d), got %r" % (n, marks[0].shape))
        h = C.c_void_p()
        check(lib().ge_classify_create(rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], rows.shape[1], sub, n_sub, lp, tp,
                                       C.byref(cls._cfg(classes, normalize, l2, tolerance, device)), C.byref(h)))
        return cls(h)

    @classmethod
    def create_glove(cls, glove_handle, labels, classes, train=None, subset=None, normalize="cosine", l2=None, tolerance=None):
        keep, sub, n_sub = Neighbors._subset(subset)
        marks, lp, tp = cls._marks(labels, train)
        h = C.c_void_p()
        check(lib().ge_glove_classify_create(glove_handle, sub, n_sub, lp, tp, C.byref(cls._cfg(classes, normalize, l2, tolerance, 0)),
                                             C.byref(h)))
        return cls(h)

    def get(self):
        """dict: n, dim, classes, n_train, iterations, stop, loss, evaluations"""
        n, nt, ev = C.c_int64(), C.c_int64(), C.c_int64()
        dim, classes, it, stop = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        loss = C.c_double()
        check(lib().ge_classify_get(self._h, C.byref(n), C.byref(dim), C.byref(classes), C.byref(nt), None, C.byref(it), C.byref(stop),
                                    C.byref(loss), C.byref(ev)))
        return {"n": n.value, "dim": dim.value, "classes": classes.value, "n_train": nt.value, "iterations": it.value,
                "stop": CLS_STOPS[stop.value], "loss": loss.value, "evaluations": ev.value}

    @property
    def weights(self):
        """fp32 [classes][dim + 1]: (float) of the master copy; column dim is the bias"""
        import numpy as np
        g = self.get()
        out = np.empty((g["classes"], g["dim"] + 1), dtype=np.float32)
        check(lib().ge_classify_get(self._h, None, None, None, None, out.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, None))
        return out

    def set_weights(self, weights):
        import numpy as np
        g = self.get()
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if weights.shape != (g["classes"], g["dim"] + 1):
            raise ValueError("weights must be %d x %d, got %r" % (g["classes"], g["dim"] + 1, weights.shape))
        check(lib().ge_classify_set_weights(self._h, weights.ctypes.data_as(C.POINTER(C.c_float))))

    def eval(self):
        """(loss, gradient fp64 [classes][dim + 1]) at the current weights; the optimiser's state does not change"""
        import numpy as np
        g = self.get()
        grad = np.empty((g["classes"], g["dim"] + 1), dtype=np.float64)
        loss = C.c_double()
        check(lib().ge_classify_eval(self._h, C.byref(loss), grad.ctypes.data_as(C.POINTER(C.c_double))))
        return loss.value, grad

    def run(self, max_iter=200):
        """Up to max_iter L-BFGS iterations: (iterations run, stop reason)."""
        it, stop = C.c_int32(), C.c_int32()
        check(lib().ge_classify_run(self._h, max_iter, C.byref(it), C.byref(stop)))
        return it.value, CLS_STOPS[stop.value]

    def predict(self):
        """(labels int32 [n], probabilities fp32 [n]) of every position"""
        import numpy as np
        n = self.get()["n"]
        label, prob = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32)
        check(lib().ge_classify_predict(self._h, label.ctypes.data_as(C.POINTER(C.c_int32)), prob.ctypes.data_as(C.POINTER(C.c_float))))
        return label, prob

    def score(self, mask=None, confusion=False):
        """dict: count, correct, accuracy, macro_f1, tp, fp, fn (int64 [classes]) and, when asked for, confusion [true][predicted]"""
        import numpy as np
        g = self.get()
        i64p = C.POINTER(C.c_int64)
        tp, fp, fn = (np.zeros(g["classes"], dtype=np.int64) for _ in range(3))
        s = ClassifySummary()
        s.tp, s.fp, s.fn = (a.ctypes.data_as(i64p) for a in (tp, fp, fn))
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape != (g["n"],):
                raise ValueError("mask must have %d entries, got %r" % (g["n"], mask.shape))
            mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        conf = np.zeros((g["classes"], g["classes"]), dtype=np.int64) if confusion else None
        check(lib().ge_classify_score(self._h, mp, C.byref(s), conf.ctypes.data_as(i64p) if confusion else None))
        out = {"count": s.count, "correct": s.correct, "accuracy": s.accuracy, "macro_f1": s.macro_f1, "tp": tp, "fp": fp, "fn": fn}
        if confusion:
            out["confusion"] = conf
        return out

    @property
    def kernel_ms(self):
        """(logits, softmax, gradient) device milliseconds of the last evaluation"""
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        check(lib().ge_classify_last_kernel_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def close(self):
        if self._h:
            lib().ge_classify_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _declare_align(L):
    """The alignment section of include/geglove.h."""
    vp, i32p, f32p, i64p, u8p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    L.ge_align_cfg_default.argtypes = [C.POINTER(AlignCfg)]; L.ge_align_cfg_default.restype = None
    L.ge_align_cfg_size.argtypes = []; L.ge_align_cfg_size.restype = C.c_int32
    L.ge_align_summary_size.argtypes = []; L.ge_align_summary_size.restype = C.c_int32
    if L.ge_align_cfg_size() != C.sizeof(AlignCfg) or L.ge_align_summary_size() != C.sizeof(AlignSummary):
        raise ImportError("libgeglove.so was built from another revision of include/geglove.h (ge_align_cfg is %d bytes there, %d here; "
                          "ge_align_summary %d there, %d here): rebuild with `make -C graph-embeddings_amd/csrc`"
                          % (L.ge_align_cfg_size(), C.sizeof(AlignCfg), L.ge_align_summary_size(), C.sizeof(AlignSummary)))
    L.ge_align_create.argtypes = [f32p, C.c_int64, C.c_int32, i32p, C.c_int64, i32p, C.c_int64, C.POINTER(AlignCfg), C.POINTER(vp)]
    L.ge_glove_align_create.argtypes = [vp, i32p, C.c_int64, i32p, C.c_int64, C.POINTER(AlignCfg), C.POINTER(vp)]
    L.ge_align_run.argtypes = [vp, C.c_float, C.c_int64]
    L.ge_align_get.argtypes = [vp, i64p, i64p, i64p, C.POINTER(i32p), C.POINTER(i32p), C.POINTER(f32p), C.POINTER(i32p), C.POINTER(f32p),
                               C.POINTER(u8p), C.POINTER(i32p), C.POINTER(AlignSummary)]
    L.ge_align_last_kernel_ms.argtypes = [vp, f32p, f32p, f32p, f32p, i32p]
    L.ge_align_destroy.argtypes = [vp]; L.ge_align_destroy.restype = None


class Alignment:
    """A ge_align index: Alignment.from_rows(rows, source, target) / Alignment.from_glove(handle, source, target), then
    run(threshold, max_pairs) -> (int32[m] a, int32[m] b, float32[m] score, int32[nA] target_of, float32[nA] target_score,
    uint8[nA] flags, int32[nB] source_of, summary dict): every (source, target) pair of original row ids whose score reaches the
    threshold, in ascending (a, b), and the one-to-one assignment a greedy walk in descending score makes of them (flags: bit 0 =
    assigned, bit 1 = mutual).  More than max_pairs candidates: GeError with status GE_ERR_OVERFLOW; found() gives the number."""

    def __init__(self, handle, stream=None):
        self._h = handle
        self._stream = stream

    @staticmethod
    def _cfg(metric, device, stream):
        cfg = AlignCfg(); lib().ge_align_cfg_default(C.byref(cfg))
        cfg.metric, cfg.device, cfg.stream = NN_METRICS.get(metric, metric), device, stream
        return cfg

    @staticmethod
    def _set(ids):
        import numpy as np
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        return ids, ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.size

    @classmethod
    def from_rows(cls, rows, source, target, metric="cosine", device=0, stream=None):
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        (_s, sp, ns), (_t, tp, nt) = cls._set(source), cls._set(target)
        h = C.c_void_p()
        check(lib().ge_align_create(rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], rows.shape[1], sp, ns, tp, nt,
                                    C.byref(cls._cfg(metric, device, stream)), C.byref(h)))
        return cls(h, stream)

    @classmethod
    def from_glove(cls, glove_handle, source, target, metric="cosine", stream=None):
        (_s, sp, ns), (_t, tp, nt) = cls._set(source), cls._set(target)
        h = C.c_void_p()
        check(lib().ge_glove_align_create(glove_handle, sp, ns, tp, nt, C.byref(cls._cfg(metric, 0, stream)), C.byref(h)))
        return cls(h, stream)

    def found(self):
        """The candidates of the last run, also after an overflow."""
        n = C.c_int64()
        check(lib().ge_align_get(self._h, None, None, C.byref(n), None, None, None, None, None, None, None, None))
        return n.value

    def run(self, threshold, max_pairs=1 << 24):
        import numpy as np
        check(lib().ge_align_run(self._h, threshold, max_pairs))
        i32p, f32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        na, nb, summary = C.c_int64(), C.c_int64(), AlignSummary()
        a, b, score, target_of, target_score, flags, source_of = i32p(), i32p(), f32p(), i32p(), f32p(), u8p(), i32p()
        check(lib().ge_align_get(self._h, C.byref(na), C.byref(nb), None, C.byref(a), C.byref(b), C.byref(score), C.byref(target_of),
                                 C.byref(target_score), C.byref(flags), C.byref(source_of), C.byref(summary)))
        m = summary.candidates

        def copy(ptr, count, dtype):          # the views are the handle's: copy them out
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count else np.empty(0, dtype)

        return (copy(a, m, np.int32), copy(b, m, np.int32), copy(score, m, np.float32), copy(target_of, na.value, np.int32),
                copy(target_score, na.value, np.float32), copy(flags, na.value, np.uint8), copy(source_of, nb.value, np.int32),
                {k: getattr(summary, k) for k, _ in AlignSummary._fields_})

    def kernel_ms(self):
        """(prepare, join, sort, assign) device milliseconds and the assignment rounds: of creation, and of the last run"""
        v = [C.c_float() for _ in range(4)]
        rounds = C.c_int32()
        check(lib().ge_align_last_kernel_ms(self._h, *[C.byref(x) for x in v], C.byref(rounds)))
        return tuple(x.value for x in v) + (rounds.value,)

    def close(self):
        if self._h:
            lib().ge_align_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
