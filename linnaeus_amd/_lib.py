"""ctypes binding of liblnx_hip.so (the C ABI declared in include/lnx.h).

The library is the product: there is no Python/CPU fallback.  If it is missing or does not
load, importing anything that needs a kernel raises immediately.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LNX_LIB_PATH") or os.path.join(_HERE, "liblnx_hip.so")  # override: A/B runs against another build

F32, BF16 = 0, 1
ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_BWD, ACT_RELU_BWD, ACT_GELU_D, ACT_MUL_AUX = 0, 1, 2, 3, 4, 5, 6
TN_WS_FLOATS = 256 * (256 * 128 + 256)  # == LNX_TN_WS_FLOATS
DROP_PARTITION_MAX = 64  # == LNX_DROP_PARTITION_MAX


def drop_list_ints(B: int) -> int:  # == LNX_DROP_LIST_INTS(B): nkeep, m_eff, perm[B], inv[B]
    return 2 * B + 2
ADDR_PLAIN, ADDR_PATCH2 = 0, 1


class LnxError(RuntimeError):
    pass


class RowMap(C.Structure):
    _fields_ = [("group", C.c_int), ("pad", C.c_int), ("off", C.c_int)]


class GemmArgs(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("A", C.c_void_p), ("lda", C.c_int64),
        ("W", C.c_void_p), ("ldw", C.c_int64),
        ("C", C.c_void_p), ("ldc", C.c_int64),
        ("out_f32", C.c_int),
        ("a_mode", C.c_int), ("Hin", C.c_int), ("Win", C.c_int), ("Cin", C.c_int),
        ("c_mode", C.c_int), ("c_map", RowMap),
        ("bias", C.c_void_p),
        ("c2", C.c_void_p), ("ldc2", C.c_int64),
        ("act", C.c_int),
        ("aux", C.c_void_p), ("ldaux", C.c_int64),
        ("gamma", C.c_void_p), ("rowscale", C.c_void_p), ("rows_per_sample", C.c_int),
        ("res", C.c_void_p), ("ldres", C.c_int64),
        ("c8", C.c_void_p), ("ldc8", C.c_int64), ("c8_scales", C.c_void_p),
        ("m_dev", C.c_void_p), ("perm", C.c_void_p),
    ]


class WgradArgs(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("dY", C.c_void_p), ("lddy", C.c_int64),
        ("A", C.c_void_p), ("lda", C.c_int64),
        ("a_mode", C.c_int), ("Hin", C.c_int), ("Win", C.c_int), ("Cin", C.c_int),
        ("dW", C.c_void_p), ("lddw", C.c_int64),
        ("k_perm_c", C.c_int),
        ("db", C.c_void_p),
        ("splits", C.c_int),
        ("k_store", C.c_int),
        ("ws", C.c_void_p), ("ws_floats", C.c_int64),
        ("defer", C.c_int),
        ("m_dev", C.c_void_p),
    ]


class TnLaunch(C.Structure):  # == lnx_tn_launch (lnx_gemm_tn_query)
    _fields_ = [("kernel", C.c_int), ("rw", C.c_int), ("cw", C.c_int), ("patch", C.c_int), ("tiles_n", C.c_int), ("tiles_k", C.c_int),
                ("splits", C.c_int), ("m_per_split", C.c_int), ("workspace", C.c_int)]


TN_KERNEL_V1, TN_KERNEL_RING = 1, 2  # lnx_tn_launch.kernel (include/lnx.h)


class SoftCEArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("C", C.c_int),
        ("logits", C.c_void_p), ("ld", C.c_int64),
        ("target", C.c_void_p),
        ("soft", C.c_void_p), ("smoothing", C.c_float),
        ("class_weight", C.c_void_p),
        ("ignore_index", C.c_int64),
        ("row_scale", C.c_void_p), ("scale", C.c_float),
        ("loss", C.c_void_p), ("loss_sum", C.c_void_p),
        ("dlogits", C.c_void_p), ("ldd", C.c_int64),
        ("form", C.c_int), ("soft_target", C.c_void_p), ("ldt", C.c_int64),
        ("tax_anc", C.c_void_p), ("tax_val", C.c_void_p), ("tax_depth", C.c_int),
        ("sum_ws", C.c_void_p),
    ]


# lnx_softce_args.form / lnx_hier_loss_task.form (the LNX_CE_FORM_* enum of include/lnx.h): how the row S is formed
CE_FORM_DEFAULT, CE_FORM_OFF_TARGET, CE_FORM_SOFT_ROW, CE_FORM_TAXONOMY = range(4)
TAX_MAX_DEPTH = 8  # == LNX_TAX_MAX_DEPTH


class TaxonomyRowsArgs(C.Structure):  # == lnx_taxonomy_rows_args
    _fields_ = [("C", C.c_int), ("depth", C.c_int), ("anc", C.c_void_p), ("val", C.c_void_p), ("rows", C.c_void_p), ("n", C.c_int),
                ("out", C.c_void_p), ("ldo", C.c_int64), ("what", C.c_int)]


ADAMW_MAX_GROUPS = 16


class AdamWDesc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("g", C.c_void_p), ("n", C.c_int64), ("group", C.c_int), ("block_start", C.c_int)]


class AdamWHyper(C.Structure):
    _fields_ = [("ngroups", C.c_int)] + [(k, C.c_float * ADAMW_MAX_GROUPS) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "bias_c1", "bias_c2", "omb1", "omb2")]


class AdEMAMixHyper(C.Structure):  # == lnx_ademamix_hyper
    _fields_ = [("ngroups", C.c_int)] + [(k, C.c_float * ADAMW_MAX_GROUPS) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "bias_c1", "bias_c2", "omb1", "omb2",
                                                                                  "alpha_t", "beta3_t", "omb3")]


class SGDHyper(C.Structure):  # == lnx_sgd_hyper
    _fields_ = ([("ngroups", C.c_int)] + [(k, C.c_float * ADAMW_MAX_GROUPS) for k in ("lr", "momentum", "dampening", "weight_decay")] +
                [(k, C.c_int * ADAMW_MAX_GROUPS) for k in ("nesterov", "first")])


class StepGuard(C.Structure):  # == lnx_step_guard (all four: device pointers)
    _fields_ = [("found_inf", C.c_void_p), ("grad_scale", C.c_void_p), ("flag", C.c_void_p), ("skipped", C.c_void_p)]


MUON_TILE = 32  # == LNX_MUON_TILE
MUON_ELEMS = 4096  # == LNX_MUON_ELEMS


class MuonMat(C.Structure):  # == lnx_muon_mat
    _fields_ = [("p", C.c_void_p), ("buf", C.c_void_p), ("g", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("mp", C.c_int), ("np", C.c_int),
                ("x_off", C.c_int64), ("xt_off", C.c_int64 * 2), ("a_off", C.c_int64), ("b_off", C.c_int64),
                ("tile_start", C.c_int * 3), ("tile_count", C.c_int * 3), ("block_start", C.c_int), ("ns_steps", C.c_int), ("nesterov", C.c_int),
                ("momentum", C.c_float), ("omm", C.c_float), ("decay", C.c_float), ("step", C.c_float)]


class MuonTile(C.Structure):  # == lnx_muon_tile
    _fields_ = [("mat", C.c_int), ("tr", C.c_int), ("tc", C.c_int), ("pad", C.c_int)]


class MuonInfo(C.Structure):  # == lnx_muon_info
    _fields_ = [("workspace_bytes", C.c_int64), ("ntiles", C.c_int64 * 3), ("total_blocks", C.c_int)]


class MuonStepArgs(C.Structure):  # == lnx_muon_step_args
    _fields_ = [("n", C.c_int), ("mats", C.c_void_p), ("mats_dev", C.c_void_p), ("tiles_dev", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("partials", C.c_void_p), ("sumsq", C.c_void_p), ("max_norm", C.c_float),
                ("guard", C.POINTER(StepGuard))]


class MuonPacked(C.Structure):  # == lnx_muon_packed
    _fields_ = [("p", C.c_void_p), ("off", C.c_int64), ("numel", C.c_int64), ("decay", C.c_float), ("step", C.c_float), ("block_start", C.c_int)]


MUON_SEG_ALIGN = 128  # == LNX_MUON_SEG_ALIGN
MUON_SHARDED_STRUCTS = {"lnx_muon_packed": MuonPacked}

# the argument structs of include/lnx.h by their C names (tests compare sizeof against a compiled probe)
MUON_STRUCTS = {"lnx_muon_mat": MuonMat, "lnx_muon_tile": MuonTile, "lnx_muon_info": MuonInfo, "lnx_muon_step_args": MuonStepArgs}
GUARD_STRUCTS = {"lnx_step_guard": StepGuard, "lnx_muon_step_args": MuonStepArgs}


class GradNormArgs(C.Structure):  # == lnx_gradnorm_args
    _fields_ = [("T", C.c_int), ("alpha", C.c_float), ("norm", C.c_void_p), ("loss_sum", C.c_void_p), ("count", C.c_void_p), ("init_loss", C.c_void_p),
                ("weights", C.c_void_p), ("initial_losses", C.c_void_p), ("initted", C.c_void_p), ("metrics", C.c_void_p)]


METRICS_MAX_TASKS = 8  # == LNX_SOFTCE_MAX_TASKS
# offsets into the counts / sums tables of lnx_metrics_update (the LNX_METRICS_* enums of include/lnx.h)
METRICS_CHAIN_N, METRICS_CHAIN_CORRECT, METRICS_PARTIAL_N, METRICS_PARTIAL_CORRECT, METRICS_SUBSET_OOR = range(5)
METRICS_HEAD = 8
METRICS_N, METRICS_CORRECT1, METRICS_CORRECT3, METRICS_NULL_N, METRICS_NULL_CORRECT1, METRICS_NONNULL_N, METRICS_NONNULL_CORRECT1, METRICS_LOSS_N = range(8)
METRICS_TASK_STRIDE = 8
METRICS_SUM_LOSS, METRICS_SUM_NULL_LOSS, METRICS_SUM_NONNULL_LOSS = range(3)
METRICS_SUM_STRIDE = 4


def metrics_task(t: int) -> int:  # == LNX_METRICS_TASK
    return METRICS_HEAD + METRICS_TASK_STRIDE * t


def metrics_subset(n_tasks: int, n_bins0: int, s: int) -> int:  # == LNX_METRICS_SUBSET
    return metrics_task(n_tasks) + (2 * n_tasks * n_bins0 if s else 0)


class MetricsTask(C.Structure):  # == lnx_metrics_task
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_int64), ("target", C.c_void_p), ("is_null", C.c_void_p), ("loss", C.c_void_p), ("C", C.c_int)]


class MetricsArgs(C.Structure):  # == lnx_metrics_args
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("n_tasks", C.c_int), ("task", MetricsTask * METRICS_MAX_TASKS),
                ("subset_ids", C.c_void_p * 2), ("n_bins", C.c_int * 2), ("counts", C.c_void_p), ("sums", C.c_void_p)]


PREDICT_MAX_K = 16  # == LNX_PREDICT_MAX_K


class PredictTask(C.Structure):  # == lnx_predict_task
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_int64), ("C", C.c_int), ("parent", C.c_void_p), ("null_index", C.c_int), ("id_map", C.c_void_p)]


class PredictArgs(C.Structure):  # == lnx_predict_args
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("n_tasks", C.c_int), ("K", C.c_int), ("consistency", C.c_int), ("k_per_sample", C.c_void_p),
                ("task", PredictTask * METRICS_MAX_TASKS), ("ids", C.c_void_p), ("probs", C.c_void_p), ("count", C.c_void_p), ("flags", C.c_void_p)]


# lnx_preprocess: filter codes (the LNX_RESIZE_* of include/lnx.h) and the largest side of a source or output image
RESIZE_NEAREST, RESIZE_BILINEAR, RESIZE_BICUBIC = range(3)
PREPROCESS_MAX_SIDE = 16384  # == LNX_PREPROCESS_MAX_SIDE


class PreprocessImage(C.Structure):  # == lnx_preprocess_image
    _fields_ = [("src", C.c_int64), ("hk", C.c_int64), ("hb", C.c_int64), ("vk", C.c_int64), ("vb", C.c_int64), ("scratch", C.c_int64),
                ("h", C.c_int32), ("w", C.c_int32), ("htaps", C.c_int32), ("vtaps", C.c_int32), ("y0", C.c_int32), ("rows", C.c_int32)]


class PreprocessArgs(C.Structure):  # == lnx_preprocess_args
    _fields_ = [("n", C.c_int), ("H", C.c_int), ("W", C.c_int), ("filter", C.c_int), ("images", C.POINTER(PreprocessImage)), ("blob", C.c_void_p),
                ("blob_bytes", C.c_int64), ("images_off", C.c_int64), ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64),
                ("mean", C.c_float * 3), ("std", C.c_float * 3), ("out", C.c_void_p)]


# lnx_hier_loss_fwd / lnx_hier_loss_bwd: rows of ws, offsets into out / counts (the LNX_HL_* enums of include/lnx.h)
HL_WS_RAW, HL_WS_LSE, HL_WS_SS, HL_WS_COEF, HL_WS_MASKED_CW, HL_WS_MASKED_W, HL_WS_FLAGS, HL_WS_ROWS = range(8)
HL_OUT_RAW_MEAN, HL_OUT_MASKED_MEAN, HL_OUT_WEIGHTED, HL_OUT_SCALE = range(4)
HL_OUT_TOTAL, HL_OUT_INCLUSION, HL_OUT_FLOATS = 32, 33, 40
HL_NULL_TOTAL, HL_NULL_INCLUDED, HL_COUNTS = 8, 9, 10


class HierLossTask(C.Structure):  # == lnx_hier_loss_task
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_int64), ("C", C.c_int), ("target", C.c_void_p), ("soft_target", C.c_void_p), ("ldt", C.c_int64),
                ("soft", C.c_void_p), ("smoothing", C.c_float), ("crit_weight", C.c_void_p), ("ignore_index", C.c_int64), ("class_weight", C.c_void_p),
                ("n_cw", C.c_int), ("p_cw", C.c_int), ("p_w", C.c_int), ("dlogits", C.c_void_p), ("ldd", C.c_int64), ("form", C.c_int),
                ("tax_anc", C.c_void_p), ("tax_val", C.c_void_p), ("tax_depth", C.c_int)]


class HierLossArgs(C.Structure):  # == lnx_hier_loss_args
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("n_tasks", C.c_int), ("prob", C.c_float), ("mask_mul", C.c_int), ("draws", C.c_void_p),
                ("weights", C.c_void_p), ("ws", C.c_void_p), ("out", C.c_void_p), ("counts", C.c_void_p), ("task", HierLossTask * METRICS_MAX_TASKS)]


# lnx_hier_refine_level.mode (the LNX_HIER_ROUTE_* enum of include/lnx.h)
HIER_ROUTE_SOFT, HIER_ROUTE_HARD, HIER_ROUTE_GUMBEL = range(3)


class HierRefineLevel(C.Structure):  # == lnx_hier_refine_level
    _fields_ = [("base", C.c_void_p), ("out", C.c_void_p), ("dout", C.c_void_p), ("dbase", C.c_void_p), ("ld", C.c_int64), ("ldd", C.c_int64),
                ("C", C.c_int), ("mode", C.c_int), ("parent", C.c_void_p), ("child_start", C.c_void_p), ("child_idx", C.c_void_p),
                ("noise", C.c_void_p), ("temperature", C.c_float)]


class HierRefineArgs(C.Structure):  # == lnx_hier_refine_args
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("n_tasks", C.c_int), ("stats", C.c_void_p), ("level", HierRefineLevel * METRICS_MAX_TASKS)]


# the argument structs of the hierarchical refinement by their C names (tests compare sizeof against a compiled probe)
HIER_REFINE_STRUCTS = {"lnx_hier_refine_level": HierRefineLevel, "lnx_hier_refine_args": HierRefineArgs}


# lnx_abstain_act / lnx_ppo_advantages / lnx_ppo_loss_fwd / lnx_ppo_loss_bwd (the LNX_ABSTAIN_* and LNX_PPO_* enums of include/lnx.h)
ABSTAIN_MULTITASK, ABSTAIN_SEQUENTIAL = range(2)
ABSTAIN_REWARD_SIMPLE, ABSTAIN_REWARD_OUTCOME = range(2)
ABSTAIN_RANKS_ALL, ABSTAIN_RANKS_FIRST = range(2)
ABSTAIN_CORRECT, ABSTAIN_CORRECT_ABSTAIN, ABSTAIN_MISCLASSIFIED, ABSTAIN_UNNECESSARY_ABSTAIN, ABSTAIN_PREDICTED_AT_NULL, ABSTAIN_OUTCOMES = range(6)
(ABSTAIN_CNT_ABSTAINED, ABSTAIN_CNT_TOTAL, ABSTAIN_CNT_CORRECT_ABSTAIN, ABSTAIN_CNT_UNNECESSARY_ABSTAIN, ABSTAIN_CNT_MISSED_ABSTAIN,
 ABSTAIN_CNT_CORRECT_CLASSIFY, ABSTAIN_CNT_MISCLASSIFY) = range(7)
ABSTAIN_CNT_STRIDE, ABSTAIN_CNT_EPISODES, ABSTAIN_CNT_LENGTH_SUM, ABSTAIN_CNT_REWARD_FIX, ABSTAIN_COUNTS = 8, 64, 65, 66, 72
ABSTAIN_REWARD_FIX_BITS = 20
PPO_WS_LSE, PPO_WS_H, PPO_WS_LOGP, PPO_WS_COEF, PPO_WS_ROWS = range(5)
PPO_OUT_POLICY, PPO_OUT_VALUE, PPO_OUT_ENTROPY, PPO_OUT_TOTAL, PPO_OUT_N, PPO_OUT_RATIO_MEAN, PPO_OUT_CLIP_FRAC = range(7)
PPO_OUT_FLOATS = 8


class AbstainRank(C.Structure):  # == lnx_abstain_rank
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_int64), ("C", C.c_int), ("abstain_index", C.c_int), ("null_index", C.c_int), ("target", C.c_void_p),
                ("dlogits", C.c_void_p), ("ldd", C.c_int64)]


class AbstainActArgs(C.Structure):  # == lnx_abstain_act_args
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("R", C.c_int), ("mode", C.c_int), ("greedy", C.c_int), ("reward_kind", C.c_int),
                ("reward_ranks", C.c_int), ("table", C.c_float * ABSTAIN_OUTCOMES), ("outcome_reward", C.c_float * 2), ("u", C.c_void_p),
                ("actions", C.c_void_p), ("logp", C.c_void_p), ("entropy", C.c_void_p), ("taken", C.c_void_p), ("length", C.c_void_p),
                ("reward", C.c_void_p), ("counts", C.c_void_p), ("rank", AbstainRank * METRICS_MAX_TASKS)]


class PpoAdvArgs(C.Structure):  # == lnx_ppo_adv_args
    _fields_ = [("B", C.c_int), ("R", C.c_int), ("mode", C.c_int), ("gamma", C.c_float), ("gae_lambda", C.c_float), ("reward", C.c_void_p),
                ("value", C.c_void_p), ("length", C.c_void_p), ("adv", C.c_void_p), ("ret", C.c_void_p), ("n_trans", C.c_void_p)]


class PpoLossArgs(C.Structure):  # == lnx_ppo_loss_args
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("R", C.c_int), ("mode", C.c_int), ("clip_eps", C.c_float), ("vf_coef", C.c_float),
                ("ent_coef", C.c_float), ("actions", C.c_void_p), ("taken", C.c_void_p), ("logp_old", C.c_void_p), ("adv", C.c_void_p),
                ("ret", C.c_void_p), ("value", C.c_void_p), ("ws", C.c_void_p), ("out", C.c_void_p), ("dvalue", C.c_void_p),
                ("rank", AbstainRank * METRICS_MAX_TASKS)]


# the argument structs of the abstention phase by their C names (tests compare sizeof against a compiled probe)
ABSTENTION_STRUCTS = {"lnx_abstain_rank": AbstainRank, "lnx_abstain_act_args": AbstainActArgs, "lnx_ppo_adv_args": PpoAdvArgs,
                      "lnx_ppo_loss_args": PpoLossArgs}


_lib = None


def lib() -> C.CDLL:
    """Load the HIP library or fail loudly (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LnxError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C linnaeus_amd/csrc`). linnaeus_amd has no CPU fallback."
            )
        _lib = C.CDLL(LIB_PATH)
        _lib.lnx_last_error.restype = C.c_char_p
        _lib.lnx_nt_kernel_launches.restype = C.c_int64
        _lib.lnx_convmlp_bwd_ws_floats.restype = C.c_int64
        _lib.lnx_meta_heads_bwd_part_floats.restype = C.c_int64
        if hasattr(_lib, "lnx_set_deterministic"):
            _lib.lnx_dwconv7_wgrad_ws_floats.restype = C.c_int64
            _lib.lnx_layerscale_bwd_ws_floats.restype = C.c_int64
        _lib.lnx_attn_bwd_ws_floats.restype = C.c_int64
        _lib.lnx_attn_bwd_ws_floats_hd.restype = C.c_int64
        if hasattr(_lib, "lnx_ademamix_step"):
            _lib.lnx_ademamix_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(AdEMAMixHyper), C.c_void_p, C.c_float, C.c_void_p]
        if hasattr(_lib, "lnx_sgd_step"):
            _lib.lnx_sgd_step.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(SGDHyper), C.c_void_p, C.c_float, C.c_void_p]
            _lib.lnx_optim_launches.restype = C.c_int64
        if hasattr(_lib, "lnx_muon_step"):
            _lib.lnx_muon_layout.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(MuonInfo)]
            _lib.lnx_muon_step.argtypes = [C.POINTER(MuonStepArgs), C.c_void_p]
            _lib.lnx_muon_launches.restype = C.c_int64
        if hasattr(_lib, "lnx_muon_partition"):
            _lib.lnx_muon_partition.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
            _lib.lnx_muon_orthogonalize.argtypes = [C.POINTER(MuonStepArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
            _lib.lnx_muon_apply_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.POINTER(StepGuard), C.c_void_p]
        if hasattr(_lib, "lnx_grad_sumsq_guarded"):
            guard = C.POINTER(StepGuard)
            _lib.lnx_grad_sumsq_guarded.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, guard, C.c_void_p]
            _lib.lnx_adamw_step_guarded.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(AdamWHyper), C.c_void_p, C.c_float, guard, C.c_void_p]
            _lib.lnx_ademamix_step_guarded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(AdEMAMixHyper), C.c_void_p, C.c_float, guard, C.c_void_p]
            _lib.lnx_sgd_step_guarded.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(SGDHyper), C.c_void_p, C.c_float, guard, C.c_void_p]
        if hasattr(_lib, "lnx_gradnorm_sumsq"):
            _lib.lnx_gradnorm_sumsq.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(_lib, "lnx_metrics_update"):
            _lib.lnx_metrics_update.argtypes = [C.POINTER(MetricsArgs), C.c_void_p]
            _lib.lnx_metrics_table_sizes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        if hasattr(_lib, "lnx_predict"):
            _lib.lnx_predict.argtypes = [C.POINTER(PredictArgs), C.c_void_p]
            _lib.lnx_predict.restype = C.c_int
        if hasattr(_lib, "lnx_hier_loss_fwd"):
            _lib.lnx_hier_loss_fwd.argtypes = [C.POINTER(HierLossArgs), C.c_void_p]
            _lib.lnx_hier_loss_bwd.argtypes = [C.POINTER(HierLossArgs), C.c_void_p, C.c_void_p]
        if hasattr(_lib, "lnx_taxonomy_rows"):
            _lib.lnx_taxonomy_rows.argtypes = [C.POINTER(TaxonomyRowsArgs), C.c_void_p]
        if hasattr(_lib, "lnx_hier_refine_fwd"):
            _lib.lnx_hier_refine_fwd.argtypes = [C.POINTER(HierRefineArgs), C.c_void_p]
            _lib.lnx_hier_refine_bwd.argtypes = [C.POINTER(HierRefineArgs), C.c_void_p]
            _lib.lnx_hier_refine_launches.restype = C.c_int64
        if hasattr(_lib, "lnx_abstain_act"):
            _lib.lnx_abstain_act.argtypes = [C.POINTER(AbstainActArgs), C.c_void_p]
            _lib.lnx_ppo_advantages.argtypes = [C.POINTER(PpoAdvArgs), C.c_void_p]
            _lib.lnx_ppo_loss_fwd.argtypes = [C.POINTER(PpoLossArgs), C.c_void_p]
            _lib.lnx_ppo_loss_bwd.argtypes = [C.POINTER(PpoLossArgs), C.c_void_p, C.c_void_p]
            _lib.lnx_abstain_launches.restype = C.c_int64
        if hasattr(_lib, "lnx_preprocess"):
            _lib.lnx_resize_taps.argtypes = [C.c_int, C.c_int, C.c_int]
            _lib.lnx_resize_coeffs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            _lib.lnx_preprocess_scratch_bytes.argtypes = [C.POINTER(PreprocessImage), C.c_int, C.c_int, C.c_int, C.c_int]
            _lib.lnx_preprocess_scratch_bytes.restype = C.c_int64
            _lib.lnx_preprocess.argtypes = [C.POINTER(PreprocessArgs), C.c_void_p]
            _lib.lnx_preprocess.restype = C.c_int
        if hasattr(_lib, "lnx_meta_mask"):
            _lib.lnx_meta_mask.argtypes = [C.POINTER(MetaMaskArgs), C.c_void_p]
            _lib.lnx_meta_mask.restype = C.c_int
        if hasattr(_lib, "lnx_drop_partition"):
            _lib.lnx_drop_partition.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
            _lib.lnx_copy_dropped_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
            _lib.lnx_drop_compact_branches.restype = C.c_int64
            if hasattr(_lib, "lnx_drop_compact_conv_blocks"):
                _lib.lnx_drop_compact_conv_blocks.restype = C.c_int64
                _lib.lnx_dwconv7_fwd_kept.argtypes = [C.POINTER(DwconvArgs), C.c_void_p, C.c_void_p, C.c_void_p]
                _lib.lnx_dwconv7_wgrad_kept.argtypes = [C.POINTER(DwconvWgradArgs), C.c_void_p, C.c_void_p, C.c_void_p]
            _lib.lnx_scale_cast_compact.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int,
                                                    C.c_void_p]
        if hasattr(_lib, "lnx_last_cls_blocks"):
            _lib.lnx_set_last_cls.argtypes = [C.c_int]
            _lib.lnx_last_cls_blocks.restype = C.c_int64
        if hasattr(_lib, "lnx_plan_forward_tail"):
            _lib.lnx_plan_forward_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            _lib.lnx_plan_trunk_valid.argtypes = [C.c_void_p]
        if hasattr(_lib, "lnx_plan_set_trainable"):
            _lib.lnx_plan_unit_name.argtypes = [C.c_void_p, C.c_int]
            _lib.lnx_plan_unit_name.restype = C.c_char_p
            _lib.lnx_plan_set_trainable.argtypes = [C.c_void_p, C.c_char_p]
        if hasattr(_lib, "lnx_plan_set_input_grads"):
            _lib.lnx_plan_set_input_grads.argtypes = [C.c_void_p, C.c_int, C.c_int]
            _lib.lnx_plan_input_grads.argtypes = [C.c_void_p]
            _lib.lnx_plan_bind_input_grads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            _lib.lnx_stem_dgrad.argtypes = [C.POINTER(StemDgradArgs), C.c_void_p]
            _lib.lnx_col2im_stem.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            _lib.lnx_meta_input_grad.argtypes = [C.POINTER(MetaInputGradArgs), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        if hasattr(_lib, "lnx_gemm_tn_query"):
            _lib.lnx_gemm_tn_query.argtypes = [C.POINTER(WgradArgs), C.POINTER(TnLaunch)]
        if hasattr(_lib, "lnx_layernorm_fwd_query"):
            _lib.lnx_layernorm_fwd_query.argtypes = [C.POINTER(LnArgs), C.POINTER(LnLaunch)]
            _lib.lnx_layernorm_bwd_query.argtypes = [C.POINTER(LnBwdArgs), C.POINTER(LnLaunch)]
        # A/B runs against an OLDER build (LNX_LIB_PATH=... LNX_LIB_OLDER=1): entry points added since are allowed to be missing; calling
        # one then fails with ctypes' AttributeError
        older = bool(os.environ.get("LNX_LIB_PATH")) and os.environ.get("LNX_LIB_OLDER") == "1"
        for name in EXPORTS:
            if not hasattr(_lib, name) and not older:
                raise LnxError(f"{LIB_PATH} does not export {name}; rebuild it")
    return _lib


def set_deterministic(on: bool) -> bool:
    """Switch the library's deterministic mode (include/lnx.h: lnx_set_deterministic); returns the previous setting.  Plans and scratch
    sized before the switch do not fit the other setting: models go through `mFormerV1.set_deterministic`, which rebuilds its plans."""
    return bool(lib().lnx_set_deterministic(1 if on else 0))


def is_deterministic() -> bool:
    return bool(lib().lnx_get_deterministic())


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise LnxError(f"{what} failed (rc={rc}): {lib().lnx_last_error().decode()}")


# lnx_aug_pointwise operations (include/lnx.h)
AUG_CLAMP, AUG_POSTERIZE, AUG_SOLARIZE, AUG_SOLARIZE_ADD, AUG_INVERT, AUG_BRIGHTNESS, AUG_CONTRAST = range(7)

# lnx_last_nt_kernel / lnx_nt_kernel_launches kinds (include/lnx.h)
NT_KERNEL_NONE, NT_KERNEL_V1, NT_KERNEL_V2, NT_KERNEL_SKINNY, NT_KERNEL_V4, NT_KERNEL_FP8, NT_KERNEL_V7, NT_KERNEL_MX8, NT_KERNEL_V9, NT_KERNEL_EXPERIMENT = 0, 1, 2, 3, 4, 6, 7, 8, 9, 15

# lnx_attn_dispatch / lnx_last_attn_kernel families (include/lnx.h)
# rope_mode of the attention structs, the table entries and lnx_mformer_cfg (include/lnx.h): cos-only scaling (the reference as it
# runs, finding F1) or the true pair rotation
ROPE_COS, ROPE_ROTATE = 0, 1

ATTN_KERNEL_NONE, ATTN_KERNEL_RES4, ATTN_KERNEL_RES8, ATTN_KERNEL_TILED4, ATTN_KERNEL_TILED8 = range(5)

# every symbol include/lnx.h declares (kept in sync by tests/test_abi.py)
EXPORTS = [
    "lnx_last_error", "lnx_version", "lnx_device_cus", "lnx_set_cu_margin", "lnx_set_deterministic", "lnx_get_deterministic", "lnx_tile_sched_static",
    "lnx_gemm_nt", "lnx_last_nt_kernel", "lnx_nt_kernel_launches", "lnx_nt_dispatch", "lnx_gemm_tn", "lnx_gemm_tn_query", "lnx_gemm_tn_flush", "lnx_gemm_tn_discard", "lnx_amax", "lnx_quantize_fp8", "lnx_gemm_nt_fp8", "lnx_quantize_mxfp8", "lnx_gemm_nt_mxfp8", "lnx_dropout_mul", "lnx_dropout_residual", "lnx_plan_dropout_bytes", "lnx_plan_set_dropout", "lnx_plan_attn_dropout_bytes", "lnx_plan_set_attn_dropout",
    "lnx_layernorm_fwd", "lnx_layernorm_bwd", "lnx_layernorm_bwd_flush", "lnx_layernorm_bwd_discard", "lnx_layernorm_fwd_query", "lnx_layernorm_bwd_query",
    "lnx_dwconv7_fwd", "lnx_dwconv7_fwd_kept", "lnx_dwconv7_wgrad", "lnx_dwconv7_wgrad_kept", "lnx_dwconv7_wgrad_ws_floats",
    "lnx_gemm_nt_group_ok", "lnx_gemm_nt_group", "lnx_rope_cos_table", "lnx_rope_cos_table_hd", "lnx_rope_cossin_table_hd", "lnx_rope_cos_tables", "lnx_attn_bwd_ws_floats", "lnx_attn_bwd_ws_floats_hd", "lnx_attn_fwd", "lnx_attn_bwd", "lnx_attn_bwd_sized", "lnx_attn_fwd_compact", "lnx_attn_bwd_compact", "lnx_attn_bwd_flush", "lnx_attn_bwd_discard", "lnx_attn_dispatch", "lnx_last_attn_kernel", "lnx_last_attn_bwd_launches",
    "lnx_im2col_stem", "lnx_scale_cast", "lnx_scale_cast_compact", "lnx_drop_partition", "lnx_copy_dropped_rows", "lnx_set_drop_compact", "lnx_drop_compact_branches", "lnx_drop_compact_conv_blocks", "lnx_set_last_cls", "lnx_last_cls_blocks", "lnx_layerscale_bwd", "lnx_layerscale_bwd_ws", "lnx_layerscale_bwd_ws_floats", "lnx_layerscale_apply_wgrad", "lnx_fill_rows", "lnx_colsum_rows",
    "lnx_agg2_fwd", "lnx_agg2_bwd", "lnx_pack_meta", "lnx_meta_heads_supported", "lnx_meta_heads_fwd", "lnx_meta_heads_bwd", "lnx_meta_heads_bwd_part_floats", "lnx_prep_weights", "lnx_prep_blocks", "lnx_softce", "lnx_softce_multi", "lnx_taxonomy_rows", "lnx_stem_fwd", "lnx_stem_fwd_ok", "lnx_adamw_blocks", "lnx_grad_sumsq", "lnx_adamw_step", "lnx_ademamix_step", "lnx_sgd_step", "lnx_optim_launches", "lnx_grad_sumsq_guarded", "lnx_adamw_step_guarded", "lnx_ademamix_step_guarded", "lnx_sgd_step_guarded", "lnx_muon_layout", "lnx_muon_step", "lnx_muon_launches", "lnx_muon_partition", "lnx_muon_orthogonalize", "lnx_muon_apply_packed", "lnx_gradnorm_sumsq", "lnx_gradnorm_update",
    "lnx_metrics_table_sizes", "lnx_metrics_update", "lnx_predict", "lnx_resize_taps", "lnx_resize_coeffs", "lnx_preprocess_scratch_bytes", "lnx_preprocess", "lnx_hier_loss_fwd", "lnx_hier_loss_bwd",
    "lnx_hier_refine_fwd", "lnx_hier_refine_bwd", "lnx_hier_refine_launches",
    "lnx_abstain_act", "lnx_ppo_advantages", "lnx_ppo_loss_fwd", "lnx_ppo_loss_bwd", "lnx_abstain_launches",
    "lnx_mix_rows", "lnx_mix_meta", "lnx_meta_mask",
    "lnx_aug_pointwise", "lnx_aug_saturation", "lnx_aug_rowstat", "lnx_aug_rescale", "lnx_aug_affine", "lnx_aug_stencil", "lnx_erase_rects", "lnx_u8hwc_to_f32chw",
    "lnx_convmlp_supported", "lnx_convmlp_fwd", "lnx_convmlp_bwd", "lnx_convmlp_bwd_ws_floats",
    "lnx_plan_create", "lnx_plan_destroy", "lnx_plan_workspace_bytes", "lnx_plan_num_params", "lnx_plan_param_name",
    "lnx_plan_param_numel", "lnx_plan_num_drop_calls", "lnx_plan_logits_numel", "lnx_plan_logits_offset", "lnx_plan_logits_ld",
    "lnx_plan_bind", "lnx_plan_forward", "lnx_plan_forward_tail", "lnx_plan_trunk_valid", "lnx_plan_backward", "lnx_plan_backward_into", "lnx_plan_segment_params", "lnx_plan_profile_begin", "lnx_plan_profile_end", "lnx_plan_profile_begin_spans", "lnx_plan_profile_end_ex", "lnx_plan_set_wgrad_stream", "lnx_plan_set_meta_stream",
    "lnx_plan_num_units", "lnx_plan_unit_name", "lnx_plan_param_unit", "lnx_plan_set_trainable", "lnx_plan_first_trained_unit", "lnx_plan_last_backward_units",
    "lnx_stem_dgrad_ok", "lnx_stem_dgrad", "lnx_col2im_stem", "lnx_meta_input_grad", "lnx_plan_set_input_grads", "lnx_plan_input_grads", "lnx_plan_bind_input_grads",
]


class MetaHeadArgs(C.Structure):  # == lnx_meta_head_args
    _fields_ = [
        ("B", C.c_int), ("C", C.c_int), ("dim", C.c_int), ("off", C.c_int),
        ("meta", C.c_void_p), ("meta_width", C.c_int), ("eps", C.c_float),
        ("w0", C.c_void_p), ("ldw0", C.c_int), ("b0", C.c_void_p), ("ln0_w", C.c_void_p), ("ln0_b", C.c_void_p),
        ("w1", C.c_void_p), ("ldw1", C.c_int), ("b1", C.c_void_p), ("ln1_w", C.c_void_p), ("ln1_b", C.c_void_p),
        ("w2", C.c_void_p), ("ldw2", C.c_int), ("b2", C.c_void_p), ("ln2_w", C.c_void_p), ("ln2_b", C.c_void_p),
        ("t0", C.c_void_p), ("h0", C.c_void_p), ("x", C.c_void_p), ("h1", C.c_void_p), ("n1", C.c_void_p), ("h2", C.c_void_p),
        ("m0", C.c_void_p), ("r0", C.c_void_p), ("m1", C.c_void_p), ("r1", C.c_void_p), ("m2", C.c_void_p), ("r2", C.c_void_p),
        ("tok", C.c_void_p), ("tok_row_stride", C.c_int64), ("tok_row_offset", C.c_int64),
    ]


class MetaHeadBwdArgs(C.Structure):  # == lnx_meta_head_bwd_args
    _fields_ = [
        ("B", C.c_int), ("C", C.c_int), ("dim", C.c_int),
        ("g", C.c_void_p), ("g_row_stride", C.c_int64), ("g_row_offset", C.c_int64),
        ("w1t", C.c_void_p), ("ldw1t", C.c_int), ("w2t", C.c_void_p), ("ldw2t", C.c_int),
        ("ln0_w", C.c_void_p), ("ln1_w", C.c_void_p), ("ln2_w", C.c_void_p),
        ("t0", C.c_void_p), ("h0", C.c_void_p), ("x", C.c_void_p), ("h1", C.c_void_p), ("n1", C.c_void_p), ("h2", C.c_void_p),
        ("m0", C.c_void_p), ("r0", C.c_void_p), ("m1", C.c_void_p), ("r1", C.c_void_p), ("m2", C.c_void_p), ("r2", C.c_void_p),
        ("dp2", C.c_void_p), ("dp1", C.c_void_p), ("dp0", C.c_void_p), ("part", C.c_void_p),
        ("d_w0", C.c_void_p), ("d_b0", C.c_void_p), ("d_ln0_w", C.c_void_p), ("d_ln0_b", C.c_void_p),
        ("d_w1", C.c_void_p), ("d_b1", C.c_void_p), ("d_ln1_w", C.c_void_p), ("d_ln1_b", C.c_void_p),
        ("d_w2", C.c_void_p), ("d_b2", C.c_void_p), ("d_ln2_w", C.c_void_p), ("d_ln2_b", C.c_void_p),
    ]


class LnArgs(C.Structure):
    _fields_ = [
        ("M", C.c_int), ("C", C.c_int), ("eps", C.c_float),
        ("x", C.c_void_p), ("x_dtype", C.c_int), ("ldx", C.c_int64), ("x_map", RowMap),
        ("w", C.c_void_p), ("b", C.c_void_p),
        ("y", C.c_void_p), ("y_dtype", C.c_int), ("ldy", C.c_int64), ("y_map", RowMap),
        ("add", C.c_void_p), ("ldadd", C.c_int64),
        ("mean", C.c_void_p), ("rstd", C.c_void_p),
        ("y8", C.c_void_p), ("ldy8", C.c_int64), ("y8_scales", C.c_void_p),
        ("perm", C.c_void_p), ("m_dev", C.c_void_p), ("rows_per_sample", C.c_int),
    ]


class LnBwdArgs(C.Structure):
    _fields_ = [
        ("M", C.c_int), ("C", C.c_int),
        ("dy", C.c_void_p), ("dy_dtype", C.c_int), ("lddy", C.c_int64), ("dy_map", RowMap),
        ("x", C.c_void_p), ("x_dtype", C.c_int), ("ldx", C.c_int64), ("x_map", RowMap),
        ("w", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
        ("gin", C.c_void_p), ("ldgin", C.c_int64),
        ("dx", C.c_void_p), ("dx_dtype", C.c_int), ("lddx", C.c_int64),
        ("dw", C.c_void_p), ("db", C.c_void_p), ("relu_mask", C.c_int),
        ("ws", C.c_void_p), ("ws_floats", C.c_int64),
        ("dx2", C.c_void_p), ("dx2_dtype", C.c_int), ("lddx2", C.c_int64), ("dx2_rowscale", C.c_void_p), ("dx2_rows_per_sample", C.c_int),
        ("dx2_8", C.c_void_p), ("dx2_8_scales", C.c_void_p), ("lddx2_8", C.c_int64),
        ("defer", C.c_int),
        ("perm", C.c_void_p), ("m_dev", C.c_void_p), ("dx2_inv", C.c_void_p), ("dx2_nkeep", C.c_void_p),
    ]


# lnx_layernorm_fwd_query / lnx_layernorm_bwd_query: the column-sum route (the LNX_LN_COLS_* of include/lnx.h)
LN_COLS_NONE, LN_COLS_ATOMICS, LN_COLS_WORKSPACE = range(3)


class LnLaunch(C.Structure):  # == lnx_ln_launch
    _fields_ = [("G", C.c_int), ("V", C.c_int), ("pair", C.c_int), ("full", C.c_int), ("mx", C.c_int), ("grid", C.c_int), ("cols", C.c_int), ("slices", C.c_int)]


class RopeTable(C.Structure):
    _fields_ = [
        ("freqs", C.c_void_p), ("cos_out", C.c_void_p), ("dsin_out", C.c_void_p),
        ("heads", C.c_int), ("H", C.c_int), ("W", C.c_int), ("head_dim", C.c_int),
        ("rope_mode", C.c_int), ("sin_out", C.c_void_p),
    ]


class DwconvArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int),
        ("x", C.c_void_p), ("x_dtype", C.c_int), ("w49", C.c_void_p), ("bias", C.c_void_p),
        ("flip", C.c_int), ("res", C.c_void_p), ("y", C.c_void_p), ("y_dtype", C.c_int),
    ]


class DwconvWgradArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int),
        ("x", C.c_void_p), ("x_dtype", C.c_int), ("dy", C.c_void_p), ("dy_dtype", C.c_int),
        ("dw", C.c_void_p), ("db", C.c_void_p),
        ("ws", C.c_void_p), ("ws_floats", C.c_int64),
    ]


class AttnArgs(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("B", C.c_int), ("N", C.c_int), ("E", C.c_int), ("heads", C.c_int),
        ("qkv", C.c_void_p), ("cos_tab", C.c_void_p), ("o", C.c_void_p), ("lse", C.c_void_p),
        ("drop_mask", C.c_void_p), ("drop_inv_keep", C.c_float), ("head_dim", C.c_int),
        ("rope_mode", C.c_int), ("sin_tab", C.c_void_p),
    ]


class AttnBwdArgs(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("B", C.c_int), ("N", C.c_int), ("E", C.c_int), ("heads", C.c_int),
        ("qkv", C.c_void_p), ("cos_tab", C.c_void_p), ("o", C.c_void_p), ("lse", C.c_void_p),
        ("d_o", C.c_void_p), ("dqkv", C.c_void_p), ("freq_ws", C.c_void_p), ("delta", C.c_void_p),
        ("drop_mask", C.c_void_p), ("drop_inv_keep", C.c_float),
        ("dsin_tab", C.c_void_p), ("dfreqs", C.c_void_p), ("defer_freqs", C.c_int), ("head_dim", C.c_int),
        ("rope_mode", C.c_int), ("sin_tab", C.c_void_p), ("grid_w", C.c_int),
    ]


class PrepDesc(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("dst", C.c_void_p), ("dst_t", C.c_void_p),
        ("rows", C.c_int), ("cols", C.c_int), ("ld", C.c_int), ("ld_t", C.c_int),
        ("P", C.c_int), ("mode", C.c_int), ("block_start", C.c_int),
    ]


PREP_CAST, PREP_CONV_PERM, PREP_DW49 = 0, 1, 2


class ConvMlpArgs(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("M", C.c_int), ("C", C.c_int),
        ("ln", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
        ("gamma", C.c_void_p), ("rowscale", C.c_void_p), ("rows_per_sample", C.c_int),
        ("x", C.c_void_p), ("out", C.c_void_p), ("z", C.c_void_p),
        ("y", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("ln_eps", C.c_float), ("ln_out", C.c_void_p),
        ("mean", C.c_void_p), ("rstd", C.c_void_p),
        ("perm", C.c_void_p), ("m_dev", C.c_void_p),
    ]


class ConvMlpBwdArgs(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("M", C.c_int), ("C", C.c_int),
        ("g", C.c_void_p), ("ln", C.c_void_p), ("z", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p),
        ("w2t", C.c_void_p), ("w1t", C.c_void_p), ("gamma", C.c_void_p), ("rowscale", C.c_void_p), ("rows_per_sample", C.c_int),
        ("act", C.c_void_p), ("dh", C.c_void_p), ("dz", C.c_void_p), ("dln", C.c_void_p), ("dgamma", C.c_void_p),
        ("y", C.c_void_p), ("ln_w", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("d_ln_w", C.c_void_p), ("d_ln_b", C.c_void_p),
        ("ws", C.c_void_p), ("ws_floats", C.c_int64),
        ("dz_plain", C.c_int), ("ln_defer", C.c_int),
        ("perm", C.c_void_p), ("m_dev", C.c_void_p),
    ]


class StemArgs(C.Structure):  # == lnx_stem_args
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("patches", C.c_void_p),
                ("pre", C.c_void_p), ("y", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("B", C.c_int), ("Cin", C.c_int), ("H", C.c_int),
                ("W", C.c_int), ("Cout", C.c_int), ("eps", C.c_float)]


class StemDgradArgs(C.Structure):  # == lnx_stem_dgrad_args
    _fields_ = [("dtype", C.c_int), ("B", C.c_int), ("Cin", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Cout", C.c_int),
                ("dy", C.c_void_p), ("ldy", C.c_int64), ("w", C.c_void_p), ("dx", C.c_void_p)]


class MetaInputGradArgs(C.Structure):  # == lnx_meta_input_grad_args
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("dim", C.c_int), ("off", C.c_int), ("dp0", C.c_void_p), ("lddp0", C.c_int64), ("w0", C.c_void_p), ("ldw0", C.c_int)]


class MixArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("perm", C.c_void_p), ("valid", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int), ("row", C.c_int64), ("H", C.c_int), ("W", C.c_int), ("lam", C.c_float),
        ("h0", C.c_int), ("h1", C.c_int), ("w0", C.c_int), ("w1", C.c_int), ("mode", C.c_int),
    ]


META_MASK_MAX_COMPONENTS = 32  # == LNX_META_MASK_MAX_COMPONENTS


class MetaMaskArgs(C.Structure):  # == lnx_meta_mask_args
    _fields_ = [
        ("aux", C.c_void_p), ("mask", C.c_void_p), ("out_aux", C.c_void_p), ("out_mask", C.c_void_p),
        ("B", C.c_int), ("D", C.c_int), ("bounds", C.c_void_p), ("ncomp", C.c_int), ("ncombo", C.c_int),
        ("combo_bits", C.c_void_p), ("combo_thr", C.c_void_p), ("draws", C.c_void_p), ("combo_idx", C.c_void_p),
        ("p_full", C.c_float), ("p_partial", C.c_float), ("partial_on", C.c_int), ("row_bits", C.c_uint), ("row_full", C.c_int),
        ("counts", C.c_void_p), ("row_combo", C.c_void_p),
    ]
