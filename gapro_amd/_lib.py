"""ctypes binding of libgapro_hip.so (the C ABI declared in include/gapro_hip.h).

The library is the product: there is no Python/NumPy/torch fallback for the hot path.  If the
shared object is missing or cannot be loaded this module raises at import of the first symbol.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgapro_hip.so")

GAPRO_OK = 0
GAPRO_ERR_BAD_ARG = -1
GAPRO_ERR_NOT_FINITE = -4
GAPRO_ERR_CHOLESKY = -5
STATUS_NAMES = {0: "OK", -1: "BAD_ARG", -2: "OOM", -3: "HIP", -4: "NOT_FINITE", -5: "CHOLESKY", -6: "SPP_RANGE",
                -7: "WORKSPACE", -8: "TIMEOUT", -9: "IO", -10: "UNSUPPORTED"}
GAPRO_ERR_WORKSPACE = -7
GAPRO_ERR_TIMEOUT = -8
GAPRO_ERR_IO = -9
GAPRO_ERR_UNSUPPORTED = -10


class GaproError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("libgapro_hip: %s (%d) %s" % (STATUS_NAMES.get(code, "?"), code, msg))
        self.code = code


class SceneHeader(C.Structure):
    _fields_ = [("coord_min", C.c_double * 3), ("coord_max", C.c_double * 3), ("spp_min", C.c_int64),
                ("spp_max", C.c_int64), ("feat_absmax", C.c_float), ("fixed_shift", C.c_int32),
                ("n_spps", C.c_int32), ("status", C.c_int32)]


class ScheduleCounts(C.Structure):
    _fields_ = [("n_events", C.c_int32), ("n_fits", C.c_int32), ("n_event_idx", C.c_int64),
                ("n_fit_idx", C.c_int64), ("n_fit_out", C.c_int64), ("max_m", C.c_int32), ("max_t", C.c_int32)]


class FitDesc(C.Structure):
    _fields_ = [("m1", C.c_int32), ("m2", C.c_int32), ("t", C.c_int32), ("b1", C.c_int32), ("b2", C.c_int32),
                ("scene", C.c_int32), ("slot", C.c_int32), ("reserved", C.c_int32), ("idx_offset", C.c_int64),
                ("out_offset", C.c_int64),
                ("ws_offset", C.c_int64)]


class FitLaunchStep(C.Structure):
    """gapro_fit_launch_step: one kernel launch of a fit batch, as gapro_fit_launch_plan reports it."""
    _fields_ = [("kernel", C.c_int32), ("variant", C.c_int32), ("first", C.c_int32), ("count", C.c_int32),
                ("grid", C.c_int32), ("stream", C.c_int32), ("ticket", C.c_int32), ("timing", C.c_int32),
                ("wait_gate", C.c_int32), ("reserved", C.c_int32), ("lds_bytes", C.c_int64)]


FIT_STEP_COPY_FREE = 8
FIT_MAX_STEPS = 10


class PredictDesc(C.Structure):
    """gapro_predict_desc: one model of a gapro_svgp_predict_batch launch."""
    _fields_ = [("state_offset", C.c_int64), ("row_offset", C.c_int64), ("out_offset", C.c_int64), ("t", C.c_int32),
                ("reserved", C.c_int32)]


class PointRefineScene(C.Structure):
    """gapro_point_refine_scene: one scene of gapro_point_refine_gather / gapro_point_refine_apply."""
    _fields_ = [("n_points", C.c_int64), ("n_spps", C.c_int32), ("reserved", C.c_int32), ("spp_inv", C.c_void_p),
                ("feats", C.c_void_p), ("sp_row", C.c_void_p), ("cursor", C.c_void_p), ("mu_spp", C.c_void_p),
                ("var_spp", C.c_void_p), ("sem", C.c_void_p), ("inst", C.c_void_p), ("prob", C.c_void_p),
                ("mu", C.c_void_p), ("var", C.c_void_p)]


class PointRefineModel(C.Structure):
    """gapro_point_refine_model: one predict model of a point-level launch, as gapro_point_refine_apply reads it."""
    _fields_ = [("row_offset", C.c_int64), ("t", C.c_int32), ("scene", C.c_int32), ("sem1", C.c_int32),
                ("inst1", C.c_int32), ("sem2", C.c_int32), ("inst2", C.c_int32)]


class PointRefineBlock(C.Structure):
    """gapro_point_refine_block: the gathered rows of one refined superpoint and its segments (point_level="compete")."""
    _fields_ = [("row_start", C.c_int64), ("n_rows", C.c_int32), ("scene", C.c_int32), ("seg_start", C.c_int32),
                ("n_seg", C.c_int32)]


class PointRefineSegment(C.Structure):
    """gapro_point_refine_segment: one (tester fit, refined superpoint) pair of the expanded predict launch."""
    _fields_ = [("out_start", C.c_int64), ("model", C.c_int32), ("reserved", C.c_int32)]


class PointRefineVoteScene(C.Structure):
    """gapro_point_refine_vote_scene: the superpoint-level label tables of one scene (point_level="vote")."""
    _fields_ = [("sem_spp", C.c_void_p), ("inst_spp", C.c_void_p), ("prob_spp", C.c_void_p), ("mu_spp", C.c_void_p),
                ("var_spp", C.c_void_p), ("n_spps", C.c_int32), ("reserved", C.c_int32)]


class TrainsetDesc(C.Structure):
    """gapro_trainset_desc: one point-level problem of gapro_trainset_count / gapro_trainset_fill."""
    _fields_ = [("idx_offset", C.c_int64), ("n1", C.c_int32), ("n2", C.c_int32), ("t", C.c_int32), ("m1", C.c_int32),
                ("m2", C.c_int32), ("reserved", C.c_int32), ("row_offset", C.c_int64)]


TRAINSET_POOL, TRAINSET_NEAREST = 0, 1
TRAINSET_MAX_NEAREST = 1024
TRAINSET_MAX_LIST_FACTOR = 2  # a list holds at most so many times N entries (the exact sums' headroom)
TRAINSET_MAX_PROBLEMS = 32767  # problems of one call (GAPRO_TRAINSET_MAX_PROBLEMS: two grid rows per problem)


class SceneTask(C.Structure):
    """gapro_scene_task: the device pointers of one scene of a batched partition call."""
    _fields_ = [("n_points", C.c_int64), ("coords", C.c_void_p), ("feats", C.c_void_p), ("spp", C.c_void_p),
                ("spp_inv", C.c_void_p), ("prepare_ws", C.c_void_p), ("spp_range_cap", C.c_int64),
                ("boxes", C.c_void_p), ("n_boxes", C.c_int32), ("n_spps", C.c_int32), ("fixed_shift", C.c_int32),
                ("thresh_spp_occu", C.c_float), ("feat_sum", C.c_void_p), ("occ_count", C.c_void_p),
                ("point_count", C.c_void_p), ("feats_spp", C.c_void_p), ("occ_bits", C.c_void_p),
                ("n_bbs", C.c_void_p), ("sem_spp", C.c_void_p), ("inst_spp", C.c_void_p), ("prob_spp", C.c_void_p),
                ("sem", C.c_void_p), ("inst", C.c_void_p), ("prob", C.c_void_p)]


class PthArray(C.Structure):
    """gapro_pth_array: one NumPy array of a torch.save()d file."""
    _fields_ = [("kind", C.c_int32), ("itemsize", C.c_int32), ("ndim", C.c_int32), ("encoded", C.c_int32),
                ("shape", C.c_int64 * 4), ("nbytes", C.c_int64)]


class InstanceHeader(C.Structure):
    _fields_ = [("instance_num", C.c_int32), ("n_boxes", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


class EvalScene(C.Structure):
    """gapro_eval_scene: one scene of a batched evaluation (gapro_eval_batch)."""
    _fields_ = [("point_offset", C.c_int64), ("n_points", C.c_int64), ("max_gt", C.c_int32), ("max_ps", C.c_int32),
                ("ws_offset", C.c_int64), ("row_offset", C.c_int64)]


class EvalApScene(C.Structure):
    """gapro_eval_ap_scene: one scene of a batched AP table launch (gapro_eval_ap_keys / gapro_eval_ap_tables)."""
    _fields_ = [("point_offset", C.c_int64), ("n_points", C.c_int64), ("max_ps", C.c_int32), ("n_keys", C.c_int32),
                ("ws_offset", C.c_int64), ("id_offset", C.c_int64), ("key_offset", C.c_int64),
                ("pair_offset", C.c_int64)]


GAPRO_LABEL_F64, GAPRO_LABEL_I32, GAPRO_LABEL_I64 = 1, 2, 3


class InstPrepHeader(C.Structure):
    """gapro_inst_prep_header: what gapro_inst_crop / gapro_inst_info / gapro_inst_prepare report."""
    _fields_ = [("instance_num", C.c_int32), ("n_ids", C.c_int32), ("max_id", C.c_int32), ("status", C.c_int32),
                ("fixed_shift", C.c_int32), ("flags", C.c_int32)]


INST_PREP_MAX_IDS = 1 << 20   # GAPRO_INST_PREP_MAX_IDS: an id at or beyond it is refused
INST_PREP_GRID_CAP = 512      # GAPRO_INST_PREP_GRID_CAP: workgroups (of 256 threads) of a pass over the points
INST_PREP_LDS_IDS = 512       # GAPRO_INST_PREP_LDS_IDS: ids tallied in LDS


class SppGtHeader(C.Structure):
    """gapro_spp_gt_header: what gapro_spp_gt_count reports; batch_size pairs (n_inst_gt, n_spp) of int32 follow it."""
    _fields_ = [("status", C.c_int32), ("bad_sample", C.c_int32), ("flags", C.c_int32), ("batch_size", C.c_int32),
                ("total_rows", C.c_int64), ("total_cols", C.c_int64), ("total_cells", C.c_int64)]


SPP_GT_MAX_SAMPLES = 1024             # GAPRO_SPP_GT_MAX_SAMPLES: samples of one call
SPP_GT_MAX_BATCH_SPPS = (1 << 31) - 1  # GAPRO_SPP_GT_MAX_BATCH_SPPS: batch_size * n_spps of one call
SPP_GT_GRID_CAP = 512                 # GAPRO_SPP_GT_GRID_CAP: workgroups (of 256 threads) of a pass over the points
class ProposalsInputs(C.Structure):
    """gapro_proposals_inputs: the sizes and device pointers of one scene (a host struct, read when the call enqueues)."""
    _fields_ = [("n_queries", C.c_int64), ("n_voxels", C.c_int64), ("n_points", C.c_int64), ("n_spps", C.c_int32),
                ("n_mask_cols", C.c_int32), ("cls_logits", C.c_void_p), ("conf_logits", C.c_void_p),
                ("box_preds", C.c_void_p), ("mask_logits", C.c_void_p), ("voxel_spps", C.c_void_p),
                ("v2p_map", C.c_void_p), ("spps", C.c_void_p), ("semantic_preds", C.c_void_p),
                ("cand_scores", C.c_void_p), ("cand_classes", C.c_void_p), ("mask_type", C.c_int32),
                ("voxel_spps_i64", C.c_int32), ("v2p_i64", C.c_int32), ("spps_i64", C.c_int32),
                ("semantic_i64", C.c_int32), ("reserved", C.c_int32)]


PROPOSALS_MAX_PRE_TOPK, PROPOSALS_MAX_SEM2INS = 1024, 8
PROPOSALS_FULL, PROPOSALS_NMS, PROPOSALS_RLE = 0, 1, 2
PROPOSALS_NMS_MATRIX, PROPOSALS_NMS_STANDARD = 0, 1
PROPOSALS_MASK_F32, PROPOSALS_MASK_U8 = 0, 1


class ProposalsParams(C.Structure):
    """gapro_proposals_params."""
    _fields_ = [("mode", C.c_int32), ("instance_classes", C.c_int32), ("pre_topk", C.c_int32),
                ("type_nms", C.c_int32), ("topk", C.c_int32), ("npoint_thresh", C.c_int32),
                ("label_shift", C.c_int32), ("n_sem2ins", C.c_int32), ("logit_thresh", C.c_float),
                ("final_score_thresh", C.c_float), ("nms_threshold", C.c_float), ("reserved", C.c_int32),
                ("sem2ins_classes", C.c_int32 * PROPOSALS_MAX_SEM2INS)]


class ProposalsHeader(C.Structure):
    """gapro_proposals_header: what gapro_proposals_count reports; n_rows int32 run counts follow it."""
    _fields_ = [("status", C.c_int32), ("flags", C.c_int32), ("n_rows", C.c_int32), ("n_sem2ins", C.c_int32),
                ("total_runs", C.c_int64), ("n_candidates", C.c_int32), ("n_after_npoints", C.c_int32),
                ("n_after_nms", C.c_int32), ("n_after_refine", C.c_int32)]


class SpfPredictInputs(C.Structure):
    """gapro_spf_predict_inputs: the sizes and device pointers of one scene (a host struct, read when the call enqueues)."""
    _fields_ = [("n_queries", C.c_int64), ("n_spps", C.c_int64), ("n_points", C.c_int64), ("labels", C.c_void_p),
                ("pred_scores", C.c_void_p), ("masks", C.c_void_p), ("superpoints", C.c_void_p),
                ("coords_float", C.c_void_p), ("superpoints_i64", C.c_int32), ("reserved", C.c_int32)]


class SpfPredictParams(C.Structure):
    """gapro_spf_predict_params."""
    _fields_ = [("num_class", C.c_int32), ("topk_insts", C.c_int32), ("npoint_thr", C.c_int32),
                ("score_thr", C.c_float)]


class SpfPredictHeader(C.Structure):
    """gapro_spf_predict_header: what gapro_spf_predict_count reports; n_rows int32 run counts follow it."""
    _fields_ = [("status", C.c_int32), ("flags", C.c_int32), ("n_candidates", C.c_int32), ("n_after_score", C.c_int32),
                ("n_rows", C.c_int32), ("reserved", C.c_int32), ("total_runs", C.c_int64)]


SPP_GT_HALF, SPP_GT_STRICT = 0, 1     # the rule of gapro_spp_gt_fill: 2 c >= n, 2 c > n
GAPRO_ERR_SPP_RANGE = -6
GAPRO_EVAL_MAX_THRESHOLDS = 32


class MatchTask(C.Structure):
    """gapro_match_task: one sample of gapro_match_cost."""
    _fields_ = [("d_mask_logits", C.c_void_p), ("ld_logits", C.c_int64), ("d_mask", C.c_void_p), ("d_cls", C.c_void_p),
                ("d_box", C.c_void_p), ("n_inst", C.c_int32), ("n_cols", C.c_int32), ("cost_offset", C.c_int64)]


class MatchWeights(C.Structure):
    """gapro_match_weights: the weights of the five cost terms (matcher.py:192 is the default)."""
    _fields_ = [("w_class", C.c_double), ("w_dice", C.c_double), ("w_bce", C.c_double), ("w_conf", C.c_double),
                ("w_giou", C.c_double)]


MATCH_STATUS_WORDS = 4  # GAPRO_MATCH_STATUS_WORDS: status, sample, flags (1: class label, 2: mask value), 0


class MatchLossTask(C.Structure):
    """gapro_match_loss_task: one sample of gapro_match_loss_forward."""
    _fields_ = [("d_mask_logits", C.c_void_p), ("ld_logits", C.c_int64), ("d_inst_labels", C.c_void_p),
                ("d_cls_labels", C.c_void_p), ("d_box_labels", C.c_void_p), ("n_gt", C.c_int32), ("n_cols", C.c_int32),
                ("col_offset", C.c_int64), ("row_offset", C.c_int64)]


MATCH_LOSS_N = 7          # GAPRO_MATCH_LOSS_N: dice, bce, cls, iou, box, giou, levelset
MATCH_LOSS_MAX_FEATS = 8  # GAPRO_MATCH_LOSS_MAX_FEATS


class SpfLossTask(C.Structure):
    """gapro_spf_loss_task: one (head, sample) of gapro_spf_loss_forward."""
    _fields_ = [("d_labels", C.c_void_p), ("d_scores", C.c_void_p), ("d_mask_logits", C.c_void_p),
                ("ld_logits", C.c_int64), ("d_gt_masks", C.c_void_p), ("d_gt_labels", C.c_void_p),
                ("d_gt_boxes", C.c_void_p), ("n_gt", C.c_int32), ("n_inst", C.c_int32), ("n_cols", C.c_int32),
                ("reserved", C.c_int32), ("col_offset", C.c_int64), ("row_offset", C.c_int64)]


class SpfLossDims(C.Structure):
    """gapro_spf_loss_dims: the sizes and switches of gapro_spf_loss_forward / _backward."""
    _fields_ = [("n_heads", C.c_int32), ("batch_size", C.c_int32), ("n_queries", C.c_int32), ("n_classes", C.c_int32),
                ("cls_type", C.c_int32), ("n_feats", C.c_int32), ("min_points", C.c_int32), ("flags", C.c_int32),
                ("non_object_weight", C.c_double)]


SPF_LOSS_N = 5                                   # GAPRO_SPF_LOSS_N: cls, mask_bce, mask_dice, score, levelset
SPF_WEIGHTED_BCE, SPF_DICE_DIV_MAIN = 1, 2       # GAPRO_SPF_WEIGHTED_BCE, GAPRO_SPF_DICE_DIV_MAIN
QS_STATUS_WORDS = 4  # GAPRO_QS_STATUS_WORDS: status, flags (1: offsets, 2: a sample without points, 4: not finite), 0, 0
FPS_SKIP_ORIGIN, QS_LOCAL_INDEX = 1, 2                # the flags of gapro_fps_batch / gapro_ball_query_batch
FPS_PATHS = ("resident", "streamed", "global")        # GAPRO_FPS_RESIDENT, _STREAMED, _GLOBAL
QS_MAX_SAMPLES, BALL_QUERY_MAX_NSAMPLE = 4096, 4096
VOXELIZE_MAX_ACTIVE = 4096    # GAPRO_VOXELIZE_MAX_ACTIVE: points of one voxel in modes 3 and 4
VOXELIZE_STATUS_WORDS = 4     # GAPRO_VOXELIZE_STATUS_WORDS: status, flags, 0, 0 (the header: n_voxels, max_active)


SPP_SORT_TILE, SPP_MAX_SEGMENTS, SPP_MAX_BATCHES, SPP_STATUS_WORDS = 4096, 1 << 24, 65536, 4   # GAPRO_SPP_*
SPP_FLAG_INDEX, SPP_FLAG_MAP, SPP_MEAN, SPP_MAX = 1, 2, 0, 1
DYCO_MAX_BATCH = 64  # GAPRO_DYCO_MAX_BATCH
SPCONV_STATUS_WORDS = 4       # GAPRO_SPCONV_STATUS_WORDS: status, flags, n_out (the down plan's header), 0
SPCONV_MAX_ROWS, SPCONV_MAX_CHANNELS, SPCONV_CIN_CHUNK, SPCONV_MIN_CHUNK_ROWS = 1 << 30, 512, 32, 256  # GAPRO_SPCONV_*


class SppPlan(C.Structure):
    """gapro_spp_plan: the sizes and device pointers of a superpoint pooling plan (a host struct, read when a call
    enqueues)."""
    _fields_ = [("n_points", C.c_int64), ("n_spps", C.c_int64), ("n_rows", C.c_int64), ("d_index", C.c_void_p),
                ("d_point_map", C.c_void_p), ("index_i64", C.c_int32), ("map_i64", C.c_int32),
                ("d_seg_off", C.c_void_p), ("d_seg_pts", C.c_void_p), ("d_counts", C.c_void_p),
                ("d_row_off", C.c_void_p), ("d_row_pts", C.c_void_p), ("d_seg_rows", C.c_void_p)]


class VoxelizeHeader(C.Structure):
    """gapro_voxelize_header: what gapro_voxelize_count / gapro_voxelize_host_count report."""
    _fields_ = [("status", C.c_int32), ("flags", C.c_int32), ("n_voxels", C.c_int32), ("max_active", C.c_int32)]


POINT_LOSS_N = 4                                     # GAPRO_POINT_LOSS_N: sem, corners, giou, conf
POINT_LOSS_MIN_CLASSES, POINT_LOSS_MAX_CLASSES = 2, 64  # GAPRO_POINT_LOSS_MIN_CLASSES / _MAX_CLASSES
POINT_LOSS_MAX_POINTS = (1 << 31) - 1                 # n_points of one call
POINT_LOSS_RUN = 1024                                 # GAPRO_POINT_LOSS_RUN: points of one workgroup
POINT_LOSS_FOLD = 256                                 # GAPRO_POINT_LOSS_FOLD: records the finishing kernel folds in one pass


class FitOptions(C.Structure):
    _fields_ = [("training_iter", C.c_int32), ("lr", C.c_double), ("jitter", C.c_double),
                ("min_variance", C.c_double), ("eval_stale_chol", C.c_int32), ("reserved", C.c_int32),
                ("psd_retries", C.c_int32), ("precision", C.c_int32), ("psd_jitter", C.c_double)]


# debug bits of FitOptions.reserved: the GAPRO_FIT_DBG_* enumerators of include/gapro_hip.h, which says what each does
FIT_DBG_NO_STRIP = 1
FIT_DBG_CALLER_STREAM = 2
FIT_DBG_NO_SMALL = 4
FIT_DBG_NO_CLUSTER = 8
FIT_DBG_CLUSTER_ALL = 16
FIT_DBG_WG_TILED_ALL = 8192
FIT_DBG_CLUSTER_STALL = 32768
FIT_DBG_WG_TILED_NONE = 131072
FIT_DBG_STATIC_MAP = 262144
FIT_DBG_NO_WAVE = 1048576


# name -> (restype, argtypes); every symbol of include/gapro_hip.h
_P = C.c_void_p
SIGNATURES = {
    "gapro_version": (C.c_int, []),
    "gapro_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "gapro_ctx_destroy": (None, [_P]),
    "gapro_last_error": (C.c_char_p, [_P]),
    "gapro_partition_prepare_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gapro_partition_prepare": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, C.c_int64, _P, C.c_size_t, _P,
                                          C.POINTER(SceneHeader)]),
    "gapro_partition_prepare_async": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, C.c_int64, _P, C.c_size_t,
                                                _P, _P]),
    "gapro_partition_pool": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                       _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gapro_broadcast_labels": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "gapro_partition_prepare_batch": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "gapro_partition_pool_batch": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "gapro_partition_pool_plan": (C.c_int, [C.c_int32, C.c_int32]),
    "gapro_broadcast_labels_batch": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "gapro_instance_info_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gapro_instance_info": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P, _P, _P, _P,
                                      _P, _P]),
    "gapro_eval_batch_workspace_bytes": (C.c_size_t, [_P, C.c_int32, C.c_int32]),
    "gapro_eval_batch": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P,
                                   C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P, _P, _P,
                                   _P, _P]),
    "gapro_eval_ap_workspace_bytes": (C.c_size_t, [_P, C.c_int32]),
    "gapro_eval_ap_keys": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P,
                                     C.c_size_t, _P, _P]),
    "gapro_eval_ap_pair_cells": (C.c_int64, [_P, C.c_int32]),
    "gapro_eval_ap_tables": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, C.c_int32,
                                       _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P,
                                       _P]),
    "gapro_eval_ap_workspace_bytes_rows": (C.c_size_t, [_P, C.c_int32, C.c_int32]),
    "gapro_eval_ap_tables_rows": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P,
                                            C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_size_t,
                                            _P, _P, _P, _P, _P, _P, _P, _P]),
    "gapro_label_heuristic_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gapro_label_heuristic": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32,
                                        C.c_int32, _P, C.c_size_t, _P, _P]),
    "gapro_label_pool_mean": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gapro_weighted_bce_with_logits": (C.c_int, [_P, _P, C.c_int32, C.c_int64, _P, _P, _P, C.c_float, _P, _P, _P]),
    "gapro_kl_gp_loss": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, _P, _P, _P,
                                   _P]),
    "gapro_inst_prep_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gapro_inst_crop": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P, _P]),
    "gapro_inst_info": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int32, _P,
                                  C.c_size_t, _P, _P, _P, _P, _P, _P, _P]),
    "gapro_inst_prepare": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int32, _P,
                                     C.c_size_t, _P, _P, _P, _P, _P, _P, _P]),
    "gapro_spp_gt_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "gapro_spp_gt_count": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P,
                                     C.c_int32, C.c_int32, _P, C.c_int32, C.c_int64, _P, C.c_size_t, _P, _P]),
    "gapro_spp_gt_fill": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P,
                                    C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int64, C.c_int32, _P, C.c_size_t, _P,
                                    C.c_int64, _P, _P, _P, C.c_int64, _P]),
    "gapro_proposals_workspace_bytes": (C.c_size_t, [_P, _P]),
    "gapro_proposals_header_bytes": (C.c_size_t, [_P, _P]),
    "gapro_proposals_count": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, _P]),
    "gapro_proposals_fill": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_int64,
                                       _P, _P]),
    "gapro_spf_predict_workspace_bytes": (C.c_size_t, [_P, _P]),
    "gapro_spf_predict_header_bytes": (C.c_size_t, [_P, _P]),
    "gapro_spf_predict_count": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, _P]),
    "gapro_spf_predict_fill": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_int64,
                                         _P, _P]),
    "gapro_match_cost_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int64]),
    "gapro_match_cost": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                   C.c_size_t, _P, C.c_int64, _P, _P, _P]),
    "gapro_match_loss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64]),
    "gapro_match_loss_forward": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                           _P, _P, _P, _P, _P, C.c_int64, _P, C.c_double, _P, C.c_size_t, _P, _P, _P]),
    "gapro_match_loss_backward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                            _P, _P, _P, _P, _P, _P, _P, C.c_double, _P, C.c_size_t, _P, _P, _P, _P,
                                            _P]),
    "gapro_spf_loss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "gapro_spf_loss_forward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_size_t, _P, _P, _P]),
    "gapro_spf_loss_backward": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P]),
    "gapro_point_loss_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "gapro_point_loss_forward": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int32, _P, C.c_int32, _P,
                                           _P, _P, _P, _P, C.c_int64, C.c_double, _P, C.c_size_t, _P, _P, _P]),
    "gapro_point_loss_backward": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int32, _P, C.c_int32, _P,
                                            _P, _P, _P, _P, C.c_int64, C.c_double, _P, C.c_size_t, _P, _P, _P, _P]),
    "gapro_fps_plan": (C.c_int, [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gapro_fps_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gapro_fps_batch": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int32,
                                  _P, C.c_size_t, _P, _P, _P, _P]),
    "gapro_ball_query_batch": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32,
                                         C.c_double, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "gapro_lsap_solve": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_int64, C.c_int32, C.POINTER(C.c_int32), _P, _P]),
    "gapro_voxelize_table_shape": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "gapro_voxelize_plan": (C.c_int64, [C.c_int64]),
    "gapro_voxelize_hash": (C.c_uint64, [_P, C.c_int32]),
    "gapro_voxelize_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gapro_voxelize_count": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, C.c_size_t, _P, _P, _P]),
    "gapro_voxelize_fill": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int64, _P,
                                      C.c_size_t, _P, _P, _P, _P, _P]),
    "gapro_voxelize_host_count": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, C.POINTER(VoxelizeHeader),
                                            C.POINTER(C.c_void_p)]),
    "gapro_voxelize_host_fill": (C.c_int, [_P, _P, _P, _P, _P]),
    "gapro_voxelize_host_free": (None, [_P]),
    "gapro_voxel_pool_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gapro_voxel_pool_forward": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int64, _P, C.c_int32,
                                           C.c_int32, _P, C.c_size_t, _P, _P, _P]),
    "gapro_voxel_pool_backward": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64, C.c_int64, _P, C.c_int32, _P,
                                            _P, _P]),
    "gapro_spp_plan_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gapro_spp_plan_build": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int32, _P, _P, C.c_size_t, _P, _P]),
    "gapro_spp_pool_forward": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "gapro_spp_pool_backward": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "gapro_dyco_param_count": (C.c_int64, [C.c_int32]),
    "gapro_dyco_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "gapro_dyco_forward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, _P, _P, C.c_int64, _P, _P,
                                     _P, _P, _P, C.c_size_t, _P]),
    "gapro_dyco_backward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, _P, _P, C.c_int64, _P, _P,
                                      _P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P]),
    "gapro_spconv_subm_plan_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gapro_spconv_subm_plan": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, _P, C.c_int32, _P, C.c_size_t, _P, _P, _P]),
    "gapro_spconv_down_plan_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gapro_spconv_down_count": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, _P, C.c_int32, _P, C.c_size_t, _P, _P]),
    "gapro_spconv_down_fill": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, _P, C.c_int32, C.c_int64, _P, C.c_size_t,
                                         _P, _P, _P, _P, _P, _P]),
    "gapro_spconv_chunk_rows": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "gapro_spconv_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "gapro_spconv_forward": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P,
                                       _P, _P]),
    "gapro_spconv_backward_input": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int32,
                                              C.c_int32, _P, _P, _P]),
    "gapro_spconv_backward_weight": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int32,
                                               _P, _P, _P, C.c_size_t, _P, _P]),
    "gapro_schedule_build": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(_P)]),
    "gapro_schedule_free": (None, [_P]),
    "gapro_schedule_get_counts": (C.c_int, [_P, C.POINTER(ScheduleCounts)]),
    "gapro_schedule_export_fits": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _P, _P]),
    "gapro_schedule_export_events": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "gapro_schedule_export_testers": (C.c_int, [_P, _P, _P, _P]),
    "gapro_schedule_merge": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "gapro_schedule_merge_ex": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "gapro_fit_options_default": (None, [C.POINTER(FitOptions)]),
    "gapro_fit_workspace_doubles": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gapro_fit_plan_workspace": (C.c_int64, [_P, C.c_int32, C.c_int32]),
    "gapro_svgp_fit_batch": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.POINTER(FitOptions), _P,
                                       C.c_size_t, _P, _P, _P, _P, _P, _P, _P]),
    "gapro_svgp_fit_batch_ex": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.POINTER(FitOptions), _P,
                                          C.c_size_t, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gapro_gp_state_doubles": (C.c_int64, [C.c_int32, C.c_int32]),
    "gapro_gp_state_plan": (C.c_int64, [_P, C.c_int32, C.c_int32, _P]),
    "gapro_svgp_fit_batch_state": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.POINTER(FitOptions), _P,
                                             C.c_size_t, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t]),
    "gapro_svgp_predict_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, _P]),
    "gapro_svgp_predict_batch": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, _P,
                                           C.POINTER(FitOptions), _P, C.c_size_t, _P, _P, _P, _P, _P, _P]),
    "gapro_point_refine_gather": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, _P, _P]),
    "gapro_point_refine_apply": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int64, _P, _P, _P, _P, _P,
                                           _P]),
    "gapro_point_refine_expand": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P]),
    "gapro_point_refine_compete": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int32,
                                             _P, _P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "gapro_point_refine_vote": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P,
                                          C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "gapro_spp_vote_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "gapro_spp_vote": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, _P,
                                 C.c_size_t, _P, _P, _P]),
    "gapro_trainset_workspace_bytes": (C.c_size_t, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32]),
    "gapro_trainset_count": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P, _P, _P, C.c_size_t,
                                       _P, _P]),
    "gapro_trainset_fill": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P, _P, _P,
                                      _P, C.c_int32, C.c_int32, _P, _P, C.c_size_t, C.c_int64, _P, _P, _P]),
    "gapro_fit_workspace_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P]),
    "gapro_fit_route": (C.c_int, [C.c_int32, C.c_int32]),
    "gapro_fit_route_flags": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "gapro_fit_launch_plan": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FitLaunchStep),
                                        C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gapro_fit_padded_m": (C.c_int, [C.c_int32, C.c_int32]),
    "gapro_fit_timing_create": (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    "gapro_fit_timing_destroy": (None, [_P]),
    "gapro_fit_timing_arm": (C.c_int, [_P, _P]),
    "gapro_fit_timing_read": (C.c_int, [_P, _P, C.POINTER(C.c_float)]),
    "gapro_fit_timing_read_wave": (C.c_int, [_P, _P, C.POINTER(C.c_float)]),
    "gapro_fit_timing_offsets": (C.c_int, [_P, _P, _P, C.POINTER(C.c_float)]),
    "gapro_fit_timing_cluster_info": (C.c_int, [_P, _P, C.POINTER(C.c_int32)]),
    "gapro_pth_open": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "gapro_pth_count": (C.c_int, [_P]),
    "gapro_pth_is_sequence": (C.c_int, [_P]),
    "gapro_pth_info": (C.c_int, [_P, C.c_int32, C.POINTER(PthArray)]),
    "gapro_pth_read": (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    "gapro_pth_close": (None, [_P]),
    "gapro_pth_write": (C.c_int, [C.c_char_p, C.c_int32, C.POINTER(PthArray), C.POINTER(_P), C.c_int32]),
    "gapro_pth_last_error": (C.c_char_p, []),
    "gapro_pth_decoder": (C.c_char_p, []),
    "gapro_pth_encoder": (C.c_char_p, []),
    "gapro_pth_crc": (C.c_char_p, []),
    "gapro_pth_crc32": (C.c_uint32, [_P, C.c_int64]),
    "gapro_pth_encode_latin1": (C.c_int64, [_P, C.c_int64, _P, C.c_int64]),
    # batch feeder of the gen_ps driver (gapro_amd/feeder.py holds the structs)
    "gapro_dev_alloc": (C.c_int, [_P, C.c_size_t, _P, C.POINTER(C.c_void_p)]),
    "gapro_dev_free": (C.c_int, [_P, _P]),
    "gapro_dev_trim": (C.c_int, [_P]),
    "gapro_dev_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64)]),
    "gapro_host_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_void_p)]),
    "gapro_host_free": (C.c_int, [_P, _P]),
    "gapro_stream_create": (C.c_int, [_P, C.POINTER(C.c_void_p)]),
    "gapro_stream_destroy": (C.c_int, [_P, _P]),
    "gapro_stream_sync": (C.c_int, [_P, _P]),
    "gapro_device_sync": (C.c_int, [_P]),
    "gapro_event_create": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_void_p)]),
    "gapro_event_destroy": (C.c_int, [_P, _P]),
    "gapro_event_record": (C.c_int, [_P, _P, _P]),
    "gapro_stream_wait_event": (C.c_int, [_P, _P, _P]),
    "gapro_event_sync": (C.c_int, [_P, _P]),
    "gapro_event_query": (C.c_int, [_P, _P]),
    "gapro_event_elapsed_ms": (C.c_int, [_P, _P, _P, C.POINTER(C.c_float)]),
    "gapro_memcpy_async": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int32, _P]),
    "gapro_memset_async": (C.c_int, [_P, _P, C.c_int32, C.c_size_t, _P]),
    "gapro_feed_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]),
    "gapro_feed_destroy": (None, [_P]),
    "gapro_feed_detach": (None, [_P]),
    "gapro_feed_last_error": (C.c_char_p, [_P]),
    "gapro_feed_submit": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    "gapro_feed_close": (C.c_int, [_P]),
    "gapro_feed_poll": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "gapro_feed_upload": (C.c_int, [_P, C.c_int32, _P, C.c_int64, _P, _P, C.POINTER(C.c_int64)]),
    "gapro_feed_batch_wait": (C.c_int, [_P, C.c_int64, _P]),
    "gapro_feed_release_batch": (C.c_int, [_P, C.c_int64]),
    "gapro_feed_export": (C.c_int, [_P, C.c_int32, _P, _P]),
    "gapro_feed_export_wait": (C.c_int, [_P, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gapro_feed_export_error": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "gapro_feed_stats": (C.c_int, [_P, _P]),
    "gapro_scene_default_feats": (C.c_int, [_P, _P, C.c_int64, _P]),
    "gapro_scene_instance_boxes": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
}

# libgapro_hip_debug.so (include/gapro_hip_debug.h): measurement / self-test entry points, loaded on request only
DEBUG_LIB_PATH = os.path.join(_HERE, "libgapro_hip_debug.so")
DEBUG_SIGNATURES = {
    "gapro_debug_mfma_tn": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32]),
    "gapro_debug_stream": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32]),
    "gapro_debug_fit_math": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32]),
    "gapro_debug_mfma_peak": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double)]),
    "gapro_debug_mfma_clock": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double),
                                         C.POINTER(C.c_double)]),
    "gapro_debug_product_bench": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                            C.POINTER(C.c_float)]),
    "gapro_debug_wgloop": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_double)]),
    "gapro_debug_exact_sum": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, _P]),
    "gapro_debug_scan": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P]),
}

_lib: Optional[C.CDLL] = None
_dbg: Optional[C.CDLL] = None


def source_build_id() -> str:
    """Identity of the DEVICE KERNELS this tree holds (sha256 over the kernel sources and the headers they include, 16
    hex digits): bench.py prints it and the committed PMC passes carry it, so that a traffic figure is only ever
    attached to a bench line of the SAME kernels.  Host-only sources (file I/O, feeder, arena,
    scheduler) are left out: they move no byte of a kernel's traffic."""
    import glob
    import hashlib

    h = hashlib.sha256()
    files = []
    for pat in ("csrc/svgp_fit*.hip", "csrc/partition.hip", "csrc/labels.hip", "csrc/consumer.hip", "csrc/*.h"):
        files += glob.glob(os.path.join(_HERE, pat))
    for fn in sorted(files, key=os.path.basename):
        h.update(os.path.basename(fn).encode())
        with open(fn, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load_debug() -> C.CDLL:
    """Load libgapro_hip_debug.so (tools, bench.py's peak_measured, the MFMA lane-map test); the product never does."""
    global _dbg
    if _dbg is not None:
        return _dbg
    if not os.path.exists(DEBUG_LIB_PATH):
        raise ImportError("libgapro_hip_debug.so not built: run gapro_amd/csrc/build.sh; expected at " + DEBUG_LIB_PATH)
    lib = C.CDLL(DEBUG_LIB_PATH)
    for name, (res, args) in DEBUG_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _dbg = lib
    return lib


_TORCH_FIRST = [True]  # was torch already in the process when the library was loaded (or never imported)?


def load() -> C.CDLL:
    """Load libgapro_hip.so; raises (never falls back) if it is absent or lacks a symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libgapro_hip.so not built: run gapro_amd/csrc/build.sh (or __graft_entry__.build()); "
                          "expected at " + LIB_PATH)
    _TORCH_FIRST[0] = "torch" in sys.modules
    lib = C.CDLL(LIB_PATH)
    default = os.path.join(_HERE, "libgapro_hip.so")
    host_only = None  # A/B tools point LIB_PATH at a variant build that may predate a host-side helper
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
        except AttributeError:
            variant = os.path.abspath(LIB_PATH) != os.path.abspath(default)
            if variant and name.startswith(("gapro_gp_state_", "gapro_svgp_predict_", "gapro_svgp_fit_batch_state",
                                            "gapro_trainset_", "gapro_point_refine_", "gapro_schedule_merge_ex",
                                            "gapro_schedule_export_testers", "gapro_spp_vote",
                                            "gapro_fit_launch_plan", "gapro_inst_", "gapro_spp_gt_", "gapro_match_",
                                            "gapro_proposals_", "gapro_fps_", "gapro_ball_query_",
                                            "gapro_lsap_", "gapro_voxelize_", "gapro_voxel_pool_", "gapro_spf_predict_",
                                            "gapro_spp_plan_", "gapro_spp_pool_", "gapro_dyco_", "gapro_spconv_")):
                continue  # an older build under A/B comparison: no model export, no training-set assembly (a call
                #           raises AttributeError)
            if not variant or not name.startswith(("gapro_pth_", "gapro_scene_", "gapro_feed_")):
                raise
            if host_only is None:
                host_only = C.CDLL(default)
            fn = getattr(host_only, name)
            setattr(lib, name, fn)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class Context:
    """One gapro_ctx per (process, device)."""

    _cache = {}

    def __init__(self, device: int = 0):
        self.lib = load()
        h = _P()
        rc = self.lib.gapro_ctx_create(int(device), C.byref(h))
        if rc != GAPRO_OK:
            raise GaproError(rc, "gapro_ctx_create(device=%d): no usable HIP device%s" % (device, (
                " (torch was imported AFTER libgapro_hip.so was loaded: the process now holds two HIP runtimes, torch's "
                "bundled one and /opt/rocm's -- import torch first, or use the torch-free backend)"
                if ("torch" in sys.modules and not _TORCH_FIRST[0]) else "")))
        self.handle = h
        self.device = int(device)

    @property
    def dbg(self) -> C.CDLL:
        """The debug library's entry points (they take this context's handle)."""
        return load_debug()

    @classmethod
    def get(cls, device: int = 0) -> "Context":
        ctx = cls._cache.get(device)
        if ctx is None:
            ctx = cls._cache[device] = cls(device)
        return ctx

    def check(self, rc: int):
        if rc != GAPRO_OK:
            raise GaproError(rc, (self.lib.gapro_last_error(self.handle) or b"").decode())

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.gapro_ctx_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def default_fit_options(training_iter: int = 50) -> FitOptions:
    opt = FitOptions()
    load().gapro_fit_options_default(C.byref(opt))
    opt.training_iter = int(training_iter)
    return opt
