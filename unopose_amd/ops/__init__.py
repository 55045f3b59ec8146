"""Fused operators of the MI355X UNOPose forward (C ABI part 2) on torch tensors, by family:
    dense      nn.Linear on the hand-written GEMMs, LayerNorm / LayerScale glue, the residual + LayerNorm fold, the trainable form
    attention  ViT attention, RPE / cross token attention, focused linear attention
    geometry   frames, Procrustes, radius normalisation, gathers, geometric embedding, positional encoding
    sampling   pixel sampling and the sparse up-projection
    pose       similarity, assignment, coarse / fine pose heads
    prep       query-side instance preparation of the BOP test provider (crops, clouds, pixel indices)
    augment    the training provider's colour augmentation for all crops of a batch, and the finishing of those crops behind it
    rle        COCO run-length masks: decode (with the depth restriction, count and extents), window crops, encode
    detect     mask proposals against reference views: patch validity, unit token rows, the masked best-match patch score, mask suppression
    items      training items from rendered views: visible masks, counts and extents, points, pixel indices, crop atlas; the scene stage (provider_online)
    score      pose errors of the BOP'19 scorer (VSD counts, MSSD / MSPD) for many (estimate, ground truth) pairs per launch
    vis        per-image composition of the pose visualisation (nearest-pose layer, boxes, blend, depth-difference image)
    train      autograd Functions of the training step
Each function cites the reference Python it replaces.  Inputs must be CUDA tensors; there is no CPU path (RuntimeError).
`from unopose_amd import ops; ops.linear(...)` keeps working as before the split; the A/B switches (ops.USE_LN_FOLD = False, ...) live in
`ops._state` and assignments on the package are forwarded there."""
import sys
import types

from . import _state
from .common import (  # noqa: F401
    _c, differentiable, is_differentiable, _fallbacks_seen, note_fallback, _params_key, _SPLIT_MEMO, _MUTATION_EPOCH, note_mutation,
    clear_split_memo, _aligned16, _no_autograd, _f32_path, _own_f32, _own_glue,
)
from .dense import (  # noqa: F401
    linear_backend, _bf16_weights, linear_bf16_hip, own_gemm_ok, bf16_linear_2d, f32x3_ok, split_f32, _f32x3_weights, linear_f32x3,
    linear_f32x3_bf16, linear_f32_raw, _transposed_weights, _LinearFn, _SmallLinearFn, small_linear_train_ok, _ZERO_BIAS, _zero_bias, linear_train, _lin, mlp, linear,
    ffn_add_layernorm, linear_add_layernorm, patch_embed, vit_prologue_ok, vit_prologue, vit_prologue_f32_ok, vit_prologue_f32, bmm_nt_f32, score_head, add_layernorm,
    _AddLayerNormFn, add_layernorm_train_ok, add_layernorm_train,
    scale_residual_, scale_residual_layernorm_f32_, vit_f32_fused_ok, scale_residual_layernorm_, ln_fold_ok, _fold_producer_weights,
    _fold_consumer_weights, linear_residual_, linear_lnfold, fold_shift, fold_row_means, _into,
)
from .attention import (  # noqa: F401
    vit_attention, vit_attention_f32_split, vit_attention_f32_ss, vit_attention_torch, _KEY_PAD, token_attention,
    _token_attention_hip_f32, _attn_weights, _token_attention_hip, token_attention_torch, _key_pad, _transpose_pad_f32, _TokenAttnFn,
    token_attention_train_ok, _token_attention_train, focused_linear_attention, _LinearAttnFn, linear_attention_train_ok,
    _focused_linear_attention_train, _la_workspace,
    _focused_linear_attention_hip_f32, _focused_linear_attention_hip, focused_linear_attention_torch,
)
from .geometry import (  # noqa: F401
    lrf_global, query_lrf_group, lrf_group_idx, weighted_procrustes, cloud_radius, scale_by_radius, gather_rows, pairwise_distance,
    _bf16_split, _mfma_fragment_order, _GEO_HINV, _GEO_D_RANGE, _GEO_TABLE_UNAVAILABLE, _geo_tables, geo_embedding, geo_embedding_torch,
    pe_group_mlp_max, pe_group_mlp_max_unfused, pe_geometry, pe_mlp_max, _pe_image, furthest_point_sample, _geo_grid, _GeoEmbedFn, geo_embedding_train_ok,
)
from .sampling import (  # noqa: F401
    bilinear_sample_native, sparse_upproj_ok, upproj_plan, sparse_pixel_features, bilinear_sample_pixels,
)
from .pose import (  # noqa: F401
    overlap_scores, set_first_rows_, pose_score, rigid_rows, feature_similarity, soft_assignment, coarse_pose_torch, fine_pose_torch, _assign_labels, _check_score_width,
    coarse_pose, fine_pose, fine_pose_fused_ok, normalize_rows_bf16, normalize_rows_f32, fine_pose_from_features,
    icp_refine, icp_refine_torch, _icp_args, _icp_stage,
)
from .prep import (  # noqa: F401
    PrepPlan, _desc_ints, _tap_table, prep_norm_table, _require, _result, prep_crop_resize, prep_lift, prep_gather,
)
from .augment import AugTables, color_augment, finish_crops  # noqa: F401
from .rle import pack_segs, rle_decode, rle_encode, window_masks  # noqa: F401
from .detect import patch_valid, token_unit_rows, patch_match_score, class_cosine, mask_nms  # noqa: F401
from .items import item_crops, item_points, item_views, min_kept_points, sense_views  # noqa: F401
from .score import vsd_counts, pose_errors, pose_metrics, adi, gt_visibility, pts_extent, ref_select, sym_deviation  # noqa: F401
from .vis import compose_poses  # noqa: F401
from .train import (  # noqa: F401
    _InfoNCEFn, infonce_two_way, _BNReLUTrain, bn_relu, _BNReLUMaxPoolTrain, bn_relu_maxpool, _SaliencyFn, saliency_pair,
    _match_split, _MatchHeadFn, _match_head_domain, match_head_train_ok, match_head, nearest_partner, _CONV_FWD_PAIRS, _CONV_WGRAD_PAIRS, _conv1x1_pair_ok, _conv1x1_wgrad_ok, _Conv1x1Fn, conv1x1,
)

_SWITCHES = frozenset(['FORBID_LIBRARY_BF16_GEMM', 'GEO_TABLE', 'GEO_TABLE_F32', 'HIP_GEMM_ALL', 'PIXEL_FEATS_BF16', 'TRAIN_FUSED_SALIENCY', 'TRAIN_OWN_ATTN', 'TRAIN_OWN_CONV', 'TRAIN_OWN_GEMM', 'TRAIN_OWN_GEMM_MIN_FLOP', 'TRAIN_OWN_GEO', 'TRAIN_OWN_LINATTN', 'TRAIN_OWN_LN', 'TRAIN_OWN_MATCH', 'TRAIN_OWN_SMALL_LINEAR', 'TRAIN_OWN_WGRAD', 'TRAIN_OWN_WGRAD_MIN_ROWS', 'USE_F32X3', 'USE_FUSED_BN_RELU', 'USE_FUSED_FINE', 'USE_FUSED_INFONCE', 'USE_FUSED_LINEAR_LN', 'USE_HIP_GEMM', 'USE_KV_VT', 'USE_LA_KV_STATE', 'USE_LN_FOLD', 'USE_OWN_TOPK', 'USE_SPARSE_UPPROJ', 'USE_STACKED_OUT', '_DIFF'])


class _OpsModule(types.ModuleType):
    """`ops.SWITCH` reads and `ops.SWITCH = value` writes go to `ops._state`, where the family modules read them at call time."""

    def __getattr__(self, name):
        if name in _SWITCHES:
            return getattr(_state, name)
        raise AttributeError(f"module {self.__name__!r} has no attribute {name!r}")

    def __setattr__(self, name, value):
        if name in _SWITCHES:
            setattr(_state, name, value)
        else:
            super().__setattr__(name, value)

    def __delattr__(self, name):
        if name in _SWITCHES:
            raise AttributeError(f"{name} is a switch of ops._state and cannot be deleted")
        super().__delattr__(name)


sys.modules[__name__].__class__ = _OpsModule
