"""ctypes binding of libstemseg_hip.so (include/stemseg_hip.h).

PyTorch appears here only as plumbing: it owns device memory (``tensor.data_ptr()``) and the HIP
stream (``torch.cuda.current_stream().cuda_stream``).  Every numeric operation of the hot path runs in
the hand-written gfx950 kernels behind the C-ABI.  There is NO fallback: if the shared library is
missing, or no GPU is visible, the ops raise.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STEMSEG_HIP_LIB") or os.path.join(_HERE, "lib", "libstemseg_hip.so")      # (override: a library built from another checkout, tools/ab_conv.py and friends)

MAX_INSTANCES = 64
MAX_EMB_DIMS = 8
ABI_VERSION = 11


class Volume(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("c_stride", C.c_int64), ("t_stride", C.c_int64), ("y_stride", C.c_int64),
                ("C", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("limit", C.c_int64)]


class DecoderDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("in_channels", C.c_int32), ("inter", C.c_int32 * 4),
                ("T", C.c_int32), ("H4", C.c_int32), ("W4", C.c_int32), ("gn_groups", C.c_int32), ("gn_eps", C.c_float),
                ("pool", C.c_int32 * 3), ("t_scale", C.c_int32 * 3), ("n_out", C.c_int32),
                ("act", C.c_int32 * (2 * MAX_EMB_DIMS)), ("grid_axis", C.c_int32 * (2 * MAX_EMB_DIMS)),
                ("input_layout", C.c_int32), ("concurrency", C.c_int32), ("detached", C.c_int32), ("precision", C.c_int32),
                ("n_clips", C.c_int32), ("feat_clip_stride", C.c_int64 * 4), ("out_clip_stride", C.c_int64),
                # added after ABI 11 (the library also takes the older descriptor size): clips every conv's split-K factor is planned for
                ("plan_clips", C.c_int32),
                # reserved: 0 = block_4x asks for the deep 3x3x3 tile, 1 = the automatic tile choice (A/B runs; stemseg_hip.h)
                ("reserved", C.c_int32)]


class DecoderWeights(C.Structure):
    _fields_ = [("conv_w", C.c_void_p * 7), ("conv_b", C.c_void_p * 7), ("gn_w", C.c_void_p * 7), ("gn_b", C.c_void_p * 7),
                ("fuse_w", C.c_void_p * 3), ("head_w", C.c_void_p), ("head_b", C.c_void_p),
                ("grid_t", C.c_void_p), ("grid_y", C.c_void_p), ("grid_x", C.c_void_p)]


MAX_ENCODER_BLOCKS = 40


class ConvEpilogue(C.Structure):
    _fields_ = [("relu", C.c_int32), ("residual", C.c_void_p), ("res_c_stride", C.c_int64), ("res_t_stride", C.c_int64),
                ("res_y_stride", C.c_int64), ("decode_H", C.c_int32), ("decode_W", C.c_int32), ("precision", C.c_int32),
                ("frames", C.c_int32), ("plan_frames", C.c_int32), ("plan_scratch_floats", C.c_int64)]


class ConvPlanRecord(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kt", "kh", "kw", "ck", "mt", "rows", "tw", "nt", "flat", "pmax", "gl", "blk", "threads", "precision",
                                         "ksplit", "chunks_per_split", "nchunks")] + [("grid", C.c_int32 * 3)] + \
               [(n, C.c_int32) for n in ("row0", "row1", "vec4", "vec_epi", "reduce", "gn", "zero_t_halo", "nb", "deep")]


class EncoderDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("blocks", C.c_int32 * 4), ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("out_channels", C.c_int32), ("precision", C.c_int32), ("n_clips", C.c_int32), ("clip_frames", C.c_int32),
                ("clip_stride", C.c_int32), ("plan_frames", C.c_int32), ("fuse_tail", C.c_int32),
                # backbone architecture (added after ABI 11; the library also takes the older descriptor size): MODEL.RESNETS.NUM_GROUPS,
                # WIDTH_PER_GROUP, not STRIDE_IN_1X1.  0 in the first two means the default (1, 64)
                ("conv2_groups", C.c_int32), ("width_per_group", C.c_int32), ("stride_in_3x3", C.c_int32)]


_BLK = C.c_void_p * MAX_ENCODER_BLOCKS


class EncoderWeights(C.Structure):
    _fields_ = [("stem_w", C.c_void_p), ("stem_b", C.c_void_p), ("stem_w_s2d", C.c_void_p),
                ("conv1_w", _BLK), ("conv1_b", _BLK), ("conv2_w", _BLK), ("conv2_b", _BLK), ("conv3_w", _BLK), ("conv3_b", _BLK),
                ("down_w", _BLK), ("down_b", _BLK),
                ("fpn_inner_w", C.c_void_p * 4), ("fpn_inner_b", C.c_void_p * 4), ("fpn_layer_w", C.c_void_p * 4), ("fpn_layer_b", C.c_void_p * 4)]


class ClusterParams(C.Structure):
    _fields_ = [("primary_prob_thresh", C.c_float), ("secondary_prob_thresh", C.c_float), ("min_seediness_prob", C.c_float),
                ("max_instances", C.c_int32), ("n_free_dims", C.c_int32), ("free_dim_bandwidths", C.c_float * MAX_EMB_DIMS)]


class ClusterMeta(C.Structure):
    _fields_ = [("K", C.c_int32), ("exhausted", C.c_int32), ("n_points", C.c_int64), ("n_unassigned_last", C.c_int64),
                ("centers", (C.c_float * MAX_EMB_DIMS) * MAX_INSTANCES), ("bandwidths", (C.c_float * MAX_EMB_DIMS) * MAX_INSTANCES),
                ("seed_prob", C.c_float * MAX_INSTANCES)]


class ClusterItem(C.Structure):
    _fields_ = [("emb", C.c_void_p), ("bw", C.c_void_p), ("seed", C.c_void_p), ("n_max", C.c_int64), ("n_points_dev", C.c_void_p),
                ("label_start", C.c_int64), ("labels", C.c_void_p), ("meta_dev", C.c_void_p), ("opt_masks", C.c_void_p), ("opt_probs", C.c_void_p),
                ("workspace", C.c_void_p), ("ws_bytes", C.c_size_t)]


class EmbeddingLossDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("embedding_size", C.c_int32), ("n_free_dims", C.c_int32), ("n_instances", C.c_int32),
                ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("reserved", C.c_int32), ("free_dim_bandwidths", C.c_float * MAX_EMB_DIMS)]


class TargetPrepDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_instances", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("reserved", C.c_int32)]


class SemsegLossDesc(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_classes", C.c_int32), ("has_foreground_channel", C.c_int32), ("T", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("reserved", C.c_int32), ("reserved2", C.c_int32), ("stride_c", C.c_int64),
                ("stride_t", C.c_int64), ("stride_h", C.c_int64), ("stride_w", C.c_int64)]


class OptTensor(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("state1", C.c_void_p), ("state2", C.c_void_p), ("n", C.c_int64), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class OptChunk(C.Structure):
    _fields_ = [("tensor", C.c_int32), ("chunk", C.c_int32)]


class OptHyper(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("flags", C.c_int32), ("lr", C.c_float), ("momentum", C.c_float), ("one_minus_dampening", C.c_float),
                ("weight_decay", C.c_float), ("one_minus_beta1", C.c_float), ("beta2", C.c_float), ("one_minus_beta2", C.c_float), ("eps", C.c_float)]


# name -> (restype, argtypes); mirrors include/stemseg_hip.h one to one (tests check the export list)
_P, _I32, _I64, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
SIGNATURES = {
    "stemseg_hip_version": (C.c_int, []),
    "stemseg_hip_last_error": (C.c_char_p, []),
    "stemseg_hip_device_count": (C.c_int, []),
    "stemseg_hip_profile_enable": (C.c_int, [_I32]),
    "stemseg_hip_profile_read": (C.c_int, [C.POINTER(C.c_double), _I32]),
    "stemseg_hip_padded_geometry": (C.c_int, [_I32, _I32, _I32, _I32, C.POINTER(_I64)]),
    "stemseg_hip_pack_conv_weight": (C.c_int, [_P, _P, _I32, _I32, _I32, _P]),
    "stemseg_hip_encoder_plan_offsets": (C.c_int, [_P, _P]),
    "stemseg_hip_encoder_stage_end_mask": (C.c_int, [_P, C.POINTER(_I32)]),
    "stemseg_hip_packed_weight_bytes_prec": (C.c_int64, [_I32, _I32, _I32, _I32]),
    "stemseg_hip_pack_conv_weight_prec": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P]),
    "stemseg_hip_conv3d": (C.c_int, [C.POINTER(Volume), _P, _P, C.POINTER(Volume), _I32, _I32, _I32, _I32, _P, _I64, C.POINTER(ConvEpilogue), _P]),
    "stemseg_hip_packed_grouped_weight_bytes": (C.c_int64, [_I32, _I32, _I32, _I32]),
    "stemseg_hip_pack_grouped_conv_weight": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P]),
    "stemseg_hip_conv2d_grouped": (C.c_int, [C.POINTER(Volume), _P, _P, C.POINTER(Volume), _I32, _I32, _I32, _I32, _I32, _P]),
    "stemseg_hip_conv3d_gn_scratch_doubles": (C.c_int64, [_I32, _I32]),
    "stemseg_hip_conv3d_plan": (C.c_int, [C.POINTER(Volume), _P, C.POINTER(Volume), _I32, _I32, _I32, _I32, _P, _I64, C.POINTER(ConvEpilogue), _I32, _I32,
                                          C.POINTER(ConvPlanRecord), _I32, C.POINTER(_I32)]),
    "stemseg_hip_conv3d_plan_clips": (C.c_int, [C.POINTER(Volume), _P, C.POINTER(Volume), _I32, _I32, _I32, _I32, _P, _I64, C.POINTER(ConvEpilogue), _I32, _I32,
                                                _I32, C.POINTER(ConvPlanRecord), _I32, C.POINTER(_I32)]),
    "stemseg_hip_conv3d_zero_t_halo": (C.c_int, [C.POINTER(Volume), _P, _P, C.POINTER(Volume), _I32, _I32, _I32, _I32, _P, _I64, C.POINTER(ConvEpilogue),
                                                _I32, _F, _P, _P, _P]),
    "stemseg_hip_conv3d_zero_t_halo_clips": (C.c_int, [C.POINTER(Volume), _P, _P, C.POINTER(Volume), _I32, _I32, _I32, _I32, _P, _I64, C.POINTER(ConvEpilogue),
                                                      _I32, _F, _P, _P, _I32, _P]),
    "stemseg_hip_conv3d_zero_t_halo_batch": (C.c_int, [C.POINTER(Volume), _P, _P, C.POINTER(Volume), _I32, _I32, _I32, _I32, C.POINTER(ConvEpilogue),
                                                      _I32, _I64, _I64, _P]),
    "stemseg_hip_conv3d_gn": (C.c_int, [C.POINTER(Volume), _P, _P, C.POINTER(Volume), _I32, _I32, _I32, _I32, _P, _I64, _I32, _I32, _F, _P, _P, _P]),
    "stemseg_hip_stem_conv": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _P]),
    "stemseg_hip_maxpool3x3s2": (C.c_int, [_P, _I64, _I32, _I32, _P, _I32, C.POINTER(_I32), _P]),
    "stemseg_hip_encoder_subsample2": (C.c_int, [_P, _I64, _I32, _I32, _P, _I32, C.POINTER(_I32), _P]),
    "stemseg_hip_upsample2x_add": (C.c_int, [C.POINTER(Volume), _P, C.POINTER(Volume), _I32, C.POINTER(_I32), _P]),
    "stemseg_hip_stem_s2d": (C.c_int, [_P, _I32, _I32, _I32, C.POINTER(Volume), _P]),
    "stemseg_hip_encoder_stream_forms": (C.c_int, [C.POINTER(EncoderDesc), C.POINTER(_I32)]),
    "stemseg_hip_encoder_workspace_bytes": (C.c_size_t, [C.POINTER(EncoderDesc)]),
    "stemseg_hip_encoder_init_workspace": (C.c_int, [C.POINTER(EncoderDesc), _P, C.c_size_t, _P]),
    "stemseg_hip_encoder_check_workspace": (C.c_int, [C.POINTER(EncoderDesc), _P, C.c_size_t, C.POINTER(_I32), C.POINTER(_I64), _P]),
    "stemseg_hip_encoder_forward": (C.c_int, [C.POINTER(EncoderDesc), C.POINTER(EncoderWeights), _P, C.POINTER(Volume), _P, C.c_size_t, _P]),
    "stemseg_hip_encoder_stem_forward": (C.c_int, [C.POINTER(EncoderDesc), C.POINTER(EncoderWeights), _P, _P, _P, _P, C.c_size_t, _P]),
    "stemseg_hip_groupnorm_stats": (C.c_int, [_P, _I32, _I64, _I32, _F, _P, _P, _P]),
    "stemseg_hip_gn_relu_pool": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _I32, C.POINTER(Volume), _P]),
    "stemseg_hip_upsample_trilinear": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, C.POINTER(Volume), _P]),
    "stemseg_hip_copy_to_volume": (C.c_int, [_P, _I32, C.POINTER(Volume), _P]),
    "stemseg_hip_heads": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _I32, C.POINTER(_I32), C.POINTER(_I32), _P, _P, _P, _P, _P]),
    "stemseg_hip_nonfinite_flags": (C.c_int, [_P, _I64, _P, _I32, _P]),
    "stemseg_hip_decoder_workspace_bytes": (C.c_size_t, [C.POINTER(DecoderDesc)]),
    "stemseg_hip_decoder_init_workspace": (C.c_int, [C.POINTER(DecoderDesc), _P, C.c_size_t, _P]),
    "stemseg_hip_decoder_check_workspace": (C.c_int, [C.POINTER(DecoderDesc), _P, C.c_size_t, C.POINTER(_I32), C.POINTER(_I64), _P]),
    "stemseg_hip_decoder_forward": (C.c_int, [C.POINTER(DecoderDesc), C.POINTER(DecoderWeights), C.POINTER(_P), _P, _P, C.c_size_t, _P]),
    "stemseg_hip_decoder_join": (C.c_int, [_I32, _P]),
    "stemseg_hip_seediness_accumulate": (C.c_int, [_P, _P, _I64, _I32, _P]),
    "stemseg_hip_fg_mask": (C.c_int, [_P, _F, _F, _P, _I64, _P]),
    "stemseg_hip_fg_mask_frames": (C.c_int, [_P, _P, _F, _P, _I32, _I64, _P]),
    "stemseg_hip_fg_gather": (C.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, _I64, _P, _P, _P, _P, _P, _P, _P]),
    "stemseg_hip_cluster_workspace_bytes": (C.c_size_t, [_I64]),
    "stemseg_hip_cluster": (C.c_int, [_P, _P, _P, _I64, _P, _I32, _I32, C.POINTER(ClusterParams), _I64, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "stemseg_hip_cluster_batch": (C.c_int, [C.POINTER(ClusterItem), _I32, _I32, _I32, C.POINTER(ClusterParams), _P]),
    "stemseg_hip_overlap_counts": (C.c_int, [_P, _P, _I64, _P, _I32, _P, _I32, _I32, _I32, _P, _P, _P, _P]),
    "stemseg_hip_label_presence": (C.c_int, [_P, _I64, _P, _I32, _P, _I32, _P]),
    "stemseg_hip_relabel": (C.c_int, [_P, _I64, _P, _I32, _P]),
    "stemseg_hip_fg_compact": (C.c_int, [_P, _I32, _I64, _P, _P, _P, _P]),
    "stemseg_hip_labels_to_codes": (C.c_int, [_P, _P, _P, _I64, _I64, _P, _I64, _P]),
    "stemseg_hip_pair_tables": (C.c_int, [_P, _P, _P, _I32, _I64, _I32, _P, _P]),
    "stemseg_hip_codes_to_labels": (C.c_int, [_P, _P, _P, _I32, _I64, _P, _I64, _I32, _P, _P]),
    "stemseg_hip_semseg_accumulate": (C.c_int, [_P, _P, _I32, _I32, _I64, C.POINTER(C.c_int32), _I32, _P]),
    "stemseg_hip_semseg_masks": (C.c_int, [_P, _P, _I32, _I32, _I64, _I32, _P, _P, _P]),
    "stemseg_hip_semseg_fg_clip": (C.c_int, [_P, _I32, _I32, _I64, _F, _P, _P, _P]),
    "stemseg_hip_preprocess_frames": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, C.POINTER(C.c_float), C.POINTER(C.c_float), _I32, _I32, _P, _P]),
    "stemseg_hip_scatter_instance_index": (C.c_int, [_P, _P, _P, _I64, _P, _I32, _P, _I32, _I32, _P]),
    "stemseg_hip_resample_instance_masks": (C.c_int, [_P, _I32, _I32, C.c_float, _I32, _I32, _I32, _I32, _P, _P]),
    "stemseg_hip_scatter_instance_index_ex": (C.c_int, [_P, _P, _P, _I64, _P, _I32, _P, _I32, _I32, _I32, _P]),
    "stemseg_hip_resample_instance_masks_ex": (C.c_int, [_P, _I32, _I32, _I32, C.c_float, _I32, _I32, _I32, _I32, _P, _P]),
    "stemseg_hip_rle_workspace_bytes": (C.c_size_t, [_I32, _I32, _I32, _I32, _I64]),
    "stemseg_hip_rle_plan": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I64, _P, C.c_size_t, _P, _P, _P, _P]),
    "stemseg_hip_rle_encode": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I64, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P]),
    "stemseg_hip_instance_class_stats": (C.c_int, [_P, _P, _P, _P, _I32, _I64, _P, _I32, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _I32, _P, _P, _P]),
    "stemseg_hip_vis_composite": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P, _I32, _P, _P]),
    "stemseg_hip_jpeg_workspace_bytes": (C.c_size_t, [_I32, _I32, _I32]),
    "stemseg_hip_jpeg_plan": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, C.c_size_t, _P, _P, _P]),
    "stemseg_hip_jpeg_encode": (C.c_int, [_I32, _I32, _I32, _I32, _P, C.c_size_t, _P, _I64, _P, _P]),
    "stemseg_hip_jpeg_decode_workspace_bytes": (C.c_size_t, [_I32, _I32, _I32, _I32, _I64, _I64, _I32]),
    "stemseg_hip_jpeg_decode": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I64, _I64, _I32, _I32, _P, C.c_size_t, _P, _P, _P]),
    "stemseg_hip_png_decode_workspace_bytes": (C.c_size_t, [_I32, _I32, _I32, _I32, _I64, _I32, _I32]),
    "stemseg_hip_png_decode": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I64, _I32, _I32, _P, C.c_size_t, _P, _P, _P]),
    "stemseg_hip_embedding_loss_workspace_bytes": (C.c_size_t, [C.POINTER(EmbeddingLossDesc)]),
    "stemseg_hip_embedding_loss_forward": (C.c_int, [C.POINTER(EmbeddingLossDesc), _P, _P, _P, _P, C.c_size_t, _P, C.POINTER(_I32), _P]),
    "stemseg_hip_embedding_loss_backward": (C.c_int, [C.POINTER(EmbeddingLossDesc), _P, _P, _P, _P, C.c_size_t, _P, _I32, _I32, _P, _P]),
    "stemseg_hip_prepare_targets": (C.c_int, [C.POINTER(TargetPrepDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    "stemseg_hip_semseg_loss_workspace_bytes": (C.c_size_t, [C.POINTER(SemsegLossDesc)]),
    "stemseg_hip_semseg_loss_forward": (C.c_int, [C.POINTER(SemsegLossDesc), _P, _P, _P, _P, C.c_size_t, _P, _P, _P]),
    "stemseg_hip_semseg_loss_backward": (C.c_int, [C.POINTER(SemsegLossDesc), _P, _P, _P, _P, C.c_size_t, _P, _I32, _P, _P]),
    "stemseg_hip_level_head": (C.c_int, [_P, _I32, _I64, _P, _I32, _P, _P, _P]),
    "stemseg_hip_heads_backward_workspace_bytes": (C.c_size_t, [_I32, _I32, _I64]),
    "stemseg_hip_heads_backward": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _I32, C.POINTER(_I32), C.POINTER(_I32), _P, _P, _P, _P, _P, _P,
                                             _P, _P, _P, C.c_size_t, _P]),
    "stemseg_hip_wide_level_head": (C.c_int, [_P, _I32, _I64, _P, _I32, _P, _P, _P]),
    "stemseg_hip_wide_heads_backward_workspace_bytes": (C.c_size_t, [_I32, _I32, _I64]),
    "stemseg_hip_wide_heads_backward_chunks": (C.c_int, [_I32, _I32, _I64]),
    "stemseg_hip_wide_heads_backward": (C.c_int, [_P, _I32, _I64, _P, _I32, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "stemseg_hip_upsample_trilinear_backward": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "stemseg_hip_gn_relu_pool_backward_workspace_bytes": (C.c_size_t, [_I32, _I32, _I32, _I32, _I32]),
    "stemseg_hip_gn_relu_pool_backward": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "stemseg_hip_conv3d_wgrad_workspace_bytes": (C.c_size_t, [_I32, _I32, _I32, _I32, _I32]),
    "stemseg_hip_conv3d_wgrad_chunks": (C.c_int, [_I32, _I32, _I32, _I32, _I32]),
    "stemseg_hip_conv3d_wgrad": (C.c_int, [C.POINTER(Volume), _P, _I32, _P, _P, _P, C.c_size_t, _P]),
    "stemseg_hip_conv3d_col2vol": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P]),
    "stemseg_hip_conv2d_wgrad_workspace_bytes": (C.c_size_t, [_I32, _I32, _I32, _I32, _I32, _I32]),
    "stemseg_hip_conv2d_wgrad_chunks": (C.c_int, [_I32, _I32, _I32, _I32, _I32, _I32]),
    "stemseg_hip_conv2d_wgrad": (C.c_int, [C.POINTER(Volume), _P, _I32, _I32, _P, _P, _P, C.c_size_t, _P]),
    "stemseg_hip_conv2d_col2img": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "stemseg_hip_conv2d_grouped_wgrad_workspace_bytes": (C.c_size_t, [_I32, _I32, _I32, _I32, _I32, _I32]),
    "stemseg_hip_conv2d_grouped_wgrad_chunks": (C.c_int, [_I32, _I32, _I32, _I32, _I32, _I32]),
    "stemseg_hip_conv2d_grouped_wgrad": (C.c_int, [C.POINTER(Volume), _P, _I32, _I32, _I32, _P, _P, C.c_size_t, _P]),
    "stemseg_hip_relu_backward": (C.c_int, [C.POINTER(Volume), _P, _P, _P, _P]),
    "stemseg_hip_conv2d_col2img_relu": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, C.POINTER(Volume), _P, _P]),
    "stemseg_hip_subsample2": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P]),
    "stemseg_hip_scatter2": (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "stemseg_hip_scale_rows": (C.c_int, [_P, _P, _I32, _I64, _P]),
    "stemseg_hip_sum_partials": (C.c_int, [_P, _I32, _I64, _P, _P, _P]),
    "stemseg_hip_maxpool3x3s2_backward": (C.c_int, [_P, _P, _I64, _I32, _I32, _I32, _P, _I32, C.POINTER(_I32), _P]),
    "stemseg_hip_stem_wgrad_workspace_bytes": (C.c_size_t, [_I32, _I32, _I32]),
    "stemseg_hip_stem_wgrad_chunks": (C.c_int, [_I32, _I32, _I32]),
    "stemseg_hip_stem_wgrad": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, C.c_size_t, _P]),
    "stemseg_hip_opt_plan": (C.c_int, [C.POINTER(OptTensor), _I32, _I32, C.POINTER(OptChunk), _I64, C.POINTER(_I64)]),
    "stemseg_hip_opt_sgd_step": (C.c_int, [_P, _I32, _P, _I64, C.POINTER(OptHyper), _P, _P]),
    "stemseg_hip_opt_adam_step": (C.c_int, [_P, _I32, _P, _I64, C.POINTER(OptHyper), _P, _P, _P]),
    "stemseg_hip_opt_grad_norm": (C.c_int, [_P, _I32, _P, _I64, _P, _P, C.c_double, _P, _P, _P, _P]),
    "stemseg_hip_opt_bucket_plan": (C.c_int, [C.POINTER(OptTensor), _I32, C.POINTER(_I64), C.POINTER(_I64)]),
    "stemseg_hip_opt_pack_grads": (C.c_int, [_P, _I32, _P, _I64, _P, _P, _I64, C.c_float, _P]),
    "stemseg_hip_opt_unpack_grads": (C.c_int, [_P, _I32, _P, _I64, _P, _P, _I64, _P]),
    "stemseg_hip_opt_reduce_ranks": (C.c_int, [_P, _I32, _I64, _P, _P]),
    "stemseg_hip_rle_decode_workspace_bytes": (C.c_size_t, [_I64, _I32, _I32]),
    "stemseg_hip_rle_decode": (C.c_int, [_P, _I64, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, C.c_size_t, _P, _P, _P]),
    "stemseg_hip_rle_decode_union_workspace_bytes": (C.c_size_t, [_I64, _I32, _I32]),
    "stemseg_hip_rle_decode_union": (C.c_int, [_P, _I64, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, C.c_size_t, _P, _P, _P]),
    "stemseg_hip_rle_decode_labels_workspace_bytes": (C.c_size_t, [_I64, _I32, _I32]),
    "stemseg_hip_rle_decode_labels": (C.c_int, [_P, _I64, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, C.c_size_t, _P, _P, _P, _P]),
    "stemseg_hip_rle_pair_inter_workspace_bytes": (C.c_size_t, [_I64, _I32, _I32]),
    "stemseg_hip_rle_pair_inter": (C.c_int, [_P, _I64, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, C.c_size_t, _P, _P, _P, _P]),
    "stemseg_hip_resize_masks": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _I32, _I32, _P, _P]),
    "stemseg_hip_warp_clip": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _I32, _P, _P, _P, _P]),
    "stemseg_hip_motion_blur": (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _P, _P]),
    "stemseg_hip_duplicate_instance": (C.c_int, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _P]),
    "stemseg_hip_preprocess_frames_masked": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, C.POINTER(C.c_float), C.POINTER(C.c_float), _I32,
                                                       _I32, _P, _P]),
    "stemseg_hip_davis_eval_counts_size": (_I64, [_I32, _I32, _I32]),
    "stemseg_hip_davis_eval_counts": (C.c_int, [_P, _I32, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _I64, _P]),
    "stemseg_hip_label_pair_counts_size": (_I64, [_I32, _I32, _I32]),
    "stemseg_hip_label_pair_counts": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _I64, _P]),
}

SEMSEG_OUTPUT_TYPES = {None: 0, "none": 0, "logits": 1, "probs": 2, "argmax": 3}

_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built -- there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libstemseg_hip.so not found at %s -- build it with `python stem-seg_amd/build.py` "
                               "(hipcc --offload-arch=gfx950); the hot path has no CPU fallback" % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        v = l.stemseg_hip_version()
        if v != ABI_VERSION:
            raise RuntimeError("libstemseg_hip.so ABI version %d != binding %d" % (v, ABI_VERSION))
        _lib = l
    return _lib


def require_gpu():
    l = lib()
    n = l.stemseg_hip_device_count()
    if n <= 0 or not torch.cuda.is_available():
        raise RuntimeError("stemseg_amd: no MI355X visible (hip device count %d, torch.cuda.is_available()=%s): %s"
                           % (n, torch.cuda.is_available(), l.stemseg_hip_last_error().decode()))
    return n


def check(rc):
    if rc != 0:
        raise RuntimeError("libstemseg_hip error %d: %s" % (rc, lib().stemseg_hip_last_error().decode()))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype=None):
    if t is None:
        return None
    assert t.is_cuda, "device tensor required"
    assert t.is_contiguous(), "contiguous tensor required"
    # kernels are enqueued on the CURRENT device's current stream (``stream()``): a tensor of another device would be touched from
    # the wrong device / an unordered stream -- wrap the call in ``torch.cuda.device(t.device)``
    assert t.device.index == torch.cuda.current_device(), "tensor on %s but the current device is cuda:%d" % (t.device, torch.cuda.current_device())
    if dtype is not None:
        assert t.dtype == dtype, "expected %s, got %s" % (dtype, t.dtype)
    return C.c_void_p(t.data_ptr())


def profile_enable(on):
    check(lib().stemseg_hip_profile_enable(int(on)))


# profiler tags: convolutions by tile class (work = FLOP) and the streaming kernels (work = algorithmic bytes)
PROFILE_CONV_TAGS = {"conv3x3x3": (9, 8, 4, 2), "conv1x3x3": (36, 28, 27, 24, 22), "conv1x1x1": (18, 17, 14, 16, 12, 19, 52)}      # (19: the fused bottleneck tail, both of its 1x1 GEMMs; 52: the stage-end tail, conv3 + the FPN lateral)
PROFILE_HBM_TAGS = {40: "upsample_trilinear", 41: "gn_stats (partial + finalize)", 42: "gn_relu (apply)", 43: "gn_relu_pool (apply + AvgPool3d)",
                    44: "heads", 45: "fg_gather (count + scan + scatter)", 46: "cluster (all rounds + final)", 47: "stem_conv7x7",
                    48: "maxpool3x3s2", 49: "subsample2", 50: "upsample2x_add (FPN top-down)",
                    63: "splitk_reduce (one launch per split-K conv launch; timed INSIDE that conv's tag as well)"}
SPLITK_REDUCE_TAG = 63


def profile_read(n_tags=64):
    """{tag: (ms, work, launches)} for the tagged launches since the last read (synchronises)."""
    buf = (C.c_double * (3 * n_tags))()
    check(lib().stemseg_hip_profile_read(buf, n_tags))
    return {t: (buf[3 * t], buf[3 * t + 1], int(buf[3 * t + 2])) for t in range(n_tags) if buf[3 * t + 2] > 0}


# ------------------------------------------------------------------------------------------------ volumes
def padded_geometry(Cn, T, H, W):
    out = (C.c_int64 * 5)()
    check(lib().stemseg_hip_padded_geometry(Cn, T, H, W, out))
    return dict(pitch=out[0], ts=out[1], cs=out[2], total=out[3], interior=out[4])


def dense_volume(t):
    """t: contiguous [C,T,H,W] float32 cuda tensor."""
    Cn, T, H, W = t.shape
    return Volume(t.data_ptr(), T * H * W, H * W, W, Cn, T, H, W, t.numel())


def flat_volume(t):
    """t: contiguous [C, V] -> one-row volume for the 1x1x1 conv."""
    Cn, V = t.shape[0], t[0].numel()
    return Volume(t.data_ptr(), V, 0, 0, Cn, 1, 1, V, t.numel())


def alloc_padded(Cn, T, H, W, device="cuda"):
    g = padded_geometry(Cn, T, H, W)
    return torch.zeros(g["total"], dtype=torch.float32, device=device), g


def alloc_padded_batch(n, Cn, T, H, W, device="cuda"):
    """``n`` zero-haloed buffers of one geometry in ONE allocation, a fixed stride apart (a multiple of 64 floats): the inputs of a
    clip-batched decoder call (StemsegDecoderDesc.feat_clip_stride).  -> (list of n buffer views, geometry, stride in floats)"""
    g = padded_geometry(Cn, T, H, W)
    stride = (g["total"] + 63) // 64 * 64
    whole = torch.zeros(n * stride, dtype=torch.float32, device=device)
    return [whole[c * stride:c * stride + g["total"]] for c in range(n)], g, stride


def padded_halo_view(buf, g, Cn, T, H, W):
    return Volume(buf.data_ptr(), g["cs"], g["ts"], g["pitch"], Cn, T + 2, H + 2, W + 2, g["total"])


def padded_interior_view(buf, g, Cn, T, H, W):
    return Volume(buf.data_ptr() + 4 * g["interior"], g["cs"], g["ts"], g["pitch"], Cn, T, H, W, g["total"] - g["interior"])


def padded_to_dense(buf, g, Cn, T, H, W):
    """Test helper: extract the interior of a zero-haloed buffer as a dense [C,T,H,W] tensor (torch indexing)."""
    v = buf[:Cn * g["cs"]].view(Cn, T + 2, H + 2, g["pitch"])
    return v[:, 1:T + 1, 1:H + 1, 1:W + 1].contiguous()


# ------------------------------------------------------------------------------------------------ decoder ops
def pack_conv_weight(w):
    """w: [Cout, Cin, kt, kh, kw] -> packed [Cin/4][taps][4][Cout] (flat tensor)."""
    w = w.contiguous()
    Cout, Cin = w.shape[0], w.shape[1]
    taps = w[0, 0].numel()
    out = torch.empty(Cout * Cin * taps, dtype=torch.float32, device=w.device)
    check(lib().stemseg_hip_pack_conv_weight(ptr(w, torch.float32), ptr(out), Cout, Cin, taps, stream()))
    return out


PRECISIONS = {"f32": 0, "bf16x6": 2, "f16x3": 3}
# what the matrix products of a mode compute with (bench.py's ``dtype`` names these, never a bare "f32"):
#   operand_significand_bits -- significand bits each fp32 operand keeps (fp32 has 24); products are exact, accumulation is fp32
PRECISION_INFO = {
    "f32": dict(operand_significand_bits=24, products_per_fp32_product=1, mfma="v_mfma_f32_32x32x2_f32", exponent_range="fp32"),
    "bf16x6": dict(operand_significand_bits=24, products_per_fp32_product=6, mfma="v_mfma_f32_32x32x16_bf16", exponent_range="fp32"),
    "f16x3": dict(operand_significand_bits=22, products_per_fp32_product=3, mfma="v_mfma_f32_32x32x16_f16",
                  exponent_range="2.5e-4 <= |activation| < 2.6e5 at full width; beyond: non-finite output, flagged, re-run in bf16x6"),
}
# MFMA mode of every convolution unless a module's ``precision`` is set (InferenceModel.set_precision).  "f16x3" (default) =
# operands scaled by powers of two and split into two fp16 terms, three products, fp32 accumulation; "bf16x6" = every fp32 operand
# split EXACTLY into three bf16 terms, six products (fp32's full exponent range, twice the matrix work).  Both give fp32-level
# results: error vs an fp64 convolution = that of the fp32-input MFMA kernel on every kernel class (tests/test_gpu_bf16x6.py),
# labels identical on every reference flow.  "f32" = v_mfma_f32_32x32x2_f32 on fp32 operands.  STEMSEG_PRECISION overrides the default.
DEFAULT_PRECISION = os.environ.get("STEMSEG_PRECISION", "f16x3")
assert DEFAULT_PRECISION in PRECISIONS, DEFAULT_PRECISION


def pack_conv_weight_any(w, precision="f32"):
    """Pack for the given MFMA mode: 'f32' (exact fp32 MFMA), 'bf16x6' (exact three-term split, 6 products: fp32-level results) or
    'f16x3' (two fp16 terms of the power-of-two-scaled operands, 3 products: fp32-level results for |activation| < 2.6e5); fp32
    accumulate throughout."""
    if precision == "f32":
        return pack_conv_weight(w)
    assert precision in ("bf16x6", "f16x3"), precision
    code = PRECISIONS[precision]
    w = w.contiguous()
    Cout, Cin = w.shape[0], w.shape[1]
    taps = w[0, 0].numel()
    nbytes = lib().stemseg_hip_packed_weight_bytes_prec(Cout, Cin, taps, code)
    if nbytes <= 0:
        raise ValueError("pack_conv_weight_any: unsupported shape / precision (%s, Cout %d, Cin %d, taps %d)" % (precision, Cout, Cin, taps))
    out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)      # opaque 16-B-aligned blob
    check(lib().stemseg_hip_pack_conv_weight_prec(ptr(w, torch.float32), ptr(out), Cout, Cin, taps, code, stream()))
    return out


def pack_grouped_conv_weight(w, groups, precision="f32"):
    """w: [Cout, Cin / groups, 3, 3] (nn.Conv2d(groups=...).weight) -> the grouped kernel's packing for the precision (opaque blob)."""
    w = w.contiguous()
    Cout, Cin_g = w.shape[0], w.shape[1]
    code = PRECISIONS[precision]
    nbytes = lib().stemseg_hip_packed_grouped_weight_bytes(Cout, Cin_g, groups, code)
    if nbytes <= 0 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError("pack_grouped_conv_weight: unsupported shape / precision (%s, %s, %d groups)" % (precision, tuple(w.shape), groups))
    out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    check(lib().stemseg_hip_pack_grouped_conv_weight(ptr(w, torch.float32), ptr(out), Cout, Cin_g, groups, code, stream()))
    return out


def conv2d_grouped(vin, packed_w, bias, vout, groups, stride=1, relu=False, precision="f32", plan_frames=0):
    """Grouped 3x3 convolution (pad 1, stride 1 / 2) + bias (+ ReLU): vin the zero-haloed view of [Cin][T][H][W], vout [Cout][T][Ho][Wo]."""
    check(lib().stemseg_hip_conv2d_grouped(C.byref(vin), ptr(packed_w), ptr(bias), C.byref(vout), int(groups), int(stride), int(bool(relu)),
                                           PRECISIONS[precision], int(plan_frames), stream()))


def stem_conv(frames, w, bias):
    """frames float32 [T,3,H,W], w [64,3,7,7] (FrozenBN folded), bias [64] -> [64,T,H/2,W/2] = relu(conv 7x7 s2 p3 + bias)."""
    require_gpu()
    T, _, H, W = frames.shape
    out = torch.empty(64, T, H // 2, W // 2, dtype=torch.float32, device=frames.device)
    wt = w.reshape(64, 147).t().contiguous()
    check(lib().stemseg_hip_stem_conv(ptr(frames.contiguous(), torch.float32), ptr(wt, torch.float32), ptr(bias.contiguous(), torch.float32), ptr(out), T, H, W, stream()))
    return out


# the encoder's streaming passes on their own (include/stemseg_hip.h: STEMSEG_STREAM_FORM_*, STEMSEG_UP2_FORM_*); form 0 = the library's choice
STREAM_FORM_SCALAR, STREAM_FORM_VEC4 = 1, 2
UP2_FORM_SCALAR, UP2_FORM_VEC4X2, UP2_FORM_DENSE = 1, 2, 3


def _stride2_pass(fn, x, out, form):
    if x.dim() != 3:
        raise ValueError("x %s must be [planes, H, W]" % (tuple(x.shape),))
    planes, H, W = x.shape
    if out is None:
        out = torch.empty(planes, H // 2, W // 2, dtype=torch.float32, device=x.device)
    used = _I32(0)
    check(fn(ptr(x, torch.float32), planes, H, W, ptr(out, torch.float32), int(form), C.byref(used), stream()))
    return out, used.value


def maxpool3x3s2(x, out=None, form=0):
    """x [planes, H, W] (H, W even) -> (max_pool2d(x, 3, 2, 1) [planes, H/2, W/2], the form that ran): the encoder's max-pool pass."""
    return _stride2_pass(lib().stemseg_hip_maxpool3x3s2, x, out, form)


def encoder_subsample2(x, out=None, form=0):
    """x [planes, H, W] (H, W even) -> (x[:, ::2, ::2], the form that ran): the encoder's stride-2 copy (``subsample2`` is the training path's)."""
    return _stride2_pass(lib().stemseg_hip_encoder_subsample2, x, out, form)


def upsample2x_add(fine, coarse, fine_dense=None, form=0):
    """FPN top-down add on the interior views ``fine`` [C][T][H][W] and ``coarse`` [C][T][H/2][W/2] of zero-haloed 2-D buffers (``Volume``):
    fine = (fine_dense if given else fine) + bilinear_x2(coarse).  -> the form that ran."""
    used = _I32(0)
    check(lib().stemseg_hip_upsample2x_add(C.byref(fine), ptr(fine_dense, torch.float32), C.byref(coarse), int(form), C.byref(used), stream()))
    return used.value


def stem_s2d(frames, s2d):
    """frames [T, 3, H, W] -> the f16x3 stem's space-to-depth image, written into the ``Volume`` s2d [12][T][H/2 + 3][W/2 + 3] (halo untouched)."""
    T, _, H, W = frames.shape
    check(lib().stemseg_hip_stem_s2d(ptr(frames, torch.float32), T, H, W, C.byref(s2d), stream()))


def encoder_stream_forms(desc):
    """[max-pool, stride-2 copy of stages 2-4, top-down add of levels 4x, 8x, 16x]: the forms an encoder pass of ``desc`` takes (host only)."""
    out = (_I32 * 7)()
    check(lib().stemseg_hip_encoder_stream_forms(C.byref(desc), out))
    return list(out)


def _conv_epilogue(epilogue):
    """The C epilogue of ``conv3d``'s dict, or None.  'residual' is a tensor, or (``conv3d_plan``) a bare address."""
    if epilogue is None:
        return None
    e = ConvEpilogue()
    e.relu = int(epilogue.get("relu", 0))
    r = epilogue.get("residual")
    if r is not None:
        e.residual = r if isinstance(r, int) else r.data_ptr()
        e.res_c_stride, e.res_t_stride, e.res_y_stride = epilogue["res_strides"]
    e.decode_H, e.decode_W = epilogue.get("decode", (0, 0))
    e.precision = PRECISIONS[epilogue.get("precision", "f32")]
    e.frames, e.plan_frames, e.plan_scratch_floats = epilogue.get("plan", (0, 0, 0))
    return e


PLAN_GN, PLAN_ZERO_T_HALO = 1, 2
TILE_CFG_DEEP = 8          # STEMSEG_TILE_CFG_DEEP: ask for the deep 3x3x3 tile (taken where eligible, tile_cfg 0 otherwise)
PLAN_REDUCE_FORMS = {0: None, 1: "vec16", 2: "scalar"}
PLAN_GN_FORMS = {0: None, 1: "tile epilogue", 2: "split-K reduce", 3: "separate pass"}


def conv3d_plan(vin, vout, k, tile_cfg=0, scratch=None, epilogue=None, bias=1 << 20, gn_groups=0, zero_t_halo=False, plan_clips=0):
    """Dry run of ``conv3d`` (``gn_groups`` > 0: ``conv3d_gn``; ``zero_t_halo``: ``conv3d_zero_t_halo``): the launches the call would make, one dict
    per launch (a planned row cut gives two), decided by the same dispatch code and without a HIP call -- no GPU needed.  The volumes' ``ptr``,
    ``bias``, the epilogue's ``residual`` and ``scratch`` = (address, floats) are ADDRESSES, read for their alignment only; they may be made up.
    For ``conv3d_gn`` the epilogue carries the precision only.  ``plan_clips``: the split-K factor as a decoder stage decides it under
    ``StemsegDecoderDesc.plan_clips`` (0 / 1: on one clip)."""
    kt, kh, kw = (k, k, k) if isinstance(k, int) else k
    e = _conv_epilogue(epilogue)
    form = (PLAN_GN if gn_groups > 0 else 0) | (PLAN_ZERO_T_HALO if zero_t_halo else 0)
    addr, floats = scratch if scratch is not None else (None, 0)
    cap = 4
    rec, count = (ConvPlanRecord * cap)(), _I32(0)
    check(lib().stemseg_hip_conv3d_plan_clips(C.byref(vin), C.c_void_p(bias) if bias else None, C.byref(vout), kt, kh, kw, tile_cfg,
                                              C.c_void_p(addr) if addr else None, floats, C.byref(e) if e is not None else None, form, int(gn_groups),
                                              int(plan_clips), rec, cap, C.byref(count)))
    assert count.value <= cap, count.value
    out = []
    for r in rec[:count.value]:
        d = {n: getattr(r, n) for n, _ in ConvPlanRecord._fields_ if n != "grid"}
        d["grid"] = tuple(r.grid)
        d["precision"] = {v: n for n, v in PRECISIONS.items()}[r.precision]
        d["reduce"], d["gn"] = PLAN_REDUCE_FORMS[r.reduce], PLAN_GN_FORMS[r.gn]
        out.append(d)
    return out


def conv3d(vin, packed_w, bias, vout, k, tile_cfg=0, splitk_scratch=None, epilogue=None):
    """k: int (k x k x k) or a (kt, kh, kw) tuple; epilogue: dict(relu=, residual=tensor, res_strides=(c,t,y), decode=(H,W),
    precision=, plan=(frames, plan_frames, plan_scratch_floats): decide tile / split-K as if the launch held plan_frames frames)."""
    n = 0 if splitk_scratch is None else splitk_scratch.numel()
    kt, kh, kw = (k, k, k) if isinstance(k, int) else k
    e = _conv_epilogue(epilogue)
    check(lib().stemseg_hip_conv3d(C.byref(vin), ptr(packed_w), ptr(bias), C.byref(vout), kt, kh, kw, tile_cfg,
                                   ptr(splitk_scratch), n, C.byref(e) if e is not None else None, stream()))


def conv3d_zero_t_halo(vin, packed_w, bias, vout, k=3, tile_cfg=0, splitk_scratch=None, precision="f32", gn_groups=0, eps=1e-5, plan_clips=0):
    """conv3d (kt == 3) on an input whose temporal halo planes (0 and T + 1 of the haloed view) are PROMISED to hold zeros: the split-staged
    kernels skip the k-groups that only see those planes.  Same output as conv3d on such an input; unspecified if the promise is broken.
    gn_groups > 0: also returns the GroupNorm statistics of the output, as conv3d_gn does.  plan_clips: the split-K factor as a stage of a decoder
    with that ``plan_clips`` decides it (0 / 1: on one clip)."""
    n = 0 if splitk_scratch is None else splitk_scratch.numel()
    kt, kh, kw = (k, k, k) if isinstance(k, int) else k
    e = ConvEpilogue()
    e.precision = PRECISIONS[precision]
    stats = scratch = None
    if gn_groups > 0:
        stats = torch.empty(2 * gn_groups, dtype=torch.float32, device=packed_w.device)
        scratch = torch.empty(lib().stemseg_hip_conv3d_gn_scratch_doubles(vout.C, gn_groups), dtype=torch.float64, device=packed_w.device)
    check(lib().stemseg_hip_conv3d_zero_t_halo_clips(C.byref(vin), ptr(packed_w), ptr(bias), C.byref(vout), kt, kh, kw, tile_cfg, ptr(splitk_scratch), n,
                                                     C.byref(e), int(gn_groups), eps, ptr(stats), ptr(scratch), int(plan_clips), stream()))
    return stats


def conv3d_zero_t_halo_batch(vin, packed_w, bias, vout, n_clips, in_clip_stride, out_clip_stride, tile_cfg=0, precision="f32"):
    """conv3d_zero_t_halo (3x3x3, un-split, no statistics) on ``n_clips`` clips in ONE launch, as a decoder stage runs a clip batch: ``vin`` /
    ``vout`` are clip 0's volumes, clip c's lie c * in_clip_stride / c * out_clip_stride floats behind them."""
    e = ConvEpilogue()
    e.precision = PRECISIONS[precision]
    check(lib().stemseg_hip_conv3d_zero_t_halo_batch(C.byref(vin), ptr(packed_w), ptr(bias), C.byref(vout), 3, 3, 3, tile_cfg, C.byref(e), int(n_clips),
                                                     int(in_clip_stride), int(out_clip_stride), stream()))


def conv3d_gn(vin, packed_w, bias, vout, k, groups, eps=1e-5, tile_cfg=0, splitk_scratch=None, precision="f32"):
    """Convolution + GroupNorm statistics of its output in one pass -> stats float32 [2 * groups] (mean, rstd per group)."""
    n = 0 if splitk_scratch is None else splitk_scratch.numel()
    kt, kh, kw = (k, k, k) if isinstance(k, int) else k
    dev = packed_w.device
    stats = torch.empty(2 * groups, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib().stemseg_hip_conv3d_gn_scratch_doubles(vout.C, groups), dtype=torch.float64, device=dev)
    check(lib().stemseg_hip_conv3d_gn(C.byref(vin), ptr(packed_w), ptr(bias), C.byref(vout), kt, kh, kw, tile_cfg, ptr(splitk_scratch), n,
                                      PRECISIONS[precision], groups, eps, ptr(stats), ptr(scratch), stream()))
    return stats


def groupnorm_stats(x, groups, eps=1e-5):
    Cn = x.shape[0]
    S = x[0].numel()
    stats = torch.empty(2 * groups, dtype=torch.float32, device=x.device)
    scratch = torch.empty(groups * 128, dtype=torch.float64, device=x.device)
    check(lib().stemseg_hip_groupnorm_stats(ptr(x, torch.float32), Cn, S, groups, eps, ptr(stats), ptr(scratch), stream()))
    return stats


def gn_relu_pool(x, groups, stats, gamma, beta, pool, vout):
    Cn, T, H, W = x.shape
    check(lib().stemseg_hip_gn_relu_pool(ptr(x, torch.float32), Cn, T, H, W, groups, ptr(stats), ptr(gamma), ptr(beta),
                                         int(pool), C.byref(vout), stream()))


def upsample_trilinear(x, st, sy, sx, vout=None):
    Cn, T, H, W = x.shape
    out = None
    if vout is None:
        out = torch.empty(Cn, T * st, H * sy, W * sx, dtype=torch.float32, device=x.device)
        vout = dense_volume(out)
    check(lib().stemseg_hip_upsample_trilinear(ptr(x, torch.float32), Cn, T, H, W, st, sy, sx, C.byref(vout), stream()))
    return out


def copy_to_volume(x, layout, vout):
    check(lib().stemseg_hip_copy_to_volume(ptr(x, torch.float32), layout, C.byref(vout), stream()))


def heads(x, w, bias, act, grid_axis, gt, gy, gx):
    Cin, T, H, W = x.shape
    n_out = w.shape[0]
    out = torch.empty(n_out, T, H, W, dtype=torch.float32, device=x.device)
    a = (C.c_int32 * n_out)(*act)
    g = (C.c_int32 * n_out)(*grid_axis)
    check(lib().stemseg_hip_heads(ptr(x, torch.float32), Cin, T, H, W, ptr(w.contiguous()), ptr(bias), n_out, a, g,
                                  ptr(gt), ptr(gy), ptr(gx), ptr(out), stream()))
    return out


# ---- backward of the decoders' tails (csrc/decoder_backward.hip) -------------------------------------------------
def level_head(x, w, add=None):
    """One level of the folded linear tail: x [Cin, ...] (any voxel count), w [n_out, Cin] -> w x (+ add) as [n_out, ...]."""
    Cin, V = x.shape[0], x[0].numel()
    n_out = w.shape[0]
    out = torch.empty((n_out,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    check(lib().stemseg_hip_level_head(ptr(x, torch.float32), Cin, V, ptr(w, torch.float32), n_out, ptr(add), ptr(out), stream()))
    return out


def _workspace(nbytes, what, device):
    if nbytes == 0:
        raise RuntimeError("%s: %s" % (what, lib().stemseg_hip_last_error().decode()))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def heads_backward(x, w, d_out, out=None, act=None, grid_axis=None, gt=None, gy=None, gx=None, want_dx=True, want_db=True):
    """Backward of ``heads`` (act / grid_axis tables and the forward output ``out`` given) or of ``level_head`` (act None: ``d_out`` is
    already the gradient of the linear part).  x [Cin, T, H, W], w [n_out, Cin], d_out [n_out, T, H, W] -> (dx | None, dw, db | None)."""
    Cin, T, H, W = x.shape
    n_out = w.shape[0]
    dev = x.device
    ws = _workspace(lib().stemseg_hip_heads_backward_workspace_bytes(Cin, n_out, T * H * W), "heads_backward", dev)
    dx = torch.empty_like(x) if want_dx else None
    dw = torch.empty(n_out, Cin, dtype=torch.float32, device=dev)
    db = torch.empty(n_out, dtype=torch.float32, device=dev) if want_db else None
    a = g = None
    if act is not None:
        a, g = (C.c_int32 * n_out)(*act), (C.c_int32 * n_out)(*grid_axis)
    check(lib().stemseg_hip_heads_backward(ptr(x, torch.float32), Cin, T, H, W, ptr(w, torch.float32), None, n_out, a, g, ptr(gt), ptr(gy), ptr(gx),
                                           ptr(out), ptr(d_out, torch.float32), ptr(dx), ptr(dw), ptr(db), ptr(ws), ws.numel(), stream()))
    return dx, dw, db


def wide_level_head(x, w, add=None):
    """``level_head`` for a wide linear head, MAX_HEAD_OUT < n_out <= MAX_WIDE_HEAD_OUT, on the fp32-input matrix cores: x [Cin, ...] (any
    voxel count), w [n_out, Cin] plain dense (not packed, not padded) -> w x (+ add) as [n_out, ...]."""
    Cin, V = x.shape[0], x[0].numel()
    n_out = w.shape[0]
    out = torch.empty((n_out,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    check(lib().stemseg_hip_wide_level_head(ptr(x, torch.float32), Cin, V, ptr(w, torch.float32), n_out, ptr(add), ptr(out), stream()))
    return out


def wide_heads_backward_chunks(Cin, n_out, V):
    """The number of voxel chunks ``wide_heads_backward`` cuts V into: a function of the shape only."""
    n = lib().stemseg_hip_wide_heads_backward_chunks(Cin, n_out, V)
    if n == 0:
        raise RuntimeError("wide_heads_backward: %s" % lib().stemseg_hip_last_error().decode())
    return n


def wide_heads_backward(x, w, dz, want_dx=True, want_db=False):
    """Backward of ``wide_level_head``: x [Cin, ...], w [n_out, Cin], dz [n_out, ...] (the gradient of w x) -> (dx | None, dw, db | None),
    both products from one read of x; fp64 across the voxel chunks, no atomics."""
    Cin, V = x.shape[0], x[0].numel()
    n_out = w.shape[0]
    dev = x.device
    ws = _workspace(lib().stemseg_hip_wide_heads_backward_workspace_bytes(Cin, n_out, V), "wide_heads_backward", dev)
    dx = torch.empty_like(x) if want_dx else None
    dw = torch.empty(n_out, Cin, dtype=torch.float32, device=dev)
    db = torch.empty(n_out, dtype=torch.float32, device=dev) if want_db else None
    check(lib().stemseg_hip_wide_heads_backward(ptr(x, torch.float32), Cin, V, ptr(w, torch.float32), n_out, ptr(dz, torch.float32), ptr(dx), ptr(dw),
                                                ptr(db), ptr(ws), ws.numel(), stream()))
    return dx, dw, db


def upsample_trilinear_backward(d_out, st, sy, sx):
    """The adjoint of ``upsample_trilinear``: d_out [C, T st, H sy, W sx] -> [C, T, H, W]."""
    Cn, To, Ho, Wo = d_out.shape
    if To % st or Ho % sy or Wo % sx:
        raise ValueError("upsample_trilinear_backward: %s is no multiple of the scale (%d, %d, %d)" % (tuple(d_out.shape), st, sy, sx))
    d_in = torch.empty(Cn, To // st, Ho // sy, Wo // sx, dtype=torch.float32, device=d_out.device)
    check(lib().stemseg_hip_upsample_trilinear_backward(ptr(d_out, torch.float32), Cn, To // st, Ho // sy, Wo // sx, st, sy, sx, ptr(d_in), stream()))
    return d_in


def gn_relu_pool_backward(x, groups, stats, gamma, beta, pool, d_out):
    """Backward of ``gn_relu_pool`` (pool 0 | 1): x the conv output [C, T, H, W], d_out [C, To, H, W] -> (dx, dgamma, dbeta); groups 0
    ('none' normalisation): (dx, None, None)."""
    Cn, T, H, W = x.shape
    dev = x.device
    dx = torch.empty_like(x)
    ws = dgamma = dbeta = None
    if groups:
        ws = _workspace(lib().stemseg_hip_gn_relu_pool_backward_workspace_bytes(Cn, T, H, W, groups), "gn_relu_pool_backward", dev)
        dgamma, dbeta = torch.empty(Cn, dtype=torch.float32, device=dev), torch.empty(Cn, dtype=torch.float32, device=dev)
    check(lib().stemseg_hip_gn_relu_pool_backward(ptr(x, torch.float32), Cn, T, H, W, groups, ptr(stats), ptr(gamma), ptr(beta), int(pool),
                                                  ptr(d_out, torch.float32), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel() if groups else 0,
                                                  stream()))
    return dx, dgamma, dbeta


# ---- backward of the tap convolutions: 3x3x3 over a volume, 3x3 and 1x1 over F frames, and of the FPN (csrc/conv_backward.hip) ----
def _backward_precision(what, precision):
    if precision == "f16x3":
        raise ValueError("%s: precision 'f16x3' holds for activations of %s only and gradients have no bounded magnitude; use 'bf16x6' or 'f32'"
                         % (what, PRECISION_INFO["f16x3"]["exponent_range"].split(" at ")[0]))
    if precision not in ("bf16x6", "f32"):
        raise ValueError("%s: precision %r (bf16x6 | f32)" % (what, precision))


def _wgrad_chunks(what, taps, Cin, Cout, T, H, W):
    """``what``: 'conv3d_wgrad' (27 taps) or 'conv2d_wgrad' (9 | 1), whose C calls take ``taps`` behind Cout."""
    n = getattr(lib(), "stemseg_hip_%s_chunks" % what)(Cin, Cout, *((taps,) if what == "conv2d_wgrad" else ()), T, H, W)
    if n <= 0:
        raise ValueError(what + ": " + lib().stemseg_hip_last_error().decode())
    return n


def _wgrad(what, taps, v, dy, halo, want_db):
    """dy [Cout, T, H, W] against the input view v, haloed by ``halo`` = (t, y, x) -> (dw [Cout, Cin, *kernel], db [Cout] | None)."""
    Cout, T, H, W = dy.shape
    if (v.T, v.H, v.W) != (T + halo[0], H + halo[1], W + halo[2]):
        raise ValueError("%s: dy %s does not fit the %sinput view (%d, %d, %d)" % (what, tuple(dy.shape), "haloed " if any(halo) else "", v.T, v.H, v.W))
    t = (taps,) if what == "conv2d_wgrad" else ()
    dev = dy.device
    ws = _workspace(getattr(lib(), "stemseg_hip_%s_workspace_bytes" % what)(v.C, Cout, *t, T, H, W), what, dev)
    dw = torch.empty(Cout, v.C, *{27: (3, 3, 3), 9: (3, 3), 1: (1, 1)}[taps], dtype=torch.float32, device=dev)
    db = torch.empty(Cout, dtype=torch.float32, device=dev) if want_db else None
    check(getattr(lib(), "stemseg_hip_" + what)(C.byref(v), ptr(dy, torch.float32), Cout, *t, ptr(dw), ptr(db), ptr(ws), ws.numel(), stream()))
    return dw, db


def _tap_dgrad(what, dy, w, spatial_dims, precision, addend=None, mask=None):
    """The data gradient of a 3^spatial_dims convolution, padding 1: dy [Cout, T, H, W], w [Cout, Cin, 3, ...] -> dx [Cin, T, H, W].  One
    1x1x1 convolution of the flat dy with W_all[(k, ci)][co] = w[co][ci][k] on the forward kernel (taps Cin output channels, Cout terms
    each), then the library's gather sums every voxel's in-range taps, and the addend, in fp64, applies the mask and rounds once."""
    _backward_precision(what, precision)
    taps = 3 ** spatial_dims
    if w.dim() != 2 + spatial_dims or tuple(w.shape[2:]) != (3,) * spatial_dims or dy.dim() != 4 or dy.shape[0] != w.shape[0]:
        raise ValueError("%s: w %s against dy %s" % (what, tuple(w.shape), tuple(dy.shape)))
    Cout, Cin = w.shape[0], w.shape[1]
    if Cin % 32:
        raise ValueError("%s: Cin = %d is no multiple of 32 (the input channels are output channels of the convolution "
                         "that computes dx, and the kernel's Cout rule applies to them)" % (what, Cin))
    if Cout % 4:
        raise ValueError("%s: Cout = %d is no multiple of 4" % (what, Cout))
    _, T, H, W = dy.shape
    if addend is not None and tuple(addend.shape) != (Cin, T, H, W):
        raise ValueError("%s: addend %s, expected %s" % (what, tuple(addend.shape), (Cin, T, H, W)))
    if mask is not None and (mask.C, mask.T, mask.H, mask.W) != (Cin, T, H, W):
        raise ValueError("%s: mask [%d](%d, %d, %d), expected %s" % (what, mask.C, mask.T, mask.H, mask.W, (Cin, T, H, W)))
    V = T * H * W
    w_all = w.detach().float().permute(*range(2, 2 + spatial_dims), 1, 0).reshape(taps * Cin, Cout, 1, 1, 1).contiguous()
    packed = pack_conv_weight_any(w_all, precision)
    dy = dy.contiguous()
    cols = torch.empty(taps * Cin, V, dtype=torch.float32, device=dy.device)
    conv3d(flat_volume(dy.view(Cout, V)), packed, None, flat_volume(cols), 1, epilogue=dict(precision=precision))
    dx = torch.empty(Cin, T, H, W, dtype=torch.float32, device=dy.device)
    a = ptr(None if addend is None else addend.contiguous(), torch.float32)
    if spatial_dims == 3:
        check(lib().stemseg_hip_conv3d_col2vol(ptr(cols), Cin, T, H, W, ptr(dx), stream()))
    elif mask is None:
        check(lib().stemseg_hip_conv2d_col2img(ptr(cols), Cin, T, H, W, a, ptr(dx), stream()))
    else:
        check(lib().stemseg_hip_conv2d_col2img_relu(ptr(cols), Cin, T, H, W, a, C.byref(mask), ptr(dx), stream()))
    return dx


def conv3d_wgrad_chunks(Cin, Cout, T, H, W):
    """The number of K chunks ``conv3d_wgrad`` cuts T H W into: a function of the shape only."""
    return _wgrad_chunks("conv3d_wgrad", 27, Cin, Cout, T, H, W)


def conv3d_wgrad(x_haloed_view, dy, want_db=True):
    """Weight and bias gradients of Conv3d(3, padding=1): x_haloed_view the ``padded_halo_view`` of the convolution's input [Cin, T, H, W],
    dy [Cout, T, H, W] -> (dw [Cout, Cin, 3, 3, 3], db [Cout] | None).  fp32-input MFMA, fp64 across the K chunks; never a split mode."""
    return _wgrad("conv3d_wgrad", 27, x_haloed_view, dy, (2, 2, 2), want_db)


def conv3d_dgrad(dy, w, precision="bf16x6"):
    """Data gradient of Conv3d(3, padding=1): dy [Cout, T, H, W], w [Cout, Cin, 3, 3, 3] -> dx [Cin, T, H, W] = conv3d(dy, W'), padding 1, no
    bias, W'[ci][co][kt][ky][kx] = w[co][ci][2 - kt][2 - ky][2 - kx].  Computed tap by tap: one 1x1x1 convolution of the flat dy with
    W_all[(k, ci)][co] = w[co][ci][k] (27 Cin output channels, Cout terms each) on the forward kernel, then ``conv3d_col2vol`` sums every
    voxel's 27 taps in fp64.  The 27 Cin rows are output channels of that convolution, so the kernel's Cout rule falls on Cin.  'bf16x6'
    (exact operand split, fp32's exponent range) or 'f32'."""
    return _tap_dgrad("conv3d_dgrad", dy, w, 3, precision)


def padded2d_geometry(Cn, F, H, W):
    """The layout of a [C][F][H][W] map that is zero-haloed in y and x only (csrc/encoder.hip Padded2D: the encoder's L[k] and M1 buffers)."""
    pitch = (W + 2 + 3) // 4 * 4
    ts = (H + 2) * pitch
    return dict(pitch=pitch, ts=ts, cs=F * ts, total=Cn * F * ts + 64, interior=pitch + 1)


def alloc_padded2d(Cn, F, H, W, device="cuda"):
    g = padded2d_geometry(Cn, F, H, W)
    return torch.zeros(g["total"], dtype=torch.float32, device=device), g


def padded2d_halo_view(buf, g, Cn, F, H, W, offset=0):
    """The haloed view [C][F][H + 2][W + 2] of a 2-D zero-haloed buffer that starts ``offset`` floats into ``buf``."""
    return Volume(buf.data_ptr() + 4 * offset, g["cs"], g["ts"], g["pitch"], Cn, F, H + 2, W + 2, g["total"])


def padded2d_interior_view(buf, g, Cn, F, H, W, offset=0):
    return Volume(buf.data_ptr() + 4 * (offset + g["interior"]), g["cs"], g["ts"], g["pitch"], Cn, F, H, W, g["total"] - g["interior"])


def conv2d_wgrad_chunks(Cin, Cout, taps, F, H, W):
    """The number of K chunks ``conv2d_wgrad`` cuts F H W into: a function of the shape only."""
    return _wgrad_chunks("conv2d_wgrad", taps, Cin, Cout, F, H, W)


def conv2d_wgrad(x_view, dy, taps, want_db=True):
    """Weight and bias gradients of a 2-D convolution over F frames.  taps 9: Conv2d(3, padding=1), x_view the y/x-zero-haloed view
    [Cin][F][H + 2][W + 2] of its input; taps 1: a 1x1 convolution, x_view any view [Cin][F][H][W].  dy [Cout, F, H, W] -> (dw [Cout, Cin,
    3, 3] | [Cout, Cin, 1, 1], db [Cout] | None).  fp32-input MFMA, fp64 across the K chunks; never a split mode."""
    if taps not in (1, 9):
        raise ValueError("conv2d_wgrad: taps %r (1 | 9)" % (taps,))
    return _wgrad("conv2d_wgrad", taps, x_view, dy, (0, 2, 2) if taps == 9 else (0, 0, 0), want_db)


def conv2d_dgrad(dy, w, precision="bf16x6", addend=None, mask=None):
    """Data gradient of Conv2d(3, padding=1) over F frames: dy [Cout, F, H, W], w [Cout, Cin, 3, 3] -> dx [Cin, F, H, W], plus ``addend``
    [Cin, F, H, W] when given.  Tap by tap, as ``conv3d_dgrad``: one 1x1x1 convolution of the flat dy with W_all[(k, ci)][co] = w[co][ci][k]
    (9 Cin output channels, so the kernel's Cout rule falls on Cin), then ``conv2d_col2img`` sums every pixel's in-range taps and the addend
    in fp64 and rounds once.  'bf16x6' or 'f32'.  ``mask``: a view [Cin][F][H][W] of the convolution's input after its ReLU (e.g. the interior
    of the haloed buffer): the gather also applies ``relu_backward``'s mask to the sum before that rounding (``conv2d_col2img_relu``)."""
    return _tap_dgrad("conv2d_dgrad", dy, w, 2, precision, addend, mask)


GROUP_WIDTHS = (4, 8, 16, 32, 64)         # channels per group the grouped kernels take with more than one group; one group: any multiple of 16


def _grouped_shape(what, Cn, groups, stride):
    """The shapes ``conv2d_grouped`` serves, refused here before any launch."""
    if groups < 1 or Cn % 16 or Cn % groups:
        raise ValueError("%s: %d channels in %d groups (a multiple of 16 channels, divisible by the groups)" % (what, Cn, groups))
    Cg = Cn // groups
    if (groups > 1 and Cg not in GROUP_WIDTHS) or (groups == 1 and Cg % 16):
        raise ValueError("%s: %d channels per group unsupported (4, 8, 16, 32, 64; one group: a multiple of 16)" % (what, Cg))
    if stride not in (1, 2):
        raise ValueError("%s: stride %r (1 | 2)" % (what, stride))
    return Cg


def conv2d_grouped_wgrad_chunks(Cn, groups, stride, F, H, W):
    """The number of K chunks ``conv2d_grouped_wgrad`` cuts F Ho Wo into: a function of the shape only (H, W: the INPUT map's extents)."""
    n = lib().stemseg_hip_conv2d_grouped_wgrad_chunks(Cn, groups, stride, F, H, W)
    if n <= 0:
        raise ValueError("conv2d_grouped_wgrad: " + lib().stemseg_hip_last_error().decode())
    return n


def conv2d_grouped_wgrad(x_haloed_view, dy, groups, stride):
    """Weight gradient of the grouped 3x3 convolution ``conv2d_grouped`` (padding 1, stride 1 | 2): x_haloed_view the y/x-zero-haloed view
    [C][F][H + 2][W + 2] of its input, dy [C, F, Ho, Wo] with Ho = (H - 1) // stride + 1 -> dw [C, C / groups, 3, 3].  fp32-input MFMA, no
    fp32 chain over more than 16 pixels, fp64 across the K chunks; never a split mode.  No bias gradient (the FrozenBN shift is a buffer)."""
    v = x_haloed_view
    Cg = _grouped_shape("conv2d_grouped_wgrad", v.C, groups, stride)
    H, W = v.H - 2, v.W - 2
    want = (v.C, v.T, (H - 1) // stride + 1, (W - 1) // stride + 1)
    if H < 1 or W < 1 or dy.dim() != 4 or tuple(dy.shape) != want:
        raise ValueError("conv2d_grouped_wgrad: dy %s does not fit the haloed input view [%d](%d, %d, %d) at stride %d (expected %s)"
                         % (tuple(dy.shape), v.C, v.T, v.H, v.W, stride, want))
    dev = dy.device
    ws = _workspace(lib().stemseg_hip_conv2d_grouped_wgrad_workspace_bytes(v.C, groups, stride, v.T, H, W), "conv2d_grouped_wgrad", dev)
    dw = torch.empty(v.C, Cg, 3, 3, dtype=torch.float32, device=dev)
    check(lib().stemseg_hip_conv2d_grouped_wgrad(C.byref(v), ptr(dy.contiguous(), torch.float32), v.C, groups, stride, ptr(dw), ptr(ws), ws.numel(), stream()))
    return dw


def grouped_dgrad_weight(w, groups):
    """W'[g Cg + cj][co_j][ky][kx] = w[g Cg + co_j][cj][2 - ky][2 - kx]: per group transposed, both taps flipped -- the weight whose forward
    grouped convolution is the data gradient of the convolution with w [C, Cg, 3, 3]."""
    Cn, Cg = w.shape[0], w.shape[1]
    return w.detach().float().reshape(groups, Cg, Cg, 3, 3).transpose(1, 2).flip(3, 4).reshape(Cn, Cg, 3, 3).contiguous()


def conv2d_grouped_dgrad(dy, w, groups, stride, precision="f32", mask=None):
    """Data gradient of the grouped 3x3 convolution (padding 1, stride 1 | 2): dy [C, F, Ho, Wo], w [C, C / groups, 3, 3] -> dx [C, F, H, W],
    H = stride Ho.  No kernel of its own: the forward ``conv2d_grouped`` at stride 1, same groups, no bias, on ``grouped_dgrad_weight(w)``,
    of dy copied into the zero-haloed layout -- for stride 2 of the zero-dilated dy (``scatter2`` without an addend), which needs even H and
    W and issues 4x the matrix work.  ``mask``: a view [C][F][H][W] of the convolution's input after its ReLU; ``relu_backward`` applies it.
    'f32' or 'bf16x6'."""
    _backward_precision("conv2d_grouped_dgrad", precision)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or dy.dim() != 4 or dy.shape[0] != w.shape[0]:
        raise ValueError("conv2d_grouped_dgrad: w %s against dy %s" % (tuple(w.shape), tuple(dy.shape)))
    Cn, F, Ho, Wo = dy.shape
    Cg = _grouped_shape("conv2d_grouped_dgrad", Cn, groups, stride)
    if w.shape[1] != Cg:
        raise ValueError("conv2d_grouped_dgrad: w %s holds %d channels per group, %d groups of %d channels need %d" % (tuple(w.shape), w.shape[1], groups, Cn, Cg))
    H, W = stride * Ho, stride * Wo
    if mask is not None and (mask.C, mask.T, mask.H, mask.W) != (Cn, F, H, W):
        if stride == 2 and (mask.C, mask.T, (mask.H + 1) // 2, (mask.W + 1) // 2) == (Cn, F, Ho, Wo):
            raise ValueError("conv2d_grouped_dgrad: stride 2 needs even H and W, the mask is %d x %d" % (mask.H, mask.W))
        raise ValueError("conv2d_grouped_dgrad: mask [%d](%d, %d, %d), expected %s" % (mask.C, mask.T, mask.H, mask.W, (Cn, F, H, W)))
    packed = pack_grouped_conv_weight(grouped_dgrad_weight(w, groups), groups, precision)
    g = dy.detach().contiguous().float()
    if stride == 2:
        g = scatter2(g)
    buf, geo = alloc_padded2d(Cn, F, H, W, dy.device)
    copy_to_volume(g, 0, padded2d_interior_view(buf, geo, Cn, F, H, W))
    dx = torch.empty(Cn, F, H, W, dtype=torch.float32, device=dy.device)
    conv2d_grouped(padded2d_halo_view(buf, geo, Cn, F, H, W), packed, None, dense_volume(dx), groups, 1, False, precision)
    if mask is not None:
        relu_backward(mask, dx, out=dx)
    return dx


# ---- the streaming kernels of the bottleneck backward (csrc/bottleneck_backward.hip); the block itself: modeling/encoder_backward.py ----
DGRAD_K_CHUNK = 256                        # conv1x1_dgrad: output channels summed in one fp32 chain; wider gradients are cut and the chunks added in fp64


def relu_backward(y_view, g, addend=None, out=None):
    """(y <= 0) ? 0 : g + addend -- torch's threshold_backward of the fp32 sum (a NaN activation lets the gradient through, +-0.0 blocks it).
    y_view: any view [C][F][H][W] of the activation AFTER its ReLU (dense, or the interior of the zero-haloed 2-D layout); g, addend dense
    [C, F, H, W]; ``out`` may be ``g`` (in place).  With the addend it is also the residual join of an identity block, in the same pass."""
    shape = (y_view.C, y_view.T, y_view.H, y_view.W)
    for name, t in (("g", g), ("addend", addend), ("out", out)):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError("relu_backward: %s %s, expected %s (the view of y)" % (name, tuple(t.shape), shape))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=g.device)
    check(lib().stemseg_hip_relu_backward(C.byref(y_view), ptr(g, torch.float32), ptr(addend, torch.float32), ptr(out, torch.float32), stream()))
    return out


def subsample2(x):
    """x [C, F, 2h, 2w] -> [C, F, h, w]: the even rows and columns (the input of a stride-2 1x1 convolution and of its weight gradient)."""
    if x.dim() != 4 or x.shape[2] % 2 or x.shape[3] % 2:
        raise ValueError("subsample2: x %s needs even H and W" % (tuple(x.shape),))
    Cn, F, H, W = x.shape
    out = torch.empty(Cn, F, H // 2, W // 2, dtype=torch.float32, device=x.device)
    check(lib().stemseg_hip_subsample2(ptr(x, torch.float32), Cn, F, H, W, ptr(out), stream()))
    return out


def scatter2(g, addend=None):
    """The adjoint of ``subsample2``: g [C, F, h, w] -> [C, F, 2h, 2w] = addend + (g at even rows and columns, zero elsewhere); the other
    positions hold the addend's own bits.  The addend is how a second gradient of the large map joins without a pass of its own."""
    Cn, F, h, w = g.shape
    if addend is not None and tuple(addend.shape) != (Cn, F, 2 * h, 2 * w):
        raise ValueError("scatter2: addend %s, expected %s" % (tuple(addend.shape), (Cn, F, 2 * h, 2 * w)))
    out = torch.empty(Cn, F, 2 * h, 2 * w, dtype=torch.float32, device=g.device)
    check(lib().stemseg_hip_scatter2(ptr(g, torch.float32), Cn, F, 2 * h, 2 * w, ptr(addend, torch.float32), ptr(out), stream()))
    return out


def scale_rows(dw, scale):
    """dw[co] *= scale[co] in place: the gradient of a convolution's own weight from that of the weight with FrozenBN folded in."""
    if scale.dim() != 1 or scale.shape[0] != dw.shape[0]:
        raise ValueError("scale_rows: scale %s against dw %s" % (tuple(scale.shape), tuple(dw.shape)))
    check(lib().stemseg_hip_scale_rows(ptr(dw, torch.float32), ptr(scale, torch.float32), dw.shape[0], dw[0].numel(), stream()))
    return dw


# ---- the backward of the stem (csrc/stem_backward.hip); its composition: modeling/encoder_backward.py stem_backward ----
def maxpool3x3s2_backward(x, g, mask_relu=False, out=None, form=0):
    """The adjoint of ``max_pool2d(x, 3, 2, 1)``: x [planes, H, W] the pool's input (H, W even), g [planes, H/2, W/2] -> (dx [planes, H, W],
    the form that ran).  torch's CPU backward bit for bit (the first maximum of a window wins, the last NaN wins; the windows of a pixel are
    added in ascending order in fp32).  ``mask_relu``: x is a map AFTER its ReLU and ``relu_backward``'s rule is applied to dx in the same
    pass (x <= 0 gives 0; a NaN lets the gradient through).  form: STREAM_FORM_SCALAR | STREAM_FORM_VEC4 | 0 (the library's choice)."""
    if x.dim() != 3 or x.shape[1] % 2 or x.shape[2] % 2:
        raise ValueError("maxpool3x3s2_backward: x %s must be [planes, H, W] with even H and W" % (tuple(x.shape),))
    planes, H, W = x.shape
    if tuple(g.shape) != (planes, H // 2, W // 2):
        raise ValueError("maxpool3x3s2_backward: g %s, expected %s" % (tuple(g.shape), (planes, H // 2, W // 2)))
    if out is None:
        out = torch.empty(planes, H, W, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (planes, H, W):
        raise ValueError("maxpool3x3s2_backward: out %s, expected %s" % (tuple(out.shape), (planes, H, W)))
    used = _I32(0)
    check(lib().stemseg_hip_maxpool3x3s2_backward(ptr(x, torch.float32), ptr(g, torch.float32), planes, H, W, int(bool(mask_relu)), ptr(out, torch.float32),
                                                  int(form), C.byref(used), stream()))
    return out, used.value


def stem_wgrad_chunks(F, H, W):
    """The number of K chunks ``stem_wgrad`` cuts F frames of H x W into: a function of the shape only (host only)."""
    n = lib().stemseg_hip_stem_wgrad_chunks(int(F), int(H), int(W))
    if n <= 0:
        raise ValueError("stem_wgrad: " + lib().stemseg_hip_last_error().decode())
    return n


def stem_wgrad(frames, g, out=None):
    """Weight gradient of the stem's Conv2d(3, 64, 7, stride 2, padding 3): frames [F, 3, H, W] (H, W even), g [64, F, H/2, W/2] the gradient
    of its output -> dw [64, 3, 7, 7] (the fp32-input MFMA, fp64 across chunks; written into ``out`` when given).  No bias gradient, no data
    gradient."""
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError("stem_wgrad: frames %s must be [F, 3, H, W]" % (tuple(frames.shape),))
    F, _, H, W = frames.shape
    if H % 2 or W % 2 or tuple(g.shape) != (64, F, H // 2, W // 2):
        raise ValueError("stem_wgrad: g %s against frames %s (expected [64, F, H/2, W/2], H and W even)" % (tuple(g.shape), tuple(frames.shape)))
    ws = _workspace(lib().stemseg_hip_stem_wgrad_workspace_bytes(F, H, W), "stem_wgrad", g.device)
    dw = torch.empty(64, 3, 7, 7, dtype=torch.float32, device=g.device) if out is None else out
    if tuple(dw.shape) != (64, 3, 7, 7):
        raise ValueError("stem_wgrad: out %s, expected (64, 3, 7, 7)" % (tuple(dw.shape),))
    check(lib().stemseg_hip_stem_wgrad(ptr(frames, torch.float32), ptr(g, torch.float32), F, H, W, ptr(dw, torch.float32), ptr(ws), ws.numel(), stream()))
    return dw


def conv1x1_dgrad(dy, w, precision="bf16x6", addend=None):
    """Data gradient of a 1x1 convolution over F frames: dy [Cout, F, H, W], w [Cout, Cin, 1, 1] -> dx [Cin, F, H, W] = w^T dy (+ ``addend``,
    added in the convolution's epilogue): the forward 1x1x1 kernel on the transposed weight, so the kernel's Cout rule falls on Cin.
    Cout > DGRAD_K_CHUNK: one convolution per chunk of that many output channels, and ``sum_partials`` adds the chunks and the addend in
    fp64 and rounds once -- the kernel's sum over the channels is one fp32 chain, and the body has chains over 512 .. 2048 channels in
    every block (one of the two changes that brought its gradients inside the tests' bound).  'bf16x6' or 'f32'."""
    _backward_precision("conv1x1_dgrad", precision)
    if w.dim() != 4 or tuple(w.shape[2:]) != (1, 1) or dy.dim() != 4 or dy.shape[0] != w.shape[0]:
        raise ValueError("conv1x1_dgrad: w %s against dy %s" % (tuple(w.shape), tuple(dy.shape)))
    Cout, Cin = w.shape[0], w.shape[1]
    if Cin % 32:
        raise ValueError("conv1x1_dgrad: Cin = %d is no multiple of 32 (the input channels are output channels of the convolution that "
                         "computes dx, and the kernel's Cout rule applies to them)" % Cin)
    if Cout % 4:
        raise ValueError("conv1x1_dgrad: Cout = %d is no multiple of 4" % Cout)
    _, F, H, W = dy.shape
    if addend is not None and tuple(addend.shape) != (Cin, F, H, W):
        raise ValueError("conv1x1_dgrad: addend %s, expected %s" % (tuple(addend.shape), (Cin, F, H, W)))
    V = F * H * W
    wt = w.detach().float().reshape(Cout, Cin)
    dy = dy.contiguous()
    dx = torch.empty(Cin, F, H, W, dtype=torch.float32, device=dy.device)
    e = dict(precision=precision)
    if Cout > DGRAD_K_CHUNK:
        n = -(-Cout // DGRAD_K_CHUNK)
        parts = torch.empty(n, Cin, V, dtype=torch.float32, device=dy.device)
        dy2 = dy.view(Cout, V)
        for j in range(n):
            lo, hi = j * DGRAD_K_CHUNK, min(Cout, (j + 1) * DGRAD_K_CHUNK)
            pj = pack_conv_weight_any(wt[lo:hi].t().reshape(Cin, hi - lo, 1, 1, 1).contiguous(), precision)
            conv3d(flat_volume(dy2[lo:hi]), pj, None, flat_volume(parts[j]), 1, epilogue=e)
        check(lib().stemseg_hip_sum_partials(ptr(parts), n, Cin * V, ptr(None if addend is None else addend.contiguous(), torch.float32), ptr(dx), stream()))
        return dx
    packed = pack_conv_weight_any(wt.t().reshape(Cin, Cout, 1, 1, 1).contiguous(), precision)
    if addend is not None:
        e.update(residual=addend.contiguous(), res_strides=(V, 0, 0))
    conv3d(flat_volume(dy.view(Cout, V)), packed, None, flat_volume(dx.view(Cin, V)), 1, epilogue=e)
    return dx


NONFINITE_FLAGS = 64
MAX_HEAD_OUT = 10          # STEMSEG_MAX_HEAD_OUT: widest head the fused heads kernel serves (wider: the 1x1x1 MFMA conv)
MAX_WIDE_HEAD_OUT = 64     # STEMSEG_MAX_WIDE_HEAD_OUT: widest linear head wide_level_head / wide_heads_backward serve (training)


class NonFiniteError(FloatingPointError):
    """A head output (embedding / bandwidth / seediness / class logits) of a clip holds inf or NaN: an operand left the range of
    the split convolution mode (f16x3: |activation| < 2.6e5).  Re-run the clip in 'bf16x6' (ClipPipeline.step_checked does)."""


def nonfinite_flags(x, flags=None):
    """x: contiguous float32 device tensor -> int32 [NONFINITE_FLAGS] on the device (1 where a chunk of x holds inf / NaN); no
    synchronisation.  ``flags``: an existing int32 view to (re)write."""
    if flags is None:
        flags = torch.empty(NONFINITE_FLAGS, dtype=torch.int32, device=x.device)
    assert x.is_contiguous() and x.dtype == torch.float32 and flags.numel() == NONFINITE_FLAGS
    check(lib().stemseg_hip_nonfinite_flags(ptr(x), x.numel(), ptr(flags, torch.int32), NONFINITE_FLAGS, stream()))
    return flags


def overflow_status(tensors):
    """Overflow flags of a clip's head outputs: int32 [k, NONFINITE_FLAGS] on the device, one launch per run of tensors that are
    adjacent in memory (embeddings and bandwidths are channel slices of one decoder output).  No synchronisation; hand the result to
    ``read_cluster_meta(meta, status)``."""
    runs = []
    for t in tensors:
        assert t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda
        if runs and runs[-1][0] + 4 * runs[-1][1] == t.data_ptr():
            runs[-1][1] += t.numel()
        else:
            runs.append([t.data_ptr(), t.numel(), t])
    status = torch.empty(len(runs), NONFINITE_FLAGS, dtype=torch.int32, device=tensors[0].device)
    for i, (p_, n, _) in enumerate(runs):
        check(lib().stemseg_hip_nonfinite_flags(C.c_void_p(p_), n, ptr(status[i], torch.int32), NONFINITE_FLAGS, stream()))
    return status


# ------------------------------------------------------------------------------------------------ clustering ops
def seediness_accumulate(acc, plane, first):
    check(lib().stemseg_hip_seediness_accumulate(ptr(acc, torch.float32), ptr(plane, torch.float32), plane.numel(), int(first), stream()))


def fg_mask(acc, count, thr):
    mask = torch.empty(acc.shape, dtype=torch.uint8, device=acc.device)
    check(lib().stemseg_hip_fg_mask(ptr(acc, torch.float32), float(count), float(thr), ptr(mask), acc.numel(), stream()))
    return mask


def fg_mask_frames(acc, counts, thr):
    """acc float32 [F,h,w] (per-frame sums), counts float32 [F] on the device -> uint8 [F,h,w]: acc / counts > thr."""
    Fn = acc.shape[0]
    mask = torch.empty(acc.shape, dtype=torch.uint8, device=acc.device)
    check(lib().stemseg_hip_fg_mask_frames(ptr(acc, torch.float32), ptr(counts, torch.float32), float(thr), ptr(mask), Fn,
                                           acc[0].numel() if Fn else 0, stream()))
    return mask


def fg_gather(emb, bw, seed, fg):
    """emb [E,T,H,W], bw [Ev,T,H,W], seed [1,T,H,W] (or [T,H,W]), fg uint8 [T,H,W].
    Returns max-size outputs (first N rows valid) + frame_offsets [T+1] int64 (device)."""
    E, T, H, W = emb.shape
    Ev = bw.shape[0]
    V = T * H * W
    dev = emb.device
    emb_o = torch.empty(V, E, dtype=torch.float32, device=dev)
    bw_o = torch.empty(V, max(Ev, 1), dtype=torch.float32, device=dev)[:, :Ev].contiguous() if Ev == 0 else \
        torch.empty(V, Ev, dtype=torch.float32, device=dev)
    seed_o = torch.empty(V, dtype=torch.float32, device=dev)
    vox = torch.empty(V, dtype=torch.int32, device=dev)
    offs = torch.empty(T + 1, dtype=torch.int64, device=dev)
    scratch = torch.empty(16 * (V // 1024 + 4), dtype=torch.uint8, device=dev)
    check(lib().stemseg_hip_fg_gather(ptr(emb, torch.float32), ptr(bw, torch.float32), ptr(seed, torch.float32), ptr(fg, torch.uint8),
                                      E, Ev, T, H * W, ptr(emb_o), ptr(bw_o), ptr(seed_o), ptr(vox), ptr(offs), ptr(scratch), stream()))
    return emb_o, bw_o, seed_o, vox, offs


def make_cluster_params(primary, secondary, min_seed, max_instances, free_dim_stds):
    p = ClusterParams()
    p.primary_prob_thresh, p.secondary_prob_thresh, p.min_seediness_prob = primary, secondary, min_seed
    p.max_instances = int(max_instances)
    p.n_free_dims = len(free_dim_stds)
    if len(free_dim_stds):
        # 1 / std^2 exactly as clusterers.py:101-103 (fp32 tensor ops on the host: a handful of scalars)
        fb = (1. / (torch.tensor(list(free_dim_stds), dtype=torch.float32) ** 2)).tolist()
        for i, v in enumerate(fb):
            p.free_dim_bandwidths[i] = v
    return p


def cluster(emb, bw, seed, params, label_start, n_points_dev=None, want_masks=False, want_probs=False):
    """emb [Nmax,E], bw [Nmax,Ev], seed [Nmax].  Returns labels int64 [Nmax], meta (device uint8 blob), masks, probs."""
    n_max, E = emb.shape
    Ev = bw.shape[1]
    dev = emb.device
    labels = torch.empty(n_max, dtype=torch.int64, device=dev)
    meta = torch.empty(C.sizeof(ClusterMeta), dtype=torch.uint8, device=dev)
    masks = torch.empty(params.max_instances, n_max, dtype=torch.uint8, device=dev) if want_masks else None
    probs = torch.empty(params.max_instances, n_max, dtype=torch.float32, device=dev) if want_probs else None
    ws_bytes = lib().stemseg_hip_cluster_workspace_bytes(n_max)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(lib().stemseg_hip_cluster(ptr(emb, torch.float32), ptr(bw, torch.float32), ptr(seed, torch.float32), n_max,
                                    ptr(n_points_dev), E, Ev, C.byref(params), int(label_start), ptr(labels), ptr(meta),
                                    ptr(masks), ptr(probs), ptr(ws), ws_bytes, stream()))
    return labels, meta, masks, probs


def cluster_batch(point_sets, params, label_start=1):
    """Several independent point sets (the clips of one step) through ONE sequence of launches (grid.y = set): point_sets = list of
    (emb [Nmax,E], bw [Nmax,Ev], seed [Nmax], n_points_dev | None).  Returns a list of (labels int64 [Nmax], meta device blob), bit
    identical to separate ``cluster`` calls; no synchronisation."""
    n = len(point_sets)
    items = (ClusterItem * n)()
    keep, outs = [], []
    E, Ev = point_sets[0][0].shape[1], point_sets[0][1].shape[1]
    for i, (emb, bw, seed, n_dev) in enumerate(point_sets):
        assert emb.shape[1] == E and bw.shape[1] == Ev
        n_max, dev = emb.shape[0], emb.device
        labels = torch.empty(n_max, dtype=torch.int64, device=dev)
        meta = torch.empty(C.sizeof(ClusterMeta), dtype=torch.uint8, device=dev)
        ws_bytes = lib().stemseg_hip_cluster_workspace_bytes(n_max)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        seed = seed.reshape(-1)
        it = items[i]
        it.emb, it.bw, it.seed = ptr(emb, torch.float32), ptr(bw, torch.float32) if Ev else None, ptr(seed, torch.float32)
        it.n_max, it.n_points_dev, it.label_start = n_max, ptr(n_dev), int(label_start)
        it.labels, it.meta_dev, it.opt_masks, it.opt_probs = ptr(labels), ptr(meta), None, None
        it.workspace, it.ws_bytes = ptr(ws), ws_bytes
        keep.append(ws)
        outs.append((labels, meta))
    check(lib().stemseg_hip_cluster_batch(items, n, E, Ev, C.byref(params), stream()))
    return outs


_meta_pinned = {}


def read_cluster_meta(meta_dev, status=None):
    """Device->host copy of the StemsegClusterMeta record (synchronises the current stream).  The copy lands in a
    persistent PINNED host buffer: a direct DMA, no pageable staging (``.cpu()`` on a tensor that lives in a hipGraph's
    private pool was seen to fault the GPU after a few replays on ROCm 7.2).  ``status``: the clip's overflow flags
    (nonfinite_flags, int32 on the device), read with the same synchronisation; raises NonFiniteError when one is set."""
    n = meta_dev.numel()
    key = (meta_dev.device.index, n)
    buf = _meta_pinned.get(key)
    if buf is None:
        buf = _meta_pinned[key] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    buf.copy_(meta_dev, non_blocking=True)
    sbuf = None
    if status is not None:
        skey = (meta_dev.device.index, "status", status.numel())
        sbuf = _meta_pinned.get(skey)
        if sbuf is None:
            sbuf = _meta_pinned[skey] = torch.empty(status.numel(), dtype=torch.int32, pin_memory=True)
        sbuf.copy_(status.reshape(-1), non_blocking=True)
    torch.cuda.current_stream(meta_dev.device).synchronize()
    if sbuf is not None and bool(sbuf.any()):
        raise NonFiniteError("a head output of this clip holds inf / NaN (an operand left the convolution mode's range): not clustered "
                             "results -- re-run the clip with precision 'bf16x6'")
    return ClusterMeta.from_buffer_copy(buf.numpy().tobytes())


def overlap_counts(labels_a, labels_b, lut_a, lut_b, Ka, Kb):
    dev = labels_a.device
    inter = torch.empty(max(Ka * Kb, 1), dtype=torch.int64, device=dev)
    ca = torch.empty(max(Ka, 1), dtype=torch.int64, device=dev)
    cb = torch.empty(max(Kb, 1), dtype=torch.int64, device=dev)
    check(lib().stemseg_hip_overlap_counts(ptr(labels_a, torch.int64), ptr(labels_b, torch.int64), labels_a.numel(),
                                           ptr(lut_a, torch.int32), lut_a.numel(), ptr(lut_b, torch.int32), lut_b.numel(),
                                           Ka, Kb, ptr(inter), ptr(ca), ptr(cb), stream()))
    return inter[:Ka * Kb].view(Ka, Kb), ca[:Ka], cb[:Kb]


def label_presence(labels_list, cap):
    """-> (present uint8 [cap + 1] on the device: byte l = label l occurs, byte ``cap`` = a negative (outlier) label occurs;
    max_plus_1 int64 [1] on the device) over all tensors of ``labels_list`` (int64, same device); no synchronisation."""
    dev = labels_list[0].device
    present = torch.empty(int(cap) + 1, dtype=torch.uint8, device=dev)
    mx = torch.empty(1, dtype=torch.int64, device=dev)
    for k, l in enumerate(labels_list):
        check(lib().stemseg_hip_label_presence(ptr(l, torch.int64) if l.numel() else None, l.numel(), ptr(present), int(cap),
                                               ptr(mx), int(k > 0), stream()))
    return present, mx


def relabel(labels, mapping):
    check(lib().stemseg_hip_relabel(ptr(labels, torch.int64), labels.numel(), ptr(mapping, torch.int64), mapping.numel(), stream()))


# ---- clip-parallel stitching (pipeline.run_sequence_sharded) ------------------------------------------------
def fg_compact(fg):
    """fg uint8 [T,H,W] -> (voxel_index int32 [V] (first N valid), frame_offsets int64 [T+1]) on the device, no sync."""
    T = fg.shape[0]
    HW = fg[0].numel()
    V = T * HW
    vox = torch.empty(V, dtype=torch.int32, device=fg.device)
    offs = torch.empty(T + 1, dtype=torch.int64, device=fg.device)
    scratch = torch.empty(16 * (V // 1024 + 4), dtype=torch.uint8, device=fg.device)
    check(lib().stemseg_hip_fg_compact(ptr(fg, torch.uint8), T, HW, ptr(vox), ptr(offs), ptr(scratch), stream()))
    return vox, offs


def labels_to_codes(labels, vox, n_points_dev, label_start, codes_out):
    """codes_out uint8 [V] (a contiguous view, e.g. one clip's [T,h,w] block of the exchange buffer) := 0, then
    codes_out[vox[i]] = labels[i] - label_start + 1 (255: outlier) for the first N points."""
    check(lib().stemseg_hip_labels_to_codes(ptr(labels, torch.int64) if labels.numel() else None, ptr(vox, torch.int32) if vox.numel() else None,
                                            ptr(n_points_dev), min(labels.numel(), codes_out.numel()), int(label_start),
                                            ptr(codes_out, torch.uint8), codes_out.numel(), stream()))
    return codes_out


def pair_tables(codes, plane_a, plane_b, B):
    """codes uint8 [P, HW]; plane_a / plane_b int32 [n] on the device -> int32 [n, B, B] on the device (no sync)."""
    n = plane_a.numel()
    HW = codes.shape[1]
    tables = torch.empty(n, B, B, dtype=torch.int32, device=codes.device)
    check(lib().stemseg_hip_pair_tables(ptr(codes, torch.uint8), ptr(plane_a, torch.int32), ptr(plane_b, torch.int32), n, HW, B,
                                        ptr(tables), stream()))
    return tables


def codes_to_labels(codes, vox, items, lut, max_count, n_out):
    """items int64 [n,5] = (src_begin, count, vbase, plane, out_begin), lut int64 [n,B] (both on the device) -> int64 [n_out]."""
    n, B = lut.shape
    out = torch.empty(n_out, dtype=torch.int64, device=codes.device)
    check(lib().stemseg_hip_codes_to_labels(ptr(codes, torch.uint8), ptr(vox, torch.int32), ptr(items, torch.int64), n, int(max_count),
                                            ptr(lut, torch.int64), codes.shape[1], B, ptr(out), stream()))
    return out


def semseg_accumulate(acc, clip_logits, frame_index):
    """acc [F,C,H,W] (zero-initialised) += clip_logits [C,T,H,W] at the clip's frames (host list of T distinct ints)."""
    require_gpu()
    Cn, T, H, W = clip_logits.shape
    assert acc.is_contiguous() and clip_logits.is_contiguous() and tuple(acc.shape[1:]) == (Cn, H, W)
    idx = (C.c_int32 * T)(*[int(t) for t in frame_index])
    check(lib().stemseg_hip_semseg_accumulate(ptr(acc, torch.float32), ptr(clip_logits, torch.float32), Cn, T, H * W, idx, acc.shape[0], stream()))


def semseg_masks(acc, counts, output_type="probs"):
    """acc [F,C,H,W], counts float32 [F] (device) -> (fg [F,H,W] float32, multiclass | None); inference_model.py:197-231."""
    require_gpu()
    Fn, Cn, H, W = acc.shape
    code = SEMSEG_OUTPUT_TYPES[output_type]
    fg = torch.empty(Fn, H, W, dtype=torch.float32, device=acc.device)
    mc = None
    if Cn > 2 and code == 3:
        mc = torch.empty(Fn, H, W, dtype=torch.int64, device=acc.device)
    elif Cn > 2 and code in (1, 2):
        mc = torch.empty(Fn, Cn - 1, H, W, dtype=torch.float32, device=acc.device)
    check(lib().stemseg_hip_semseg_masks(ptr(acc, torch.float32), ptr(counts, torch.float32), Fn, Cn, H * W, code, ptr(fg), ptr(mc) if mc is not None else None, stream()))
    return fg, mc


def semseg_fg_clip(clip_logits, thr=0.5, want_prob=False):
    """One independent clip: logits [C,T,H,W] -> (fg mask uint8 [T,H,W], fg probability float [T,H,W] | None)."""
    require_gpu()
    Cn, T, H, W = clip_logits.shape
    mask = torch.empty(T, H, W, dtype=torch.uint8, device=clip_logits.device)
    prob = torch.empty(T, H, W, dtype=torch.float32, device=clip_logits.device) if want_prob else None
    check(lib().stemseg_hip_semseg_fg_clip(ptr(clip_logits, torch.float32), Cn, T, H * W, float(thr), ptr(prob), ptr(mask), stream()))
    return mask, prob


def scatter_instance_index(ys, xs, labels, lut, H, W):
    """dense uint8 [H,W]: lut[label + 1] at the (ys, xs) of the frame's foreground points, 0 elsewhere (davis.py:76-77)."""
    require_gpu()
    dense = torch.empty(H, W, dtype=torch.uint8, device=lut.device)
    n = labels.numel()
    check(lib().stemseg_hip_scatter_instance_index(ptr(ys, torch.int64) if n else None, ptr(xs, torch.int64) if n else None,
                                                   ptr(labels, torch.int64) if n else None, n, ptr(lut, torch.int32), lut.numel(),
                                                   ptr(dense), H, W, stream()))
    return dense


def resample_instance_masks(dense, mask_scale, crop_hw, out_hw):
    """dense uint8 [h,w] -> condensed uint8 [out_h,out_w] through x mask_scale, crop, resize, > 0.5 (davis.py:79-110)."""
    require_gpu()
    h, w = dense.shape
    out = torch.empty(out_hw[0], out_hw[1], dtype=torch.uint8, device=dense.device)
    check(lib().stemseg_hip_resample_instance_masks(ptr(dense, torch.uint8), h, w, float(mask_scale), int(crop_hw[0]), int(crop_hw[1]),
                                                    int(out_hw[0]), int(out_hw[1]), ptr(out), stream()))
    return out


def preprocess_frames(frames_u8, new_hw, pad_hw, mean, std, unit_scale=False, flip_channels=False, invalid=None):
    """uint8 [T,H0,W0,3] (device) -> float32 [T,3,pad_h,pad_w]: resize, normalise, pad in one launch.  invalid: uint8 [T,H0,W0]
    (``warp_clip``'s): the resize of normalise(pixel) * (1 - invalid) instead, the same bits wherever the four taps are valid."""
    require_gpu()
    T, H0, W0, ch = frames_u8.shape
    assert ch == 3
    out = torch.empty(T, 3, pad_hw[0], pad_hw[1], dtype=torch.float32, device=frames_u8.device)
    m, s = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    if invalid is not None:
        assert tuple(invalid.shape) == (T, H0, W0), "invalid must be [T,H0,W0], got %s" % (tuple(invalid.shape),)
        check(lib().stemseg_hip_preprocess_frames_masked(ptr(frames_u8, torch.uint8), ptr(invalid, torch.uint8), T, H0, W0, int(new_hw[0]), int(new_hw[1]),
                                                         int(pad_hw[0]), int(pad_hw[1]), m, s, int(bool(unit_scale)), int(bool(flip_channels)), ptr(out),
                                                         stream()))
        return out
    check(lib().stemseg_hip_preprocess_frames(ptr(frames_u8, torch.uint8), T, H0, W0, int(new_hw[0]), int(new_hw[1]), int(pad_hw[0]), int(pad_hw[1]),
                                              m, s, int(bool(unit_scale)), int(bool(flip_channels)), ptr(out), stream()))
    return out


INDEX_DTYPES = {1: torch.uint8, 2: torch.int16}        # (torch has no uint16 arithmetic everywhere: the 16-bit map travels as int16 bits)


def index_bytes_for(n_instances):
    """1 while the kept-instance indices fit uint8 (<= 255), else 2 (<= 65534)."""
    assert n_instances <= 65534, "at most 65534 kept instances"
    return 1 if n_instances <= 255 else 2


def scatter_instance_index_ex(ys, xs, labels, lut, H, W, index_bytes):
    """``scatter_instance_index`` onto a uint8 (index_bytes 1) or 16-bit (2, stored as int16 bits) map."""
    require_gpu()
    dense = torch.empty(H, W, dtype=INDEX_DTYPES[index_bytes], device=lut.device)
    n = labels.numel()
    check(lib().stemseg_hip_scatter_instance_index_ex(ptr(ys, torch.int64) if n else None, ptr(xs, torch.int64) if n else None,
                                                      ptr(labels, torch.int64) if n else None, n, ptr(lut, torch.int32), lut.numel(),
                                                      ptr(dense), int(index_bytes), H, W, stream()))
    return dense


def resample_instance_masks_ex(dense, mask_scale, crop_hw, out_hw, index_bytes):
    """``resample_instance_masks`` on a uint8 / 16-bit condensed map (same index type out)."""
    require_gpu()
    h, w = dense.shape
    out = torch.empty(out_hw[0], out_hw[1], dtype=INDEX_DTYPES[index_bytes], device=dense.device)
    check(lib().stemseg_hip_resample_instance_masks_ex(ptr(dense, INDEX_DTYPES[index_bytes]), int(index_bytes), h, w, float(mask_scale),
                                                       int(crop_hw[0]), int(crop_hw[1]), int(out_hw[0]), int(out_hw[1]), ptr(out), stream()))
    return out


class RleBatch(object):
    """Host copy of one ``rle_encode`` call: plane q = f * K + n - 1.  ``strings[q]`` is the pycocotools ``counts`` string."""

    def __init__(self, F, H, W, K, counts, count_offsets, chars, char_offsets, area, bbox):
        self.F, self.H, self.W, self.K = F, H, W, K
        self.counts, self.count_offsets, self.chars, self.char_offsets = counts, count_offsets, chars, char_offsets
        self.area, self.bbox = area, bbox
        blob = chars.tobytes().decode("ascii")
        self.strings = [blob[char_offsets[q]:char_offsets[q + 1]] for q in range(F * K)]

    def plane(self, f, n):
        return f * self.K + n - 1

    def plane_counts(self, f, n):
        q = self.plane(f, n)
        return self.counts[self.count_offsets[q]:self.count_offsets[q + 1]]


def rle_encode(maps, K, max_changes=None, with_counts=True, extra=None):
    """COCO RLE of the K instance planes of every frame of ``maps`` ([F,H,W] uint8 / int16-as-uint16 on the device) -> RleBatch.
    Two host syncs: the plan's totals, and the one copy of the results (a third only when ``max_changes`` was too small).
    ``extra``: device tensors to bring back in that same copy -> returns (RleBatch, [numpy arrays of the same shapes])."""
    require_gpu()
    assert maps.dim() == 3 and maps.dtype in (torch.uint8, torch.int16) and maps.is_contiguous()
    ib = 1 if maps.dtype == torch.uint8 else 2
    F, H, W = maps.shape
    dev = maps.device
    if max_changes is None:          # typical masks: a few boundaries per instance and column; the plan reports the real need
        max_changes = min(2 * F * H * W, max(1 << 16, 8 * F * W * min(K, 16)))
    for _ in range(2):
        ws_bytes = lib().stemseg_hip_rle_workspace_bytes(F, H, W, K, int(max_changes))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        plane_counts = torch.empty(F * K, dtype=torch.int32, device=dev)
        plane_chars = torch.empty(F * K, dtype=torch.int64, device=dev)
        totals = torch.empty(3, dtype=torch.int64, device=dev)
        check(lib().stemseg_hip_rle_plan(ptr(maps), ib, F, H, W, K, int(max_changes), ptr(ws), ws_bytes, ptr(plane_counts), ptr(plane_chars),
                                         ptr(totals), stream()))
        n_counts, n_chars, need = totals.tolist()
        if n_counts >= 0:
            break
        max_changes = need
    else:
        raise RuntimeError("rle_encode: the plan still overflows with max_changes=%d" % max_changes)
    counts = torch.empty(max(n_counts, 1), dtype=torch.int32, device=dev)
    chars = torch.empty(max(n_chars, 1), dtype=torch.uint8, device=dev)
    cofs = torch.empty(F * K + 1, dtype=torch.int64, device=dev)
    chofs = torch.empty(F * K + 1, dtype=torch.int64, device=dev)
    area = torch.empty(F * K, dtype=torch.int32, device=dev)
    bbox = torch.empty(F * K, 4, dtype=torch.int32, device=dev)
    check(lib().stemseg_hip_rle_encode(ptr(maps), ib, F, H, W, K, int(max_changes), ptr(ws), ws_bytes, ptr(counts), ptr(cofs), ptr(chars),
                                       ptr(chofs), ptr(area), ptr(bbox), stream()))
    # one D2H of everything (a single byte buffer: one copy, one sync)
    parts = [chars[:n_chars], chofs.view(torch.uint8), area.view(torch.uint8), bbox.view(torch.uint8).reshape(-1)]
    if with_counts:
        parts += [cofs.view(torch.uint8), counts[:n_counts].view(torch.uint8)]
    extra = list(extra or [])
    parts += [t.contiguous().reshape(-1).view(torch.uint8) for t in extra]
    host = torch.cat(parts).cpu().numpy()
    o = 0

    def take(nbytes, dtype):
        nonlocal o
        a = host[o:o + nbytes].view(dtype)
        o += nbytes
        return a
    ch = take(n_chars, "u1")
    chof = take(8 * (F * K + 1), "<i8")
    ar = take(4 * F * K, "<i4")
    bb = take(16 * F * K, "<i4").reshape(F * K, 4)
    cof, cn = (take(8 * (F * K + 1), "<i8"), take(4 * n_counts, "<i4")) if with_counts else (None, None)
    batch = RleBatch(F, H, W, K, cn, cof, ch, chof, ar, bb)
    if not extra:
        return batch
    np_types = {torch.int64: "<i8", torch.float64: "<f8", torch.int32: "<i4", torch.float32: "<f4"}
    return batch, [take(t.numel() * t.element_size(), np_types[t.dtype]).reshape(tuple(t.shape)) for t in extra]


def instance_class_stats(ys, xs, labels, frame_sizes, lut, K, hw, logits=None, argmax=None, n_votes=0):
    """Per-instance statistics of F frames in one call.  ys / xs / labels: the frames' points concatenated (device int64),
    frame_sizes: host list of the per-frame point counts.  Returns (points int64 [F,K], sums float64 [K,C-1] | None,
    votes int64 [K,n_votes] | None), all on the device."""
    require_gpu()
    F = len(frame_sizes)
    dev = lut.device
    offs = [0]
    for n in frame_sizes:
        offs.append(offs[-1] + int(n))
    frame_off = torch.tensor(offs, dtype=torch.int64).to(dev, non_blocking=True)
    h, w = hw
    n = offs[-1]
    points = torch.empty(F, K, dtype=torch.int64, device=dev)
    sums = partial = votes = None
    C = 0
    if logits is not None:
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.shape[0] == F and tuple(logits.shape[2:]) == (h, w)
        C = logits.shape[1]
        sums = torch.empty(K, C - 1, dtype=torch.float64, device=dev)
        partial = torch.empty(F, K, C - 1, dtype=torch.float64, device=dev)
    if argmax is not None:
        assert argmax.dtype == torch.int64 and argmax.is_contiguous() and argmax.shape[0] == F and tuple(argmax.shape[1:]) == (h, w)
        votes = torch.empty(K, n_votes, dtype=torch.int64, device=dev)
    check(lib().stemseg_hip_instance_class_stats(ptr(ys, torch.int64) if n else None, ptr(xs, torch.int64) if n else None,
                                                 ptr(labels, torch.int64) if n else None, ptr(frame_off), F, max([int(s) for s in frame_sizes] + [0]),
                                                 ptr(lut, torch.int32), lut.numel(), K, h, w, ptr(logits), C, ptr(partial), ptr(sums), ptr(argmax),
                                                 int(n_votes), ptr(points), ptr(votes), stream()))
    return points, sums, votes


def vis_composite(frames, index_map, colors):
    """The reference's overlay of every kept instance on BGR frames (``utils/vis.py`` overlay_mask_on_image per instance n of a
    condensed map): frames [F,H,W,3] uint8, index_map [F,H,W] uint8 / int16-as-uint16, colors [K+1,3] uint8 (row n = colour of
    instance n, in the palette's order) -> new frames [F,H,W,3] uint8, all on the device."""
    require_gpu()
    assert frames.dim() == 4 and frames.shape[3] == 3 and frames.dtype == torch.uint8
    assert index_map.dtype in (torch.uint8, torch.int16) and tuple(index_map.shape) == tuple(frames.shape[:3])
    assert colors.dim() == 2 and colors.shape[1] == 3 and colors.dtype == torch.uint8 and colors.shape[0] >= 1
    ib = 1 if index_map.dtype == torch.uint8 else 2
    F, H, W = index_map.shape
    out = torch.empty_like(frames)
    check(lib().stemseg_hip_vis_composite(ptr(frames), ptr(index_map), ib, F, H, W, ptr(colors), colors.shape[0] - 1, ptr(out), stream()))
    return out


def jpeg_encode(frames, quality=95):
    """Baseline JFIF files of BGR uint8 frames [F,H,W,3] on the device, byte-identical to PIL's (libjpeg-turbo) encode of the same
    frames as RGB at ``quality`` (4:2:0, standard tables; cv2.imwrite's defaults at 95).  Returns (data, offsets): one numpy uint8
    buffer with the F files back to back and int64 offsets [F+1].  Two host syncs: the plan's total size, and the one copy of
    the files and offsets."""
    require_gpu()
    assert frames.dim() == 4 and frames.shape[3] == 3 and frames.dtype == torch.uint8
    F, H, W = (int(v) for v in frames.shape[:3])
    dev = frames.device
    ws_bytes = lib().stemseg_hip_jpeg_workspace_bytes(F, H, W)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    sizes = torch.empty(F + 1, dtype=torch.int64, device=dev)
    check(lib().stemseg_hip_jpeg_plan(ptr(frames), F, H, W, int(quality), ptr(ws), ws_bytes, ptr(sizes), ptr(sizes[F:]), stream()))
    total = int(sizes[F])
    o = (total + 7) // 8 * 8
    out = torch.empty(o + 8 * (F + 1), dtype=torch.uint8, device=dev)
    offsets = out[o:].view(torch.int64)
    check(lib().stemseg_hip_jpeg_encode(F, H, W, int(quality), ptr(ws), ws_bytes, ptr(out), total, ptr(offsets), stream()))
    host = out.cpu().numpy()
    return host[:total], host[o:].view("<i8").copy()


JPEG_STATUS_CORRUPT, JPEG_STATUS_MULTI_ROUND, JPEG_STATUS_BACKSTOP, JPEG_STATUS_HOST = 1, 2, 4, 0x80


def _host_jpeg(data):
    """BGR uint8 of one file's bytes, exactly as ``InferenceModel.load_images`` reads a path (cv2, else PIL)."""
    import io
    import numpy as np
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        im = cv2.imdecode(np.frombuffer(data, np.uint8), cv2.IMREAD_COLOR)
        if im is None:
            raise ValueError("cv2 could not decode the image")
        return im
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


def jpeg_decode(files, device=None, sub_bits=0, max_rounds=0):
    """Decode JPEG files (paths or bytes) -> (frames uint8 [F,H,W,3] BGR on the device, status numpy uint8 [F]).  Every frame equals
    ``InferenceModel.load_images`` of the same file.  The device decodes the frames the marker parser classifies for it
    (utils/jpeg.py), one call per geometry; frames it flags as corrupt (status bit 0) and host-classified frames (status 0x80) are
    read by the host loader.  Status bits 1 / 2: the synchronisation took more than one round / the serial backstop decoded the frame.
    One host sync: the status read.  sub_bits / max_rounds: see stemseg_hip_jpeg_decode (0 = defaults)."""
    import numpy as np
    from .utils import jpeg as J
    require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    blobs = [f if isinstance(f, (bytes, bytearray, memoryview)) else J.read_file(f) for f in files]
    infos = [J.parse(b) for b in blobs]
    F = len(blobs)
    status = np.zeros(F, np.uint8)
    groups = {}
    for i, info in enumerate(infos):
        if info.device:
            groups.setdefault(info.geometry, []).append(i)
        else:
            status[i] = JPEG_STATUS_HOST
    dims = set((info.H, info.W) for info in infos if info.device)
    host = {}
    for i in np.flatnonzero(status == JPEG_STATUS_HOST):
        host[i] = _host_jpeg(blobs[i])
        dims.add(host[i].shape[:2])
    if len(dims) != 1:
        raise ValueError("jpeg_decode: the frames do not share one size: %s" % sorted(dims))
    H, W = dims.pop()
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    st_dev = torch.zeros(F, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for (gh, gw, sampling), idx in groups.items():
            segs = [blobs[i][infos[i].ecs_begin:infos[i].ecs_end] for i in idx]
            lens = np.array([len(s) for s in segs], np.int64)
            ends = np.cumsum(lens)
            offs = np.stack([ends - lens, ends], 1).astype(np.int64)
            n_int = sum(-(-J.mcu_count(infos[i]) // (infos[i].restart or J.mcu_count(infos[i]))) for i in idx)
            total = int(ends[-1])
            o_off = (total + 7) // 8 * 8
            o_tab = o_off + offs.nbytes
            stage = torch.empty(o_tab + len(idx) * J.BLOB_BYTES, dtype=torch.uint8, pin_memory=True)
            sv = stage.numpy()
            sv[:total] = np.frombuffer(b"".join(segs), np.uint8)
            sv[o_off:o_tab] = offs.reshape(-1).view(np.uint8)
            sv[o_tab:] = np.concatenate([J.table_blob(infos[i]) for i in idx])
            buf = stage.to(dev, non_blocking=True)
            n = len(idx)
            ws_bytes = lib().stemseg_hip_jpeg_decode_workspace_bytes(n, gh, gw, sampling, total, n_int, int(sub_bits))
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            dst = out if len(idx) == F else torch.empty((n, gh, gw, 3), dtype=torch.uint8, device=dev)
            gst = torch.empty(n, dtype=torch.uint8, device=dev)
            check(lib().stemseg_hip_jpeg_decode(ptr(buf), ptr(buf[o_off:o_tab]), ptr(buf[o_tab:]), n, gh, gw, sampling, total, n_int,
                                                int(sub_bits), int(max_rounds), ptr(ws), ws_bytes, ptr(dst), ptr(gst), stream()))
            ii = torch.as_tensor(idx, device=dev)
            if dst is not out:
                out.index_copy_(0, ii, dst)
            st_dev.index_copy_(0, ii, gst)
        st = st_dev.cpu().numpy()
    status |= st
    for i in range(F):
        if status[i] & JPEG_STATUS_CORRUPT:
            host[i] = _host_jpeg(blobs[i])
    for i, im in host.items():
        out[i].copy_(torch.from_numpy(np.ascontiguousarray(im)))
    return out, status


PNG_STATUS_CORRUPT, PNG_STATUS_MULTI_ROUND, PNG_STATUS_BACKSTOP, PNG_STATUS_HOST = 1, 2, 4, 0x80
PNG_BATCH_BYTES = 1 << 29          # bound on the inflated bytes of one device call (the workspace is about 5x that)
# decode_frames: PNG frames go to the device from this many per call (profiles/png_decode_bench.json: at 1242x375 the device call
# costs 15.9 / 4.6 / 3.9 ms per frame at F = 1 / 8 / 16 against 4.6 ms for PIL on one host thread)
PNG_MIN_DEVICE_FRAMES = 8


def _host_png(data):
    """BGR uint8 of one PNG file's bytes, exactly as ``InferenceModel.load_images`` reads a path (cv2, else PIL)."""
    return _host_jpeg(data)


def png_decode(files, device=None, sub_bits=0, flags=0):
    """Decode PNG files (paths or bytes) -> (frames uint8 [F,H,W,3] BGR on the device, status numpy uint8 [F]).  Every frame equals
    ``InferenceModel.load_images`` of the same file.  The device decodes the frames the chunk walker classifies for it
    (utils/png.py), in calls of one geometry and at most PNG_BATCH_BYTES inflated bytes; frames it flags as corrupt (status bit 0)
    and host-classified frames (status 0x80) are read by the host loader.  Status bits 1 / 2: a block's synchronisation took more
    than one round / the serial backstop decoded a block of the frame.  One host sync: the status read.  sub_bits / flags: see
    stemseg_hip_png_decode (0 = defaults; flags 1 = no block finder, every block by the backstop)."""
    import numpy as np
    from .utils import png as P
    require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    blobs = [f if isinstance(f, (bytes, bytearray, memoryview)) else P.read_file(f) for f in files]
    infos = [P.parse(b) for b in blobs]
    F = len(blobs)
    status = np.zeros(F, np.uint8)
    groups = {}
    for i, info in enumerate(infos):
        if info.device:
            groups.setdefault(info.geometry, []).append(i)
        else:
            status[i] = PNG_STATUS_HOST
    dims = set((info.H, info.W) for info in infos if info.device)
    host = {}
    for i in np.flatnonzero(status == PNG_STATUS_HOST):
        host[i] = _host_png(blobs[i])
        dims.add(host[i].shape[:2])
    if len(dims) != 1:
        raise ValueError("png_decode: the frames do not share one size: %s" % sorted(dims))
    H, W = dims.pop()
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    st_dev = torch.zeros(F, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for (gh, gw, ch), members in groups.items():
            per_call = max(1, PNG_BATCH_BYTES // (gh * (1 + gw * ch)))
            for b in range(0, len(members), per_call):
                idx = members[b:b + per_call]
                n = len(idx)
                segs = [P.stream(infos[i], blobs[i]) for i in idx]
                lens = np.array([len(x) for x in segs], np.int64)
                offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                total = int(offs[-1])
                hdr, recs = P.header_blob([infos[i] for i in idx])
                o_off = (total + 8 + 7) // 8 * 8                  # 8 zero bytes after the streams
                o_hdr = o_off + offs.nbytes
                stage = torch.zeros(o_hdr + hdr.nbytes + recs.nbytes, dtype=torch.uint8, pin_memory=True)
                sv = stage.numpy()
                sv[:total] = np.frombuffer(b"".join(segs), np.uint8)
                sv[o_off:o_hdr] = offs.view(np.uint8)
                sv[o_hdr:o_hdr + hdr.nbytes] = hdr.reshape(-1).view(np.uint8)
                sv[o_hdr + hdr.nbytes:] = recs.reshape(-1).view(np.uint8)
                buf = stage.to(dev, non_blocking=True)
                ws_bytes = lib().stemseg_hip_png_decode_workspace_bytes(n, gh, gw, ch, total, int(sub_bits), int(flags))
                ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
                dst = out if n == F else torch.empty((n, gh, gw, 3), dtype=torch.uint8, device=dev)
                gst = torch.empty(n, dtype=torch.uint8, device=dev)
                check(lib().stemseg_hip_png_decode(ptr(buf), ptr(buf[o_off:o_hdr]), ptr(buf[o_hdr:]), n, gh, gw, ch, total, int(sub_bits), int(flags),
                                                   ptr(ws), ws_bytes, ptr(dst), ptr(gst), stream()))
                ii = torch.as_tensor(idx, device=dev)
                if dst is not out:
                    out.index_copy_(0, ii, dst)
                st_dev.index_copy_(0, ii, gst)
        st = st_dev.cpu().numpy()
    status |= st
    for i in range(F):
        if status[i] & PNG_STATUS_CORRUPT:
            host[i] = _host_png(blobs[i])
    for i, im in host.items():
        out[i].copy_(torch.from_numpy(np.ascontiguousarray(im)))
    return out, status


def decode_frames(files, device=None):
    """Decode image files (paths or bytes) of one size -> (frames uint8 [F,H,W,3] BGR on the device, status numpy uint8 [F]), each
    equal to ``InferenceModel.load_images`` of the file.  Sorted by magic bytes: JPEG files go to ``jpeg_decode``, PNG files to
    ``png_decode`` when the call holds at least PNG_MIN_DEVICE_FRAMES of them (below the break-even the host loader reads them),
    anything else to the host loader (status 0x80); a call may mix them.  Status bits are those of the decoder
    that took the frame."""
    import numpy as np
    from .utils import jpeg as J
    from .utils import png as P
    require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    blobs = [f if isinstance(f, (bytes, bytearray, memoryview)) else J.read_file(f) for f in files]
    kind = np.array([1 if bytes(b[:2]) == b"\xff\xd8" else 2 if P.is_png(b) else 0 for b in blobs])
    if (kind == 2).sum() < PNG_MIN_DEVICE_FRAMES:
        kind[kind == 2] = 0
    F = len(blobs)
    status = np.full(F, JPEG_STATUS_HOST, np.uint8)
    parts = {}
    for k, fn in ((1, jpeg_decode), (2, png_decode)):
        idx = np.flatnonzero(kind == k)
        if idx.size:
            parts[k] = (idx, fn([blobs[i] for i in idx], dev))
    host = {i: _host_jpeg(blobs[i]) for i in np.flatnonzero(kind == 0)}
    dims = set(tuple(fr.shape[1:3]) for _, (fr, _) in parts.values()) | set(im.shape[:2] for im in host.values())
    if len(dims) != 1:
        raise ValueError("decode_frames: the frames do not share one size: %s" % sorted(dims))
    if len(parts) == 1 and not host:
        return next(iter(parts.values()))[1]
    H, W = dims.pop()
    out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    for idx, (fr, st) in parts.values():
        out.index_copy_(0, torch.as_tensor(idx, device=dev), fr)
        status[idx] = st
    for i, im in host.items():
        out[i].copy_(torch.from_numpy(np.ascontiguousarray(im)))
    return out, status



# ------------------------------------------------------------------------------------------------ embedding loss
def embedding_loss_desc(embedding_size, free_dim_bandwidths, n_instances, T, H, W):
    """free_dim_bandwidths: 1 / std^2 per free dim, fp32 values (EmbeddingLoss computes them as the reference's buffer does)."""
    d = EmbeddingLossDesc()
    d.struct_bytes = C.sizeof(EmbeddingLossDesc)
    d.embedding_size, d.n_free_dims, d.n_instances = int(embedding_size), len(free_dim_bandwidths), int(n_instances)
    d.T, d.H, d.W = int(T), int(H), int(W)
    for i, v in enumerate(free_dim_bandwidths):
        d.free_dim_bandwidths[i] = float(v)
    return d


def _mask_bytes(m):
    """bool / uint8 masks as contiguous uint8 memory (a view for bool: same bytes)."""
    assert m.dtype in (torch.bool, torch.uint8), "masks must be bool or uint8, got %s" % m.dtype
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def embedding_loss_forward(desc, embedding_map, masks, ignore_masks):
    """One sample: embedding_map float32 [C,T,H,W], masks [I,T,H,W], ignore_masks [T,H,W] (bool / uint8, device).  -> (out float64 [4] on
    the device = lovasz sum, smoothness term, seediness terms, K; K and the number of kept pairs as ints; the workspace, which the
    backward call needs).  Synchronises once, for the two counts."""
    require_gpu()
    nbytes = lib().stemseg_hip_embedding_loss_workspace_bytes(C.byref(desc))
    if nbytes == 0:
        raise ValueError("embedding_loss: %s" % lib().stemseg_hip_last_error().decode())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=embedding_map.device)
    out = torch.empty(4, dtype=torch.float64, device=embedding_map.device)
    counts = (C.c_int32 * 2)()
    check(lib().stemseg_hip_embedding_loss_forward(C.byref(desc), ptr(embedding_map, torch.float32), ptr(_mask_bytes(masks)),
                                                   ptr(_mask_bytes(ignore_masks)), ptr(ws), nbytes, ptr(out), counts, stream()))
    return out, int(counts[0]), int(counts[1]), ws


def embedding_loss_backward(desc, embedding_map, masks, ignore_masks, ws, upstream, total_instances, batch_size, grad):
    """grad float32 [C,T,H,W] (a contiguous view of the batch's gradient) := the sample's gradient; upstream float32 [3] on the device."""
    check(lib().stemseg_hip_embedding_loss_backward(C.byref(desc), ptr(embedding_map, torch.float32), ptr(_mask_bytes(masks)),
                                                    ptr(_mask_bytes(ignore_masks)), ptr(ws), ws.numel(), ptr(upstream, torch.float32),
                                                    int(total_instances), int(batch_size), ptr(grad, torch.float32), stream()))


# ------------------------------------------------------------------------------------------------ training targets, semseg + foreground loss
MAX_SEMSEG_CLASSES = 128


def target_prep_desc(n_instances, T, H, W):
    d = TargetPrepDesc()
    d.struct_bytes = C.sizeof(TargetPrepDesc)
    d.n_instances, d.T, d.H, d.W = int(n_instances), int(T), int(H), int(W)
    return d


def prepare_targets(masks, ignore_masks, category_ids):
    """One sample: masks [I,T,H,W] and ignore_masks [T,H,W] (bool / uint8, device, full resolution), category_ids [I] (integer).
    -> (masks [I,T,H//4,W//4], ignore_masks [T,H//4,W//4], semseg_masks [T,H//4,W//4], all uint8; flag int32 [1] on the device, non-zero
    if a category id is outside 0..255).  No synchronisation: the caller reads the flag when it wants to."""
    require_gpu()
    assert masks.dim() == 4 and ignore_masks.dim() == 3 and tuple(masks.shape[1:]) == tuple(ignore_masks.shape), \
        "masks %s and ignore_masks %s do not match" % (tuple(masks.shape), tuple(ignore_masks.shape))
    I, T, H, W = masks.shape
    assert len(category_ids) == I, "Number of instances do not match: {}, {}".format(len(category_ids), I)
    dev = ignore_masks.device
    desc = target_prep_desc(I, T, H, W)
    cat = torch.as_tensor(category_ids).to(dev).long().clamp(-1, 256).to(torch.int32).contiguous()
    m_out = torch.empty((I, T, H // 4, W // 4), dtype=torch.uint8, device=dev)
    i_out = torch.empty((T, H // 4, W // 4), dtype=torch.uint8, device=dev)
    s_out = torch.empty((T, H // 4, W // 4), dtype=torch.uint8, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    rc = lib().stemseg_hip_prepare_targets(C.byref(desc), ptr(_mask_bytes(masks)) if I else None, ptr(_mask_bytes(ignore_masks)),
                                           ptr(cat) if I else None, ptr(m_out) if I else None, ptr(i_out), ptr(s_out), ptr(flag), stream())
    if rc == -1:
        raise ValueError("prepare_targets: %s" % lib().stemseg_hip_last_error().decode())
    check(rc)
    return m_out, i_out, s_out, flag


def semseg_loss_desc(n_classes, has_foreground_channel, T, H, W, strides):
    """strides: element strides (channel, t, y, x) of the sample's logits; the gradient is written with the same."""
    d = SemsegLossDesc()
    d.struct_bytes = C.sizeof(SemsegLossDesc)
    d.n_classes, d.has_foreground_channel = int(n_classes), int(bool(has_foreground_channel))
    d.T, d.H, d.W = int(T), int(H), int(W)
    d.stride_c, d.stride_t, d.stride_h, d.stride_w = (int(v) for v in strides)
    return d


def _base_ptr(t, dtype):
    """Address of a strided view's first element (``ptr`` asks for contiguity; these calls take the strides)."""
    assert t.is_cuda and t.dtype == dtype, "expected a %s device tensor, got %s on %s" % (dtype, t.dtype, t.device)
    assert t.device.index == torch.cuda.current_device(), "tensor on %s but the current device is cuda:%d" % (t.device, torch.cuda.current_device())
    return C.c_void_p(t.data_ptr())


def semseg_loss_forward(desc, logits, semseg_mask, ignore_mask):
    """One sample: logits float32, any strided [C,T,H,W] view whose strides ``desc`` names; semseg_mask uint8 [T,H,W] class ids,
    ignore_mask bool / uint8 [T,H,W].  -> (out float64 [4] on the device = ce sum, voxels, fg sum, non-ignored voxels; flag int32 [1] on
    the device, non-zero for a target id >= n_classes; the workspace, which the backward call needs).  No synchronisation."""
    require_gpu()
    nbytes = lib().stemseg_hip_semseg_loss_workspace_bytes(C.byref(desc))
    if nbytes == 0:
        raise ValueError("semseg_loss: %s" % lib().stemseg_hip_last_error().decode())
    dev = logits.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().stemseg_hip_semseg_loss_forward(C.byref(desc), _base_ptr(logits, torch.float32), ptr(semseg_mask, torch.uint8),
                                                ptr(_mask_bytes(ignore_mask)), ptr(ws), nbytes, ptr(out), ptr(flag), stream()))
    return out, flag, ws


def semseg_loss_backward(desc, logits, semseg_mask, ignore_mask, ws, upstream, batch_size, grad):
    """grad float32: a view with the strides of ``logits`` := the sample's gradient; upstream float32 [2] on the device (d / d mean
    cross-entropy over the batch, d / d mean foreground loss)."""
    check(lib().stemseg_hip_semseg_loss_backward(C.byref(desc), _base_ptr(logits, torch.float32), ptr(semseg_mask, torch.uint8),
                                                 ptr(_mask_bytes(ignore_mask)), ptr(ws), ws.numel(), ptr(upstream, torch.float32),
                                                 int(batch_size), _base_ptr(grad, torch.float32), stream()))


# ------------------------------------------------------------------------------------------------ optimiser step, gradient norm (csrc/optimizer.hip)
OPT_CHUNK = 16384              # STEMSEG_OPT_CHUNK: elements per chunk of the multi-tensor launches
OPT_STATE_UNINIT = 1           # STEMSEG_OPT_STATE_UNINIT: the tensor's momentum buffer holds nothing yet
OPT_NESTEROV = 1               # STEMSEG_OPT_NESTEROV


def opt_plan(entries, n_states):
    """entries: [(p, g, state1, state2, n, flags)] as integers (addresses; 0 = none) -> (OptTensor array, OptChunk array), both on the host:
    the descriptor table and its chunk table (include/stemseg_hip.h, the chunk rule).  Checks the descriptors; needs no GPU."""
    n = len(entries)
    tensors = (OptTensor * max(n, 1))()
    for d, (p, g, s1, s2, numel, flags) in zip(tensors, entries):
        d.p, d.g, d.state1, d.state2, d.n, d.flags, d.reserved = p or None, g or None, s1 or None, s2 or None, numel, flags, 0
    count = C.c_int64(0)
    check(lib().stemseg_hip_opt_plan(tensors, n, n_states, None, 0, C.byref(count)))
    chunks = (OptChunk * max(count.value, 1))()
    check(lib().stemseg_hip_opt_plan(tensors, n, n_states, chunks, count.value, C.byref(count)))
    return tensors, (OptChunk * count.value).from_buffer(chunks) if count.value else (OptChunk * 0)()


class OptTables(object):
    """The two tables of one parameter group on the device."""

    def __init__(self, entries, n_states, device):
        require_gpu()
        tensors, chunks = opt_plan(entries, n_states)
        self.n_tensors, self.n_chunks, self.device = len(entries), len(chunks), torch.device(device)
        up = lambda a: torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).pin_memory().to(self.device, non_blocking=True)
        self.tensors, self.chunks = up(tensors), (up(chunks) if self.n_chunks else None)


def opt_hyper(lr=0.0, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, beta1=0.9, beta2=0.999, eps=1e-8):
    """The hyper-parameters by value; the differences 1 - x are taken in Python floats and rounded to fp32 once, as torch's scalars are."""
    h = OptHyper()
    h.struct_bytes, h.flags = C.sizeof(OptHyper), OPT_NESTEROV if nesterov else 0
    h.lr, h.momentum, h.one_minus_dampening, h.weight_decay = lr, momentum, 1 - dampening, weight_decay
    h.one_minus_beta1, h.beta2, h.one_minus_beta2, h.eps = 1 - beta1, beta2, 1 - beta2, eps
    return h


def opt_sgd_step(tables, hyper, grad_scale=None):
    """One launch over the group; grad_scale: None or a device float32 [1] the kernel multiplies every gradient element by.  No synchronisation."""
    if tables.n_chunks:
        with torch.cuda.device(tables.device):
            check(lib().stemseg_hip_opt_sgd_step(ptr(tables.tensors), tables.n_tensors, ptr(tables.chunks), tables.n_chunks, C.byref(hyper),
                                                 ptr(grad_scale, torch.float32), stream()))


def opt_adam_step(tables, hyper, tensor_scalars, grad_scale=None):
    """tensor_scalars: device float32 [n_tensors, 2] = (lr / bias_correction1, sqrt(bias_correction2)) per tensor."""
    assert tuple(tensor_scalars.shape) == (tables.n_tensors, 2)
    if tables.n_chunks:
        with torch.cuda.device(tables.device):
            check(lib().stemseg_hip_opt_adam_step(ptr(tables.tensors), tables.n_tensors, ptr(tables.chunks), tables.n_chunks, C.byref(hyper),
                                                  ptr(tensor_scalars, torch.float32), ptr(grad_scale, torch.float32), stream()))


def opt_grad_norm(tables, max_norm=None):
    """-> (norm float64 [1], coef float32 [1], flag int32 [1]) on the device: the L2 norm over every gradient of the tables, min(1, max_norm /
    (norm + 1e-6)) (1 without a max_norm) and whether a gradient element is inf or NaN.  Two launches, no synchronisation."""
    dev = tables.device
    norm, coef, flag = (torch.empty(1, dtype=t, device=dev) for t in (torch.float64, torch.float32, torch.int32))
    if not tables.n_chunks:
        return norm.zero_(), coef.fill_(1.0), flag.zero_()
    part, pflag = torch.empty(tables.n_chunks, dtype=torch.float64, device=dev), torch.empty(tables.n_chunks, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().stemseg_hip_opt_grad_norm(ptr(tables.tensors), tables.n_tensors, ptr(tables.chunks), tables.n_chunks, ptr(part), ptr(pflag),
                                              -1.0 if max_norm is None else float(max_norm), ptr(norm), ptr(coef), ptr(flag), stream()))
    return norm, coef, flag


# ------------------------------------------------------------------------------------------------ gradient bucket (csrc/optimizer.hip)
OPT_MAX_WORLD = 64             # STEMSEG_OPT_MAX_WORLD


def opt_bucket_plan(sizes):
    """sizes: element counts in table order -> (offsets, total): the layout rule of include/stemseg_hip.h, each slice rounded up to 4
    elements.  Host only; needs no GPU."""
    n = len(sizes)
    tensors = (OptTensor * max(n, 1))()
    for d, numel in zip(tensors, sizes):
        d.n = numel
    offsets, total = (_I64 * max(n, 1))(), _I64(0)
    check(lib().stemseg_hip_opt_bucket_plan(tensors, n, offsets, C.byref(total)))
    return list(offsets[:n]), total.value


class BucketTables(object):
    """The tables of one pack or unpack launch on the device: descriptors (p := a destination or 0, g := a source or 0), the chunk
    table and the slice offsets.  entries: [(p, g, n)] as integers."""

    def __init__(self, entries, device):
        require_gpu()
        sizes = [n for _, _, n in entries]
        self.offsets_host, self.total = opt_bucket_plan(sizes)
        # (the chunk table is a function of the sizes alone: planned on a placeholder address, since a slice may have no source)
        _, chunks = opt_plan([(16, 16, 0, 0, n, 0) for n in sizes], 0)
        tensors = (OptTensor * len(entries))()
        for d, (p, g, n) in zip(tensors, entries):
            if p % 4 or g % 4 or n < 0:
                raise ValueError("BucketTables: a pointer that is not 4-byte aligned, or a negative size (p 0x%x, g 0x%x, n %d)" % (p, g, n))
            d.p, d.g, d.state1, d.state2, d.n, d.flags, d.reserved = p or None, g or None, None, None, n, 0, 0
        self.n_tensors, self.n_chunks, self.device = len(entries), len(chunks), torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        up = lambda a: torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).pin_memory().to(self.device, non_blocking=True)
        self.tensors, self.chunks = up(tensors), (up(chunks) if self.n_chunks else None)
        self.offsets = up((_I64 * len(entries))(*self.offsets_host))


def _bucket_args(tables, bucket):
    if bucket.numel() != tables.total or bucket.device != tables.device:
        raise ValueError("the bucket holds %d elements on %s, the plan's total is %d on %s" % (bucket.numel(), bucket.device, tables.total, tables.device))
    return (ptr(tables.tensors), tables.n_tensors, ptr(tables.chunks), tables.n_chunks, ptr(tables.offsets), ptr(bucket, torch.float32), tables.total)


def opt_pack_grads(tables, bucket, scale=1.0):
    """bucket float32 [tables.total] := every source of the tables times ``scale`` (1.0: the bits), zeros where there is none and in the
    padding.  One launch, no synchronisation."""
    if tables.n_chunks:
        with torch.cuda.device(tables.device):
            check(lib().stemseg_hip_opt_pack_grads(*(_bucket_args(tables, bucket) + (float(scale), stream()))))


def opt_unpack_grads(tables, bucket):
    """Every destination of the tables := its slice of the bucket.  One launch, no synchronisation."""
    if tables.n_chunks:
        with torch.cuda.device(tables.device):
            check(lib().stemseg_hip_opt_unpack_grads(*(_bucket_args(tables, bucket) + (stream(),))))


def opt_reduce_ranks(gathered, bucket):
    """gathered float32 [world, total] -> bucket float32 [total] := the mean over the ranks, summed in fp64 in rank order and rounded
    once.  One launch, no synchronisation."""
    if gathered.dim() != 2 or bucket.numel() != gathered.shape[1] or bucket.device != gathered.device:
        raise ValueError("opt_reduce_ranks: gathered %s on %s does not go with a bucket of %d elements on %s"
                         % (tuple(gathered.shape), gathered.device, bucket.numel(), bucket.device))
    world, total = gathered.shape
    if total:
        with torch.cuda.device(gathered.device):
            check(lib().stemseg_hip_opt_reduce_ranks(ptr(gathered, torch.float32), world, total, ptr(bucket, torch.float32), stream()))


# ------------------------------------------------------------------------------------------------ training data loader (csrc/data_loader.hip)
RLE_EMPTY, RLE_BAD_CHAR, RLE_OPEN_GROUP, RLE_BAD_COUNT, RLE_BAD_SUM = 1, 2, 4, 8, 16
RLE_STATUS_NAMES = {RLE_EMPTY: "the string is empty", RLE_BAD_CHAR: "a character outside 48..111", RLE_OPEN_GROUP: "the last group is left open",
                    RLE_BAD_COUNT: "a count is negative or too large", RLE_BAD_SUM: "the counts do not sum to height x width"}
MAX_UNION_RANGES = 64


def rle_pack(strings, plane_of_string):
    """Host side of ``rle_decode``: (chars uint8 [n], offsets int64 [M + 1], planes int32 [M]) as contiguous numpy arrays."""
    import numpy as np
    def encode(s):
        if not isinstance(s, str):
            return bytes(s)
        try:
            return s.encode("latin-1")
        except UnicodeEncodeError:          # beyond one byte: 0xFF, which is outside the alphabet, so the status names the character
            return bytes(min(ord(ch), 0xFF) for ch in s)
    blobs = [encode(s) for s in strings]
    offsets = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=offsets[1:])
    return np.frombuffer(b"".join(blobs), np.uint8), offsets, np.ascontiguousarray(plane_of_string, dtype=np.int32).reshape(-1)


def upload(array, device):
    """A numpy array through pinned memory to the device, without waiting for the copy (torch keeps the pinned block until the stream
    has passed it).  -> the device tensor, same dtype and shape."""
    stage = torch.empty(array.shape, dtype=torch.from_numpy(array[:0]).dtype, pin_memory=True)
    stage.numpy()[...] = array
    return stage.to(device, non_blocking=True)


def _check_refused(name, rc):
    """-1 (the library refuses the arguments) -> ValueError with its message; any other failure -> ``check``'s RuntimeError."""
    if rc == -1:
        raise ValueError("%s: %s" % (name, lib().stemseg_hip_last_error().decode()))
    check(rc)


def _check_plane_order(name, pidx):
    """``rle_decode_union`` and ``rle_decode_labels``: the plane indices must not decrease."""
    import numpy as np
    down = np.flatnonzero(np.diff(pidx) < 0)
    if down.size:
        at_m = int(down[0]) + 1
        raise ValueError("%s: the plane indices decrease at string %d (%d after %d): the strings of one plane must be contiguous"
                         % (name, at_m, pidx[at_m], pidx[at_m - 1]))


def _rle_stage(device, chars, offsets, tables):
    """The host arrays of an RLE call through ONE pinned buffer: offsets (int64) | the int32 tables | characters, every section 8-byte
    aligned.  -> (the device, the buffer -- to be kept until the call is made --, the sections' device addresses in that order, None
    for an empty section)."""
    import numpy as np
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    parts = [offsets] + list(tables) + [chars]
    starts = np.cumsum([0] + [(a.nbytes + 7) // 8 * 8 for a in parts])
    stage = np.zeros(starts[-1], np.uint8)
    for a, o in zip(parts, starts):
        stage[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    buf = upload(stage, dev)
    return dev, buf, [C.c_void_p(buf.data_ptr() + int(o)) if a.size else None for a, o in zip(parts, starts)]


def _rle_decode(name, strings, plane_of_string, P, H, W, device, planes):
    """``rle_decode`` and ``rle_decode_union``: the same staging and the same arguments, entry points ``stemseg_hip_<name>[_workspace_bytes]``."""
    chars, offsets, pidx = rle_pack(strings, plane_of_string)
    M, n = len(offsets) - 1, int(chars.size)
    assert pidx.size == M, "%s: %d strings, %d plane indices" % (name, M, pidx.size)
    if name == "rle_decode_union":
        _check_plane_order(name, pidx)
    require_gpu()
    nbytes = getattr(lib(), "stemseg_hip_%s_workspace_bytes" % name)(n, M, int(P))
    if nbytes == 0:
        raise ValueError("%s: %d characters in %d strings for %d planes: out of range" % (name, n, M, P))
    dev, buf, (d_offsets, d_pidx, d_chars) = _rle_stage(device, chars, offsets, [pidx])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if planes is None:
        planes = torch.empty((int(P), int(H), int(W)), dtype=torch.uint8, device=dev)
    assert tuple(planes.shape) == (int(P), int(H), int(W))
    status = torch.empty(max(M, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check_refused(name, getattr(lib(), "stemseg_hip_" + name)(
            d_chars, n, offsets.ctypes.data_as(C.c_void_p), pidx.ctypes.data_as(C.c_void_p) if M else None, d_offsets, d_pidx, M, int(P), int(H),
            int(W), ptr(ws), nbytes, ptr(planes, torch.uint8), ptr(status), stream()))
    return planes, status[:M]


def rle_decode(strings, plane_of_string, P, H, W, device=None, planes=None):
    """COCO RLE strings (str or bytes) -> (planes uint8 [P,H,W] on the device, status uint8 [M] on the device): string m is decoded
    into plane ``plane_of_string[m]``; planes that no string names are zero, and so is the plane of a string whose status is not 0
    (RLE_* bits).  The offsets, the plane indices and the characters go up in ONE pinned staging buffer, copied without waiting; the
    call does not synchronise: the caller reads the status when it wants to.  planes: an output buffer to fill."""
    return _rle_decode("rle_decode", strings, plane_of_string, P, H, W, device, planes)


def rle_decode_union(strings, plane_of_string, P, H, W, device=None, planes=None):
    """``rle_decode`` where a plane may be named by SEVERAL strings: plane p is the OR of the accepted strings that name it (a refused
    one contributes nothing and keeps its status), rasterised straight into the one plane -- no plane per string is ever stored.
    ``plane_of_string`` must not decrease (the strings of one plane are contiguous), else ValueError; M may exceed P.  Staging, return
    values and the absence of any wait are ``rle_decode``'s."""
    return _rle_decode("rle_decode_union", strings, plane_of_string, P, H, W, device, planes)


def rle_decode_labels(strings, plane_of_string, label_of_string, P, H, W, device=None, maps=None, overlap=None, status=None):
    """``rle_decode_union`` into LABEL MAPS: string m carries ``label_of_string[m]`` (1 .. 65535) -> (maps uint16 [P,H,W]: at a pixel the
    largest label among the accepted strings of the plane that are 1 there, else 0; overlap int32 [P]: the pixels of the plane that
    more than one accepted string covers; status uint8 [M]), all on the device.  ``plane_of_string`` must not decrease.  Staging (one
    pinned buffer, copied without waiting) and the absence of any wait are ``rle_decode``'s.  maps / overlap / status: output buffers to
    fill (the evaluator hands in views of the one buffer it reads back).  ValueError for what the library refuses."""
    import numpy as np
    chars, offsets, pidx = rle_pack(strings, plane_of_string)
    labels = np.ascontiguousarray(label_of_string, dtype=np.int64).reshape(-1)
    M, n = len(offsets) - 1, int(chars.size)
    if pidx.size != M or labels.size != M:
        raise ValueError("rle_decode_labels: %d strings, %d plane indices, %d labels" % (M, pidx.size, labels.size))
    if M and (labels.min() < 1 or labels.max() > 65535):
        at_m = int(np.flatnonzero((labels < 1) | (labels > 65535))[0])
        raise ValueError("rle_decode_labels: string %d has label %d, outside 1 .. 65535" % (at_m, labels[at_m]))
    labels = labels.astype(np.int32)
    _check_plane_order("rle_decode_labels", pidx)
    require_gpu()
    nbytes = lib().stemseg_hip_rle_decode_labels_workspace_bytes(n, M, int(P))
    if nbytes == 0:
        raise ValueError("rle_decode_labels: %d characters in %d strings for %d planes: out of range" % (n, M, P))
    dev, buf, (d_offsets, d_pidx, d_labels, d_chars) = _rle_stage(device, chars, offsets, [pidx, labels])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if maps is None:
        maps = torch.empty((int(P), int(H), int(W)), dtype=torch.uint16, device=dev)
    if overlap is None:
        overlap = torch.empty(int(P), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty(max(M, 1), dtype=torch.uint8, device=dev)
    if tuple(maps.shape) != (int(P), int(H), int(W)) or maps.dtype not in (torch.uint16, torch.int16):
        raise ValueError("rle_decode_labels: maps must be a 16-bit tensor of shape %s, not %s %s" % ((P, H, W), maps.dtype, tuple(maps.shape)))
    if overlap.dtype != torch.int32 or overlap.numel() != int(P) or status.dtype != torch.uint8 or status.numel() < M:
        raise ValueError("rle_decode_labels: overlap must be int32 [%d] and status uint8 [>= %d]" % (P, M))
    with torch.cuda.device(dev):
        _check_refused("rle_decode_labels", lib().stemseg_hip_rle_decode_labels(
            d_chars, n, offsets.ctypes.data_as(C.c_void_p), pidx.ctypes.data_as(C.c_void_p) if M else None,
            labels.ctypes.data_as(C.c_void_p) if M else None, d_offsets, d_pidx, d_labels, M, int(P), int(H), int(W), ptr(ws), nbytes, ptr(maps),
            ptr(overlap, torch.int32), ptr(status, torch.uint8), stream()))
    return maps, overlap, status[:M]


def rle_pair_inter_workspace_bytes(n_chars, M, n_pairs):
    """The workspace of ``rle_pair_inter`` in bytes: a function of the characters, the strings and the pairs alone (0: refused)."""
    return int(lib().stemseg_hip_rle_pair_inter_workspace_bytes(int(n_chars), int(M), int(n_pairs)))


def rle_pair_inter(strings, pairs, H, W, device=None, area=None, inter=None, status=None, workspace=None):
    """COCO RLE strings (str or bytes) of ONE H x W and ``pairs`` (int [n_pairs, 2], string indices; a pair may repeat or name one
    string twice) -> (area int32 [M]: the 1-pixels of each string, inter int32 [n_pairs]: the pixels that are 1 in both strings of the
    pair, status uint8 [M]: the RLE_* bits), all on the device.  A refused string has area 0 and its pairs inter 0.  The intersection
    is taken on the runs: no plane is made, and the workspace does not depend on H * W.  Staging (the offsets, the pairs and the
    characters in one pinned buffer, copied without waiting) and the absence of any wait are ``rle_decode``'s.  area / inter / status:
    output buffers to fill; when none is given they are views of ONE uint8 buffer (area | inter | status), so one read-back serves all
    three.  workspace: a uint8 device tensor of at least ``rle_pair_inter_workspace_bytes``.  ValueError for what the library refuses."""
    import numpy as np
    chars, offsets, _ = rle_pack(strings, [])
    pidx = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    M, n, K = len(offsets) - 1, int(chars.size), int(pidx.shape[0])
    if K and (pidx.min() < 0 or pidx.max() >= M):
        at_k = int(np.flatnonzero(((pidx < 0) | (pidx >= M)).any(axis=1))[0])
        raise ValueError("rle_pair_inter: pair %d names strings (%d, %d) of %d" % (at_k, pidx[at_k, 0], pidx[at_k, 1], M))
    pidx = pidx.astype(np.int32)
    require_gpu()
    nbytes = rle_pair_inter_workspace_bytes(n, M, K)
    if nbytes == 0:
        raise ValueError("rle_pair_inter: %d characters in %d strings with %d pairs: out of range" % (n, M, K))
    dev, buf, (d_offsets, d_pairs, d_chars) = _rle_stage(device, chars, offsets, [pidx])
    ws = workspace if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if area is None and inter is None and status is None:
        out = torch.empty(4 * (M + K) + max(M, 1), dtype=torch.uint8, device=dev)
        area, inter, status = out[:4 * M].view(torch.int32), out[4 * M:4 * (M + K)].view(torch.int32), out[4 * (M + K):]
    if area is None or inter is None or status is None:
        raise ValueError("rle_pair_inter: give all of area, inter and status, or none")
    if area.dtype != torch.int32 or area.numel() < M or inter.dtype != torch.int32 or inter.numel() < K or status.dtype != torch.uint8 or \
            status.numel() < M or ws.dtype != torch.uint8:
        raise ValueError("rle_pair_inter: area must be int32 [>= %d], inter int32 [>= %d], status uint8 [>= %d], the workspace uint8" % (M, K, M))
    with torch.cuda.device(dev):
        _check_refused("rle_pair_inter", lib().stemseg_hip_rle_pair_inter(
            d_chars, n, offsets.ctypes.data_as(C.c_void_p), pidx.ctypes.data_as(C.c_void_p) if K else None, d_offsets, d_pairs, M, K, int(H), int(W),
            ptr(ws), ws.numel(), ptr(area, torch.int32) if M else None, ptr(inter, torch.int32) if K else None,
            ptr(status, torch.uint8) if M else None, stream()))
    return area[:M], inter[:K], status[:M]


def resize_masks(planes, new_hw, pad_hw, ignore_from=None, flip_x=False):
    """planes uint8 [P,H0,W0] (device) -> uint8 [P + R, pad_h, pad_w]: bilinear to ``new_hw`` (torch's align_corners=False rule) > 0.5,
    zero padded.  ignore_from: R tuples (start, count, stride); output plane P + r is the resize of
    1 - any(planes[start + k * stride], k < count), taken before the resize."""
    import numpy as np
    require_gpu()
    P, H0, W0 = planes.shape
    ranges = np.ascontiguousarray(ignore_from if ignore_from is not None else [], dtype=np.int32).reshape(-1, 3)
    R = int(ranges.shape[0])
    out = torch.empty((P + R, int(pad_hw[0]), int(pad_hw[1])), dtype=torch.uint8, device=planes.device)
    rc = lib().stemseg_hip_resize_masks(ptr(planes, torch.uint8), P, H0, W0, int(new_hw[0]), int(new_hw[1]), int(pad_hw[0]), int(pad_hw[1]),
                                        ranges.ctypes.data_as(C.c_void_p) if R else None, R, int(bool(flip_x)), ptr(out), stream())
    _check_refused("resize_masks", rc)
    return out


# ------------------------------------------------------------------------------------------------ augmentation (csrc/augment.hip)
WARP_MAX_PLANES = 127
JITTER_ADD, JITTER_HUE_SAT = 1, 2
BLUR_MAX_K = 11
BLUR_MAX_FRAMES = 128


def warp_clip(src, planes, hinv, jitter=None):
    """src uint8 [H,W,3], planes uint8 [N,H,W] or None (device); hinv: F inverse homographies (output pixel -> source coordinate, [F,3,3]
    or [F,9], host); jitter: F tuples (add, hs, flags) or None -> (frames uint8 [F,H,W,3], out_planes uint8 [N,F,H,W], invalid uint8
    [F,H,W]) as include/stemseg_hip.h defines them.  The parameters go up in one pinned buffer, copied without waiting; one launch."""
    import numpy as np
    require_gpu()
    H, W, ch = src.shape
    assert ch == 3
    hm = np.ascontiguousarray(hinv, dtype=np.float64).reshape(-1, 9)
    F = int(hm.shape[0])
    jt = np.zeros((F, 3), np.int32) if jitter is None else np.ascontiguousarray(jitter, dtype=np.int32).reshape(-1, 3)
    assert jt.shape[0] == F, "warp_clip: %d homographies, %d jitter tuples" % (F, jt.shape[0])
    N = 0 if planes is None else int(planes.shape[0])
    if N:
        assert tuple(planes.shape[1:]) == (H, W), "warp_clip: planes %s for a %d x %d source" % (tuple(planes.shape), H, W)
    stage = np.zeros(hm.nbytes + jt.nbytes, np.uint8)
    stage[:hm.nbytes], stage[hm.nbytes:] = hm.reshape(-1).view(np.uint8), jt.reshape(-1).view(np.uint8)
    buf = upload(stage, src.device)
    frames = torch.empty((F, H, W, 3), dtype=torch.uint8, device=src.device)
    out_planes = torch.empty((N, F, H, W), dtype=torch.uint8, device=src.device)
    invalid = torch.empty((F, H, W), dtype=torch.uint8, device=src.device)
    _check_refused("warp_clip", lib().stemseg_hip_warp_clip(
        ptr(src, torch.uint8), ptr(planes, torch.uint8) if N else None, N, H, W, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + hm.nbytes), F,
        ptr(frames), ptr(out_planes) if N else None, ptr(invalid), stream()))
    return frames, out_planes, invalid


def motion_blur(frames, matrices):
    """frames uint8 [F,H,W,3] (device); matrices: per frame a k x k float array (k odd, <= BLUR_MAX_K) or None for a copy -> the blurred
    frames (a new tensor): correlation, reflect-101 border, floor(sum + 0.5).  One launch; ``frames`` itself if no frame has a matrix."""
    import numpy as np
    require_gpu()
    F, H, W, ch = frames.shape
    assert ch == 3 and len(matrices) == F
    if F > BLUR_MAX_FRAMES:
        raise ValueError("motion_blur: %d frames (at most %d per call)" % (F, BLUR_MAX_FRAMES))
    if all(m is None for m in matrices):
        return frames
    ks = np.zeros(F, np.int32)
    taps = np.zeros((F, BLUR_MAX_K * BLUR_MAX_K), np.float32)
    for f, m in enumerate(matrices):
        if m is None:
            continue
        m = np.asarray(m, np.float32)
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] > BLUR_MAX_K:
            raise ValueError("motion_blur: frame %d has a matrix of shape %s (square, at most %d x %d)" % (f, m.shape, BLUR_MAX_K, BLUR_MAX_K))
        ks[f] = m.shape[0]
        taps[f, :m.size] = m.reshape(-1)
    buf = upload(taps, frames.device)
    out = torch.empty_like(frames)
    _check_refused("motion_blur", lib().stemseg_hip_motion_blur(ptr(frames, torch.uint8), F, H, W, ks.ctypes.data_as(C.c_void_p), C.c_void_p(buf.data_ptr()),
                                                                ptr(out), stream()))
    return out


def duplicate_params(boxes, flip, shifts):
    """The int32 [T,8] table of ``duplicate_instance``: boxes: per frame (xmin, ymin, xmax, ymax) with exclusive maxima, or None;
    shifts: per frame (shift_x, shift_y), rounded to float32 as the reference's matrix is."""
    import numpy as np
    p = np.zeros((len(boxes), 8), np.int32)
    for t, (box, sh) in enumerate(zip(boxes, shifts)):
        if box is None:
            continue
        p[t, 0], p[t, 1:5], p[t, 5] = 1, [int(v) for v in box], int(bool(flip))
        p[t, 6:8] = np.asarray(sh, np.float32).view(np.int32)
    return p


def duplicate_instance(frames, mask, boxes, flip, shifts):
    """frames uint8 [T,H,W,3], mask uint8 [T,H,W] (device) -> (frames_out uint8 [T,H,W,3], masks_out uint8 [2,T,H,W]: the original
    instance without what the copy covers, and the copy), the reference's InstanceDuplicator applied with the host's decisions."""
    require_gpu()
    T, H, W, ch = frames.shape
    assert ch == 3 and tuple(mask.shape) == (T, H, W) and len(boxes) == T and len(shifts) == T
    buf = upload(duplicate_params(boxes, flip, shifts), frames.device)
    frames_out = torch.empty_like(frames)
    masks_out = torch.empty((2, T, H, W), dtype=torch.uint8, device=frames.device)
    _check_refused("duplicate_instance", lib().stemseg_hip_duplicate_instance(ptr(frames, torch.uint8), ptr(mask, torch.uint8), T, H, W,
                                                                              C.c_void_p(buf.data_ptr()), ptr(frames_out), ptr(masks_out), stream()))
    return frames_out, masks_out


# ------------------------------------------------------------------------------------------------ DAVIS evaluation (csrc/davis_eval.hip)
DAVIS_EVAL_TABLES = ("inter", "m_p", "m_g", "area_p", "n_p", "area_g", "n_g")


def davis_eval_index_bytes(pred):
    """1 or 2 for an index map tensor: uint8, or 16 bits (int16 carrying the bits, as the writers' maps do; uint16 where torch has it)."""
    if pred.dtype == torch.uint8:
        return 1
    if pred.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
        return 2
    raise ValueError("davis_eval_counts: the index map is %s, not uint8 or a 16-bit integer type" % pred.dtype)


def davis_eval_table_shapes(T, Kp, Kg):
    """The shapes of the seven tables, in the order they lie in the one buffer."""
    return [(T, Kp, Kg)] * 3 + [(T, Kp)] * 2 + [(T, Kg)] * 2


def davis_eval_counts(pred, gt_planes, Kp, r, counts=None):
    """pred: index map [T,H,W] on the device, uint8 or 16-bit (labels 1 .. Kp are proposals, everything else background); gt_planes uint8
    [Kg,T,H,W] on the device (what ``rle_decode`` yields; non-zero = member; planes may overlap); r: the dilation radius, 1 .. 32.
    -> the seven int32 tables of csrc/davis_eval.hip as device tensors, in the order of ``DAVIS_EVAL_TABLES``: inter, m_p, m_g [T,Kp,Kg],
    area_p, n_p [T,Kp], area_g, n_g [T,Kg] -- views of ONE buffer (``counts`` when given: an int32 vector of at least
    ``stemseg_hip_davis_eval_counts_size`` elements), so one copy reads them all back.  No synchronisation.  ValueError beyond the
    limits (Kp <= 64, Kg <= 32, 1 <= r <= 32, H * W < 2^31; the library names the one that is passed) and for shapes or dtypes that do
    not go together."""
    index_bytes = davis_eval_index_bytes(pred)
    if gt_planes.dtype != torch.uint8:
        raise ValueError("davis_eval_counts: the ground-truth planes are %s, not uint8" % gt_planes.dtype)
    if pred.dim() != 3 or gt_planes.dim() != 4 or tuple(gt_planes.shape[1:]) != tuple(pred.shape):
        raise ValueError("davis_eval_counts: the index map %s [T,H,W] and the planes %s [Kg,T,H,W] do not go together"
                         % (tuple(pred.shape), tuple(gt_planes.shape)))
    (T, H, W), Kg = (int(v) for v in pred.shape), int(gt_planes.shape[0])
    if pred.device != gt_planes.device:
        raise ValueError("davis_eval_counts: the index map is on %s, the planes on %s" % (pred.device, gt_planes.device))
    require_gpu()
    need = int(lib().stemseg_hip_davis_eval_counts_size(T, int(Kp), Kg))
    if need == 0:          # (arguments the size function refuses: the call below names the limit)
        need = 1
    if counts is None:
        counts = torch.empty(need, dtype=torch.int32, device=pred.device)
    if counts.dtype != torch.int32 or counts.dim() != 1 or counts.numel() < need or counts.device != pred.device:
        raise ValueError("davis_eval_counts: counts must be an int32 vector of at least %d elements on %s" % (need, pred.device))
    with torch.cuda.device(pred.device):
        rc = lib().stemseg_hip_davis_eval_counts(ptr(pred), index_bytes, ptr(gt_planes, torch.uint8), T, H, W, int(Kp), Kg, int(r),
                                                 ptr(counts, torch.int32), counts.numel(), stream())
    if rc == -1:
        raise ValueError("davis_eval_counts: %s" % lib().stemseg_hip_last_error().decode())
    check(rc)
    out, at = [], 0
    for shape in davis_eval_table_shapes(T, int(Kp), Kg):
        n = 1
        for v in shape:
            n *= v
        out.append(counts[at:at + n].view(shape))
        at += n
    return tuple(out)


# ------------------------------------------------------------------------------------------------ KITTI-MOTS evaluation (csrc/mots_eval.hip)
LABEL_PAIR_MAX_LABELS = 63


def _label_map_check(name, which, t):
    if t.dtype not in (torch.uint16, torch.int16):
        raise ValueError("%s: label map %s is %s, not a 16-bit integer type" % (name, which, t.dtype))


def label_pair_counts(a, b, Ka, Kb, counts=None):
    """a, b: label maps [T,H,W] on the device, 16-bit (uint16, or int16 carrying the bits; what ``rle_decode_labels`` yields) -> counts
    int32 [T, Ka + 1, Kb + 1] on the device: counts[t, i, j] = the pixels of frame t with a == i and b == j; a label above Ka (Kb) counts
    as 0, so every frame's table sums to H * W.  counts: an int32 vector of at least T * (Ka + 1) * (Kb + 1) elements to fill (a view
    of it is returned).  No synchronisation.  ValueError beyond the limits (Ka, Kb in 1 .. 63, H * W < 2^31; the library names the one
    that is passed) and for shapes or dtypes that do not go together."""
    _label_map_check("label_pair_counts", "a", a)
    _label_map_check("label_pair_counts", "b", b)
    if a.dim() != 3 or tuple(a.shape) != tuple(b.shape):
        raise ValueError("label_pair_counts: the label maps %s and %s [T,H,W] do not go together" % (tuple(a.shape), tuple(b.shape)))
    if a.device != b.device:
        raise ValueError("label_pair_counts: a is on %s, b on %s" % (a.device, b.device))
    T, H, W = (int(v) for v in a.shape)
    require_gpu()
    need = int(lib().stemseg_hip_label_pair_counts_size(T, int(Ka), int(Kb)))
    if need == 0:          # (arguments the size function refuses: the call below names the limit)
        need = 1
    if counts is None:
        counts = torch.empty(need, dtype=torch.int32, device=a.device)
    if counts.dtype != torch.int32 or counts.dim() != 1 or counts.numel() < need or counts.device != a.device:
        raise ValueError("label_pair_counts: counts must be an int32 vector of at least %d elements on %s" % (need, a.device))
    with torch.cuda.device(a.device):
        rc = lib().stemseg_hip_label_pair_counts(ptr(a), ptr(b), T, H, W, int(Ka), int(Kb), ptr(counts, torch.int32), counts.numel(), stream())
    if rc == -1:
        raise ValueError("label_pair_counts: %s" % lib().stemseg_hip_last_error().decode())
    check(rc)
    return counts[:need].view(T, int(Ka) + 1, int(Kb) + 1)
