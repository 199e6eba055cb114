"""ctypes binding of libivosw_hip.so — the only way the host classes reach the arithmetic.

No CPU fallback exists: ``lib()`` raises if the shared library is missing, and ``dptr`` rejects
non-CUDA tensors, so a product call without the HIP extension fails loudly.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libivosw_hip.so")

F32, BF16, F32X3 = 0, 1, 2
DQN_LOSS_MSE, DQN_LOSS_HUBER = 0, 1                  # IVOSW_DQN_LOSS_* (include/ivosw.h)
TARGET_SOFT, TARGET_PERIODIC = 1, 2                  # IVOSW_TARGET_*
OPT_ADAM, OPT_SGD = 0, 1                             # IVOSW_OPT_*
U8_HWC3, U8_CHW3 = 0, 1                              # IVOSW_U8_* (source layouts of ivosw_frames_pack_u8)
BRAIN_NPARAMS = 180993
ASSESS_NTENSORS = 326

_p, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
MAX_VIDEOS = 32                                      # IVOSW_MAX_VIDEOS
MAX_SEQS = 128                                       # IVOSW_MAX_SEQS
MAX_CANDIDATES = 16                                  # IVOSW_MAX_CANDIDATES
FRAMES_F32, FRAMES_RGBX8 = 0, 1                      # IVOSW_FRAMES_*
MAX_JF_VIDEOS = 32                                   # IVOSW_MAX_JF_VIDEOS
QA_AUG_MAX_CAND = 12                                 # IVOSW_QA_AUG_MAX_CAND
HEAD_FIT_MAX_FITS, HEAD_FIT_MAX_BATCH = 32, 256      # IVOSW_HEAD_FIT_MAX_*
METRIC_J, METRIC_F, METRIC_J_AND_F = 0, 1, 2         # IVOSW_METRIC_*
OUT_RGB8, OUT_RGBX8 = 0, 1                           # IVOSW_OUT_*
OVERLAY_DAVIS, OVERLAY_FADE, OVERLAY_CHECKER, OVERLAY_COLOR = 0, 1, 2, 3      # IVOSW_OVERLAY_*


class Video(C.Structure):
    """ivosw_video_t: one video of a multi-video assessment call (device pointers, mask strides in elements)."""
    _fields_ = [("frames", C.c_void_p), ("masks", C.c_void_p), ("mask_stride_frame", C.c_long), ("mask_stride_obj", C.c_long),
                ("frames_kind", C.c_int), ("n_frames", C.c_int), ("n_obj", C.c_int), ("H", C.c_int), ("W", C.c_int)]


class Labels(C.Structure):
    """ivosw_labels_t: the label map of one video of a *_lab call (device pointer, frame stride in elements); map = None: a float video."""
    _fields_ = [("map", C.c_void_p), ("stride_frame", C.c_long)]


class JfVideo(C.Structure):
    """ivosw_jf_video_t: one video of a multi-video J / F pass (device label maps, the label values to score, the F tolerance in pixels)."""
    _fields_ = [("gt", C.c_void_p), ("pred", C.c_void_p), ("n_frames", C.c_int), ("H", C.c_int), ("W", C.c_int), ("n_obj", C.c_int),
                ("obj_ids", C.c_uint8 * 32), ("bound_pix", C.c_int)]


class QaVideo(C.Structure):
    """ivosw_qa_video_t: one video of ivosw_qa_counts_videos (device label map and byte planes [O,N,H,W], the plane threshold)."""
    _fields_ = [("gt", C.c_void_p), ("planes", C.c_void_p), ("n_frames", C.c_int), ("H", C.c_int), ("W", C.c_int), ("n_obj", C.c_int),
                ("obj_ids", C.c_uint8 * 32), ("bound_pix", C.c_int), ("thr", C.c_uint8)]


class AugVideo(C.Structure):
    """ivosw_qa_aug_video_t: one source video of ivosw_qa_augment (device frames, label map and byte planes [O,N,H,W])."""
    _fields_ = [("frames", C.c_void_p), ("gt", C.c_void_p), ("planes", C.c_void_p), ("frames_kind", C.c_int), ("n_frames", C.c_int),
                ("H", C.c_int), ("W", C.c_int), ("n_obj", C.c_int), ("obj_ids", C.c_uint8 * 32)]


class AugSample(C.Structure):
    """ivosw_qa_aug_sample_t: one sample of ivosw_qa_augment (host row: source unit, candidate and post inverse maps, noise, contrast)."""
    _fields_ = [("v", C.c_int), ("f", C.c_int), ("o", C.c_int), ("n_cand", C.c_int), ("cand", C.c_float * 6 * 12), ("post", C.c_float * 6),
                ("noise", C.c_float), ("contrast", C.c_float)]


class Overlay(C.Structure):
    """ivosw_overlay_t: how ivosw_overlay_frames draws (host struct, read during the call)."""
    _fields_ = [("style", C.c_int), ("n_objects", C.c_int), ("select", C.c_int), ("alpha", C.c_double), ("palette", C.c_uint8 * 3 * 32),
                ("color", C.c_uint8 * 3)]


SIGNATURES = {
    "ivosw_last_error": (C.c_char_p, []),
    "ivosw_version": (_i, []),
    "ivosw_brain_ws_bytes": (_sz, [_i, _i]),
    "ivosw_brain_forward": (_i, [_p, _p, _i, _i, _p, _p, _sz, _p]),
    "ivosw_brain_argmax": (_i, [_p, _i, _i, _p, _p]),
    "ivosw_brain_ragged_rows": (C.c_long, [_p, _i]),
    "ivosw_brain_ragged_ws_bytes": (_sz, [C.c_long]),
    "ivosw_brain_forward_ragged": (_i, [_p, _p, _p, _i, _p, _p, _sz, _p]),
    "ivosw_brain_argmax_ragged": (_i, [_p, _p, _i, _p, _p]),
    "ivosw_brain_topk_ragged": (_i, [_p, _p, _p, _i, _i, _i, _p, _p, _p]),
    "ivosw_brain_topk_spread_ragged": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "ivosw_dqn_ws_bytes": (_sz, [_i, _i]),
    "ivosw_dqn_loss_grad": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _f, _p, _p, _p, _sz, _p]),
    "ivosw_dqn_loss_grad_ex": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _f, _i, _f, _p, _p, _p, _sz, _p]),
    "ivosw_clamp_adam": (_i, [_p, _p, _p, _p, _i, _i, _f, _f, _f, _f, _f, _f, _f, _p]),
    "ivosw_adam_state_bytes": (_sz, []),
    "ivosw_clamp_adam_dev": (_i, [_p, _p, _p, _p, _i, _p, _f, _f, _f, _f, _f, _f, _f, _p]),
    "ivosw_clamp_sgd": (_i, [_p, _p, _p, _i, _f, _f, _f, _i, _f, _f, _p]),
    "ivosw_clamp_adam_dev_sched": (_i, [_p, _p, _p, _p, _i, _p, _p, _i, _f, _f, _f, _f, _f, _f, _p]),
    "ivosw_sgd_state_bytes": (_sz, []),
    "ivosw_clamp_sgd_dev_sched": (_i, [_p, _p, _p, _i, _p, _p, _i, _f, _f, _i, _f, _f, _p]),
    "ivosw_copy_f32": (_i, [_p, _p, _sz, _p]),
    "ivosw_target_state_bytes": (_sz, []),
    "ivosw_target_update": (_i, [_p, _p, _i, _i, _f, _i, _p, _p]),
    "ivosw_p2p_arena_bytes": (_sz, [_i, _sz]),
    "ivosw_p2p_handle_bytes": (_sz, []),
    "ivosw_p2p_alloc": (_i, [_sz, C.POINTER(_p), _p, _sz]),
    "ivosw_p2p_open": (_i, [_p, C.POINTER(_p)]),
    "ivosw_p2p_close": (_i, [_p]),
    "ivosw_p2p_free": (_i, [_p]),
    "ivosw_p2p_error": (_i, [_p, C.POINTER(_i)]),
    "ivosw_p2p_allreduce": (_i, [_p, _p, _i, _i, _i, C.POINTER(_p), C.c_uint, _i, _p]),
    "ivosw_p2p_allreduce_clamp_adam": (_i, [_p, _p, _i, _i, _i, C.POINTER(_p), C.c_uint, _i, _p, _p, _p, _i] + [_f] * 6 + [_p]),
    "ivosw_p2p_allreduce_clamp_sgd": (_i, [_p, _p, _i, _i, _i, C.POINTER(_p), C.c_uint, _i, _p, _p, _f, _f, _f, _i, _f, _p]),
    "ivosw_replay_gather": (_i, [_p] * 8 + [_i, _i] + [_p] * 5 + [_p]),
    "ivosw_replay_draw_state_bytes": (_sz, []),
    "ivosw_replay_draw_index": (C.c_ulonglong, [C.c_ulonglong, C.c_uint, C.c_uint, _i]),
    "ivosw_replay_draw_gather": (_i, [_p] * 8 + [_i, _i, _i] + [_p] * 6 + [_p]),
    "ivosw_dqn_loss_grad_per": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _f, _i, _f, _p, _p, _p, _p, _p, _sz, _p]),
    "ivosw_per_state_bytes": (_sz, []),
    "ivosw_per_tree_floats": (_sz, [_i]),
    "ivosw_per_build": (_i, [_p, _i, _p, _i, _p, _f, _p]),
    "ivosw_per_draw_gather": (_i, [_p] * 9 + [_i, _i, _i, _f, _i] + [_p] * 7 + [_p]),
    "ivosw_per_update": (_i, [_p, _i, _p, _p, _p, _i, _f, _f, _p]),
    "ivosw_dqn_step_drawn": (_i, [_p] * 10 + [_i, _i, _i, _f] + [_p] * 9 + [_sz] + [_p] * 3 + [_f] * 7 + [_p]),
    "ivosw_dqn_step_drawn_ex": (_i, [_p] * 10 + [_i, _i, _i, _f, _i, _f] + [_p] * 9 + [_sz] + [_p] * 3 + [_f] * 7 + [_p]),
    "ivosw_dqn_step_drawn_sgd": (_i, [_p] * 10 + [_i, _i, _i, _f, _i, _f] + [_p] * 9 + [_sz] + [_p, _f, _f, _f, _i, _f, _f] + [_p]),
    "ivosw_dqn_step_drawn_sched": (_i, [_p] * 10 + [_i, _i, _i, _f, _i, _f] + [_p] * 9 + [_sz] + [_p] * 3 + [_p, _i] + [_f] * 6 + [_p]),
    "ivosw_dqn_step_drawn_sgd_sched": (_i, [_p] * 10 + [_i, _i, _i, _f, _i, _f] + [_p] * 9 + [_sz] + [_p, _p, _p, _i, _f, _f, _i, _f, _f] + [_p]),
    "ivosw_dqn_step_drawn_tgt": (_i, [_p] * 10 + [_i, _i, _i, _f, _i, _f] + [_p] * 9 + [_sz] + [_i, _p, _p, _p, _f, _p, _i, _f, _f, _f, _f, _i, _f, _f, _f] +
                                 [_i, _f, _i, _p] + [_p]),
    "ivosw_mask_bbox": (_i, [_p, _i, _i, _i, _p, _p, _p]),
    "ivosw_roi_sample": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "ivosw_frames_pack_u8": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "ivosw_roi_sample_u8": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "ivosw_assess_packed_bytes": (_sz, [_i]),
    "ivosw_assess_pack": (_i, [_p, _i, C.POINTER(_p), _i, _p]),
    "ivosw_assess_ws_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "ivosw_assess_split": (_i, [_i, _i, _i]),
    "ivosw_assess_describe": (_i, [_i, _i, _i, _i, C.c_char_p, _sz]),
    "ivosw_assess_forward": (_i, [_p, _i, _p, _p, _i, _i, _i, _p, _p, _sz, _i, _i, _p, _p]),
    "ivosw_assess_forward_objects": (_i, [_p, _i, _p, _i, _p, C.c_long, C.c_long, _i, _i, _i, _p, _p, _sz, _i, _p]),
    "ivosw_assess_forward_u8": (_i, [_p, _i, _p, _p, _i, _i, _i, _p, _p, _sz, _i, _i, _p, _p]),
    "ivosw_assess_forward_objects_u8": (_i, [_p, _i, _p, _i, _p, C.c_long, C.c_long, _i, _i, _i, _p, _p, _sz, _i, _p]),
    "ivosw_assess_forward_features": (_i, [_p, _i, _p, _p, _i, _i, _i, _p, _p, _p, _sz, _i, _p]),
    "ivosw_assess_forward_features_u8": (_i, [_p, _i, _p, _p, _i, _i, _i, _p, _p, _p, _sz, _i, _p]),
    "ivosw_assess_videos_units": (C.c_long, [_p, _i]),
    "ivosw_mask_bbox_videos": (_i, [_p, _i, _p, _p, _p]),
    "ivosw_roi_sample_videos": (_i, [_p, _i, _p, _i, _p, _p]),
    "ivosw_assess_forward_videos": (_i, [_p, _i, _p, _i, _p, _p, _sz, _i, _i, _p, _p]),
    "ivosw_mask_delta_videos": (_i, [_p, _i, _p, _p, _p, _p, _p, _p]),
    "ivosw_mask_bbox_units": (_i, [_p, _i, _p, _i, _p, _p, _p]),
    "ivosw_roi_sample_units": (_i, [_p, _i, _p, _i, _p, _i, _p, _p]),
    "ivosw_assess_units_ws_bytes": (_sz, [_i, _i, _i]),
    "ivosw_assess_forward_units": (_i, [_p, _i, _p, _i, _p, _i, _p, _p, _sz, _i, _p]),
    # the *_lab twins: `labels` (a host array of Labels) right behind `videos`, nothing else
    "ivosw_mask_bbox_videos_lab": (_i, [_p, _p, _i, _p, _p, _p]),
    "ivosw_roi_sample_videos_lab": (_i, [_p, _p, _i, _p, _i, _p, _p]),
    "ivosw_assess_forward_videos_lab": (_i, [_p, _i, _p, _p, _i, _p, _p, _sz, _i, _i, _p, _p]),
    "ivosw_mask_delta_videos_lab": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _p]),
    "ivosw_mask_bbox_units_lab": (_i, [_p, _p, _i, _p, _i, _p, _p, _p]),
    "ivosw_roi_sample_units_lab": (_i, [_p, _p, _i, _p, _i, _p, _i, _p, _p]),
    "ivosw_assess_forward_units_lab": (_i, [_p, _i, _p, _p, _i, _p, _i, _p, _p, _sz, _i, _p]),
    "ivosw_quality_state": (_i, [_p, _i, _i, _p, _p, _p, _p]),
    "ivosw_quality_state_ragged": (_i, [_p, _p, _p, _i, _p, _p, _p, _p]),
    "ivosw_assess_dominant_kernel": (C.c_char_p, [_i]),
    "ivosw_jf_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "ivosw_jf_counts": (_i, [_p, _p, _i, _i, _i, C.c_char_p, _i, _i, _p, _p, _sz, _p]),
    "ivosw_jf_videos_ws_bytes": (_sz, [_p, _i]),
    "ivosw_jf_counts_videos": (_i, [_p, _i, _p, _p, _sz, _p]),
    "ivosw_jf_reduce_ragged": (_i, [_p, _p, _p, _i, _i, _p, _p, _p, _p, _p]),
    "ivosw_qa_quantize": (_i, [_p, _i, _i, _i, _i, C.c_long, C.c_long, _p, _p]),
    "ivosw_qa_counts_ws_bytes": (_sz, [_p, _i]),
    "ivosw_qa_counts_videos": (_i, [_p, _i, _p, _p, _sz, _p]),
    "ivosw_qa_targets": (_i, [_p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "ivosw_qa_augment_ws_bytes": (_sz, [_i]),
    "ivosw_qa_augment": (_i, [_p, _i, _p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "ivosw_head_fit": (_i, [_p, _p, _p, _i, _p, _p, _i, _i, _i, _p, _p, _p, _p] + [_p] * 8 + [_p]),
    "ivosw_seg_epilogue": (_i, [_p, _i, _i, _i, _i, _i, _i, _p, C.c_long, C.c_long, _p, _p, _p, _p]),
    "ivosw_atnet_epilogue": (_i, [_p, _p] + [_i] * 8 + [_f, _f, _f, _p, _p, C.c_long, _p, _p, _p]),
    "ivosw_ipn_dilate": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "ivosw_ipn_merge": (_i, [_p, _p, _i, _i, _i, _i, _p, _p, _p, _p, C.c_long, _p, _p, _p]),
    "ivosw_overlay_lane_pixels": (_i, [_p, _p, _i, _p, _i]),
    "ivosw_overlay_frames": (_i, [_p, _i, _p, _i, _i, _i, _p, _i, _p, _p, _i, _p]),
    "ivosw_scribble_raster_ws_bytes": (_sz, [_i, _i, _i]),
    "ivosw_scribble_raster": (_i, [_p, _i, _p, _p] + [_i] * 7 + [_p, _p, _p, _sz, _p]),
    "ivosw_rough_roi_ws_bytes": (_sz, [_i]),
    "ivosw_rough_roi": (_i, [_p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "ivosw_robot_skeleton_fits": (_i, [_i, _i]),
    "ivosw_robot_skeleton": (_i, [_p, _p, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p]),
    "ivosw_robot_box_workspace_bytes": (C.c_long, [_i, _i, _i]),
    "ivosw_robot_skeleton_box": (_i, [_p, _p, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "ivosw_robot_paths_max_cap": (_i, []),
    "ivosw_robot_paths": (_i, [_p, _p] + [_i] * 8 + [_p, _p, _p, _p]),
    "ivosw_graph_begin": (_i, [_p]),
    "ivosw_graph_end": (_i, [_p, C.POINTER(_p), C.POINTER(_i)]),
    "ivosw_graph_launch": (_i, [_p, _p]),
    "ivosw_graph_destroy": (_i, [_p]),
    "ivosw_profile_start": (_i, []),
    "ivosw_profile_span_start": (_i, []),
    "ivosw_profile_span_stop": (_i, [C.POINTER(C.c_double), C.POINTER(_i), C.POINTER(_i)]),
    "ivosw_profile_stop": (_i, [C.POINTER(C.c_double), C.POINTER(_i)]),
    "ivosw_profile_report": (_i, [C.c_char_p, _sz]),
    "ivosw_tune_set": (_i, [C.c_char_p, _i]),
    "ivosw_ablation_build": (_i, []),
    "ivosw_clock_probe": (_i, [_p, _i, _p]),
    "ivosw_assess_forget": (_i, [_p]),
}

# the tuning probes (include/ivosw_probe.h) live in a superset build of the same sources, libivosw_probe.so: never part of the product ABI
PROBE_LIB_PATH = os.path.join(_HERE, "libivosw_probe.so")
PROBE_SIGNATURES = {
    "ivosw_lstm_probe": (_i, [_p, _p]),
    "ivosw_bneck_probe": (_i, [_p] * 11 + [_i] * 5 + [_p, _p]),
    "ivosw_bneck_wide_probe": (_i, [_p] * 9 + [_i] * 5 + [_p, _p]),
    "ivosw_bneck_wide_stage_probe": (_i, [_p] * 5 + [_i] * 4 + [_p, _p]),
    "ivosw_res2_stage_probe": (_i, [_p] * 4 + [_i] * 2 + [_p, _p]),
    "ivosw_gemm_bt_probe": (_i, [_p] * 4 + [_i] * 4 + [_p, _p]),
    "ivosw_conv_probe": (_i, [_p] * 8 + [_i] * 15 + [C.POINTER(_i), _p]),
    "ivosw_stage_first_probe": (_i, [_p] * 9 + [_i] * 7 + [_p]),
    "ivosw_res2_probe": (_i, [_p] * 7 + [_i] * 4 + [C.POINTER(_i), _p]),      # w, bias: host arrays of RES2_PROBE_NW device pointers
    "ivosw_stem_probe": (_i, [_p] * 4 + [_i] * 2 + [_p]),
    "ivosw_robot_box_probe": (_i, [_p, _p, _i, _i, _i, _p, _i, _i, _p, _p, _p, _p, _p, _sz, _i, _p]),
    # the DQN step's backward kernels alone (tests/test_gpu_dqn_kernels.py)
    "ivosw_bwd_wgrad_probe": (_i, [_p] * 4 + [_i] * 7 + [C.POINTER(_i), _p]),
    "ivosw_bwd_dgrad_probe": (_i, [_p] * 7 + [_i, _p]),
    "ivosw_bwd_csum_probe": (_i, [_p] * 4 + [_i] * 4 + [_p]),
    "ivosw_bwd_group_probe": (_i, [_p] * 14 + [_i, _i, _p]),
    "ivosw_head_fused_probe": (_i, [_p, _i, _i] + [_p] * 6 + [_i, _i, _f, _i, _f] + [_p] * 9 + [_i, _p, _p, _p]),
    "ivosw_lstm_bwd_probe": (_i, [_p] * 6 + [_i] * 3 + [_p]),
    # the Brain forward kernels alone (tests/test_gpu_dqn_fwd_kernels.py); per-job arguments are host arrays (ctypes arrays of c_void_p / c_int)
    "ivosw_enc_fused_probe": (_i, [_i] + [_p] * 10),
    "ivosw_dec_fused_probe": (_i, [_i] + [_p] * 7),
    "ivosw_lstm_fwd_probe": (_i, [_p] * 6 + [_i] * 4 + [C.POINTER(_i), _p]),
    "ivosw_lstm_fwd_pair_probe": (_i, [_p] * 7 + [_i, _p, _p]),
    "ivosw_lstm_fwd_ragged_probe": (_i, [_p] * 4 + [_i, _p]),
    "ivosw_fwd_mega_probe": (_i, [_i] + [_p] * 9 + [_i, _p, _p, _p]),
}
BWD_GROUP_WS_FLOATS = (16 + 40 + 40) * 512 * 128 + 8 * 512  # IVOSW_BWD_GROUP_WS_FLOATS
RES2_PROBE_NW, RES2_PROBE_FRAG_BYTES = 11, 655360           # IVOSW_RES2_PROBE_NW, IVOSW_RES2_PROBE_FRAG_BYTES of include/ivosw_probe.h

_lib = None
_probe = None


def available():
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"ivos_w_amd: {LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc, gfx950). There is no CPU fallback for the hot path.")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("IVOSW_BRINGUP_PARTIAL") and not hasattr(h, name):
                continue                    # bring-up only: a partially built library
            fn = getattr(h, name)           # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = h
    return _lib


def probe_lib():
    """libivosw_probe.so: every entry of the product library plus the probes of include/ivosw_probe.h (tools/, one GPU test)."""
    global _probe
    if _probe is None:
        if not os.path.exists(PROBE_LIB_PATH):
            raise RuntimeError(f"ivos_w_amd: {PROBE_LIB_PATH} not found - build it with `python ivos-w_amd/build.py`")
        h = C.CDLL(PROBE_LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(PROBE_SIGNATURES.items()):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        _probe = h
    return _probe


def use_probe_lib():
    """Tuning tools: route EVERY library call of this process through the probe build (the probes steer state inside the library - stamp
    pointers, tunables - that the product entries called afterwards read).  Call before anything else touches the library."""
    global _lib
    if _lib is not None and _lib is not _probe:
        raise RuntimeError("use_probe_lib() must run before the first library call of the process")
    _lib = probe_lib()
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError(f"ivosw {what} failed ({rc}): {lib().ivosw_last_error().decode()}")


def tune_set(key, value):
    """ivosw_tune_set with its status checked: a switch that was silently not set would make an A/B test compare the default
    with itself."""
    if isinstance(key, str):
        key = key.encode()
    check(lib().ivosw_tune_set(key, int(value)), f"tune_set({key!r})")


def assess_describe(dtype, B, chunk=0, tap_stage=0):
    """ivosw_assess_describe: the tower launches of one forward pass as (slot, kernel, frames, direction) tuples, asked without a device."""
    buf = C.create_string_buffer(1 << 20)
    check(lib().ivosw_assess_describe(dtype, B, chunk, tap_stage, buf, len(buf)), "assess_describe")
    return [(int(s), k, int(n), int(d)) for s, k, n, d in (ln.split() for ln in buf.value.decode().splitlines())]


def dptr(t, dtype=None):
    """Raw device pointer of a contiguous CUDA tensor (raises for CPU tensors: no fallback)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("ivos_w_amd: the hot path runs on the MI355X only — got a non-CUDA tensor "
                           "(move inputs/modules to the GPU; there is no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def torch_ptr(t, elem_offset):
    """Raw device pointer of element ``elem_offset`` of a contiguous CUDA tensor (``dptr``'s checks)."""
    dptr(t)
    return C.c_void_p(t.data_ptr() + int(elem_offset) * t.element_size())


def int_array(values):
    """A host int array as the ragged entries take their lengths / n_obj (read during the call only)."""
    values = [int(v) for v in values]
    return (C.c_int * len(values))(*values)


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Workspace:
    """Grow-only byte workspace on one device (torch caching allocator owns the memory)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.buf


class Graph:
    """A captured launch sequence (ivosw_graph_*): ``with Graph.capture(device) as g: <ivosw calls via stream_ptr(device)>``
    records every library call made inside the block on a private stream into one HIP graph; ``g.launch()`` replays it on
    the caller's current stream.  No torch allocation may happen inside the block: hand in preallocated tensors."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.handle = None
        self.kernel_nodes = 0
        self._stream = None
        self._ctx = None

    @classmethod
    def capture(cls, device):
        return cls(device)

    def __enter__(self):
        self._stream = torch.cuda.Stream(self.device)
        self._stream.wait_stream(torch.cuda.current_stream(self.device))
        self._ctx = torch.cuda.stream(self._stream)
        self._ctx.__enter__()
        check(lib().ivosw_graph_begin(C.c_void_p(self._stream.cuda_stream)), "graph_begin")
        return self

    def __exit__(self, et, ev, tb):
        h, n = C.c_void_p(), C.c_int(0)
        rc = lib().ivosw_graph_end(C.c_void_p(self._stream.cuda_stream), C.byref(h), C.byref(n))
        self._ctx.__exit__(et, ev, tb)
        if et is None:
            check(rc, "graph_end")
            self.handle, self.kernel_nodes = h, n.value
        return False

    def launch(self):
        check(lib().ivosw_graph_launch(self.handle, stream_ptr(self.device)), "graph_launch")

    def __del__(self):
        if getattr(self, "handle", None):
            try:
                lib().ivosw_graph_destroy(self.handle)
            except Exception:
                pass
            self.handle = None
