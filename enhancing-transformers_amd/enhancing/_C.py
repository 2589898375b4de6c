"""ctypes binding of libenh_hip.so (the C ABI declared in include/enh_hip.h).

PyTorch tensors are used only as device-memory containers: every wrapper checks device / dtype /
contiguity (the reference's native ops do the same with CHECK_CUDA / CHECK_CONTIGUOUS,
enhancing/losses/op/fused_bias_act.cpp:9-15), passes raw ``data_ptr()`` values plus the current HIP
stream, and raises ``RuntimeError`` with ``enh_last_error()`` on a non-zero return code.

Timing labels (``KernelTimer``) of the GEMM and attention-forward calls are not worked out here: the library names the kernel it launched
(``enh_last_kernel()``), so the planner in csrc/gemm.hip has no second copy on this side.

There is NO fallback: if the shared library is missing or a tensor is not on a ROCm device the call
fails loudly.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("ENH_HIP_LIB", os.path.join(_PKG_ROOT, "lib", "libenh_hip.so"))

ACT_NONE, ACT_TANH, ACT_DTANH = 0, 1, 2
# Reductions across workgroups (LayerNorm dgamma / dbeta / fused bias sums, bias column sums, split-K weight gradients) run in their two-pass,
# fixed-order form by default: gradients are bit-reproducible from run to run (tests/test_parity_base_gpu.py).  ENH_DETERMINISTIC=0 selects the
# f32-atomic forms for A/B timing.
DETERMINISTIC = os.environ.get("ENH_DETERMINISTIC", "1") != "0"

_c = ctypes
_vp, _i64, _i32, _f32, _sz = _c.c_void_p, _c.c_int64, _c.c_int, _c.c_float, _c.c_size_t
_f64 = _c.c_double
_u64, _u32 = _c.c_uint64, _c.c_uint32

# name -> (restype, argtypes); must list every symbol include/enh_hip.h declares (checked by tests)
SIGNATURES = {
    "enh_last_error": (_c.c_char_p, []),
    "enh_last_kernel": (_c.c_char_p, []),
    "enh_abi_version": (_i32, []),
    "enh_vq_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "enh_vq_workspace_bytes_d": (_sz, [_i64, _i32, _i32, _i32]),
    "enh_vq_forward": (_i32, [_vp, _vp, _i64, _i32, _i32, _f32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "enh_vq_backward": (_i32, [_vp, _vp, _vp, _vp, _f32, _vp, _i64, _i32, _i32, _f32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "enh_vq_lookup": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "enh_gumbel_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "enh_gumbel_forward": (_i32, [_vp, _vp, _i64, _i32, _i32, _f32, _i32, _i32, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "enh_gumbel_backward": (_i32, [_vp, _vp, _vp, _vp, _vp, _f32, _vp, _i64, _i32, _i32, _f32, _i32, _vp, _i32, _u64, _u32, _vp, _vp, _vp, _sz, _vp]),
    "enh_gumbel_noise": (_i32, [_u64, _u32, _i64, _i32, _vp, _vp]),
    "enh_layernorm_forward": (_i32, [_vp, _vp, _vp, _i64, _i32, _f32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "enh_layernorm_backward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "enh_layernorm_backward_ws": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "enh_layernorm_backward_workspace_bytes": (_sz, [_i64, _i32]),
    "enh_gemm_h16": (_i32, [_vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i64, _vp, _i32, _vp, _i64, _vp, _i64, _i64,
                            _i32, _vp, _vp, _i64, _i32, _vp]),
    "enh_gemm_h16_ws": (_i32, [_vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i64, _vp, _i32, _vp, _i64, _vp, _i64, _i64,
                               _i32, _vp, _vp, _i64, _vp, _sz, _i32, _vp]),
    "enh_gemm_h16_workspace_bytes": (_sz, [_i32, _i32, _i64, _i64, _i64]),
    "enh_gemm_set_kernel": (_i32, [_i32]),
    "enh_gemm_set_scheduler": (_i32, [_i32]),
    "enh_set_cu_budget": (_i32, [_i32]),
    "enh_get_cu_budget": (_i32, []),
    "enh_debug_occupy_cus": (_i32, [_i32, _f32, _vp]),
    "enh_gemm_h16_variant": (_c.c_char_p, [_i32, _i32, _i64, _i64, _i64]),
    "enh_gemm_h16_variant_mode": (_c.c_char_p, [_i32, _i32, _i64, _i64, _i64, _i32]),
    "enh_gemm_h16_dtanh_colsum_workspace_bytes": (_c.c_size_t, [_i32, _i64, _i64, _i64]),
    "enh_gemm_h16_dtanh_colsum": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _c.c_size_t, _i32, _vp]),
    "enh_attention_set_kernel": (_i32, [_i32, _i32, _i32]),
    "enh_attention_forward": (_i32, [_vp, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _i32, _vp]),
    "enh_attention_backward": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _i32, _vp]),
    "enh_attention_forward_dh": (_i32, [_vp, _i32, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _i32, _vp]),
    "enh_attention_backward_dh": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _i32, _vp]),
    "enh_patchify": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_unpatchify_loss": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "enh_colsum_h16": (_i32, [_vp, _i64, _i64, _i64, _vp, _i32, _i32, _vp]),
    "enh_colsum_h16_ws": (_i32, [_vp, _i64, _i64, _i64, _vp, _i32, _vp, _sz, _i32, _vp]),
    "enh_colsum_h16_workspace_bytes": (_sz, [_i64, _i64]),
    "enh_cast_f32_h16": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "enh_cast_f32_h16_head_scaled": (_i32, [_vp, _vp, _i64, _i64, _f32, _i32, _vp]),
    "enh_cast_f32_h16_head_scaled_strided": (_i32, [_vp, _i64, _vp, _i64, _i64, _i64, _f32, _i32, _i32, _vp]),
    "enh_crop_flip_u8": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp]),
    "enh_resize_u8_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "enh_resize_u8": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _sz, _vp]),
    "enh_fused_bias_act": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _f32, _f32, _vp]),
    "enh_channel_sum_f32": (_i32, [_vp, _i32, _i32, _i64, _vp, _i32, _vp]),
    "enh_upfirdn2d": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "enh_im2col": (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "enh_col2im": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i64, _i32, _vp]),
    "enh_conv_nhwc_h16": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _f32, _f32, _vp, _i32, _vp]),
    "enh_conv_nhwc_h16_ws": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _sz, _i32, _vp]),
    "enh_conv_workspace_bytes": (_sz, [_vp]),
    "enh_conv_set_kernel": (_i32, [_i32]),
    "enh_conv_wgrad_workspace_bytes": (_sz, [_vp]),
    "enh_conv_wgrad_nhwc_h16": (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "enh_conv_pack_weight": (_i32, [_vp, _i32, _i32, _i32, _f32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_conv_unpack_wgrad": (_i32, [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp]),
    "enh_blur_set_kernel": (_i32, [_i32]),
    "enh_debug_gemm_lab": (_i32, [_i32]),
    "enh_debug_gemm_order": (_i32, [_i32, _i32]),
    "enh_debug_gemm_splits": (_i32, [_i32]),
    "enh_blur_nhwc_h16": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_lrelu_gate_h16": (_i32, [_vp, _vp, _i64, _f32, _f32, _vp, _i32, _vp]),
    "enh_img_to_nhwc8": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_nhwc8_to_img": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_minibatch_stddev_nhwc": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_minibatch_stddev_nhwc_backward": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_gemm_f32": (_i32, [_vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i64, _vp, _i32, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp]),
    "enh_attention_forward_f32": (_i32, [_vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "enh_attention_backward_f32": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "enh_attention_forward_f32_dh": (_i32, [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "enh_attention_backward_f32_dh": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "enh_colsum_f32": (_i32, [_vp, _i64, _i64, _i64, _vp, _i32, _vp]),
    "enh_patch_perm_f32": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "enh_unpatchify_loss_f32": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "enh_conv3x3_nhwc_h16": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp]),
    "enh_vgg_conv1": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_vgg_conv1_backward": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_maxpool2_nhwc_h16": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_maxpool2_nhwc_h16_backward": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_lpips_head": (_i32, [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _i32, _i32, _vp]),
    "enh_lpips_head_backward": (_i32, [_vp, _vp, _vp, _i32, _i64, _i32, _vp, _i32, _vp]),
    "enh_split3_bf16": (_i32, [_vp, _i64, _i64, _i64, _vp, _i32, _i32, _vp, _i64, _vp, _i64, _vp]),
    "enh_split2_bf16": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "enh_gemm_bf16_split_fused": (_i32, [_i64, _i64, _i64]),
    "enh_gemm_bf16_split": (_i32, [_vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "enh_layernorm_forward_x3": (_i32, [_vp, _vp, _vp, _i64, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "enh_attention_forward_x3": (_i32, [_vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "enh_adamw_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _f32, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _f32, _vp, _i32, _vp]),
    "enh_grad_clip_coef_workspace_bytes": (_sz, [_i64]),
    "enh_grad_clip_coef": (_i32, [_vp, _i64, _f32, _f32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "enh_adam_step_segments": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _f32, _f64, _f64, _f32, _f32, _vp, _vp, _vp, _f32, _i32, _vp]),
    "enh_adam_step_segments_s16": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _f32, _f64, _f64, _f32, _f32, _vp, _vp, _vp, _f32, _u64, _vp,
                                          _i32, _vp]),
    "enh_loss_scale_update": (_i32, [_vp, _vp, _vp, _f32, _f32, _i32, _vp]),
    "enh_nonfinite_flag": (_i32, [_vp, _i64, _vp, _vp]),
    "enh_skinny_gemm_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "enh_skinny_gemm_h16": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "enh_decode_attention_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "enh_decode_attention": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _sz, _i32, _vp]),
    "enh_row_ln_scale": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _i32, _vp]),
    "enh_gpt_embed": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp]),
    "enh_skinny_gemm_f32": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp]),
    "enh_mxfp8_quantize": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
    "enh_skinny_gemm_w8": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "enh_mxfp4_quantize": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
    "enh_skinny_gemm_w4_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "enh_skinny_gemm_w4": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "enh_mxfp6_quantize": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
    "enh_skinny_gemm_w6_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "enh_skinny_gemm_w6": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    "enh_causal_attention_forward": (_i32, [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _i32, _vp]),
    "enh_causal_attention_forward_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "enh_ln_timeshift": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _vp, _vp, _i32, _vp]),
    "enh_gpt_embed_seq": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "enh_relu_sq_h16": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "enh_cross_entropy_rows": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "enh_mean_f32": (_i32, [_vp, _i64, _vp, _vp]),
    "enh_rq_embed_seq": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "enh_ln_rows_strided": (_i32, [_vp, _vp, _vp, _i64, _i32, _f32, _vp, _i64, _vp]),
    "enh_short_causal_attention_forward": (_i32, [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _i32, _vp]),
    "enh_causal_attention_backward_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "enh_causal_attention_backward": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _sz, _i32, _vp]),
    "enh_cross_entropy_backward": (_i32, [_vp, _vp, _i64, _i32, _f32, _vp, _vp, _i32, _vp, _vp]),
    "enh_relu_sq_backward": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "enh_ln_timeshift_backward_workspace_bytes": (_sz, [_i64, _i32]),
    "enh_ln_timeshift_backward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _sz, _i32, _vp]),
    "enh_gpt_embed_seq_backward": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "enh_sample_logits": (_i32, [_vp, _i32, _i32, _f32, _i32, _f32, _vp, _u64, _u32, _u32, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    "enh_short_causal_attention_backward": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _i32, _vp]),
    "enh_ln_rows_strided_backward": (_i32, [_vp, _i64, _vp, _vp, _i64, _i32, _f32, _vp, _vp, _vp, _vp, _i32, _vp, _sz, _i32, _vp]),
    "enh_rq_embed_seq_backward": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "enh_rq_embed_step": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "enh_short_decode_attention": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "enh_cursor_advance": (_i32, [_vp, _vp]),
    "enh_decode_attention_at": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _sz, _i32, _vp]),
    "enh_decode_attention_kv8": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _sz, _i32, _vp]),
    "enh_decode_attention_kv8_at": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _sz, _i32, _vp]),
    "enh_kv_cache_fill": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "enh_kv_cache_fill_kv8": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "enh_embed_step_at": (_i32, [_vp, _vp, _i64, _i64, _i64, _i32, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "enh_sample_logits_at": (_i32, [_vp, _i32, _i32, _f32, _i32, _f32, _u64, _u32, _vp, _i32, _i32, _i32, _i64, _vp, _i64, _vp, _i64, _vp]),
}

_LIB = None
ABI_VERSION = 37 # ENH_ABI_VERSION of the include/enh_hip.h these signatures were written against


def lib():
    """Loads libenh_hip.so (once).  Raises if it has not been built: there is no CPU / eager fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                               f"(or `make -C enhancing-transformers_amd/csrc`). There is no fallback path.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here == ABI drift: fail loudly
            fn.restype, fn.argtypes = res, args
        if L.enh_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} reports ABI version {L.enh_abi_version()}, the bindings expect {ABI_VERSION}: rebuild the library")
        _LIB = L
        # kernel-family override for A/B measurements: explicit library state behind enh_gemm_set_kernel(); the environment is read HERE, in
        # the binding, never inside the library (reg = 0, pipe2 = 3, w256 = 7)
        sel = os.environ.get("ENH_GEMM_KERNEL")
        if sel:
            fam = {"reg": 0, "pipe2": 3, "w256": 7, "w256p": 8, "w256r": 9}.get(sel)
            if fam is None:
                raise RuntimeError(f"ENH_GEMM_KERNEL={sel!r}: expected reg | pipe2 | w256 | w256p | w256r")
            _check_rc = L.enh_gemm_set_kernel(fam)
            if _check_rc != 0:
                raise RuntimeError(L.enh_last_error().decode())
        sched = os.environ.get("ENH_GEMM_SCHEDULER")      # "static" | "dynamic" tile schedule of the persistent GEMMs (A/B)
        if sched:
            if sched not in ("static", "dynamic") or L.enh_gemm_set_scheduler(int(sched == "dynamic")) != 0:
                raise RuntimeError(f"ENH_GEMM_SCHEDULER={sched!r}: expected static | dynamic")
        att = os.environ.get("ENH_ATTN_KERNEL")       # "fwd,dq,dkv" families, e.g. "1,1,1" (0 = library default; include/enh_hip.h enh_attention_set_kernel)
        if att:
            f, q, k = (int(x) for x in att.split(","))
            if L.enh_attention_set_kernel(f, q, k) != 0:
                raise RuntimeError(L.enh_last_error().decode())
        conv = os.environ.get("ENH_CONV_KERNEL")      # A/B: "reg" register-staged everywhere | "t128" no 256-row kernels | "t256" 256-row wherever the shape allows
        if conv:
            if conv not in CONV_KERNELS or L.enh_conv_set_kernel(CONV_KERNELS[conv]) != 0:
                raise RuntimeError(f"ENH_CONV_KERNEL={conv!r}: expected one of {sorted(CONV_KERNELS)}")
    return _LIB


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {lib().enh_last_error().decode()}")


def _p(t: Optional[torch.Tensor], dtype: Optional[torch.dtype] = None, name: str = "tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be on a ROCm device (got {t.device}); the HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if dtype is not None and (t.dtype not in dtype if isinstance(dtype, tuple) else t.dtype != dtype):
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


F32, BF16, F16, I64, F64 = torch.float32, torch.bfloat16, torch.float16, torch.int64, torch.float64
H16 = (BF16, F16)      # the two 16-bit operand formats of the product path (include/enh_hip.h ENH_DT_BF16 / ENH_DT_F16)
DT_BF16, DT_F16, DT_F32 = 0, 1, 2


def _dt(*tensors) -> int:
    """the C ABI's dtype argument of a call, inferred from its 16-bit containers (torch.bfloat16 -> ENH_DT_BF16, torch.float16 -> ENH_DT_F16): all of one call's
    16-bit tensors must have the same format.  Calls without a 16-bit tensor pass the default (bf16)."""
    dts = {t.dtype for t in tensors if t is not None and t.dtype in H16}
    if len(dts) > 1:
        raise RuntimeError("the 16-bit operands of one call must all be bf16 or all be fp16")
    return DT_F16 if dts == {F16} else DT_BF16


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (torch's current stream is the stream every
    kernel of this library is enqueued on).  bench.py installs one to compute the roofline figures live."""

    def __init__(self) -> None:
        self.records = {}
        self.units = {}      # name -> "flop" (bf16 MFMA work), "flop_f32" (exact-f32 MFMA work) or "byte" (algorithmic HBM bytes)

    def run(self, name: Optional[str], work: float, fn, unit: str = "flop") -> None:
        """name=None: the label is the symbol of the kernel the library launched in fn() (enh_last_kernel), asked for outside the event pair"""
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        if name is None:
            name = lib().enh_last_kernel().decode()
        self.records.setdefault(name, []).append((s, e, work))
        self.units[name] = unit

    def summary(self) -> dict:
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            ms = [s.elapsed_time(e) for s, e, _ in recs]
            out[name] = dict(launches=len(recs), total_ms=sum(ms), avg_ms=sum(ms) / len(ms), work=sum(w for _, _, w in recs), unit=self.units[name])
        return out


TIMER: Optional[KernelTimer] = None


def _timed(name: Optional[str], work: float, fn, unit: str = "flop") -> None:
    if TIMER is None:
        fn()
    else:
        TIMER.run(name, work, fn, unit)

# ------------------------------------------------------------------------------------------------
# quantizer
# ------------------------------------------------------------------------------------------------
_WS = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 22), dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def vq_forward(z: torch.Tensor, codebook: torch.Tensor, beta: float, depth: int, use_norm: bool, want_bf16: bool = True, h16: torch.dtype = BF16):
    """z [M,d] f32, codebook [K,d] f32 (d % 8 == 0, 8 <= d <= 256) -> (zq f32 [M,d], zq 16-bit copy (format h16) | None, idx i64 [M,depth],
    loss f32 [1])."""
    _p(z, F32, "z"); _p(codebook, F32, "codebook")  # device / dtype / contiguity first: fail before allocating
    M, d = z.shape
    K = codebook.shape[0]
    zq = torch.empty_like(z)
    zq16 = torch.empty(M, d, dtype=h16, device=z.device) if want_bf16 else None
    idx = torch.empty(M, depth, dtype=I64, device=z.device)
    loss = torch.empty(1, dtype=F32, device=z.device)
    L = lib()
    nb = L.enh_vq_workspace_bytes_d(M, K, d, depth)
    ws = _workspace(nb, z.device)
    # work model: 2*K*d FLOP per token per depth on the exact-f32 MFMA (157.3 TF peak); the call = vq_prep + vq_nn + vq_loss_finalize
    _timed("vq_forward (vq_prep + vq_nn_kernel + vq_loss_finalize)", 2.0 * M * K * d * depth,
           lambda: _check(L.enh_vq_forward(_p(z, F32, "z"), _p(codebook, F32, "codebook"), M, K, d, beta, depth, int(use_norm), _p(zq), _p(zq16),
                                           _p(idx), _p(loss), _p(ws), ws.numel(), _dt(zq16), _stream()), "enh_vq_forward"), unit="flop_f32")
    return zq, zq16, idx, loss


def vq_backward(z, codebook, idx, g_out, g_loss: float, g_loss_dev: Optional[torch.Tensor], beta: float, depth: int,
                use_residual: bool, use_norm: bool, d_codebook: torch.Tensor, want_bf16: bool = True, h16: torch.dtype = BF16):
    """Returns (dz f32 [M,d], dz_bf16|None); ACCUMULATES into d_codebook [K,d] f32."""
    _p(z, F32, "z"); _p(codebook, F32, "codebook")
    M, d = z.shape
    K = codebook.shape[0]
    dz = torch.empty_like(z)
    dz16 = torch.empty(M, d, dtype=h16, device=z.device) if want_bf16 else None
    L = lib()
    nb = L.enh_vq_workspace_bytes_d(M, K, d, depth)
    ws = _workspace(nb, z.device)
    _check(L.enh_vq_backward(_p(z, F32, "z"), _p(codebook, F32, "codebook"), _p(idx, I64, "idx"), _p(g_out, F32, "g_out"),
                             float(g_loss), _p(g_loss_dev, F32, "g_loss_dev"), M, K, d, beta, depth, int(use_residual),
                             int(use_norm), _p(dz), _p(dz16), _p(d_codebook, F32, "d_codebook"), _p(ws), ws.numel(), _dt(dz16), _stream()),
           "enh_vq_backward")
    return dz, dz16


def vq_lookup(codebook, idx, use_norm: bool, want_bf16: bool = True, h16: torch.dtype = BF16):
    """idx [M,depth] i64, codebook [K,d] f32 -> (sum_i n(E[idx_i]) f32 [M,d], 16-bit copy)."""
    _p(idx, I64, "idx"); _p(codebook, F32, "codebook")
    M, depth = idx.shape
    K, d = codebook.shape
    out = torch.empty(M, d, dtype=F32, device=idx.device)
    out16 = torch.empty(M, d, dtype=h16, device=idx.device) if want_bf16 else None
    _check(lib().enh_vq_lookup(_p(codebook, F32, "codebook"), _p(idx, I64, "idx"), M, K, d, depth, int(use_norm), _p(out), _p(out16),
                               _dt(out16), _stream()), "enh_vq_lookup")
    return out, out16


def gumbel_forward(z: torch.Tensor, codebook: torch.Tensor, tau: float, hard: bool, use_norm: bool, seed: int, call: int):
    """one level of the fused Gumbel-softmax quantizer: z [M,d] f32, codebook [K,d] f32 (d % 8 == 0, 8 <= d <= 32) ->
    (z_q [M,d], soft z_q [M,d] (z_q itself unless hard), idx i64 [M], loss [1], stats [5,M] for gumbel_backward)."""
    _p(z, F32, "z"); _p(codebook, F32, "codebook")
    M, d = z.shape
    K = codebook.shape[0]
    zq = torch.empty_like(z)
    zq_soft = torch.empty_like(z) if hard else None
    idx = torch.empty(M, dtype=I64, device=z.device)
    loss = torch.empty(1, dtype=F32, device=z.device)
    stats = torch.empty(5, M, dtype=F32, device=z.device)
    L = lib()
    ws = _workspace(L.enh_gumbel_workspace_bytes(M, K, d), z.device)
    # work model: two M x K x 32 products (scores, y @ en) on the exact-f32 MFMA
    _timed("gumbel_forward (gumbel_prep + gumbel_fwd_kernel + gumbel_loss)", 4.0 * M * K * 32,
           lambda: _check(L.enh_gumbel_forward(_p(z), _p(codebook), M, K, d, float(tau), int(hard), int(use_norm), int(seed), int(call), _p(zq),
                                               _p(zq_soft), _p(idx), _p(loss), _p(stats), _p(ws), ws.numel(), _stream()), "enh_gumbel_forward"),
           unit="flop_f32")
    return zq, (zq_soft if hard else zq), idx, loss, stats


def gumbel_backward(z, codebook, zq_soft, stats, g_zq, g_loss: float, g_loss_dev: Optional[torch.Tensor], tau: float, hard: bool,
                    idx: Optional[torch.Tensor], use_norm: bool, seed: int, call: int, d_codebook: torch.Tensor):
    """Returns dz f32 [M,d]; ACCUMULATES into d_codebook [K,d] f32.  hard: the forward's mode, idx [M] i64 its indices (needed when hard)."""
    _p(z, F32, "z"); _p(codebook, F32, "codebook")
    M, d = z.shape
    K = codebook.shape[0]
    dz = torch.empty_like(z)
    L = lib()
    ws = _workspace(L.enh_gumbel_workspace_bytes(M, K, d), z.device)
    # work model: seven M x K x 32 products (dz: scores, dy, dl @ en; dE: scores, dy, dl^T zn, y^T g_zq) on the exact-f32 MFMA
    _timed("gumbel_backward (gumbel_prep + gumbel_bwd_dz + gumbel_bwd_de + gumbel_de_finalize)", 14.0 * M * K * 32,
           lambda: _check(L.enh_gumbel_backward(_p(z), _p(codebook), _p(zq_soft, F32, "zq_soft"), _p(stats, F32, "stats"), _p(g_zq, F32, "g_zq"), float(g_loss),
                                     _p(g_loss_dev, F32, "g_loss_dev"), M, K, d, float(tau), int(hard), _p(idx, I64, "idx"), int(use_norm), int(seed), int(call),
                                     _p(dz), _p(d_codebook, F32, "d_codebook"), _p(ws), ws.numel(), _stream()), "enh_gumbel_backward"),
           unit="flop_f32")
    return dz


def gumbel_noise(seed: int, call: int, M: int, K: int, device) -> torch.Tensor:
    """the [M,K] noise the fused Gumbel quantizer uses at (seed, call): out[m,k] = g(seed, call, m, k)"""
    out = torch.empty(M, K, dtype=F32, device=device)
    _check(lib().enh_gumbel_noise(int(seed), int(call), M, K, _p(out), _stream()), "enh_gumbel_noise")
    return out


# ------------------------------------------------------------------------------------------------
# layernorm
# ------------------------------------------------------------------------------------------------
def layernorm_forward(x, w, b, eps: float = 1e-5, y_bf16=None, y_f32=None, mean=None, rstd=None):
    M, D = x.shape
    _check(lib().enh_layernorm_forward(_p(x, F32, "x"), _p(w, F32, "w"), _p(b, F32, "b"), M, D, eps, _p(y_bf16, H16, "y_bf16"),
                                       _p(y_f32, F32, "y_f32"), _p(mean, F32, "mean"), _p(rstd, F32, "rstd"), _dt(y_bf16), _stream()),
           "enh_layernorm_forward")


def layernorm_backward(dy, x, w, mean, rstd, dres, dx_f32, dx_bf16, dw, db, dx_colsum=None):
    M, D = x.shape
    dy32, dy16 = (None, dy) if dy.dtype in H16 else (dy, None)   # upstream gradient: f32, or the dgrad GEMM's 16-bit output
    dt = _dt(dy16, dx_bf16)
    if not DETERMINISTIC:
        _check(lib().enh_layernorm_backward(_p(dy32, F32, "dy"), _p(dy16, H16, "dy_bf16"), _p(x, F32, "x"), _p(w, F32, "w"), _p(mean, F32, "mean"),
                                            _p(rstd, F32, "rstd"), _p(dres, F32, "dres"), M, D, _p(dx_f32, F32, "dx_f32"),
                                            _p(dx_bf16, H16, "dx_bf16"), _p(dw, F32, "dw"), _p(db, F32, "db"), _p(dx_colsum, F32, "dx_colsum"),
                                            dt, _stream()), "enh_layernorm_backward")
        return
    # deterministic form: per-workgroup column partials in a caller-owned workspace + a fixed-order second pass (no f32 atomics)
    nb = lib().enh_layernorm_backward_workspace_bytes(M, D)
    ws = _workspace(nb, x.device)
    # algorithmic HBM bytes per element: dy (2 or 4) + x 4 + dres 4 in, dx f32 4 + dx bf16 2 out  (16 B/elem with bf16 dy)
    bpe = (2 if dy16 is not None else 4) + 4 + (4 if dres is not None else 0) + (4 if dx_f32 is not None else 0) + (2 if dx_bf16 is not None else 0)
    _timed("ln_bwd_kernel", float(bpe) * M * D, lambda: _check(lib().enh_layernorm_backward_ws(_p(dy32, F32, "dy"), _p(dy16, H16, "dy_bf16"), _p(x, F32, "x"), _p(w, F32, "w"), _p(mean, F32, "mean"),
                                           _p(rstd, F32, "rstd"), _p(dres, F32, "dres"), M, D, _p(dx_f32, F32, "dx_f32"),
                                           _p(dx_bf16, H16, "dx_bf16"), _p(dw, F32, "dw"), _p(db, F32, "db"), _p(dx_colsum, F32, "dx_colsum"),
                                           _p(ws), ws.numel(), dt, _stream()), "enh_layernorm_backward_ws"), unit="byte")


# ------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------
def gemm(a, b, M: int, N: int, K: int, trans_a: bool = False, trans_b: bool = False, bias=None, act: int = ACT_NONE, aux=None,
         res=None, res_rows: int = 0, accumulate: bool = False, out_f32=None, out_bf16=None, lda: Optional[int] = None,
         ldb: Optional[int] = None, ldc: Optional[int] = None):
    """C[M,N] = epilogue(A(m,k) * B(n,k)); see include/enh_hip.h.  a / b are 2-D 16-bit tensors (row-major storage), both torch.bfloat16 or both
    torch.float16: the container dtype selects the MFMA operand format (ENH_DT_BF16 / ENH_DT_F16)."""
    lda = a.stride(0) if lda is None else lda
    ldb = b.stride(0) if ldb is None else ldb
    out = out_f32 if out_f32 is not None else out_bf16
    ldc = out.stride(0) if ldc is None else ldc
    # split-K calls (weight gradients; also any accumulate-into-f32 call with a long K and few tiles, e.g. the discriminator's 8192 -> 512 linear at a
    # small batch): partial slabs in a caller-owned workspace + a fixed-order second pass — deterministic, no f32 atomics.  (Until round 4 only the
    # weight-gradient layout got the workspace; the other layouts fell back to atomics and made the discriminator's forward differ by an ulp from call
    # to call — found by the graph-replay bit-identity test.)
    # Round 6: any f32-output call without an activation may be split (bias / residual / accumulate move into the second pass): what fills the chip at
    # 2 - 4 images per GPU, where the N = dim GEMMs are 96 - 192 tiles (csrc/gemm.hip gemm_splittable).
    ws, ws_bytes = None, 0
    if act == ACT_NONE and ldc == N and ((out_f32 is not None and out_bf16 is None) or
                                         (out_bf16 is not None and out_f32 is None and bias is None and res is None and not accumulate)):
        ws_bytes = lib().enh_gemm_h16_workspace_bytes(int(trans_a), int(trans_b), M, N, K)
        if ws_bytes:
            ws = _gemm_workspace(a.device, ws_bytes)
    dt = _dt(a, b, aux, out_bf16)
    args = (_p(a, H16, "A"), lda, int(trans_a), _p(b, H16, "B"), ldb, int(trans_b), M, N, K, _p(bias, F32, "bias"),
            act, _p(aux, H16, "aux"), aux.stride(0) if aux is not None else 0, _p(res, F32, "res"),
            res.stride(0) if res is not None else 0, res_rows if res is not None else 0, int(accumulate),
            _p(out_f32, F32, "out_f32"), _p(out_bf16, H16, "out_bf16"), ldc, _p(ws), ws_bytes if ws is not None else 0, dt, _stream())
    _timed(None, 2.0 * M * N * K, lambda: _check(lib().enh_gemm_h16_ws(*args), "enh_gemm_h16"))


def gemm_dtanh_colsum(a, b, M: int, N: int, K: int, aux, out_bf16, colsum_out, trans_b: bool = True, accumulate_colsum: bool = True):
    """out = (a b) * (1 - aux^2) -> bf16 and colsum_out (+)= column sums of out: enh_gemm_bf16_dtanh_colsum (the tanh' input gradient with the bias
    gradient of the Linear in front of the tanh taken in the GEMM's epilogue instead of by a second pass over `out`)"""
    nb = lib().enh_gemm_h16_dtanh_colsum_workspace_bytes(int(trans_b), M, N, K)
    ws = _workspace(nb, a.device)
    dt = _dt(a, b, aux, out_bf16)
    args = (_p(a, H16, "A"), a.stride(0), _p(b, H16, "B"), b.stride(0), int(trans_b), M, N, K, _p(aux, H16, "aux"), aux.stride(0),
            _p(out_bf16, H16, "out_bf16"), out_bf16.stride(0), _p(colsum_out, F32, "colsum"), int(accumulate_colsum), _p(ws), ws.numel(), dt, _stream())
    # (labelled with the GEMM kernel's symbol: the partial-row second pass and, off the tile grid, the column-sum kernel ride along)
    _timed(None, 2.0 * M * N * K, lambda: _check(lib().enh_gemm_h16_dtanh_colsum(*args), "enh_gemm_h16_dtanh_colsum"))


def set_cu_budget(n: int) -> None:
    """CUs the GEMM launches may count on (0 = all); see include/enh_hip.h"""
    _check(lib().enh_set_cu_budget(int(n)), "enh_set_cu_budget")


def get_cu_budget() -> int:
    return int(lib().enh_get_cu_budget())


def device_cus() -> int:
    """CUs of the current device"""
    L = lib()
    cur = int(L.enh_get_cu_budget())
    if _DEVICE_CUS[0] is None:
        L.enh_set_cu_budget(0)
        _DEVICE_CUS[0] = int(L.enh_get_cu_budget())
        L.enh_set_cu_budget(cur if cur != _DEVICE_CUS[0] else 0)
    return _DEVICE_CUS[0]


_DEVICE_CUS = [None]


CONV_KERNELS = {"auto": 0, "reg": 1, "t128": 2, "t256": 3}


def conv_set_kernel(name: str) -> None:
    """kernel family of the implicit-GEMM convolutions (enh_conv_set_kernel / enh_conv_wgrad_set_kernel are one switch here): auto | reg | t128 | t256"""
    _check(lib().enh_conv_set_kernel(CONV_KERNELS[name]), "enh_conv_set_kernel")


def gemm_set_scheduler(dynamic: bool) -> None:
    _check(lib().enh_gemm_set_scheduler(int(bool(dynamic))), "enh_gemm_set_scheduler")


def occupy_cus(n_wg: int, ms: float, stream=None) -> None:
    """measurement aid: hold n_wg CUs for ms milliseconds on `stream` (a torch stream; default: the current one)"""
    st = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    _check(lib().enh_debug_occupy_cus(int(n_wg), float(ms), st), "enh_debug_occupy_cus")


_GEMM_WS = {}


def _gemm_workspace(device, nbytes: int):
    """one grow-only split-K workspace per (device, stream) (the library never allocates: SURVEY.md §8b ownership rule): the GEMMs of one stream run in
    order, so they share a buffer; the engine's weight-gradient side stream (small batches, engine/stage1.py) gets its own"""
    key = (device, torch.cuda.current_stream().cuda_stream)
    t = _GEMM_WS.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _GEMM_WS[key] = t
    return t


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def attention_set_kernel(fwd: int = 0, dq: int = 0, dkv: int = 0) -> None:
    """A/B aid: kernel family per pass (include/enh_hip.h enh_attention_set_kernel)"""
    _check(lib().enh_attention_set_kernel(fwd, dq, dkv), "enh_attention_set_kernel")


def attention_forward(qkv, B: int, N: int, H: int, scale: float, out, lse, q_prescaled: bool = False, dim_head: int = 64):
    """q_prescaled: the q third of qkv holds q * scale * log2(e) (include/enh_hip.h).  dim_head: 64 (the tuned kernels, enh_attention_forward) or
    32 | 96 | 128 (enh_attention_forward_dh); anything else is the library's shape error."""
    dt = _dt(qkv, out)
    if dim_head == 64:
        _timed(None, 4.0 * B * H * N * N * 64,
               lambda: _check(lib().enh_attention_forward(_p(qkv, H16, "qkv"), B, N, H, scale, int(q_prescaled), _p(out, H16, "out"), _p(lse, F32, "lse"),
                                                          dt, _stream()), "enh_attention_forward"))
        return
    _timed(None, 4.0 * B * H * N * N * dim_head,
           lambda: _check(lib().enh_attention_forward_dh(_p(qkv, H16, "qkv"), B, N, H, dim_head, scale, int(q_prescaled), _p(out, H16, "out"),
                                                         _p(lse, F32, "lse"), dt, _stream()), "enh_attention_forward_dh"))


def attention_backward(qkv, out, dout, lse, B: int, N: int, H: int, scale: float, dqkv, delta_ws, q_prescaled: bool = False, dim_head: int = 64):
    dt = _dt(qkv, out, dout, dqkv)
    if dim_head == 64:
        _timed("attn_bwd_tail (dq+dkv kernels)" if N % 64 else "attn_bwd (dq+dkv kernels)", 10.0 * B * H * N * N * 64,
               lambda: _check(lib().enh_attention_backward(_p(qkv, H16, "qkv"), _p(out, H16, "out"), _p(dout, H16, "dout"), _p(lse, F32, "lse"), B, N, H,
                                                           scale, int(q_prescaled), _p(dqkv, H16, "dqkv"), _p(delta_ws, F32, "delta_ws"), dt, _stream()),
                              "enh_attention_backward"))
        return
    _timed(f"attn_dh_bwd_dq_kernel<{dim_head}> + attn_dh_bwd_dkv_kernel<{dim_head}>", 10.0 * B * H * N * N * dim_head,
           lambda: _check(lib().enh_attention_backward_dh(_p(qkv, H16, "qkv"), _p(out, H16, "out"), _p(dout, H16, "dout"), _p(lse, F32, "lse"), B, N, H,
                                                          dim_head, scale, int(q_prescaled), _p(dqkv, H16, "dqkv"), _p(delta_ws, F32, "delta_ws"), dt,
                                                          _stream()), "enh_attention_backward_dh"))


# ------------------------------------------------------------------------------------------------
# data movement / loss / optimizer
# ------------------------------------------------------------------------------------------------
def patchify(img, p: int, out):
    B, C, H, W = img.shape
    _check(lib().enh_patchify(_p(img, F32, "img"), B, C, H, W, p, _p(out, H16, "patches"), _dt(out), _stream()), "enh_patchify")


def unpatchify_loss(pix, target, B: int, C: int, H: int, W: int, p: int, w_l1: float, w_l2: float, xrec, sums, dpix, grad_scale=None):
    """grad_scale: optional device scalar (f32 [1]) multiplying the gradient dpix only (the loss scale of the fp16 backward)"""
    _check(lib().enh_unpatchify_loss(_p(pix, F32, "pix"), _p(target, F32, "target"), B, C, H, W, p, w_l1, w_l2, _p(xrec, F32, "xrec"),
                                     _p(sums, F64, "sums"), _p(dpix, H16, "dpix"), _p(grad_scale, F32, "grad_scale"), _dt(dpix), _stream()), "enh_unpatchify_loss")


def colsum(x, M: int, N: int, out, accumulate: bool = False):
    """out[n] (+)= sum_m x[m, n]; deterministic two-pass form (per-chunk partials in a workspace, fixed-order second pass)"""
    if not DETERMINISTIC:
        _check(lib().enh_colsum_h16(_p(x, H16, "x"), M, N, x.stride(0), _p(out, F32, "out"), int(accumulate), _dt(x), _stream()), "enh_colsum_h16")
        return
    nb = lib().enh_colsum_h16_workspace_bytes(M, N)
    ws = _workspace(nb, x.device)
    _check(lib().enh_colsum_h16_ws(_p(x, H16, "x"), M, N, x.stride(0), _p(out, F32, "out"), int(accumulate), _p(ws), ws.numel(), _dt(x), _stream()), "enh_colsum_h16_ws")


def cast_bf16_head_scaled(x, y, n_scaled: int, alpha: float):
    """y = bf16(x * alpha) for the first n_scaled elements, bf16(x) for the rest"""
    _check(lib().enh_cast_f32_h16_head_scaled(_p(x, F32, "x"), _p(y, H16, "y"), x.numel(), n_scaled, alpha, _dt(y), _stream()), "enh_cast_f32_h16_head_scaled")


def cast_bf16_head_scaled_strided(x0, x_stride: int, y, n: int, n_scaled: int, alpha: float):
    """y [count, n] bf16 (contiguous) <- the blocks x0 + b * x_stride (x0: the first block, a view into the flat f32 store), q rows scaled by alpha"""
    count = y.shape[0]
    _check(lib().enh_cast_f32_h16_head_scaled_strided(_p(x0, F32, "x"), x_stride, _p(y, H16, "y"), y.stride(0), n, n_scaled, alpha, count, _dt(y), _stream()),
           "enh_cast_f32_h16_head_scaled_strided")


def cast_bf16(x, y):
    """y = round-to-nearest-even 16-bit image of x; y's container dtype (torch.bfloat16 / torch.float16) selects the format"""
    _check(lib().enh_cast_f32_h16(_p(x, F32, "x"), _p(y, H16, "y"), x.numel(), _dt(y), _stream()), "enh_cast_f32_h16")


def crop_flip_u8(src, meta, R: int):
    """src uint8 [B,Hs,Ws,3], meta int32 [B,3] = (y0, x0, flip) -> f32 [B,3,R,R] in [0,1] (enh_crop_flip_u8)"""
    B, Hs, Ws, _ = src.shape
    out = torch.empty(B, 3, R, R, dtype=F32, device=src.device)
    _check(lib().enh_crop_flip_u8(_p(src, torch.uint8, "src"), B, Hs, Ws, _p(meta, torch.int32, "meta"), R, _p(out), _stream()), "enh_crop_flip_u8")
    return out


def resize_u8(src, meta, bounds, weights, dst):
    """src uint8 [B,HS,WS,3] -> dst uint8 [B,HD,WD,3] (enh_resize_u8: PIL bilinear resize, per-image sizes / tables in meta, bounds, weights)"""
    B, HS, WS, _ = src.shape
    _, HD, WD, _ = dst.shape
    nb = lib().enh_resize_u8_workspace_bytes(B, HS, WD)
    ws = _workspace(nb, src.device)
    _check(lib().enh_resize_u8(_p(src, torch.uint8, "src"), B, HS, WS, _p(meta, torch.int32, "meta"), _p(bounds, torch.int32, "bounds"),
                               _p(weights, torch.int32, "weights"), _p(dst, torch.uint8, "dst"), HD, WD, _p(ws), ws.numel(), _stream()), "enh_resize_u8")
    return dst


def nonfinite_flag(x, flag):
    """flag[0] = 1.0 if x (f32, flat) holds an inf / nan; untouched otherwise (zero it once per step)"""
    _timed("nonfinite_flag_kernel", 4.0 * x.numel(),
           lambda: _check(lib().enh_nonfinite_flag(_p(x, F32, "x"), x.numel(), _p(flag, F32, "flag"), _stream()), "enh_nonfinite_flag"), unit="byte")


def grad_clip_coef(g, max_norm: float, grad_scale: float, out, loss_scale=None, found_inf=None):
    """out[0] = total_norm = ||g||_2 * grad_scale / (loss_scale or 1), out[1] = coef = min(1, max_norm / (total_norm + 1e-6)) — the coefficient of
    torch.nn.utils.clip_grad_norm_ over one flat f32 gradient, left on the device (out f32 [2]; enh_adamw_step's clip_coef operand is out[1:]).
    max_norm = inf: the norm alone (coef = 1).  found_inf (f32 [1]): additionally set to 1.0 on an inf / nan, in the same pass (never cleared)."""
    nb = lib().enh_grad_clip_coef_workspace_bytes(g.numel())
    ws = _workspace(nb, g.device)
    _timed("grad_sumsq_kernel", 4.0 * g.numel(),
           lambda: _check(lib().enh_grad_clip_coef(_p(g, F32, "g"), g.numel(), float(max_norm), float(grad_scale), _p(loss_scale, F32, "loss_scale"),
                                                   _p(found_inf, F32, "found_inf"), _p(out, F32, "out"), _p(ws), ws.numel(), _stream()),
                          "enh_grad_clip_coef"), unit="byte")


def adamw_step(p, g, m, v, p_bf16, step, lr: float, beta1: float = 0.9, beta2: float = 0.99, eps: float = 1e-8,
               weight_decay: float = 1e-4, grad_scale: float = 1.0, skip_flag=None, loss_scale=None, clip_coef=None, clip_value: float = 0.0):
    """step: the step number t >= 1 whose bias corrections this launch applies, or a device f64 [4] = (applied steps, 1 / (1 - beta1^t),
    1 / sqrt(1 - beta2^t), 0): the count then lives on the device and is advanced in front of the update unless skip_flag is set — a dropped step
    does not count, as under GradScaler.step (engine/optim.py step_operand).
    clip_coef (device f32 [1], optional): multiplies the gradient after the loss-scale division (grad_clip_coef's out[1:]); clip_value > 0: the unscaled
    gradient is clamped to [-clip_value, clip_value] before the moments (0 = off)"""
    state = step if isinstance(step, torch.Tensor) else None
    if state is not None and state.numel() < 3:
        raise RuntimeError("adamw_step: a device step state is f64 [4] (applied steps, the two bias-correction factors, 0)")
    # 30 B per parameter: p, g, m, v read (16) + p, m, v written (12) + the bf16 operand shadow written (2)
    _timed("adamw_kernel", (28.0 + (2.0 if p_bf16 is not None else 0.0)) * p.numel(),
           lambda: _check(lib().enh_adamw_step(_p(p, F32, "p"), _p(g, F32, "g"), _p(m, F32, "m"), _p(v, F32, "v"), _p(p_bf16, H16, "p_bf16"),
                                               p.numel(), 0 if state is not None else int(step), lr, beta1, beta2, eps, weight_decay, grad_scale,
                                               _p(skip_flag, F32, "skip_flag"), _p(loss_scale, F32, "loss_scale"), _p(clip_coef, F32, "clip_coef"),
                                               float(clip_value), _p(state, F64, "step"), _dt(p_bf16), _stream()), "enh_adamw_step"), unit="byte")


def adam_segment_table(segments, n: int, arena_n: int, device):
    """the device segment table of adam_step_segments from a host list of (begin, end, dst16, weight_decay): checked here, once, because the kernel
    trusts it — sorted, disjoint, inside [0, n), every bound a multiple of 64, destinations (dst16 = -1: none) inside the arena, multiples of 8 and
    disjoint.  Returns an int64 [nseg, 4] tensor (32 bytes per entry: begin, end, dst16, the f32 bits of weight_decay in the low word)."""
    import struct
    rows, last, dsts = [], 0, []
    for b, e, d, wd in segments:
        b, e, d = int(b), int(e), int(d)
        if not (last <= b < e <= n) or b % 64 or e % 64:
            raise RuntimeError(f"adam_segment_table: segment [{b}, {e}) must follow the one before it, lie inside [0, {n}) and have bounds that are multiples of 64")
        if d != -1:
            if d < 0 or d % 8 or d + (e - b) > arena_n:
                raise RuntimeError(f"adam_segment_table: destination {d} of segment [{b}, {e}) must be a multiple of 8 inside the arena of {arena_n} elements")
            dsts.append((d, d + e - b))
        rows.append([b, e, d, struct.unpack("<q", struct.pack("<fi", float(wd), 0))[0]])
        last = e
    if not rows:
        raise RuntimeError("adam_segment_table: no segment")
    dsts.sort()
    if any(a[1] > b[0] for a, b in zip(dsts, dsts[1:])):
        raise RuntimeError("adam_segment_table: two segments share arena elements")
    return torch.tensor(rows, dtype=I64).to(device)


def adam_step_segments(p, g, m, v, arena, table, state, lr: float, beta1: float = 0.9, beta2: float = 0.96, eps: float = 1e-8, grad_scale: float = 1.0,
                       skip_flag=None, loss_scale=None, clip_coef=None, clip_value: float = 0.0, dtype=None):
    """one torch.optim.Adam step over flat f32 p, g, m, v driven by `table` (adam_segment_table: per segment an L2 weight decay and an optional
    destination in the 16-bit operand `arena`, which receives the new p in the same pass); state: device f64 [4] = (t, beta1^t, beta2^t, 0), advanced on
    the device unless skip_flag is set, in which case nothing at all is written.  dtype: the arena's format when there is no arena tensor."""
    n = p.numel()
    if g.numel() != n or m.numel() != n or v.numel() != n:
        raise RuntimeError("adam_step_segments: p, g, m and v must be equally long")
    if table.dim() != 2 or table.shape[1] != 4 or state.numel() != 4:
        raise RuntimeError("adam_step_segments: table must be [nseg, 4] (adam_segment_table) and state f64 [4]")
    dt = _dt(arena) if arena is not None else (DT_F16 if dtype == F16 else DT_BF16)
    # 30 B per parameter: p, g, m, v read (16) + p, m, v written (12) + the 16-bit operand written (2; only the segments with a destination)
    _timed(None, 30.0 * n,
           lambda: _check(lib().enh_adam_step_segments(_p(p, F32, "p"), _p(g, F32, "g"), _p(m, F32, "m"), _p(v, F32, "v"), n, _p(arena, H16, "arena"),
                                                       0 if arena is None else arena.numel(), _p(table, I64, "table"), table.shape[0],
                                                       _p(state, F64, "state"), float(lr), float(beta1), float(beta2), float(eps), float(grad_scale),
                                                       _p(skip_flag, F32, "skip_flag"), _p(loss_scale, F32, "loss_scale"), _p(clip_coef, F32, "clip_coef"),
                                                       float(clip_value), dt, _stream()), "enh_adam_step_segments"), unit="byte")


def adam_step_segments_s16(p, g, m16, v16, arena, table, state, lr: float, beta1: float = 0.9, beta2: float = 0.96, eps: float = 1e-8,
                           grad_scale: float = 1.0, skip_flag=None, loss_scale=None, clip_coef=None, clip_value: float = 0.0, seed: int = 0, sr_words=None,
                           dtype=None):
    """adam_step_segments with bf16 moments m16, v16 (torch.bfloat16 [n]): widened exactly, p updated from the unrounded f32 moments, the stored moments
    rounded stochastically with Philox words of (seed, group of 4 elements, applied step count) — include/enh_hip.h enh_adam_step_segments_s16.
    sr_words (int32 [n], tests only) replaces the Philox words: element e's low half rounds m, its high half v."""
    n = p.numel()
    if g.numel() != n or m16.numel() != n or v16.numel() != n or (sr_words is not None and sr_words.numel() != n):
        raise RuntimeError("adam_step_segments_s16: p, g, m16, v16 (and sr_words) must be equally long")
    if table.dim() != 2 or table.shape[1] != 4 or state.numel() != 4:
        raise RuntimeError("adam_step_segments_s16: table must be [nseg, 4] (adam_segment_table) and state f64 [4]")
    dt = _dt(arena) if arena is not None else (DT_F16 if dtype == F16 else DT_BF16)
    # 22 B per parameter: p, g (8) + m16, v16 (4) read, p (4) + m16, v16 (4) + the 16-bit operand (2) written
    _timed(None, 22.0 * n,
           lambda: _check(lib().enh_adam_step_segments_s16(_p(p, F32, "p"), _p(g, F32, "g"), _p(m16, BF16, "m16"), _p(v16, BF16, "v16"), n,
                                                           _p(arena, H16, "arena"), 0 if arena is None else arena.numel(), _p(table, I64, "table"),
                                                           table.shape[0], _p(state, F64, "state"), float(lr), float(beta1), float(beta2), float(eps),
                                                           float(grad_scale), _p(skip_flag, F32, "skip_flag"), _p(loss_scale, F32, "loss_scale"),
                                                           _p(clip_coef, F32, "clip_coef"), float(clip_value), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                           _p(sr_words, torch.int32, "sr_words"), dt, _stream()), "enh_adam_step_segments_s16"),
           unit="byte")


def loss_scale_update(scale, found_inf, tracker, growth: float = 2.0, backoff: float = 0.5, interval: int = 2000):
    """torch.cuda.amp.GradScaler.update() on the device (scale f32 [1], found_inf f32 [1], tracker int32 [1])"""
    _check(lib().enh_loss_scale_update(_p(scale, F32, "scale"), _p(found_inf, F32, "found_inf"), _p(tracker, torch.int32, "tracker"), growth, backoff, int(interval),
                                       _stream()), "enh_loss_scale_update")


# ------------------------------------------------------------------------------------------------
# discriminator native ops (reference enhancing/losses/op/*)
# ------------------------------------------------------------------------------------------------
def fused_bias_act(x, bias, ref, grad: int, alpha: float, scale: float):
    """fused.fused_bias_act(input, bias, refer, 3, grad, alpha, scale) -> new tensor (the op allocates its output, as the reference's does)."""
    _p(x, F32, "input")
    y = torch.empty_like(x)
    step_b = 1
    for d in x.shape[2:]:
        step_b *= d
    size_b = bias.numel() if bias is not None and bias.numel() else 0
    b = bias if size_b else None
    _check(lib().enh_fused_bias_act(_p(x, F32, "input"), _p(b, F32, "bias"), _p(ref if ref is not None and ref.numel() else None, F32, "refer"),
                                    _p(y), x.numel(), step_b, size_b, 3, grad, alpha, scale, _stream()), "enh_fused_bias_act")
    return y


def channel_sum(x):
    """sum over every axis except 1 of an f32 [B, C, ...] tensor -> [C]"""
    _p(x, F32, "x")
    B, C = x.shape[0], x.shape[1]
    inner = x.numel() // (B * C)
    out = torch.empty(C, dtype=F32, device=x.device)
    _check(lib().enh_channel_sum_f32(_p(x), B, C, inner, _p(out), 0, _stream()), "enh_channel_sum_f32")
    return out


def upfirdn2d(x, kernel, up_x: int, up_y: int, down_x: int, down_y: int, pad_x0: int, pad_x1: int, pad_y0: int, pad_y1: int):
    """upfirdn2d_op.upfirdn2d on x viewed [major, in_h, in_w]; returns [major, out_h, out_w]."""
    _p(x, F32, "input"); _p(kernel, F32, "kernel")
    major, in_h, in_w = x.shape
    kh, kw = kernel.shape
    out_h = (in_h * up_y + pad_y0 + pad_y1 - kh + down_y) // down_y
    out_w = (in_w * up_x + pad_x0 + pad_x1 - kw + down_x) // down_x
    out = torch.empty(major, out_h, out_w, dtype=F32, device=x.device)
    _check(lib().enh_upfirdn2d(_p(x), _p(kernel), _p(out), major, in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1,
                               _stream()), "enh_upfirdn2d")
    return out


def conv_out_size(n: int, k: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - k) // stride + 1


_DT_OF = {BF16: DT_BF16, F16: DT_F16, F32: DT_F32}


def im2col(x, sb: int, sc: int, B: int, C: int, H: int, W: int, k: int, stride: int, pad: int, dtype: torch.dtype = BF16):
    """x f32, element (b,c,h,w) at b*sb + c*sc + h*W + w  ->  cols [B*Ho*Wo, Kp] in `dtype` (bf16 | fp16: MFMA operands; f32: the exact instrument),
    Kp = C*k*k rounded up to 8 (pad columns zero)."""
    _p(x, F32, "x")
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    ld = (C * k * k + 7) // 8 * 8
    cols = torch.empty(B * Ho * Wo, ld, dtype=dtype, device=x.device)
    _check(lib().enh_im2col(_p(x), sb, sc, B, C, H, W, k, stride, pad, Ho, Wo, _p(cols), ld, _DT_OF[dtype], _stream()), "enh_im2col")
    return cols


def col2im(dcols, B: int, C: int, H: int, W: int, k: int, stride: int, pad: int, out, sb: int, sc: int):
    """adjoint of im2col: dcols [B*Ho*Wo, Kp] (bf16 | fp16 | f32) -> f32 `out`, element (b,c,h,w) at b*sb + c*sc + h*W + w (overwritten)."""
    _p(dcols, (BF16, F16, F32), "dcols"); _p(out, F32, "dx")
    Ho, Wo = conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    _check(lib().enh_col2im(_p(dcols), dcols.stride(0), B, C, H, W, k, stride, pad, Ho, Wo, _p(out), sb, sc, _DT_OF[dcols.dtype], _stream()), "enh_col2im")
    return out


# ------------------------------------------------------------------------------------------------
# implicit-GEMM convolutions and element-wise kernels on channels-last bf16 activations (discriminator, LPIPS trunk)
# ------------------------------------------------------------------------------------------------
class ConvGeom(ctypes.Structure):
    """enh_conv_geom of include/enh_hip.h"""
    _fields_ = [(n, _c.c_int) for n in "B Hs Ws C Hm Wm gs oy0 ox0 nty ntx sty stx N HO WO os oph opw".split()]


def _geom(g) -> ConvGeom:
    return g if isinstance(g, ConvGeom) else ConvGeom(**{k: int(v) for k, v in g.items()})


def conv_nhwc(src, wt, geom, mode: int, bias=None, aux=None, add=None, p0: float = 0.0, p1: float = 1.0, out=None):
    """src [B,Hs,Ws,C], wt [N, taps*C] -> out [B,HO,WO,N] (allocated unless given), all in src's 16-bit format (bf16 | fp16); see enh_conv_nhwc_h16"""
    g = _geom(geom)
    if out is None:
        out = torch.empty(g.B, g.HO, g.WO, g.N, dtype=src.dtype, device=src.device)
    work = 2.0 * g.B * g.Hm * g.Wm * g.N * g.nty * g.ntx * g.C
    nb = lib().enh_conv_workspace_bytes(ctypes.byref(g))       # > 0: a small grid that the library splits over the contraction
    ws = _gemm_workspace(src.device, nb) if nb else None
    _timed("conv_igemm_kernel", work,
           lambda: _check(lib().enh_conv_nhwc_h16_ws(_p(src, H16, "src"), _p(wt, H16, "wt"), ctypes.byref(g), mode, _p(bias, F32, "bias"), _p(aux, H16, "aux"),
                                                     _p(add, H16, "add"), p0, p1, _p(out, H16, "out"), _p(ws), nb, _dt(src, wt, aux, add, out), _stream()), "enh_conv_nhwc_h16_ws"))
    return out


def conv_wgrad_nhwc(src, dy, geom):
    """-> f32 [N, taps*C]: sum over the pixels of dy of dy[pix, n] * gathered src[pix, (tap, c)]"""
    g = _geom(geom)
    dw = torch.empty(g.N, g.nty * g.ntx * g.C, dtype=F32, device=src.device)
    nb = lib().enh_conv_wgrad_workspace_bytes(ctypes.byref(g))
    ws = _gemm_workspace(src.device, nb) if nb else None
    work = 2.0 * g.B * g.Hm * g.Wm * g.N * g.nty * g.ntx * g.C
    _timed("conv_wgrad_igemm_kernel", work,
           lambda: _check(lib().enh_conv_wgrad_nhwc_h16(_p(src, H16, "src"), _p(dy, H16, "dy"), ctypes.byref(g), _p(dw), _p(ws), nb, _dt(src, dy), _stream()),
                          "enh_conv_wgrad_nhwc_h16"))
    return dw


def conv_pack_weight(w, scale: float, transposed: bool, kh0: int, kw0: int, kstep: int, nty: int, ntx: int, rows_padded: int, cols_padded: int,
                     dtype: torch.dtype = BF16):
    """w [Cout,Cin,k,k] f32 -> 16-bit operand image [rows_padded, nty*ntx*cols_padded] in `dtype` (bf16 | fp16)"""
    Cout, Cin, k, _ = w.shape
    out = torch.empty(rows_padded, max(nty * ntx * cols_padded, 8), dtype=dtype, device=w.device)
    if nty * ntx:
        _check(lib().enh_conv_pack_weight(_p(w, F32, "w"), Cout, Cin, k, scale, int(transposed), kh0, kw0, kstep, nty, ntx, rows_padded, cols_padded,
                                          _p(out), _dt(out), _stream()), "enh_conv_pack_weight")
    return out


def conv_unpack_wgrad(dwp, Cout: int, Cin: int, cin_padded: int, k: int, scale: float):
    dw = torch.empty(Cout, Cin, k, k, dtype=F32, device=dwp.device)
    _check(lib().enh_conv_unpack_wgrad(_p(dwp, F32, "dwp"), Cout, Cin, cin_padded, k, scale, _p(dw), _stream()), "enh_conv_unpack_wgrad")
    return dw


def blur_nhwc(x, kernel, pad0: int, pad1: int, flip: bool):
    """x [B,H,W,C] bf16, kernel [kh,kw] f32 -> [B, H+pad0+pad1-kh+1, W+pad0+pad1-kw+1, C] bf16"""
    B, H, W, C = x.shape
    kh, kw = kernel.shape
    out = torch.empty(B, H + pad0 + pad1 - kh + 1, W + pad0 + pad1 - kw + 1, C, dtype=x.dtype, device=x.device)
    _check(lib().enh_blur_nhwc_h16(_p(x, H16, "x"), _p(kernel, F32, "kernel"), B, H, W, C, kh, kw, pad0, pad1, pad0, pad1, int(flip), _p(out), _dt(x), _stream()),
           "enh_blur_nhwc_h16")
    return out


def blur_set_kernel(variant: int) -> None:
    """0 = per shape (the row-marching 4 x 4 kernel where it applies), 1 = the one-row kernel everywhere (A/B, tests)"""
    _check(lib().enh_blur_set_kernel(int(variant)), "enh_blur_set_kernel")


def lrelu_gate(g, ref, slope: float, scale: float):
    y = torch.empty_like(g)
    _check(lib().enh_lrelu_gate_h16(_p(g, H16, "g"), _p(ref, H16, "ref"), g.numel(), slope, scale, _p(y), _dt(g, ref), _stream()), "enh_lrelu_gate_h16")
    return y


def img_to_nhwc8(img, dtype: torch.dtype = BF16):
    B, C, H, W = img.shape
    out = torch.empty(B, H, W, 8, dtype=dtype, device=img.device)
    _check(lib().enh_img_to_nhwc8(_p(img, F32, "img"), B, C, H, W, _p(out), _dt(out), _stream()), "enh_img_to_nhwc8")
    return out


def nhwc8_to_img(src, C: int):
    B, H, W, _ = src.shape
    img = torch.empty(B, C, H, W, dtype=F32, device=src.device)
    _check(lib().enh_nhwc8_to_img(_p(src, H16, "src"), B, C, H, W, _p(img), _dt(src), _stream()), "enh_nhwc8_to_img")
    return img


def minibatch_stddev_nhwc(x, group: int, Cp: int):
    """x [B,H,W,C] bf16 -> [B,H,W,Cp] bf16: x, the slot's mean standard deviation in channel C, zeros above (enh_minibatch_stddev_nhwc)"""
    B, H, W, C = x.shape
    out = torch.empty(B, H, W, Cp, dtype=x.dtype, device=x.device)
    _check(lib().enh_minibatch_stddev_nhwc(_p(x, H16, "x"), B, H * W, C, Cp, group, _p(out), _dt(x), _stream()), "enh_minibatch_stddev_nhwc")
    return out


def minibatch_stddev_nhwc_backward(x, g, group: int):
    B, H, W, C = x.shape
    dx = torch.empty_like(x)
    _check(lib().enh_minibatch_stddev_nhwc_backward(_p(x, H16, "x"), _p(g, H16, "g"), B, H * W, C, g.shape[3], group, _p(dx), _dt(x, g), _stream()),
           "enh_minibatch_stddev_nhwc_backward")
    return dx


def colsum_nhwc(x):
    """sum over every axis but the last of a channels-last bf16 tensor -> f32 [C]; narrow C is folded so that a row of the kernel covers 512 columns"""
    C = x.shape[-1]
    M = x.numel() // C
    r = 1
    while C * r < 512 and M % (2 * r) == 0:
        r *= 2
    out = torch.empty(C * r, dtype=F32, device=x.device)
    colsum(x.view(M // r, C * r), M // r, C * r, out)
    return out.view(r, C).sum(0) if r > 1 else out


# ------------------------------------------------------------------------------------------------
# dtype-dispatching front-ends (bf16 product path / fp32 exact mode) used by the engine
# ------------------------------------------------------------------------------------------------
def mm(a, b, M: int, N: int, K: int, out, trans_a: bool = False, trans_b: bool = False, bias=None, act: int = ACT_NONE, aux=None, res=None,
       res_rows: int = 0, accumulate: bool = False):
    """C = epilogue(A B^T) into `out`; bf16 operands -> MFMA kernel (out may be bf16 or f32), f32 operands -> exact f32 kernel."""
    if a.dtype in H16:
        if out.dtype in H16:
            gemm(a, b, M, N, K, trans_a, trans_b, bias, act, aux, res, res_rows, accumulate, out_bf16=out)
        else:
            gemm(a, b, M, N, K, trans_a, trans_b, bias, act, aux, res, res_rows, accumulate, out_f32=out)
        return
    _check(lib().enh_gemm_f32(_p(a, F32, "A"), a.stride(0), int(trans_a), _p(b, F32, "B"), b.stride(0), int(trans_b), M, N, K, _p(bias, F32, "bias"), act,
                              _p(aux, F32, "aux"), aux.stride(0) if aux is not None else 0, _p(res, F32, "res"), res.stride(0) if res is not None else 0,
                              res_rows if res is not None else 0, int(accumulate), _p(out, F32, "out"), out.stride(0), _stream()), "enh_gemm_f32")


def ln_fwd(x, w, b, y, mean, rstd, y_extra_f32=None):
    if y.dtype in H16:
        layernorm_forward(x, w, b, 1e-5, y, y_extra_f32, mean, rstd)
    else:
        layernorm_forward(x, w, b, 1e-5, None, y, mean, rstd)


def ln_bwd(dy, x, w, mean, rstd, dres, dx, dx_operand, dw, db, dx_colsum=None):
    """dx_operand: the tensor the following GEMMs read (a bf16 copy in the product path, dx itself in exact mode)."""
    layernorm_backward(dy, x, w, mean, rstd, dres, dx, dx_operand if dx_operand.dtype in H16 else None, dw, db, dx_colsum)


def attn_fwd(qkv, B, N, H, scale, out, lse, q_prescaled: bool = False, dim_head: int = 64):
    if qkv.dtype in H16:
        attention_forward(qkv, B, N, H, scale, out, lse, q_prescaled, dim_head)
    elif dim_head == 64:
        _check(lib().enh_attention_forward_f32(_p(qkv, F32, "qkv"), B, N, H, scale, _p(out, F32, "out"), _p(lse, F32, "lse"), _stream()), "enh_attention_forward_f32")
    else:
        _check(lib().enh_attention_forward_f32_dh(_p(qkv, F32, "qkv"), B, N, H, dim_head, scale, _p(out, F32, "out"), _p(lse, F32, "lse"), _stream()),
               "enh_attention_forward_f32_dh")


def attn_bwd(qkv, out, dout, lse, B, N, H, scale, dqkv, delta_ws, q_prescaled: bool = False, dim_head: int = 64):
    if qkv.dtype in H16:
        attention_backward(qkv, out, dout, lse, B, N, H, scale, dqkv, delta_ws, q_prescaled, dim_head)
    elif dim_head == 64:
        _check(lib().enh_attention_backward_f32(_p(qkv, F32, "qkv"), _p(out, F32, "out"), _p(dout, F32, "dout"), _p(lse, F32, "lse"), B, N, H, scale,
                                                _p(dqkv, F32, "dqkv"), _p(delta_ws, F32, "delta_ws"), _stream()), "enh_attention_backward_f32")
    else:
        _check(lib().enh_attention_backward_f32_dh(_p(qkv, F32, "qkv"), _p(out, F32, "out"), _p(dout, F32, "dout"), _p(lse, F32, "lse"), B, N, H, dim_head,
                                                   scale, _p(dqkv, F32, "dqkv"), _p(delta_ws, F32, "delta_ws"), _stream()), "enh_attention_backward_f32_dh")


# ------------------------------------------------------------------------------------------------
# x3 split-bf16 operands (parity-grade encoder forward; include/enh_hip.h "x3")
# ------------------------------------------------------------------------------------------------
def split3(x, y3, bias=None, act: int = ACT_NONE, order: int = 0, y_hi=None):
    """x f32 [M,K] -> y3 bf16 [M,3K] = [hi | lo | hi] (order 0) / [hi | hi | lo] (order 1) of f(x + bias); y_hi: optional bf16 [M,K] copy of the hi plane"""
    M, K = x.shape
    # algorithmic HBM bytes: 4 in + 6 out (+ 2)
    _timed("split3_kernel", (10.0 + (2.0 if y_hi is not None else 0.0)) * M * K,
           lambda: _check(lib().enh_split3_bf16(_p(x, F32, "x"), x.stride(0), M, K, _p(bias, F32, "bias"), act, order, _p(y3, BF16, "y3"), y3.stride(0),
                                                _p(y_hi, BF16, "y_hi"), y_hi.stride(0) if y_hi is not None else 0, _stream()), "enh_split3_bf16"), unit="byte")


def split2(x, hi, lo):
    _timed("split2_kernel", 8.0 * x.numel(),
           lambda: _check(lib().enh_split2_bf16(_p(x, F32, "x"), x.numel(), _p(hi, BF16, "hi"), _p(lo, BF16, "lo"), _stream()), "enh_split2_bf16"), unit="byte")


def gemm_split_fused(M: int, N: int, K: int) -> bool:
    """does enh_gemm_bf16_split serve this shape (the persistent 256 x 256 kernel)?  Otherwise: mm -> f32, then split2 / split3."""
    return bool(lib().enh_gemm_bf16_split_fused(M, N, K))


def _poff(t: torch.Tensor, elems: int):
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def gemm_split2(a, b, M: int, N: int, K: int, hi, lo):
    """hi = bf16(a b^T), lo = bf16(a b^T - hi): mm(...) -> f32 followed by split2, without the f32 round trip (bit-identical)"""
    _timed(None, 2.0 * M * N * K,
           lambda: _check(lib().enh_gemm_bf16_split(_p(a, BF16, "A"), a.stride(0), _p(b, BF16, "B"), b.stride(0), M, N, K, None, ACT_NONE,
                                                    _p(hi, BF16, "hi"), hi.stride(0), _p(lo, BF16, "lo"), lo.stride(0), None, 0, None, 0, _stream()), "enh_gemm_bf16_split"))


def gemm_split3_tanh(a, b, M: int, N: int, K: int, bias, y3, y_hi=None):
    """y3 [M, 3N] = the x3 row [hi | lo | hi] of tanh(a b^T + bias) (+ y_hi [M, N] = the hi plane): mm(...) -> f32 followed by split3(act = tanh), fused"""
    if not (y3.is_cuda and y3.is_contiguous() and y3.dtype == BF16 and y3.shape[-1] == 3 * N):
        raise RuntimeError("y3 must be a contiguous bf16 [M, 3N] device tensor")
    ld3 = y3.stride(0)
    _timed(None, 2.0 * M * N * K,
           lambda: _check(lib().enh_gemm_bf16_split(_p(a, BF16, "A"), a.stride(0), _p(b, BF16, "B"), b.stride(0), M, N, K, _p(bias, F32, "bias"), ACT_TANH,
                                                    _poff(y3, 0), ld3, _poff(y3, N), ld3, _poff(y3, 2 * N), ld3,
                                                    _p(y_hi, BF16, "y_hi"), y_hi.stride(0) if y_hi is not None else 0, _stream()), "enh_gemm_bf16_split"))


def ln_fwd_x3(x, w, b, y3, mean, rstd, y_bf16=None, y_f32=None):
    M, D = x.shape
    _check(lib().enh_layernorm_forward_x3(_p(x, F32, "x"), _p(w, F32, "w"), _p(b, F32, "b"), M, D, 1e-5, _p(y3, BF16, "y3"), _p(y_bf16, BF16, "y_bf16"),
                                          _p(y_f32, F32, "y_f32"), _p(mean, F32, "mean"), _p(rstd, F32, "rstd"), _stream()), "enh_layernorm_forward_x3")


def attention_forward_x3(qkv_hi, qkv_lo, B: int, N: int, H: int, scale: float, out3, out_bf16, lse):
    # executed MFMA work: three passes of the 4 N^2 64 algorithmic FLOP per (image, head)
    _timed("attn_fwd_tail_x3_kernel" if N % 64 else "attn_fwd_x3_kernel", 3 * 4.0 * B * H * N * N * 64,
           lambda: _check(lib().enh_attention_forward_x3(_p(qkv_hi, BF16, "qkv_hi"), _p(qkv_lo, BF16, "qkv_lo"), B, N, H, scale, _p(out3, BF16, "out3"),
                                                         _p(out_bf16, BF16, "out_bf16"), _p(lse, F32, "lse"), _stream()), "enh_attention_forward_x3"))


def colsum_any(x, M, N, out, accumulate=False):
    if x.dtype in H16:
        colsum(x, M, N, out, accumulate)
    else:
        _check(lib().enh_colsum_f32(_p(x, F32, "x"), M, N, x.stride(0), _p(out, F32, "out"), int(accumulate), _stream()), "enh_colsum_f32")


def patchify_any(img, p, out):
    if out.dtype in H16:
        patchify(img, p, out)
    else:
        B, C, H, W = img.shape
        _check(lib().enh_patch_perm_f32(_p(img, F32, "img"), _p(out, F32, "patches"), B, C, H, W, p, 1, _stream()), "enh_patch_perm_f32")


def unpatchify_loss_any(pix, target, B, C, H, W, p, w_l1, w_l2, xrec, sums, dpix, grad_scale=None):
    if dpix is None or dpix.dtype in H16 or target is None:
        unpatchify_loss(pix, target, B, C, H, W, p, w_l1, w_l2, xrec, sums, dpix, grad_scale)
    else:
        _check(lib().enh_unpatchify_loss_f32(_p(pix, F32, "pix"), _p(target, F32, "target"), B, C, H, W, p, w_l1, w_l2, _p(xrec, F32, "xrec"),
                                             _p(sums, F64, "sums"), _p(dpix, F32, "dpix"), _stream()), "enh_unpatchify_loss_f32")


# ------------------------------------------------------------------------------------------------
# LPIPS (lpips 0.1.4, net="vgg"): channels-last bf16 activations
# ------------------------------------------------------------------------------------------------
def conv3x3_nhwc(x, wt, B: int, H: int, W: int, Cin: int, Cout: int, out, bias=None, mode: int = 0, aux=None, add=None):
    _timed("conv3x3_igemm_kernel", 2.0 * B * H * W * Cout * 9 * Cin,
           lambda: _check(lib().enh_conv3x3_nhwc_h16(_p(x, H16, "x"), _p(wt, H16, "wt"), B, H, W, Cin, Cout, _p(bias, F32, "bias"), mode, _p(aux, H16, "aux"),
                                                     _p(add, H16, "add"), _p(out, H16, "out"), _dt(x, wt, aux, add, out), _stream()), "enh_conv3x3_nhwc_h16"))
    return out


def vgg_conv1(img, w, bias, shift, scale, normalize: bool, out):
    B, _, H, W = img.shape
    _check(lib().enh_vgg_conv1(_p(img, F32, "img"), _p(w, F32, "w"), _p(bias, F32, "bias"), _p(shift, F32, "shift"), _p(scale, F32, "scale"), int(normalize), B, H, W,
                               _p(out, H16, "out"), _dt(out), _stream()), "enh_vgg_conv1")
    return out


def vgg_conv1_backward(gpre, w, scale, normalize: bool, B: int, H: int, W: int, dimg):
    _check(lib().enh_vgg_conv1_backward(_p(gpre, H16, "gpre"), _p(w, F32, "w"), _p(scale, F32, "scale"), int(normalize), B, H, W, _p(dimg, F32, "dimg"), _dt(gpre), _stream()),
           "enh_vgg_conv1_backward")
    return dimg


def maxpool2_nhwc(x, B: int, H: int, W: int, C: int, y):
    _check(lib().enh_maxpool2_nhwc_h16(_p(x, H16, "x"), B, H, W, C, _p(y, H16, "y"), _dt(x, y), _stream()), "enh_maxpool2_nhwc_h16")
    return y


def maxpool2_nhwc_backward(x, gy, add, B: int, H: int, W: int, C: int, gx):
    _check(lib().enh_maxpool2_nhwc_h16_backward(_p(x, H16, "x"), _p(gy, H16, "gy"), _p(add, H16, "add"), B, H, W, C, _p(gx, H16, "gx"), _dt(x, gy, add, gx), _stream()),
           "enh_maxpool2_nhwc_h16_backward")
    return gx


def lpips_head(feat, lin, B: int, HW: int, C: int, val_ws, out, accumulate: bool):
    _check(lib().enh_lpips_head(_p(feat, H16, "feat"), _p(lin, F32, "lin"), B, HW, C, _p(val_ws, F32, "val_ws"), _p(out, F32, "out"), int(accumulate), _dt(feat), _stream()),
           "enh_lpips_head")


def lpips_head_backward(feat, lin, gout, B: int, HW: int, C: int, dfeat1):
    _check(lib().enh_lpips_head_backward(_p(feat, H16, "feat"), _p(lin, F32, "lin"), _p(gout, F32, "gout"), B, HW, C, _p(dfeat1, H16, "dfeat1"), _dt(feat, dfeat1), _stream()),
           "enh_lpips_head_backward")


# ------------------------------------------------------------------------------------------------
# stage-2 sampling: decode-shaped kernels (csrc/gpt_decode.hip; LayerNorm and embedding: csrc/gpt_rows.hip)
# ------------------------------------------------------------------------------------------------
ACT_RELU_SQ = 1      # enh_skinny_gemm_h16's own activation code: square(relu(.))


def skinny_gemm(x, w, out, bias=None, relu_sq: bool = False, res=None):
    """out[M,N] = act(x[M,K] w[N,K]^T + bias) (+ res): x, w 16-bit (one format), M <= 64; out f32 or 16-bit (enh_skinny_gemm_h16)"""
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or tuple(out.shape) != (M, N) or (res is not None and tuple(res.shape) != (M, N)) or (bias is not None and bias.numel() != N):
        raise RuntimeError(f"skinny_gemm: x {tuple(x.shape)} w {tuple(w.shape)} out {tuple(out.shape)} do not fit")
    L = lib()
    nb = L.enh_skinny_gemm_workspace_bytes(M, N, K)
    ws = _workspace(nb, x.device) if nb else None
    o32, o16 = (out, None) if out.dtype == F32 else (None, out)
    # algorithmic bytes: the weight once, x, the result
    _timed(None, 2.0 * N * K + 2.0 * M * K + float(out.element_size()) * M * N,
           lambda: _check(L.enh_skinny_gemm_h16(_p(x, H16, "x"), _p(w, H16, "w"), M, N, K, _p(bias, F32, "bias"), ACT_RELU_SQ if relu_sq else 0,
                                                _p(res, F32, "res"), _p(o32, F32, "out"), _p(o16, H16, "out"), _p(ws), nb, _dt(x, w, o16), _stream()),
                          "enh_skinny_gemm_h16"), unit="byte")


U8 = torch.uint8
MX_BLOCK = 32        # k per E8M0 scale of an MXFP8, MXFP6 or MXFP4 operand (include/enh_hip.h)


def quantize_mxfp8(w, codes, scales, row0: int = 0):
    """the MXFP8 operand of a weight (enh_mxfp8_quantize): w [N, K] f32, K % 32 == 0, rows contiguous (any row stride that keeps them 16-byte
    aligned) -> rows row0 .. row0 + N - 1 of codes [Nt, K] uint8 (e4m3fn) and scales [Nt, K / 32] uint8 (E8M0); the other rows are not touched"""
    if w.dim() != 2 or codes.dim() != 2 or scales.dim() != 2:
        raise RuntimeError(f"quantize_mxfp8: w {tuple(w.shape)} codes {tuple(codes.shape)} scales {tuple(scales.shape)} must be matrices")
    N, K = w.shape
    if K % MX_BLOCK or codes.shape[1] != K or tuple(scales.shape) != (codes.shape[0], K // MX_BLOCK) or row0 < 0 or row0 + N > codes.shape[0]:
        raise RuntimeError(f"quantize_mxfp8: w {tuple(w.shape)} codes {tuple(codes.shape)} scales {tuple(scales.shape)} row0 {row0} do not fit "
                           f"(K must be a multiple of {MX_BLOCK}, scales [rows, K / {MX_BLOCK}])")
    if not w.is_cuda or w.dtype != F32 or (K > 1 and w.stride(1) != 1):
        raise RuntimeError(f"quantize_mxfp8: w must be an f32 device tensor whose rows are contiguous, got {w.dtype} on {w.device} strides {w.stride()}")
    stride = w.stride(0) if N > 1 else K
    # bytes moved: the masters once, the codes and the scales
    _timed(None, 4.0 * N * K + N * K + N * (K // MX_BLOCK),
           lambda: _check(lib().enh_mxfp8_quantize(ctypes.c_void_p(w.data_ptr()), N, K, int(stride), _p(codes, U8, "codes"), int(row0),
                                                   _p(scales, U8, "scales"), int(row0), _stream()), "enh_mxfp8_quantize"), unit="byte")


def skinny_gemm_w8(x, codes, scales, out, bias=None, relu_sq: bool = False, res=None):
    """skinny_gemm with the weight given as its MXFP8 operand (enh_skinny_gemm_w8): out[M,N] = act(x[M,K] dequant(codes, scales)^T + bias) (+ res);
    x 16-bit, codes [N, K] uint8, scales [N, K / 32] uint8, M <= 64, N % 8 == 0, K % 32 == 0; out f32 or x's 16-bit format"""
    M, K = x.shape
    N = codes.shape[0]
    if (codes.dim() != 2 or codes.shape[1] != K or K % MX_BLOCK or tuple(scales.shape) != (N, K // MX_BLOCK) or tuple(out.shape) != (M, N)
            or (res is not None and tuple(res.shape) != (M, N)) or (bias is not None and bias.numel() != N)):
        raise RuntimeError(f"skinny_gemm_w8: x {tuple(x.shape)} codes {tuple(codes.shape)} scales {tuple(scales.shape)} out {tuple(out.shape)} do not fit "
                           f"(K must be a multiple of {MX_BLOCK}, scales [N, K / {MX_BLOCK}])")
    L = lib()
    nb = L.enh_skinny_gemm_workspace_bytes(M, N, K)
    ws = _workspace(nb, x.device) if nb else None
    o32, o16 = (out, None) if out.dtype == F32 else (None, out)
    # bytes moved: the codes and the scales once, x, the result
    _timed(None, float(N) * K + float(N) * (K // MX_BLOCK) + 2.0 * M * K + float(out.element_size()) * M * N,
           lambda: _check(L.enh_skinny_gemm_w8(_p(x, H16, "x"), _p(codes, U8, "codes"), _p(scales, U8, "scales"), M, N, K, _p(bias, F32, "bias"),
                                               ACT_RELU_SQ if relu_sq else 0, _p(res, F32, "res"), _p(o32, F32, "out"), _p(o16, H16, "out"), _p(ws), nb,
                                               _dt(x, o16), _stream()), "enh_skinny_gemm_w8"), unit="byte")


def quantize_mxfp4(w, codes, scales, row0: int = 0):
    """the MXFP4 operand of a weight (enh_mxfp4_quantize): w [N, K] f32, K % 32 == 0, rows contiguous (any row stride that keeps them 16-byte
    aligned) -> rows row0 .. row0 + N - 1 of codes [Nt, K / 2] uint8 (two e2m1 codes per byte, k even in the low nibble) and scales [Nt, K / 32]
    uint8 (E8M0); the other rows are not touched"""
    if w.dim() != 2 or codes.dim() != 2 or scales.dim() != 2:
        raise RuntimeError(f"quantize_mxfp4: w {tuple(w.shape)} codes {tuple(codes.shape)} scales {tuple(scales.shape)} must be matrices")
    N, K = w.shape
    if K % MX_BLOCK or codes.shape[1] != K // 2 or tuple(scales.shape) != (codes.shape[0], K // MX_BLOCK) or row0 < 0 or row0 + N > codes.shape[0]:
        raise RuntimeError(f"quantize_mxfp4: w {tuple(w.shape)} codes {tuple(codes.shape)} scales {tuple(scales.shape)} row0 {row0} do not fit "
                           f"(K must be a multiple of {MX_BLOCK}, codes [rows, K / 2], scales [rows, K / {MX_BLOCK}])")
    if not w.is_cuda or w.dtype != F32 or (K > 1 and w.stride(1) != 1):
        raise RuntimeError(f"quantize_mxfp4: w must be an f32 device tensor whose rows are contiguous, got {w.dtype} on {w.device} strides {w.stride()}")
    stride = w.stride(0) if N > 1 else K
    # bytes moved: the masters once, the codes and the scales
    _timed(None, 4.0 * N * K + N * (K // 2) + N * (K // MX_BLOCK),
           lambda: _check(lib().enh_mxfp4_quantize(ctypes.c_void_p(w.data_ptr()), N, K, int(stride), _p(codes, U8, "codes"), int(row0),
                                                   _p(scales, U8, "scales"), int(row0), _stream()), "enh_mxfp4_quantize"), unit="byte")


def skinny_gemm_w4(x, codes, scales, out, bias=None, relu_sq: bool = False, res=None):
    """skinny_gemm with the weight given as its MXFP4 operand (enh_skinny_gemm_w4): out[M,N] = act(x[M,K] dequant(codes, scales)^T + bias) (+ res);
    x 16-bit, codes [N, K / 2] uint8, scales [N, K / 32] uint8, M <= 64, N % 8 == 0, K % 32 == 0; out f32 or x's 16-bit format"""
    M, K = x.shape
    N = codes.shape[0]
    if (codes.dim() != 2 or K % MX_BLOCK or codes.shape[1] != K // 2 or tuple(scales.shape) != (N, K // MX_BLOCK) or tuple(out.shape) != (M, N)
            or (res is not None and tuple(res.shape) != (M, N)) or (bias is not None and bias.numel() != N)):
        raise RuntimeError(f"skinny_gemm_w4: x {tuple(x.shape)} codes {tuple(codes.shape)} scales {tuple(scales.shape)} out {tuple(out.shape)} do not fit "
                           f"(K must be a multiple of {MX_BLOCK}, codes [N, K / 2], scales [N, K / {MX_BLOCK}])")
    L = lib()
    nb = L.enh_skinny_gemm_w4_workspace_bytes(M, N, K)
    ws = _workspace(nb, x.device) if nb else None
    o32, o16 = (out, None) if out.dtype == F32 else (None, out)
    # bytes moved: the codes and the scales once, x, the result
    _timed(None, 0.5 * N * K + float(N) * (K // MX_BLOCK) + 2.0 * M * K + float(out.element_size()) * M * N,
           lambda: _check(L.enh_skinny_gemm_w4(_p(x, H16, "x"), _p(codes, U8, "codes"), _p(scales, U8, "scales"), M, N, K, _p(bias, F32, "bias"),
                                               ACT_RELU_SQ if relu_sq else 0, _p(res, F32, "res"), _p(o32, F32, "out"), _p(o16, H16, "out"), _p(ws), nb,
                                               _dt(x, o16), _stream()), "enh_skinny_gemm_w4"), unit="byte")


def mxfp6_row_bytes(K: int) -> int:
    """bytes of a row of MXFP6 codes (include/enh_hip.h): whole 128-k chunks of 96 bytes"""
    return 96 * ((K + 127) // 128)


def quantize_mxfp6(w, codes, scales, row0: int = 0):
    """the MXFP6 operand of a weight (enh_mxfp6_quantize): w [N, K] f32, K % 32 == 0, rows contiguous (any row stride that keeps them 16-byte
    aligned) -> rows row0 .. row0 + N - 1 of codes [Nt, 96 ceil(K / 128)] uint8 (e2m3 codes, 128-k chunks of 96 bytes in the product's order;
    include/enh_hip.h) and scales [Nt, K / 32] uint8 (E8M0); the other rows are not touched"""
    if w.dim() != 2 or codes.dim() != 2 or scales.dim() != 2:
        raise RuntimeError(f"quantize_mxfp6: w {tuple(w.shape)} codes {tuple(codes.shape)} scales {tuple(scales.shape)} must be matrices")
    N, K = w.shape
    if (K % MX_BLOCK or codes.shape[1] != mxfp6_row_bytes(K) or tuple(scales.shape) != (codes.shape[0], K // MX_BLOCK) or row0 < 0
            or row0 + N > codes.shape[0]):
        raise RuntimeError(f"quantize_mxfp6: w {tuple(w.shape)} codes {tuple(codes.shape)} scales {tuple(scales.shape)} row0 {row0} do not fit "
                           f"(K must be a multiple of {MX_BLOCK}, codes [rows, 96 ceil(K / 128)], scales [rows, K / {MX_BLOCK}])")
    if not w.is_cuda or w.dtype != F32 or (K > 1 and w.stride(1) != 1):
        raise RuntimeError(f"quantize_mxfp6: w must be an f32 device tensor whose rows are contiguous, got {w.dtype} on {w.device} strides {w.stride()}")
    stride = w.stride(0) if N > 1 else K
    # bytes moved: the masters once, the codes and the scales
    _timed(None, 4.0 * N * K + N * mxfp6_row_bytes(K) + N * (K // MX_BLOCK),
           lambda: _check(lib().enh_mxfp6_quantize(ctypes.c_void_p(w.data_ptr()), N, K, int(stride), _p(codes, U8, "codes"), int(row0),
                                                   _p(scales, U8, "scales"), int(row0), _stream()), "enh_mxfp6_quantize"), unit="byte")


def skinny_gemm_w6(x, codes, scales, out, bias=None, relu_sq: bool = False, res=None):
    """skinny_gemm with the weight given as its MXFP6 operand (enh_skinny_gemm_w6): out[M,N] = act(x[M,K] dequant(codes, scales)^T + bias) (+ res);
    x 16-bit, codes [N, 96 ceil(K / 128)] uint8, scales [N, K / 32] uint8, M <= 64, N % 8 == 0, K % 32 == 0; out f32 or x's 16-bit format"""
    M, K = x.shape
    N = codes.shape[0]
    if (codes.dim() != 2 or K % MX_BLOCK or codes.shape[1] != mxfp6_row_bytes(K) or tuple(scales.shape) != (N, K // MX_BLOCK)
            or tuple(out.shape) != (M, N) or (res is not None and tuple(res.shape) != (M, N)) or (bias is not None and bias.numel() != N)):
        raise RuntimeError(f"skinny_gemm_w6: x {tuple(x.shape)} codes {tuple(codes.shape)} scales {tuple(scales.shape)} out {tuple(out.shape)} do not fit "
                           f"(K must be a multiple of {MX_BLOCK}, codes [N, 96 ceil(K / 128)], scales [N, K / {MX_BLOCK}])")
    L = lib()
    nb = L.enh_skinny_gemm_w6_workspace_bytes(M, N, K)
    ws = _workspace(nb, x.device) if nb else None
    o32, o16 = (out, None) if out.dtype == F32 else (None, out)
    # bytes moved: the codes and the scales once, x, the result
    _timed(None, float(N) * mxfp6_row_bytes(K) + float(N) * (K // MX_BLOCK) + 2.0 * M * K + float(out.element_size()) * M * N,
           lambda: _check(L.enh_skinny_gemm_w6(_p(x, H16, "x"), _p(codes, U8, "codes"), _p(scales, U8, "scales"), M, N, K, _p(bias, F32, "bias"),
                                               ACT_RELU_SQ if relu_sq else 0, _p(res, F32, "res"), _p(o32, F32, "out"), _p(o16, H16, "out"), _p(ws), nb,
                                               _dt(x, o16), _stream()), "enh_skinny_gemm_w6"), unit="byte")


def decode_attention(qkv, k_cache, v_cache, t: int, out):
    """one token per (batch, head): appends the step's k / v at slot t of k_cache / v_cache [B,H,Tmax,hs] and writes
    out[B,C] = softmax(q K[0..t]^T / sqrt(hs)) V[0..t]; qkv [B,3C], caches and out share one dtype (bf16 | fp16 | f32)"""
    B, H, Tmax, hs = k_cache.shape
    if tuple(v_cache.shape) != (B, H, Tmax, hs) or tuple(qkv.shape) != (B, 3 * H * hs) or tuple(out.shape) != (B, H * hs):
        raise RuntimeError(f"decode_attention: qkv {tuple(qkv.shape)} caches {tuple(k_cache.shape)} {tuple(v_cache.shape)} out {tuple(out.shape)} do not fit")
    dt = qkv.dtype
    if dt not in _DT_OF:
        raise RuntimeError(f"decode_attention: dtype must be bf16, fp16 or f32, got {dt}")
    L = lib()
    nb = L.enh_decode_attention_workspace_bytes(B, H, hs, Tmax)
    ws = _workspace(nb, qkv.device)
    _timed(None, 2.0 * qkv.element_size() * B * H * (int(t) + 1) * hs,
           lambda: _check(L.enh_decode_attention(_p(qkv, dt, "qkv"), _p(k_cache, dt, "k_cache"), _p(v_cache, dt, "v_cache"), B, H, hs, Tmax, int(t),
                                                 _p(out, dt, "out"), _p(ws), ws.numel(), _DT_OF[dt], _stream()), "enh_decode_attention"), unit="byte")


def _kv8_shapes(who: str, qkv, k_codes, k_scales, v_codes, v_scales, out):
    """(B, H, Tmax, hs, dtype) of a decode attention over MXFP8 caches, or a RuntimeError: codes [B,H,Tmax,hs] and scales [B,H,Tmax,hs/32] uint8,
    qkv [B,3C] and out [B,C] in one 16-bit format"""
    if k_codes.dim() != 4:
        raise RuntimeError(f"{who}: k_codes {tuple(k_codes.shape)} must be [B, H, Tmax, hs]")
    B, H, Tmax, hs = k_codes.shape
    if (tuple(v_codes.shape) != (B, H, Tmax, hs) or hs % MX_BLOCK or tuple(k_scales.shape) != (B, H, Tmax, hs // MX_BLOCK)
            or tuple(v_scales.shape) != (B, H, Tmax, hs // MX_BLOCK) or tuple(qkv.shape) != (B, 3 * H * hs) or tuple(out.shape) != (B, H * hs)):
        raise RuntimeError(f"{who}: qkv {tuple(qkv.shape)} codes {tuple(k_codes.shape)} {tuple(v_codes.shape)} scales {tuple(k_scales.shape)} "
                           f"{tuple(v_scales.shape)} out {tuple(out.shape)} do not fit (scales [B, H, Tmax, hs / {MX_BLOCK}])")
    dt = qkv.dtype
    if dt not in H16:
        raise RuntimeError(f"{who}: qkv and out must be bf16 or fp16 (the exact f32 mode has no MXFP8 cache), got {dt}")
    return B, H, Tmax, hs, dt


def decode_attention_kv8(qkv, k_codes, k_scales, v_codes, v_scales, t: int, out):
    """decode_attention over an MXFP8 cache (enh_decode_attention_kv8): quantizes the step's k / v rows, appends their codes and scales at slot t
    of k_codes / v_codes [B,H,Tmax,hs] and k_scales / v_scales [B,H,Tmax,hs/32] (uint8) and writes out[B,C] = softmax(q K[0..t]^T / sqrt(hs)) V[0..t]
    over the dequantized cache, slot t included; qkv [B,3C] and out bf16 | fp16"""
    B, H, Tmax, hs, dt = _kv8_shapes("decode_attention_kv8", qkv, k_codes, k_scales, v_codes, v_scales, out)
    L = lib()
    ws = _workspace(L.enh_decode_attention_workspace_bytes(B, H, hs, Tmax), qkv.device)
    # bytes moved: the codes and the scales of slots 0 .. t of both caches
    _timed(None, 2.0 * B * H * (int(t) + 1) * (hs + hs // MX_BLOCK),
           lambda: _check(L.enh_decode_attention_kv8(_p(qkv, dt, "qkv"), _p(k_codes, U8, "k_codes"), _p(k_scales, U8, "k_scales"), _p(v_codes, U8, "v_codes"),
                                                     _p(v_scales, U8, "v_scales"), B, H, hs, Tmax, int(t), _p(out, dt, "out"), _p(ws), ws.numel(),
                                                     _DT_OF[dt], _stream()), "enh_decode_attention_kv8"), unit="byte")


def kv_cache_fill(qkv, S: int, k_cache, v_cache, slot0: int = 0):
    """the k and v columns of row (b, s) of the packed qkv [B S, 3C] copied bit for bit to slot slot0 + s of k_cache / v_cache [B,H,Tmax,hs]
    (enh_kv_cache_fill): what S decode_attention calls append, in one launch; one dtype (bf16 | fp16 | f32); other slots are not touched"""
    if k_cache.dim() != 4:
        raise RuntimeError(f"kv_cache_fill: k_cache {tuple(k_cache.shape)} must be [B, H, Tmax, hs]")
    B, H, Tmax, hs = k_cache.shape
    dt = qkv.dtype
    if tuple(v_cache.shape) != (B, H, Tmax, hs) or tuple(qkv.shape) != (B * int(S), 3 * H * hs) or k_cache.dtype != dt or v_cache.dtype != dt:
        raise RuntimeError(f"kv_cache_fill: qkv {tuple(qkv.shape)} {dt} caches {tuple(k_cache.shape)} {tuple(v_cache.shape)} {k_cache.dtype} do not fit S={S}")
    if dt not in _DT_OF:
        raise RuntimeError(f"kv_cache_fill: dtype must be bf16, fp16 or f32, got {dt}")
    # bytes moved: the k and v columns read and written once
    _timed(None, 4.0 * qkv.element_size() * B * int(S) * H * hs,
           lambda: _check(lib().enh_kv_cache_fill(_p(qkv, dt, "qkv"), B, int(S), H, hs, Tmax, int(slot0), _p(k_cache, dt, "k_cache"), _p(v_cache, dt, "v_cache"),
                                                  _DT_OF[dt], _stream()), "enh_kv_cache_fill"), unit="byte")


def kv_cache_fill_kv8(qkv, S: int, k_codes, k_scales, v_codes, v_scales, slot0: int = 0):
    """kv_cache_fill into an MXFP8 cache (enh_kv_cache_fill_kv8): row (b, s) of qkv [B S, 3C] (bf16 | fp16) is quantized as decode_attention_kv8's
    append quantizes it and its codes and scales go to slot slot0 + s; the dequantized values are written back over the k and v columns of qkv"""
    if k_codes.dim() != 4:
        raise RuntimeError(f"kv_cache_fill_kv8: k_codes {tuple(k_codes.shape)} must be [B, H, Tmax, hs]")
    B, H, Tmax, hs = k_codes.shape
    if (tuple(v_codes.shape) != (B, H, Tmax, hs) or hs % MX_BLOCK or tuple(k_scales.shape) != (B, H, Tmax, hs // MX_BLOCK)
            or tuple(v_scales.shape) != (B, H, Tmax, hs // MX_BLOCK) or tuple(qkv.shape) != (B * int(S), 3 * H * hs)):
        raise RuntimeError(f"kv_cache_fill_kv8: qkv {tuple(qkv.shape)} codes {tuple(k_codes.shape)} {tuple(v_codes.shape)} scales {tuple(k_scales.shape)} "
                           f"{tuple(v_scales.shape)} do not fit S={S} (scales [B, H, Tmax, hs / {MX_BLOCK}])")
    dt = qkv.dtype
    if dt not in H16:
        raise RuntimeError(f"kv_cache_fill_kv8: qkv must be bf16 or fp16 (the exact f32 mode has no MXFP8 cache), got {dt}")
    # bytes moved: the k and v columns read and written back, the codes and the scales written
    _timed(None, 2.0 * B * int(S) * H * (4 * hs + hs + hs // MX_BLOCK),
           lambda: _check(lib().enh_kv_cache_fill_kv8(_p(qkv, dt, "qkv"), B, int(S), H, hs, Tmax, int(slot0), _p(k_codes, U8, "k_codes"),
                                                      _p(k_scales, U8, "k_scales"), _p(v_codes, U8, "v_codes"), _p(v_scales, U8, "v_scales"), _DT_OF[dt],
                                                      _stream()), "enh_kv_cache_fill_kv8"), unit="byte")


def row_ln_scale(x, w, b, out, colscale=None, eps: float = 1e-5):
    """out = LayerNorm(x) (* colscale): x [M,D] f32, M <= 64, D % 8 == 0 up to 8192; out f32 or 16-bit"""
    M, D = x.shape
    o32, o16 = (out, None) if out.dtype == F32 else (None, out)
    _check(lib().enh_row_ln_scale(_p(x, F32, "x"), _p(w, F32, "w"), _p(b, F32, "b"), _p(colscale, F32, "colscale"), M, D, eps, _p(o32, F32, "out"),
                                  _p(o16, H16, "out"), _dt(o16), _stream()), "enh_row_ln_scale")


def gpt_embed(table, ids, pos_row, out):
    """out[b] = table[ids[b]] + pos_row; ids: an int64 device tensor view with one element per row (any stride, e.g. codes[:, t])"""
    B, C = out.shape
    if not ids.is_cuda or ids.dtype != I64 or ids.dim() != 1 or ids.numel() != B:
        raise RuntimeError("gpt_embed: ids must be a 1-D int64 tensor on the device, one per output row")
    stride = ids.stride(0) if B > 1 else 1
    _check(lib().enh_gpt_embed(_p(table, F32, "table"), ctypes.c_void_p(ids.data_ptr()), max(int(stride), 1), _p(pos_row, F32, "pos_row"), B, C,
                               table.shape[0], _p(out, F32, "out"), _stream()), "enh_gpt_embed")


def skinny_gemm_f32(x, w, out, bias=None, relu_sq: bool = False, res=None):
    """the exact mode's skinny_gemm: every tensor f32 (enh_skinny_gemm_f32)"""
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or tuple(out.shape) != (M, N) or (res is not None and tuple(res.shape) != (M, N)) or (bias is not None and bias.numel() != N):
        raise RuntimeError(f"skinny_gemm_f32: x {tuple(x.shape)} w {tuple(w.shape)} out {tuple(out.shape)} do not fit")
    _check(lib().enh_skinny_gemm_f32(_p(x, F32, "x"), _p(w, F32, "w"), M, N, K, _p(bias, F32, "bias"), ACT_RELU_SQ if relu_sq else 0, _p(res, F32, "res"),
                                     _p(out, F32, "out"), _stream()), "enh_skinny_gemm_f32")


def sample_logits(logits, codes_col, temperature: float = 1.0, top_k=None, top_p=None, uniforms=None, seed: int = 0, call: int = 0, step: int = 0,
                  row0: int = 0, logits_out=None, mask_out=None, probs_out=None):
    """GPT.sample's filter and draw (enh_sample_logits).  logits [B,V] f32; codes_col: an int64 view with one element per row (e.g. codes[:, t]);
    logits_out: an f32 view [B,V] whose rows are contiguous (e.g. logits[:, t*V:(t+1)*V]); mask_out uint8 [B,V]; probs_out f32 [B,V]"""
    B, V = logits.shape
    if not codes_col.is_cuda or codes_col.dtype != I64 or codes_col.numel() != B:
        raise RuntimeError("sample_logits: codes_col must be an int64 device view with one element per row")
    lo_ptr, lo_stride = None, 0
    if logits_out is not None:
        if not logits_out.is_cuda or logits_out.dtype != F32 or tuple(logits_out.shape) != (B, V) or logits_out.stride(1) != 1:
            raise RuntimeError("sample_logits: logits_out must be an f32 device view [B,V] with contiguous rows")
        lo_ptr, lo_stride = ctypes.c_void_p(logits_out.data_ptr()), (logits_out.stride(0) if B > 1 else V)
    _check(lib().enh_sample_logits(_p(logits, F32, "logits"), B, V, float(temperature), int(top_k) if top_k is not None else 0,
                                   float(top_p) if top_p is not None else -1.0, _p(uniforms, F32, "uniforms"), int(seed) & (2 ** 64 - 1), int(call), int(step),
                                   int(row0), ctypes.c_void_p(codes_col.data_ptr()), max(int(codes_col.stride(0)) if B > 1 else 1, 1), lo_ptr, lo_stride,
                                   _p(mask_out, torch.uint8, "mask_out"), _p(probs_out, F32, "probs_out"), _stream()), "enh_sample_logits")


# ------------------------------------------------------------------------------------------------
# stage-2 teacher-forced forward: sequence-shaped kernels (csrc/gpt_prefill.hip: the attention; the row kernels: csrc/gpt_rows.hip)
# ------------------------------------------------------------------------------------------------
def causal_attention(qkv, B: int, N: int, H: int, D: int, out, lse=None, scale: Optional[float] = None):
    """out [B,N,H*D] = causal softmax attention of the packed qkv [B,N,3*H*D]; 16-bit tensors run the MFMA kernel, f32 tensors the exact mode's
    instrument; lse [B,H,N] f32 optional; scale defaults to D ** -0.5"""
    scale = float(D) ** -0.5 if scale is None else float(scale)
    if qkv.numel() != B * N * 3 * H * D or out.numel() != B * N * H * D or (lse is not None and lse.numel() != B * H * N):
        raise RuntimeError(f"causal_attention: qkv {tuple(qkv.shape)} out {tuple(out.shape)} do not fit B={B} N={N} H={H} D={D}")
    L = lib()
    if qkv.dtype == F32:
        _check(L.enh_causal_attention_forward_f32(_p(qkv, F32, "qkv"), B, N, H, D, scale, _p(out, F32, "out"), _p(lse, F32, "lse"), _stream()),
               "enh_causal_attention_forward_f32")
        return
    # executed MFMA work: the score product over D and P V over D, on the lower triangle
    _timed(None, 2.0 * B * H * N * (N + 1) * D,
           lambda: _check(L.enh_causal_attention_forward(_p(qkv, H16, "qkv"), B, N, H, D, scale, _p(out, H16, "out"), _p(lse, F32, "lse"), _dt(qkv, out),
                                                         _stream()), "enh_causal_attention_forward"))


def ln_timeshift(x, w, b, out, S: int, colscale=None, eps: float = 1e-5, out_f32=None):
    """out = LayerNorm(x) [* colscale + LayerNorm(previous row of the same sequence) * (1 - colscale)]: x [M,D] f32, M whole sequences of S rows;
    out f32 or 16-bit; out_f32: an f32 copy beside a 16-bit out"""
    M, D = x.shape
    o32, o16 = (out, None) if out.dtype == F32 else (out_f32, out)
    _check(lib().enh_ln_timeshift(_p(x, F32, "x"), _p(w, F32, "w"), _p(b, F32, "b"), _p(colscale, F32, "colscale"), M, int(S), D, eps, _p(o32, F32, "out"),
                                  _p(o16, H16, "out"), _dt(o16), _stream()), "enh_ln_timeshift")


def gpt_embed_seq(conds, codes, tok_cond, pos_cond, tok_code, pos_code, out):
    """out [B,S,C] f32: the condition row and the first S - 1 codes of every row of codes [B,T] (int64, contiguous rows), S <= T + 1"""
    B, S, C = out.shape
    if conds.dtype != I64 or conds.numel() != B or codes.dtype != I64 or codes.dim() != 2 or codes.shape[0] != B or codes.shape[1] < S - 1 or codes.stride(1) != 1:
        raise RuntimeError("gpt_embed_seq: conds [B] and codes [B,T >= S-1] must be int64 device tensors with contiguous rows")
    _check(lib().enh_gpt_embed_seq(_p(conds, I64, "conds"), ctypes.c_void_p(codes.data_ptr()), codes.stride(0) if B > 1 else codes.shape[1],
                                   _p(tok_cond, F32, "tok_cond"), _p(pos_cond, F32, "pos_cond"), _p(tok_code, F32, "tok_code"), _p(pos_code, F32, "pos_code"),
                                   B, S, C, tok_cond.shape[0], tok_code.shape[0], _p(out, F32, "out"), _stream()), "enh_gpt_embed_seq")


def relu_sq(y, x=None):
    """y = square(relu(x)) (x f32, y 16-bit or f32), or in place on y when x is None"""
    if y.dtype not in _DT_OF or (x is not None and x.numel() != y.numel()):
        raise RuntimeError("relu_sq: y must be bf16, fp16 or f32 and x as long as y")
    _check(lib().enh_relu_sq_h16(_p(x, F32, "x"), _p(y, y.dtype, "y"), y.numel(), _DT_OF[y.dtype], _stream()), "enh_relu_sq_h16")


def cross_entropy_rows(logits, target, nll, mean=None):
    """nll[m] = logsumexp(logits[m]) - logits[m, target[m]]: logits [M,V] f32, target [M] int64, nll [M] f32; mean [1] f32 optional"""
    M, V = logits.shape
    if target.numel() != M or nll.numel() != M:
        raise RuntimeError("cross_entropy_rows: one target and one result per row")
    _check(lib().enh_cross_entropy_rows(_p(logits, F32, "logits"), _p(target, I64, "target"), M, V, _p(nll, F32, "nll"), _p(mean, F32, "mean"), _stream()),
           "enh_cross_entropy_rows")


def mean_f32(v, mean):
    _check(lib().enh_mean_f32(_p(v, F32, "v"), v.numel(), _p(mean, F32, "mean"), _stream()), "enh_mean_f32")


# ------------------------------------------------------------------------------------------------
# stage-2 RQTransformer forward (csrc/rq_prefill.hip): the embedding stage, the strided LayerNorm and the short-sequence attention
# ------------------------------------------------------------------------------------------------
def rq_embed_seq(conds, codes, tok_cond, pos_cond, tok_code, pos_code, pos_depth, spatial, depth):
    """spatial [B,T,C] f32 (the condition row, then the depth sums of positions 0 .. T - 2) and slots 1 .. D - 1 of depth [B*T,D,C] f32 (the running
    sums) from conds [B] and codes [B,T,D] (int64, contiguous); pos_code [>= T - 1, C], pos_depth [D - 1, C]; slot 0 of depth is left alone"""
    B, T, C = spatial.shape
    if conds.dtype != I64 or conds.numel() != B or codes.dtype != I64 or codes.dim() != 3 or tuple(codes.shape[:2]) != (B, T):
        raise RuntimeError("rq_embed_seq: conds [B] and codes [B,T,D] must be int64 device tensors")
    D = codes.shape[2]
    if tuple(depth.shape) != (B * T, D, C) or pos_code.shape[0] < T - 1 or pos_code.shape[-1] != C or tuple(pos_depth.shape) != (D - 1, C) \
            or tok_cond.shape[1] != C or tok_code.shape[1] != C or pos_cond.numel() != C:
        raise RuntimeError(f"rq_embed_seq: depth {tuple(depth.shape)}, pos_code {tuple(pos_code.shape)}, pos_depth {tuple(pos_depth.shape)} do not fit "
                           f"B={B} T={T} D={D} C={C}")
    _check(lib().enh_rq_embed_seq(_p(conds, I64, "conds"), _p(codes, I64, "codes"), _p(tok_cond, F32, "tok_cond"), _p(pos_cond, F32, "pos_cond"),
                                  _p(tok_code, F32, "tok_code"), _p(pos_code, F32, "pos_code"), _p(pos_depth, F32, "pos_depth"), B, T, D, C,
                                  tok_cond.shape[0], tok_code.shape[0], _p(spatial, F32, "spatial"), _p(depth, F32, "depth"), _stream()), "enh_rq_embed_seq")


def ln_rows_strided(x, w, b, out, out_stride: int, eps: float = 1e-5):
    """row m of LayerNorm(x [M,D] f32) written at out.view(-1)[m * out_stride:][:D]: `out` is any contiguous f32 tensor that holds those rows"""
    M, D = x.shape
    if w.numel() != D or b.numel() != D or out.numel() < (M - 1) * int(out_stride) + D:
        raise RuntimeError(f"ln_rows_strided: x {tuple(x.shape)} with row stride {out_stride} does not fit out {tuple(out.shape)}")
    _check(lib().enh_ln_rows_strided(_p(x, F32, "x"), _p(w, F32, "w"), _p(b, F32, "b"), M, D, eps, _p(out, F32, "out"), int(out_stride), _stream()),
           "enh_ln_rows_strided")


def short_causal_attention(qkv, NSEQ: int, L: int, H: int, D: int, out, lse=None, scale: Optional[float] = None):
    """out [NSEQ,L,H*D] = causal softmax attention of NSEQ sequences of L <= 8 tokens, qkv packed [NSEQ,L,3*H*D]; 16-bit tensors of one format;
    lse [NSEQ,H,L] f32 optional; scale defaults to D ** -0.5"""
    scale = float(D) ** -0.5 if scale is None else float(scale)
    if qkv.numel() != NSEQ * L * 3 * H * D or out.numel() != NSEQ * L * H * D or (lse is not None and lse.numel() != NSEQ * H * L):
        raise RuntimeError(f"short_causal_attention: qkv {tuple(qkv.shape)} out {tuple(out.shape)} do not fit NSEQ={NSEQ} L={L} H={H} D={D}")
    L_ = lib()
    # algorithmic HBM bytes: q, k and v read once, out written once
    _timed(None, 8.0 * NSEQ * L * H * D,
           lambda: _check(L_.enh_short_causal_attention_forward(_p(qkv, H16, "qkv"), NSEQ, L, H, D, scale, _p(out, H16, "out"), _p(lse, F32, "lse"),
                                                                _dt(qkv, out), _stream()), "enh_short_causal_attention_forward"), unit="byte")


# ------------------------------------------------------------------------------------------------
# stage-2 backward (csrc/gpt_attn_bwd.hip: the attention; the row kernels: csrc/gpt_rows.hip)
# ------------------------------------------------------------------------------------------------
def causal_attention_backward(qkv, out, dout, lse, B: int, N: int, H: int, D: int, dqkv, scale: Optional[float] = None):
    """dqkv [B,N,3*H*D] of causal_attention from qkv, the out and lse [B,H,N] it stored, and dout [B,N,H*D]; 16-bit tensors of one format"""
    scale = float(D) ** -0.5 if scale is None else float(scale)
    if qkv.numel() != B * N * 3 * H * D or dqkv.numel() != qkv.numel() or out.numel() != B * N * H * D or dout.numel() != out.numel() or lse.numel() != B * H * N:
        raise RuntimeError(f"causal_attention_backward: qkv {tuple(qkv.shape)} out {tuple(out.shape)} dout {tuple(dout.shape)} lse {tuple(lse.shape)} "
                           f"do not fit B={B} N={N} H={H} D={D}")
    L = lib()
    nb = L.enh_causal_attention_backward_workspace_bytes(B, N, H)
    ws = _workspace(nb, qkv.device)
    # MFMA work of an unsplit kernel on the lower triangle: S and dP twice (both kernels), dQ, dK, dV
    _timed(None, 7.0 * B * H * N * (N + 1) * D,
           lambda: _check(L.enh_causal_attention_backward(_p(qkv, H16, "qkv"), _p(out, H16, "out"), _p(dout, H16, "dout"), _p(lse, F32, "lse"), B, N, H, D, scale,
                                                          _p(dqkv, H16, "dqkv"), _p(ws), ws.numel(), _dt(qkv, out, dout, dqkv), _stream()),
                          "enh_causal_attention_backward"))


def cross_entropy_backward(logits, target, nll, dlogits, gscale: float, gscale_dev=None):
    """nll[m] as cross_entropy_rows (the same bits) and dlogits [M,V] 16-bit = (softmax(logits[m]) - onehot(target[m])) * gscale; V % 8 == 0.
    gscale_dev (device f32 [1], optional) multiplies gscale: a loss scale that lives on the device"""
    M, V = logits.shape
    if target.numel() != M or nll.numel() != M or tuple(dlogits.shape) != (M, V):
        raise RuntimeError("cross_entropy_backward: one target and one result per row, dlogits as the logits")
    _timed(None, 6.0 * M * V, lambda: _check(lib().enh_cross_entropy_backward(_p(logits, F32, "logits"), _p(target, I64, "target"), M, V, float(gscale),
                                                                               _p(nll, F32, "nll"), _p(dlogits, H16, "dlogits"), _dt(dlogits),
                                                                               _p(gscale_dev, F32, "gscale_dev"), _stream()),
                                             "enh_cross_entropy_backward"), unit="byte")


def relu_sq_backward(dy, y, dx):
    """dx (16-bit) = dy (f32) * 2 relu(h), relu(h) = sqrt(y) from the stored 16-bit y = relu(h)^2; n % 8 == 0"""
    if dy.numel() != y.numel() or dx.numel() != y.numel():
        raise RuntimeError("relu_sq_backward: dy, y and dx must be equally long")
    _timed(None, 8.0 * y.numel(), lambda: _check(lib().enh_relu_sq_backward(_p(dy, F32, "dy"), _p(y, H16, "y"), _p(dx, H16, "dx"), y.numel(), _dt(y, dx), _stream()),
                                                 "enh_relu_sq_backward"), unit="byte")


def ln_timeshift_backward(dy, x, w, S: int, dx, dw, db, b=None, colscale=None, dcolscale=None, dres=None, dx16=None, eps: float = 1e-5, accumulate: bool = False):
    """backward of ln_timeshift: dy, x [M,D] f32 -> dx f32 (+ dres), dx16 an optional 16-bit copy; dw, db, dcolscale [D] set or (accumulate) added to"""
    M, D = x.shape
    L = lib()
    nb = L.enh_ln_timeshift_backward_workspace_bytes(M, D)
    ws = _workspace(nb, x.device)
    _timed(None, 4.0 * M * D * (3 + (1 if dres is not None else 0)),
           lambda: _check(L.enh_ln_timeshift_backward(_p(dy, F32, "dy"), _p(x, F32, "x"), _p(w, F32, "w"), _p(b, F32, "b"), _p(colscale, F32, "colscale"),
                                                      _p(dres, F32, "dres"), M, int(S), D, eps, _p(dx, F32, "dx"), _p(dx16, H16, "dx16"), _p(dw, F32, "dw"),
                                                      _p(db, F32, "db"), _p(dcolscale, F32, "dcolscale"), int(accumulate), _p(ws), ws.numel(), _dt(dx16),
                                                      _stream()), "enh_ln_timeshift_backward"), unit="byte")


def gpt_embed_seq_backward(g, conds, codes, dtok_cond, dpos_cond, dtok_code, dpos_code, accumulate: bool = False):
    """gradients of gpt_embed_seq's four tables from g [B,S,C] f32: dtok_cond [Vc,C], dpos_cond [C], dtok_code [V,C], dpos_code [P >= S-1, C]"""
    B, S, C = g.shape
    if conds.dtype != I64 or conds.numel() != B or codes.dtype != I64 or codes.dim() != 2 or codes.shape[0] != B or codes.shape[1] < S - 1 or codes.stride(1) != 1:
        raise RuntimeError("gpt_embed_seq_backward: conds [B] and codes [B,T >= S-1] must be int64 device tensors with contiguous rows")
    _timed(None, 4.0 * (B * S * C + dtok_cond.numel() + dtok_code.numel() + dpos_code.numel() + C),
           lambda: _check(lib().enh_gpt_embed_seq_backward(_p(g, F32, "g"), _p(conds, I64, "conds"), ctypes.c_void_p(codes.data_ptr()),
                                                           codes.stride(0) if B > 1 else codes.shape[1], B, S, C, dtok_cond.shape[0], dtok_code.shape[0],
                                                           dpos_code.shape[0], _p(dtok_cond, F32, "dtok_cond"), _p(dpos_cond, F32, "dpos_cond"),
                                                           _p(dtok_code, F32, "dtok_code"), _p(dpos_code, F32, "dpos_code"), int(accumulate), _stream()),
                          "enh_gpt_embed_seq_backward"), unit="byte")


# ------------------------------------------------------------------------------------------------
# stage-2 RQTransformer backward (csrc/rq_backward.hip; the strided LayerNorm backward: csrc/gpt_rows.hip)
# ------------------------------------------------------------------------------------------------
def short_causal_attention_backward(qkv, out, dout, lse, NSEQ: int, L: int, H: int, D: int, dqkv, scale: Optional[float] = None):
    """dqkv [NSEQ,L,3*H*D] of short_causal_attention from qkv, the out and lse [NSEQ,H,L] it stored, and dout [NSEQ,L,H*D]; 16-bit tensors of one
    format; L <= 8"""
    scale = float(D) ** -0.5 if scale is None else float(scale)
    if qkv.numel() != NSEQ * L * 3 * H * D or dqkv.numel() != qkv.numel() or out.numel() != NSEQ * L * H * D or dout.numel() != out.numel() \
            or lse.numel() != NSEQ * H * L:
        raise RuntimeError(f"short_causal_attention_backward: qkv {tuple(qkv.shape)} out {tuple(out.shape)} dout {tuple(dout.shape)} lse {tuple(lse.shape)} "
                           f"do not fit NSEQ={NSEQ} L={L} H={H} D={D}")
    L_ = lib()
    # algorithmic HBM bytes: q, k, v, out and dout read once, dq, dk and dv written once
    _timed(None, 16.0 * NSEQ * L * H * D,
           lambda: _check(L_.enh_short_causal_attention_backward(_p(qkv, H16, "qkv"), _p(out, H16, "out"), _p(dout, H16, "dout"), _p(lse, F32, "lse"), NSEQ, L, H,
                                                                 D, scale, _p(dqkv, H16, "dqkv"), _dt(qkv, out, dout, dqkv), _stream()),
                          "enh_short_causal_attention_backward"), unit="byte")


def ln_rows_strided_backward(dy, dy_stride: int, x, w, dx, dw, db, dx16=None, eps: float = 1e-5, accumulate: bool = False):
    """backward of ln_rows_strided: row m of dy is dy.view(-1)[m * dy_stride:][:D] (`dy` any contiguous f32 tensor that holds those rows; nothing
    between them is read), x [M,D] f32 -> dx f32 [M,D], dx16 an optional 16-bit copy; dw, db [D] set or (accumulate) added to"""
    M, D = x.shape
    if w.numel() != D or dw.numel() != D or db.numel() != D or dx.numel() != M * D or dy.numel() < (M - 1) * int(dy_stride) + D \
            or (dx16 is not None and dx16.numel() != M * D):
        raise RuntimeError(f"ln_rows_strided_backward: x {tuple(x.shape)} with row stride {dy_stride} does not fit dy {tuple(dy.shape)}, dx {tuple(dx.shape)}")
    L = lib()
    nb = L.enh_ln_timeshift_backward_workspace_bytes(M, D)
    ws = _workspace(nb, x.device)
    _timed(None, 4.0 * M * D * 3,
           lambda: _check(L.enh_ln_rows_strided_backward(_p(dy, F32, "dy"), int(dy_stride), _p(x, F32, "x"), _p(w, F32, "w"), M, D, eps, _p(dx, F32, "dx"),
                                                         _p(dx16, H16, "dx16"), _p(dw, F32, "dw"), _p(db, F32, "db"), int(accumulate), _p(ws), ws.numel(),
                                                         _dt(dx16), _stream()), "enh_ln_rows_strided_backward"), unit="byte")


def rq_embed_seq_backward(gs, gd, conds, codes, dtok_cond, dpos_cond, dtok_code, dpos_code, dpos_depth, accumulate: bool = False):
    """gradients of rq_embed_seq's five tables from gs [B,T,C] and gd [B*T,D,C] f32 (slot 0 of gd is not read): dtok_cond [Vc,C], dpos_cond [C],
    dtok_code [V,C], dpos_code [P >= T-1, C], dpos_depth [D-1, C]; conds [B], codes [B,T,D] int64 contiguous"""
    B, T, C = gs.shape
    if conds.dtype != I64 or conds.numel() != B or codes.dtype != I64 or codes.dim() != 3 or tuple(codes.shape[:2]) != (B, T):
        raise RuntimeError("rq_embed_seq_backward: conds [B] and codes [B,T,D] must be int64 device tensors")
    D = codes.shape[2]
    if tuple(gd.shape) != (B * T, D, C) or dpos_code.dim() != 2 or dpos_code.shape[0] < T - 1 or dpos_code.shape[1] != C or tuple(dpos_depth.shape) != (D - 1, C) \
            or dtok_cond.shape[1] != C or dtok_code.shape[1] != C or dpos_cond.numel() != C:
        raise RuntimeError(f"rq_embed_seq_backward: gd {tuple(gd.shape)}, dpos_code {tuple(dpos_code.shape)}, dpos_depth {tuple(dpos_depth.shape)} do not fit "
                           f"B={B} T={T} D={D} C={C}")
    _timed(None, 4.0 * (B * T * D * C + dtok_cond.numel() + dtok_code.numel() + dpos_code.numel() + dpos_depth.numel() + C),
           lambda: _check(lib().enh_rq_embed_seq_backward(_p(gs, F32, "gs"), _p(gd, F32, "gd"), _p(conds, I64, "conds"), _p(codes, I64, "codes"), B, T, D, C,
                                                          dtok_cond.shape[0], dtok_code.shape[0], dpos_code.shape[0], _p(dtok_cond, F32, "dtok_cond"),
                                                          _p(dpos_cond, F32, "dpos_cond"), _p(dtok_code, F32, "dtok_code"), _p(dpos_code, F32, "dpos_code"),
                                                          _p(dpos_depth, F32, "dpos_depth"), int(accumulate), _stream()),
                          "enh_rq_embed_seq_backward"), unit="byte")


# ------------------------------------------------------------------------------------------------
# stage-2 RQTransformer sampling (csrc/rq_decode.hip): a step's input row from the codes on the device, the decode attention over a short cache
# ------------------------------------------------------------------------------------------------
def rq_embed_step(table, ids, pos_row, out):
    """out[b] = (((e_0 + e_1) + ...) + e_{n-1}) + pos_row, e_j = table[ids[b, j]]: ids an int64 device view [B, n], 1 <= n <= 8, whose rows are
    contiguous (any row stride, e.g. codes[:, t - 1, :] or codes[:, t, :d] of the sampler's [B, T, D] codes); table [V,C], pos_row [C], out [B,C] f32"""
    B, C = out.shape
    if not ids.is_cuda or ids.dtype != I64 or ids.dim() != 2 or ids.shape[0] != B:
        raise RuntimeError("rq_embed_step: ids must be a 2-D int64 tensor on the device, one row of n ids per output row")
    n = ids.shape[1]
    if n > 1 and ids.stride(1) != 1:
        raise RuntimeError("rq_embed_step: the n ids of a row must be contiguous")
    stride = ids.stride(0) if B > 1 else n
    if table.shape[1] != C or pos_row.numel() != C:
        raise RuntimeError(f"rq_embed_step: table {tuple(table.shape)}, pos_row {tuple(pos_row.shape)} do not fit out {tuple(out.shape)}")
    _check(lib().enh_rq_embed_step(_p(table, F32, "table"), ctypes.c_void_p(ids.data_ptr()), int(stride), n, _p(pos_row, F32, "pos_row"), B, C,
                                   table.shape[0], _p(out, F32, "out"), _stream()), "enh_rq_embed_step")


def short_decode_attention(qkv, k_cache, v_cache, t: int, out):
    """decode_attention for caches [B,H,Tmax <= 8,hs] (the depth transformer's): the same arguments and arithmetic contract, eight lanes per
    (row, head) pair, no workspace (enh_short_decode_attention)"""
    B, H, Tmax, hs = k_cache.shape
    if tuple(v_cache.shape) != (B, H, Tmax, hs) or tuple(qkv.shape) != (B, 3 * H * hs) or tuple(out.shape) != (B, H * hs):
        raise RuntimeError(f"short_decode_attention: qkv {tuple(qkv.shape)} caches {tuple(k_cache.shape)} {tuple(v_cache.shape)} out {tuple(out.shape)} do not fit")
    dt = qkv.dtype
    if dt not in _DT_OF:
        raise RuntimeError(f"short_decode_attention: dtype must be bf16, fp16 or f32, got {dt}")
    _timed(None, 2.0 * qkv.element_size() * B * H * (int(t) + 1) * hs,
           lambda: _check(lib().enh_short_decode_attention(_p(qkv, dt, "qkv"), _p(k_cache, dt, "k_cache"), _p(v_cache, dt, "v_cache"), B, H, hs, Tmax, int(t),
                                                           _p(out, dt, "out"), _DT_OF[dt], _stream()), "enh_short_decode_attention"), unit="byte")


# ------------------------------------------------------------------------------------------------
# stage-2 sampling, the cursor forms (csrc/gpt_decode.hip): the loop's position t is a device int32 [1], so the launches of
# one position can be captured into a HIP graph and replayed for the next.  No argument below depends on t.  Not timed per kernel: the graphed
# sampler falls back to the eager loop while TIMER is set.
# ------------------------------------------------------------------------------------------------
def _cursor_ptr(cursor, who: str):
    if not (torch.is_tensor(cursor) and cursor.is_cuda and cursor.dtype == torch.int32 and cursor.numel() == 1):
        raise RuntimeError(f"{who}: cursor must be a device int32 tensor of one element")
    return ctypes.c_void_p(cursor.data_ptr())


def cursor_advance(cursor) -> None:
    """cursor += 1 on the device (enh_cursor_advance)"""
    _check(lib().enh_cursor_advance(_cursor_ptr(cursor, "cursor_advance"), _stream()), "enh_cursor_advance")


def decode_attention_at(qkv, k_cache, v_cache, cursor, out, t_offset: int = 0) -> None:
    """decode_attention at t = cursor + t_offset, read on the device (enh_decode_attention_at): its bits at the same t; t outside the cache:
    nothing is read or written"""
    B, H, Tmax, hs = k_cache.shape
    if tuple(v_cache.shape) != (B, H, Tmax, hs) or tuple(qkv.shape) != (B, 3 * H * hs) or tuple(out.shape) != (B, H * hs):
        raise RuntimeError(f"decode_attention_at: qkv {tuple(qkv.shape)} caches {tuple(k_cache.shape)} {tuple(v_cache.shape)} out {tuple(out.shape)} do not fit")
    dt = qkv.dtype
    if dt not in _DT_OF:
        raise RuntimeError(f"decode_attention_at: dtype must be bf16, fp16 or f32, got {dt}")
    L = lib()
    ws = _workspace(L.enh_decode_attention_workspace_bytes(B, H, hs, Tmax), qkv.device)
    _check(L.enh_decode_attention_at(_p(qkv, dt, "qkv"), _p(k_cache, dt, "k_cache"), _p(v_cache, dt, "v_cache"), B, H, hs, Tmax,
                                     _cursor_ptr(cursor, "decode_attention_at"), int(t_offset), _p(out, dt, "out"), _p(ws), ws.numel(), _DT_OF[dt],
                                     _stream()), "enh_decode_attention_at")


def decode_attention_kv8_at(qkv, k_codes, k_scales, v_codes, v_scales, cursor, out, t_offset: int = 0) -> None:
    """decode_attention_kv8 at t = cursor + t_offset, read on the device (enh_decode_attention_kv8_at): its bits at the same t, in the output and in
    the cache; t outside the cache: nothing is read or written"""
    B, H, Tmax, hs, dt = _kv8_shapes("decode_attention_kv8_at", qkv, k_codes, k_scales, v_codes, v_scales, out)
    L = lib()
    ws = _workspace(L.enh_decode_attention_workspace_bytes(B, H, hs, Tmax), qkv.device)
    _check(L.enh_decode_attention_kv8_at(_p(qkv, dt, "qkv"), _p(k_codes, U8, "k_codes"), _p(k_scales, U8, "k_scales"), _p(v_codes, U8, "v_codes"),
                                         _p(v_scales, U8, "v_scales"), B, H, hs, Tmax, _cursor_ptr(cursor, "decode_attention_kv8_at"), int(t_offset),
                                         _p(out, dt, "out"), _p(ws), ws.numel(), _DT_OF[dt], _stream()), "enh_decode_attention_kv8_at")


def embed_step_at(table, ids, n: int, id_t_stride: int, id_offset: int, pos, pos_t_stride: int, pos_offset: int, cursor, t_lo: int, t_hi: int, out) -> None:
    """the input row of a step at t = cursor (enh_embed_step_at): out[b] = sum_{j < n} table[ids[b].flat[t id_t_stride + id_offset + j]] (ascending j)
    + pos.flat[t pos_t_stride + pos_offset .. + C).  ids: an int64 device view with one row per output row whose rows are contiguous (e.g. the
    sampler's codes [B, T] or [B, T, D], or a chunk of their rows); pos: f32, contiguous (e.g. pos_emb_code[0]).  Every position of [t_lo, t_hi) must
    stay inside a row of ids and inside pos (checked here); outside that range of positions the kernel does nothing."""
    B, C = out.shape
    if not (ids.is_cuda and ids.dtype == I64 and ids.dim() >= 2 and ids.shape[0] == B and ids[0].is_contiguous()):
        raise RuntimeError("embed_step_at: ids must be an int64 device view with one contiguous row per output row")
    if table.shape[1] != C or not 0 <= t_lo < t_hi:
        raise RuntimeError(f"embed_step_at: table {tuple(table.shape)} does not fit out {tuple(out.shape)}, or no position in [{t_lo}, {t_hi})")
    row = ids[0].numel()
    for t in (t_lo, t_hi - 1):
        if not (0 <= t * id_t_stride + id_offset and t * id_t_stride + id_offset + n <= row):
            raise RuntimeError(f"embed_step_at: position {t} reads ids outside a row of {row}")
        if not (0 <= t * pos_t_stride + pos_offset and t * pos_t_stride + pos_offset + C <= pos.numel()):
            raise RuntimeError(f"embed_step_at: position {t} reads outside the {pos.numel()} position values")
    _check(lib().enh_embed_step_at(_p(table, F32, "table"), ctypes.c_void_p(ids.data_ptr()), int(ids.stride(0)) if B > 1 else row, int(id_t_stride),
                                   int(id_offset), int(n), _p(pos, F32, "pos"), int(pos_t_stride), int(pos_offset), _cursor_ptr(cursor, "embed_step_at"),
                                   int(t_lo), int(t_hi), B, C, table.shape[0], _p(out, F32, "out"), _stream()), "enh_embed_step_at")


def sample_logits_at(logits, codes, cursor, step_mul: int = 1, step_add: int = 0, temperature: float = 1.0, top_k=None, top_p=None, seed: int = 0,
                     call: int = 0, row0: int = 0, logits_out=None) -> None:
    """sample_logits at step = cursor * step_mul + step_add (enh_sample_logits_at): the code of row b goes to codes[b].flat[step], the filtered
    logits to logits_out[b].flat[step V .. + V).  codes: an int64 device view with one contiguous row of n_steps codes per row of logits (the
    sampler's [B, T] or [B, T, D]); logits_out: None or an f32 view with one contiguous row of n_steps V values per row.  A step outside
    [0, n_steps) writes nothing."""
    B, V = logits.shape
    if not (codes.is_cuda and codes.dtype == I64 and codes.dim() >= 2 and codes.shape[0] == B and codes[0].is_contiguous()):
        raise RuntimeError("sample_logits_at: codes must be an int64 device view with one contiguous row per row of logits")
    n_steps = codes[0].numel()
    lo_ptr, lo_stride = None, 0
    if logits_out is not None:
        if not (logits_out.is_cuda and logits_out.dtype == F32 and logits_out.dim() >= 2 and logits_out.shape[0] == B and logits_out[0].is_contiguous()
                and logits_out[0].numel() == n_steps * V):
            raise RuntimeError("sample_logits_at: logits_out must be an f32 device view with one contiguous row of n_steps * V values per row")
        lo_ptr, lo_stride = ctypes.c_void_p(logits_out.data_ptr()), (int(logits_out.stride(0)) if B > 1 else n_steps * V)
    _check(lib().enh_sample_logits_at(_p(logits, F32, "logits"), B, V, float(temperature), int(top_k) if top_k is not None else 0,
                                      float(top_p) if top_p is not None else -1.0, int(seed) & (2 ** 64 - 1), int(call),
                                      _cursor_ptr(cursor, "sample_logits_at"), int(step_mul), int(step_add), n_steps, int(row0),
                                      ctypes.c_void_p(codes.data_ptr()), int(codes.stride(0)) if B > 1 else n_steps, lo_ptr, lo_stride, _stream()),
           "enh_sample_logits_at")
