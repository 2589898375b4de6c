// attention_dh.hip — the fused attention with dim_head as an argument: D = 64 forwards to the tuned kernels (attention.hip / attention_tail.hip, kernel
// selection and tail forms included), D = 32 | 96 | 128 launch the kernels of attention_dh.h, anything else is ENH_E_SHAPE.
// Reference: Attention takes dim_head as a constructor argument (enhancing/modules/stage1/layers.py:108-120; ViTEncoder / ViTDecoder pass it on, 154-155,186-187).
#include "attention_dh.h"

#define DH_SUPPORTED(D) ((D) == 32 || (D) == 64 || (D) == 96 || (D) == 128)
// run CALL with the constant `DH` bound to the head width (32 | 96 | 128: checked by the caller) and `OT` to the operand type
#define DH_DISPATCH(D, dtype, CALL)                                            \
  do {                                                                         \
    if ((D) == 32) { constexpr int DH = 32; ENH_DT_DISPATCH(dtype, CALL); }    \
    else if ((D) == 96) { constexpr int DH = 96; ENH_DT_DISPATCH(dtype, CALL); } \
    else { constexpr int DH = 128; ENH_DT_DISPATCH(dtype, CALL); }             \
  } while (0)

extern "C" int enh_attention_forward_dh(const enh_h16* qkv, int B, int N, int H, int D, float scale, int q_prescaled, enh_h16* out, float* lse, int dtype,
                                        void* stream) {
  ENH_REQUIRE(DH_SUPPORTED(D), ENH_E_SHAPE, "enh_attention_forward_dh: dim_head must be 32, 64, 96 or 128, got %d", D);
  if (D == 64) return enh_attention_forward(qkv, B, N, H, scale, q_prescaled, out, lse, dtype, stream);
  ENH_REQUIRE_DT(dtype, "enh_attention_forward_dh");
  ENH_REQUIRE(qkv && out && lse, ENH_E_BADARG, "enh_attention_forward_dh: null pointer");
  ENH_REQUIRE(B > 0 && H > 0 && N > 0, ENH_E_SHAPE, "enh_attention_forward_dh: need positive B, N, H (B=%d N=%d H=%d)", B, N, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_attention_forward_dh: scale must be positive");
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H;
  const dim3 grid((unsigned)(((heads + 7) / 8) * 8 * nblk));  // 1-D: see att_block_coords
  const float sl2 = q_prescaled ? 1.0f : scale * ATT_LOG2E;    // pre-scaled q: the products are log2-domain scores already
  enh_note_kernel_dh("attn_dh_fwd_kernel", D, dtype);
  DH_DISPATCH(D, dtype, (attn_dh_fwd_kernel<DH, OT><<<grid, 256, 0, (hipStream_t)stream>>>(qkv, B, N, H, sl2, out, lse)));
  return enh_check_launch("enh_attention_forward_dh");
}

extern "C" int enh_attention_backward_dh(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse, int B, int N, int H, int D, float scale,
                                         int q_prescaled, enh_h16* dqkv, float* delta_ws, int dtype, void* stream) {
  ENH_REQUIRE(DH_SUPPORTED(D), ENH_E_SHAPE, "enh_attention_backward_dh: dim_head must be 32, 64, 96 or 128, got %d", D);
  if (D == 64) return enh_attention_backward(qkv, out, dout, lse, B, N, H, scale, q_prescaled, dqkv, delta_ws, dtype, stream);
  ENH_REQUIRE_DT(dtype, "enh_attention_backward_dh");
  ENH_REQUIRE(qkv && out && dout && lse && dqkv && delta_ws, ENH_E_BADARG, "enh_attention_backward_dh: null pointer");
  ENH_REQUIRE(B > 0 && H > 0 && N > 0, ENH_E_SHAPE, "enh_attention_backward_dh: need positive B, N, H (B=%d N=%d H=%d)", B, N, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_attention_backward_dh: scale must be positive");
  hipStream_t s = (hipStream_t)stream;
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H;
  const dim3 grid((unsigned)(((heads + 7) / 8) * 8 * nblk));
  const float sl2 = q_prescaled ? 1.0f : scale * ATT_LOG2E;
  // dQ is the gradient with respect to the UNSCALED q in both conventions: factor `scale`.  dK is formed from the q tile as stored: with pre-scaled
  // q' = q * scale * log2e the factor is scale / (scale * log2e) = ln 2 (as enh_attention_backward).
  const float kscale = q_prescaled ? ATT_LN2 : scale;
  DH_DISPATCH(D, dtype, (attn_dh_bwd_dq_kernel<DH, OT><<<grid, 256, 0, s>>>(qkv, out, dout, lse, delta_ws, B, N, H, scale, sl2, dqkv)));
  DH_DISPATCH(D, dtype, (attn_dh_bwd_dkv_kernel<DH, OT><<<grid, 256, 0, s>>>(qkv, dout, lse, delta_ws, B, N, H, kscale, sl2, dqkv)));
  return enh_check_launch("enh_attention_backward_dh");
}
