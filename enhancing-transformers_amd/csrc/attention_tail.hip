// attention_tail.hip — the attention kernels for token counts that are no multiple of 64: the text of attention_kernels.h compiled in its tail form
// (see the head of that file), in a translation unit of its own so that the aligned kernels of attention.hip are compiled exactly as before.
#include "attention_common.h"

#define ATT_TAIL 1
#define ATT_K(pass, what) attn_##pass##_tail_##what
#include "attention_kernels.h"

// One kernel per pass and q convention (the tail forms of the default families; forward: of family 1 for plain q), whatever enh_attention_set_kernel selected.
int enh_attention_tail_forward(const enh_h16* qkv, int B, int N, int H, float scale, int q_prescaled, enh_h16* out, float* lse, int dtype, void* stream) {
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H;
  const dim3 grid((unsigned)(((heads + 7) / 8) * 8 * nblk));  // 1-D: see att_block_coords
  enh_note_kernel(q_prescaled ? "attn_fwd_tail_pre_kernel" : "attn_fwd_tail_kernel", dtype);
  if (q_prescaled) ENH_DT_DISPATCH(dtype, (attn_fwd_tail_pre_kernel<OT><<<grid, 256, 0, (hipStream_t)stream>>>(qkv, B, N, H, out, lse)));
  else ENH_DT_DISPATCH(dtype, (attn_fwd_tail_kernel<OT><<<grid, 256, 0, (hipStream_t)stream>>>(qkv, B, N, H, scale * ATT_LOG2E, out, lse)));
  return enh_check_launch("enh_attention_forward");
}

int enh_attention_tail_backward(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse, int B, int N, int H, float scale, int q_prescaled,
                                enh_h16* dqkv, float* delta_ws, int dtype, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H;
  const dim3 grid((unsigned)(((heads + 7) / 8) * 8 * nblk));
  // (scale factors as in enh_attention_backward)
  if (q_prescaled) {
    ENH_DT_DISPATCH(dtype, (attn_bwd_tail_dq_kernel<2, OT><<<grid, 256, 0, s>>>(qkv, out, dout, lse, delta_ws, B, N, H, scale, 1.0f, dqkv)));
    ENH_DT_DISPATCH(dtype, (attn_bwd_tail_dkv_kernel<true, true, OT><<<grid, 256, 0, s>>>(qkv, dout, lse, delta_ws, B, N, H, ATT_LN2, 1.0f, dqkv)));
  } else {
    ENH_DT_DISPATCH(dtype, (attn_bwd_tail_dq_kernel<1, OT><<<grid, 256, 0, s>>>(qkv, out, dout, lse, delta_ws, B, N, H, scale, scale * ATT_LOG2E, dqkv)));
    ENH_DT_DISPATCH(dtype, (attn_bwd_tail_dkv_kernel<true, false, OT><<<grid, 256, 0, s>>>(qkv, dout, lse, delta_ws, B, N, H, scale, scale * ATT_LOG2E, dqkv)));
  }
  return enh_check_launch("enh_attention_backward");
}
