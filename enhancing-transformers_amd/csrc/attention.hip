// attention.hip — fused (flash-style) multi-head attention forward / backward for gfx950, d_head = 64.
//
// Replaces Attention.forward between to_qkv and to_out (reference enhancing/modules/stage1/layers.py:123-130):
// chunk(3) + 'b n (h d) -> b h n d' + softmax(q k^T * 64^-0.5) v + 'b h n d -> b n (h d)'.  The kernels read the
// packed [B, N, 3*H*64] bf16 QKV GEMM output directly and write the [B, N, H*64] layout to_out consumes, so
// neither einops rearrange nor the N x N score matrix (50 MB fp32 per image per layer at base) ever touches HBM;
// only the row log-sum-exp is saved for backward.
//
// MFMA: v_mfma_f32_32x32x16_bf16 with the product computed "swapped" (S^T = K Q^T): each lane then owns ONE
// query column, so the online-softmax row statistics are lane-local (one cross-half exchange) and the
// probabilities feed the second MFMA straight from registers (the k-slot permutation of the C layout is applied
// to the other operand instead).  Operands contracted over their slow storage index (V in P V, K in dS K,
// dO / Q in the dK / dV products) are read from LDS with ds_read_b64_tr_b16.
//
// Forward / dQ: workgroup = 128 queries (4 waves x 32), K/V streamed in 64-key tiles through a 2-stage LDS ring.
// dK/dV: workgroup = 128 keys (4 waves x 32), Q / dO streamed in 64-query tiles.  dQ and dK/dV are separate
// kernels (S is recomputed twice) so that no atomics are needed and the result is deterministic.
#include "attention_common.h"

// ---- the kernels: attention_kernels.h, compiled here as the aligned kernels (and in attention_tail.hip as their tail forms) -------------------------
#define ATT_TAIL 0
#define ATT_K(pass, what) attn_##pass##_##what
#include "attention_kernels.h"

// =================================================================================================
// C ABI
// =================================================================================================
// kernel family per pass (explicit state behind an explicit call, as enh_gemm_set_kernel); 0 = the library's choice:
//   forward: 1 round-2 kernel | 5 round-2 skeleton with -m_ref as the MFMA C operand, packed row sum, K / V by LDS-DMA (round 5; pre-scaled q only, else family 1)
//   dQ     : 1 round-2 arithmetic | 3 -delta (and, pre-scaled q, -lse) as MFMA C operands
//   dK/dV  : 1 round-2 arithmetic | 2 -delta (and, pre-scaled q, -lse) as MFMA C operands
// (forward 2 / 3, dQ 2: the software-pipelined round-3 kernels; forward 4, dK/dV 3: the eight-wave antiphase kernels of round 4 — all measured slower and deleted;
//  their lab notes stay in profiles/r03_attention_lab.txt, r04_attention_lab.txt.)
// The families are the ALIGNED kernels (N % 64 == 0).  A ragged N has one kernel per pass and q convention — the tail form of the default family (forward:
// of family 1 for plain q; attention_tail.hip) — and runs it whatever is selected here.
static int g_att_fwd = 0, g_att_dq = 0, g_att_dkv = 0;
#define ATT_DEFAULT_FWD 5
#define ATT_DEFAULT_DQ 3
#define ATT_DEFAULT_DKV 2

extern "C" int enh_attention_set_kernel(int fwd, int dq, int dkv) {
  ENH_REQUIRE((fwd == 0 || fwd == 1 || fwd == 5) && (dq == 0 || dq == 1 || dq == 3) && dkv >= 0 && dkv <= 2, ENH_E_BADARG,
              "enh_attention_set_kernel: fwd in {0, 1, 5}, dq in {0, 1, 3}, dkv in 0..2");
  g_att_fwd = fwd; g_att_dq = dq; g_att_dkv = dkv;
  return ENH_OK;
}


extern "C" int enh_attention_forward(const enh_h16* qkv, int B, int N, int H, float scale, int q_prescaled, enh_h16* out, float* lse, int dtype, void* stream) {
  ENH_REQUIRE_DT(dtype, "enh_attention_forward");
  ENH_REQUIRE(qkv && out && lse, ENH_E_BADARG, "enh_attention_forward: null pointer");
  ENH_REQUIRE(B > 0 && H > 0 && N > 0, ENH_E_SHAPE, "enh_attention_forward: need positive B, N, H (B=%d N=%d H=%d)", B, N, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_attention_forward: scale must be positive");
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H;
  const dim3 grid((unsigned)(((heads + 7) / 8) * 8 * nblk));  // 1-D: see att_block_coords
  if (N % 64 != 0) return enh_attention_tail_forward(qkv, B, N, H, scale, q_prescaled, out, lse, dtype, stream);
  int fam = g_att_fwd ? g_att_fwd : ATT_DEFAULT_FWD;
  if (fam == 5 && !q_prescaled) fam = 1;                         // -m_ref as a C operand needs log2-domain products
  const float sl2 = q_prescaled ? 1.0f : scale * ATT_LOG2E;       // pre-scaled q: the products are log2-domain scores already
  enh_note_kernel(fam == 5 ? "attn_fwd_pre_kernel" : "attn_fwd_kernel", dtype);
  if (fam == 5) ENH_DT_DISPATCH(dtype, (attn_fwd_pre_kernel<OT><<<grid, 256, 0, (hipStream_t)stream>>>(qkv, B, N, H, out, lse)));
  else ENH_DT_DISPATCH(dtype, (attn_fwd_kernel<OT><<<grid, 256, 0, (hipStream_t)stream>>>(qkv, B, N, H, sl2, out, lse)));
  return enh_check_launch("enh_attention_forward");
}

extern "C" int enh_attention_backward(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse, int B, int N,
                                      int H, float scale, int q_prescaled, enh_h16* dqkv, float* delta_ws, int dtype, void* stream) {
  ENH_REQUIRE_DT(dtype, "enh_attention_backward");
  ENH_REQUIRE(qkv && out && dout && lse && dqkv && delta_ws, ENH_E_BADARG, "enh_attention_backward: null pointer");
  ENH_REQUIRE(B > 0 && H > 0 && N > 0, ENH_E_SHAPE, "enh_attention_backward: need positive B, N, H (B=%d N=%d H=%d)", B, N, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_attention_backward: scale must be positive");
  if (N % 64 != 0) return enh_attention_tail_backward(qkv, out, dout, lse, B, N, H, scale, q_prescaled, dqkv, delta_ws, dtype, stream);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H;
  const dim3 grid((unsigned)(((heads + 7) / 8) * 8 * nblk));
  const bool pre = q_prescaled != 0;
  const float sl2 = pre ? 1.0f : scale * ATT_LOG2E;
  // dQ is the gradient with respect to the UNSCALED q in both conventions (what the projection's weight / input gradients need): factor `scale`.
  // dK is formed from the q tile as stored: with pre-scaled q' = q * scale * log2e the factor is scale / (scale * log2e) = ln 2.
  const float kscale = pre ? ATT_LN2 : scale;
  // (either dQ kernel also writes delta_ws = rowsum(dO * O) for the dK/dV kernel that follows)
  const int fq = g_att_dq ? g_att_dq : ATT_DEFAULT_DQ;
  const int fk = g_att_dkv ? g_att_dkv : ATT_DEFAULT_DKV;
  if (fq == 1) ENH_DT_DISPATCH(dtype, (attn_bwd_dq_kernel<0, OT><<<grid, 256, 0, s>>>(qkv, out, dout, lse, delta_ws, B, N, H, scale, sl2, dqkv)));
  else if (pre) ENH_DT_DISPATCH(dtype, (attn_bwd_dq_kernel<2, OT><<<grid, 256, 0, s>>>(qkv, out, dout, lse, delta_ws, B, N, H, scale, sl2, dqkv)));
  else ENH_DT_DISPATCH(dtype, (attn_bwd_dq_kernel<1, OT><<<grid, 256, 0, s>>>(qkv, out, dout, lse, delta_ws, B, N, H, scale, sl2, dqkv)));
  if (fk == 1) ENH_DT_DISPATCH(dtype, (attn_bwd_dkv_kernel<false, false, OT><<<grid, 256, 0, s>>>(qkv, dout, lse, delta_ws, B, N, H, kscale, sl2, dqkv)));
  else if (pre) ENH_DT_DISPATCH(dtype, (attn_bwd_dkv_kernel<true, true, OT><<<grid, 256, 0, s>>>(qkv, dout, lse, delta_ws, B, N, H, kscale, sl2, dqkv)));
  else ENH_DT_DISPATCH(dtype, (attn_bwd_dkv_kernel<true, false, OT><<<grid, 256, 0, s>>>(qkv, dout, lse, delta_ws, B, N, H, kscale, sl2, dqkv)));
  return enh_check_launch("enh_attention_backward");
}
