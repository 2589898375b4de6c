// x3_tail.hip — the split-operand attention forward for token counts that are no multiple of 64: x3_attention.h compiled in its tail form, in a
// translation unit of its own (attention_tail.hip says why).
#include "attention_common.h"
typedef BF16 OT;   // as x3.hip

#define ATT_TAIL 1
#define ATT_K(pass, what) attn_##pass##_tail_##what
#include "x3_attention.h"

int enh_attention_tail_forward_x3(const enh_bf16* qkv_hi, const enh_bf16* qkv_lo, int B, int N, int H, float scale, enh_bf16* out3, enh_bf16* out_bf16, float* lse,
                                  void* stream) {
  static const bool attr = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_tail_x3_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * X3_STAGE_BYTES);
    return true;
  }();
  (void)attr;
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H;
  const dim3 grid((unsigned)(((heads + 7) / 8) * 8 * nblk));
  attn_fwd_tail_x3_kernel<<<grid, 256, 2 * X3_STAGE_BYTES, (hipStream_t)stream>>>(qkv_hi, qkv_lo, B, N, H, scale * ATT_LOG2E, out3, out_bf16, lse);
  return enh_check_launch("enh_attention_forward_x3");
}
