// x3.hip — "split-bf16" (x3) operands: the parity-grade encoder forward on the bf16 matrix cores (round 4).
//
// The reference's forward is fp32 end to end (enhancing/modules/stage1/layers.py:118-132,145-150, vitvqgan.py:61-66); a bf16-operand MFMA product
// carries 2^-9 per operand and flips ~2 % of the 8192-way argmin decisions downstream.  Here a value v is carried as the PAIR
//     hi = bf16(v),  lo = bf16(v - hi)            (v - hi - lo <= 2^-17 |v|)
// and a product a.b is formed as  a_hi b_hi + a_lo b_hi + a_hi b_lo  in the fp32 MFMA accumulator (the dropped a_lo b_lo term is 2^-18): three bf16
// passes = 833 TF/s of peak instead of the 157 TF/s of the exact-f32 MFMA, at ~1e-5 relative error end to end (measured: tests/test_x3_gpu.py).
//
// GEMMs need NO new kernel: the three passes are ONE enh_gemm_bf16 call on K-concatenated operands
//     A' [M][3K] = [ a_hi | a_lo | a_hi ]      B' [N][3K] = [ b_hi | b_hi | b_lo ]          sum_k' A' B' = the three-term product,
// so this file only holds what produces those rows — the split of an f32 matrix (optionally through bias + tanh: FeedForward's activation,
// layers.py:99-100), the split of the packed q | k | v projection into two planes — and the attention forward on split operands
// (S = Q K^T and O = P V each as three MFMA passes, softmax statistics in fp32 as in attention.hip).  LayerNorm writes its x3 row itself
// (layernorm.hip, enh_layernorm_forward_x3).
#include "attention_common.h"
typedef BF16 OT;   // the x3 path is bf16 by construction (hi / lo bf16 planes): the shared helpers of attention_common.h are used at that operand type

// hi / lo of eight consecutive values -> two 16-byte packets
__device__ __forceinline__ void split8(const float (&v)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t h = pack_bf16x2(v[2 * i], v[2 * i + 1]);
    hi[i] = h;
    lo[i] = pack_bf16x2(v[2 * i] - __builtin_bit_cast(float, h << 16), v[2 * i + 1] - __builtin_bit_cast(float, h & 0xffff0000u));
  }
}

// y3[m] = [hi | lo | hi] (ORDER 0: activation operand) or [hi | hi | lo] (ORDER 1: weight operand) of f(x[m]), f = identity / (+ bias) / tanh(+ bias);
// optional contiguous copy of the hi plane (what the bf16 path would have stored: the backward's operand).  8 elements per thread.
template <int ORDER, bool TANH>
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ x, int64_t ldx, int64_t M, int K, const float* __restrict__ bias,
                                                     uint16_t* __restrict__ y3, int64_t ldy3, uint16_t* __restrict__ yh, int64_t ldyh) {
  const int kc = K >> 3;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * kc) return;
  const int64_t m = i / kc;
  const int c = (int)(i - m * kc);
  const float4 a = *reinterpret_cast<const float4*>(x + m * ldx + c * 8), b = *reinterpret_cast<const float4*>(x + m * ldx + c * 8 + 4);
  float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  if (bias) {
    const float4 p = *reinterpret_cast<const float4*>(bias + c * 8), q = *reinterpret_cast<const float4*>(bias + c * 8 + 4);
    v[0] += p.x; v[1] += p.y; v[2] += p.z; v[3] += p.w; v[4] += q.x; v[5] += q.y; v[6] += q.z; v[7] += q.w;
  }
  if (TANH) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tanh_x3(v[e]);      // (common.h; the fused GEMM epilogue uses the same function: identical bits)
  }
  u32x4 hi, lo;
  split8(v, hi, lo);
  uint16_t* r = y3 + m * ldy3 + c * 8;
  *reinterpret_cast<u32x4*>(r) = hi;
  *reinterpret_cast<u32x4*>(r + K) = ORDER == 0 ? lo : hi;
  *reinterpret_cast<u32x4*>(r + 2 * K) = ORDER == 0 ? hi : lo;
  if (yh) *reinterpret_cast<u32x4*>(yh + m * ldyh + c * 8) = hi;
}

__global__ __launch_bounds__(256) void split2_kernel(const float* __restrict__ x, int64_t n8, uint16_t* __restrict__ yh, uint16_t* __restrict__ yl) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const float4 a = *reinterpret_cast<const float4*>(x + i * 8), b = *reinterpret_cast<const float4*>(x + i * 8 + 4);
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  u32x4 hi, lo;
  split8(v, hi, lo);
  *reinterpret_cast<u32x4*>(yh + i * 8) = hi;
  *reinterpret_cast<u32x4*>(yl + i * 8) = lo;
}

extern "C" int enh_split3_bf16(const float* x, int64_t ldx, int64_t M, int64_t K, const float* bias, int act, int order, enh_bf16* y3, int64_t ldy3,
                               enh_bf16* y_hi, int64_t ldy_hi, void* stream) {
  ENH_REQUIRE(x && y3, ENH_E_BADARG, "enh_split3_bf16: null pointer");
  ENH_REQUIRE(M > 0 && K > 0 && K % 8 == 0 && K < (1 << 28) && ldx % 4 == 0 && ldy3 % 8 == 0 && ldy3 >= 3 * K && (!y_hi || ldy_hi % 8 == 0), ENH_E_SHAPE,
              "enh_split3_bf16: need K %% 8 == 0, ldx %% 4 == 0, ldy3 %% 8 == 0 and >= 3 K (M=%lld K=%lld ldx=%lld ldy3=%lld)", (long long)M, (long long)K,
              (long long)ldx, (long long)ldy3);
  ENH_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15u) == 0 && (reinterpret_cast<uintptr_t>(y3) & 15u) == 0 && (reinterpret_cast<uintptr_t>(y_hi) & 15u) == 0 &&
              (reinterpret_cast<uintptr_t>(bias) & 15u) == 0, ENH_E_SHAPE, "enh_split3_bf16: 16-byte aligned bases");
  ENH_REQUIRE((act == ENH_ACT_NONE || act == ENH_ACT_TANH) && (order == 0 || order == 1), ENH_E_BADARG, "enh_split3_bf16: act in {0, 1}, order in {0, 1}");
  const int64_t n = M * (K / 8);
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  if (order == 0 && act == ENH_ACT_TANH) split3_kernel<0, true><<<grid, 256, 0, s>>>(x, ldx, M, (int)K, bias, y3, ldy3, y_hi, ldy_hi);
  else if (order == 0) split3_kernel<0, false><<<grid, 256, 0, s>>>(x, ldx, M, (int)K, bias, y3, ldy3, y_hi, ldy_hi);
  else if (act == ENH_ACT_TANH) split3_kernel<1, true><<<grid, 256, 0, s>>>(x, ldx, M, (int)K, bias, y3, ldy3, y_hi, ldy_hi);
  else split3_kernel<1, false><<<grid, 256, 0, s>>>(x, ldx, M, (int)K, bias, y3, ldy3, y_hi, ldy_hi);
  return enh_check_launch("enh_split3_bf16");
}

extern "C" int enh_split2_bf16(const float* x, int64_t n, enh_bf16* hi, enh_bf16* lo, void* stream) {
  ENH_REQUIRE(x && hi && lo, ENH_E_BADARG, "enh_split2_bf16: null pointer");
  ENH_REQUIRE(n > 0 && n % 8 == 0, ENH_E_SHAPE, "enh_split2_bf16: n %% 8 == 0 (n=%lld)", (long long)n);
  ENH_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(hi) | reinterpret_cast<uintptr_t>(lo)) & 15u) == 0, ENH_E_SHAPE,
              "enh_split2_bf16: 16-byte aligned bases");
  split2_kernel<<<dim3((unsigned)((n / 8 + 255) / 256)), 256, 0, (hipStream_t)stream>>>(x, n / 8, hi, lo);
  return enh_check_launch("enh_split2_bf16");
}

#define ATT_TAIL 0
#define ATT_K(pass, what) attn_##pass##_##what
#include "x3_attention.h"

extern "C" int enh_attention_forward_x3(const enh_bf16* qkv_hi, const enh_bf16* qkv_lo, int B, int N, int H, float scale, enh_bf16* out3, enh_bf16* out_bf16,
                                        float* lse, void* stream) {
  ENH_REQUIRE(qkv_hi && qkv_lo && out3 && lse, ENH_E_BADARG, "enh_attention_forward_x3: null pointer");
  ENH_REQUIRE(B > 0 && H > 0 && N > 0, ENH_E_SHAPE, "enh_attention_forward_x3: need positive B, N, H (B=%d N=%d H=%d)", B, N, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_attention_forward_x3: scale must be positive");
  if (N % 64 != 0) return enh_attention_tail_forward_x3(qkv_hi, qkv_lo, B, N, H, scale, out3, out_bf16, lse, stream);
  static const bool attr = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_x3_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * X3_STAGE_BYTES);
    return true;
  }();
  (void)attr;
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H;
  const dim3 grid((unsigned)(((heads + 7) / 8) * 8 * nblk));
  attn_fwd_x3_kernel<<<grid, 256, 2 * X3_STAGE_BYTES, (hipStream_t)stream>>>(qkv_hi, qkv_lo, B, N, H, scale * 1.4426950408889634f, out3, out_bf16, lse);
  return enh_check_launch("enh_attention_forward_x3");
}
