// gpt_decode_w4.hip — stage-2 sampling with MXFP4 weights for gfx950: the weight-only 4-bit form of a decode step's products.  A step streams every
// Block weight once and is bound by those bytes (profiles/gpt_sample.txt); here a weight W [N, K] is one e2m1 code per element, two to a byte, and
// one E8M0 scale per 32 consecutive k of a row (mxfp4.h; include/enh_hip.h states the layout), 0.53 bytes per weight instead of 2.
//
//   enh_mxfp4_quantize    f32 master rows -> (codes, scales), written at a row offset of the operand so that q, k and v land as the row blocks of one
//                         fused [3C, C] operand.  One pass: four lanes hold the 32 values of a block in registers (two 16-byte loads each), the block
//                         maximum crosses them by two shuffles, every lane stores its eight codes as one dword.
//   enh_skinny_gemm_w4    enh_skinny_gemm_w8's contract (gpt_decode_w8.hip) with e2m1 codes: the same workgroup (16 rows of W, four waves taking the K
//                         chunks round-robin), the same fixed-order sums and slab pass (skinny_gemm.h).  x stays in the 16-bit operand format; the
//                         codes are widened to it in registers (v_cvt_scalef32_pk_{f16,bf16}_fp4 at scale 1: exact, e2m1 has 2 significant bits) and
//                         v_mfma_f32_16x16x32 multiplies them.
//
// The scale.  As in the 8-bit kernel an MFMA step covers exactly one 32-wide block, starts from a zero accumulator, and its f32 result is multiplied
// by the block's 2^(s - 127) as it is added to the running sum: exact whatever the scale's size.  The scale byte 0xff widens to +infinity, and
// 0 x infinity makes every result of a row that holds such a block a NaN, which is what the byte says.
//
// The lane mapping.  W is the B operand: lane (r = lane % 16, q = lane / 16) supplies column n = r.  Loads stay 64 contiguous bytes per row and
// instruction (the 16-bit kernel's finding), so lane (r, q) reads with one 16-byte load the WHOLE block q of the four blocks that the four lanes of
// row r cover: dword i of the load is the codes k = 8 i .. 8 i + 7 of that block.  An MFMA step takes 8 k from each of the four lanes of a column, so
// as loaded a step would mix four blocks.  A 4 x 4 transpose of (lane group q, dword i) puts it right: v_permlane32_swap on the dword pairs (0, 2)
// and (1, 3) exchanges the halves of the wave (bit 1 of q), v_permlane16_swap on the resulting pairs (0, 1) and (2, 3) exchanges odd and even rows of
// 16 lanes (bit 0 of q).  Afterwards dword i of lane (r, q) is the codes k = 8 q .. 8 q + 7 of block i: step i is block i in the natural k order, and
// x is read where the 16-bit kernel reads it.  Four swaps per 128 k, against two in the 8-bit kernel.
//
// The plan.  A chunk is 128 k as in the other two kernels, which here is ONE 16-byte load of W per lane.  Measured at the shipped shapes (DESIGN.md
// §3.15): two loads per lane and chunk (256 k, the 8-bit kernel's bytes in flight per wave) took 1.04 - 1.51 x the time and four loads 1.31 - 1.82 x;
// the kernel is bound by its instructions and their latency, not by bytes in flight, and the shorter chunk keeps 42 fewer registers per lane (62 against 104 at M <= 16).  The
// slab count is gd_gemm_plan's with a wave keeping at least two chunks instead of one (w4_gemm_plan below): at the GPT's shapes the two rules agree,
// at the RQ prior's C = 1536 the 16-bit rule cuts three of the four products into slabs of one or two chunks per wave and pays a slab pass per product,
// which is what its launch-bound position cannot afford.  So the workspace has a query of its own, enh_skinny_gemm_w4_workspace_bytes.
// W is read exactly once, non-temporal.
// Every result is the same bits on every run: no atomics, all sums in a fixed order.
#include "common.h"
#include "mxfp4.h"
#include "skinny_gemm.h"

// ---------------------------------------------------------------------------------------------
// quantizer
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpt_mxfp4_quantize_kernel(const float* __restrict__ w, int64_t N, int K, int64_t w_row_stride,
                                                                 uint8_t* __restrict__ codes, uint8_t* __restrict__ scales) {
  const int per_row = K >> 3;                                   // eight values per thread, four threads per block (K % 32 == 0: a block never straddles rows or waves)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < N * per_row;
  const int64_t n = live ? i / per_row : 0;
  const int g = live ? (int)(i - n * per_row) : 0;
  const float* p = w + n * w_row_stride + (int64_t)g * 8;
  const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
  const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t amax = 0;                                            // magnitudes order like their bit patterns; a NaN sorts above infinity
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t a = __builtin_bit_cast(uint32_t, v[e]) & 0x7fffffffu;
    amax = a > amax ? a : amax;
  }
  uint32_t o = (uint32_t)__shfl_xor((int)amax, 1, 64);
  amax = o > amax ? o : amax;
  o = (uint32_t)__shfl_xor((int)amax, 2, 64);
  amax = o > amax ? o : amax;
  if (!live) return;
  const bool nan = mx4_block_is_nan(amax);
  const int X = mx4_block_exponent(amax);
  const float inv = mx_inv_scale(X);
  uint32_t c = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) c |= (uint32_t)mx_e2m1_rne(v[e] * inv) << (4 * e);
  *reinterpret_cast<uint32_t*>(codes + n * (K / 2) + (int64_t)g * 4) = nan ? 0u : c;
  if ((g & 3) == 0) scales[n * (K / MX_BLOCK) + (g >> 2)] = nan ? (uint8_t)MX4_NAN_SCALE : (uint8_t)(X + 127);
}

extern "C" int enh_mxfp4_quantize(const float* w, int64_t N, int64_t K, int64_t w_row_stride, uint8_t* codes, int64_t code_row0, uint8_t* scales,
                                  int64_t scale_row0, void* stream) {
  ENH_REQUIRE(w && codes && scales, ENH_E_BADARG, "enh_mxfp4_quantize: null pointer");
  ENH_REQUIRE(N >= 1 && K >= MX_BLOCK && K % MX_BLOCK == 0 && K < (1LL << 30) && N < (1LL << 30), ENH_E_SHAPE,
              "enh_mxfp4_quantize: K must be a positive multiple of 32 and N positive, got N=%lld K=%lld", (long long)N, (long long)K);
  ENH_REQUIRE(w_row_stride >= K && w_row_stride % 4 == 0 && ((uintptr_t)w & 15) == 0 && code_row0 >= 0 && scale_row0 >= 0, ENH_E_BADARG,
              "enh_mxfp4_quantize: the rows of w must be 16-byte aligned (row stride %lld) and the row offsets non-negative (%lld, %lld)",
              (long long)w_row_stride, (long long)code_row0, (long long)scale_row0);
  ENH_REQUIRE(((uintptr_t)codes & 3) == 0, ENH_E_BADARG, "enh_mxfp4_quantize: codes must be 4-byte aligned");
  enh_note_kernel_plain("gpt_mxfp4_quantize_kernel");
  const int64_t threads = N * (K / 8);
  gpt_mxfp4_quantize_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, N, (int)K, w_row_stride, codes + code_row0 * (K / 2),
                                                                                               scales + scale_row0 * (K / MX_BLOCK));
  return enh_check_launch("enh_mxfp4_quantize");
}

// ---------------------------------------------------------------------------------------------
// skinny GEMM, W in MXFP4
// ---------------------------------------------------------------------------------------------
// eight e2m1 codes (one dword, k ascending from the low nibble) -> eight 16-bit operands; scale 1: exact in either format
template <typename OT>
__device__ __forceinline__ s16x8 w4_widen(uint32_t c) {
  u32x4 r;
  if constexpr (OT::id == 0) {
    r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, 1.0f, 0));
    r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, 1.0f, 1));
    r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, 1.0f, 2));
    r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, 1.0f, 3));
  } else {
    r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, 1.0f, 0));
    r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, 1.0f, 1));
    r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, 1.0f, 2));
    r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, 1.0f, 3));
  }
  return __builtin_bit_cast(s16x8, r);
}

// K chunks per slab and the slab count, a function of (N, K) alone: gd_gemm_plan's rule, but a wave keeps at least TWO chunks
static inline void w4_gemm_plan(int64_t N, int64_t K, int* chunks_per_split, int* splits) {
  const int64_t tiles = (N + 15) / 16, nchunks = (K + 127) / 128;
  int64_t s = 768 / tiles;                // about three 4-wave workgroups per CU
  if (s > nchunks / 8) s = nchunks / 8;   // a chunk is 64 bytes per row here, a quarter of the 16-bit kernel's
  if (s > GD_MAX_SPLITS) s = GD_MAX_SPLITS;
  if (s < 1) s = 1;
  const int64_t cps = (nchunks + s - 1) / s;
  *chunks_per_split = (int)cps;
  *splits = (int)((nchunks + cps - 1) / cps);
}

// x rows past M read row M - 1 and W rows past N row N - 1 (memory the caller owns); their rows and columns of D are dropped.  K % 32 == 0, so a
// lane's 16-byte piece of codes is one block and lies wholly inside K or wholly outside; what lies outside is zero codes, zero x and a zero scale.
template <typename OT, int MT>
__global__ __launch_bounds__(256) void gpt_skinny_gemm_w4_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ codes,
                                                                 const uint8_t* __restrict__ scales, int M, int N, int K, int chunks_per_split,
                                                                 const float* __restrict__ bias, int act, const float* __restrict__ res,
                                                                 float* __restrict__ out_f32, uint16_t* __restrict__ out_h16, float* __restrict__ part) {
  __shared__ float s_acc[4][MT * 16][17];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nrow = n0 + r < N ? n0 + r : N - 1;
  const int KB = K / MX_BLOCK;
  const uint8_t* wp = codes + (size_t)nrow * (K / 2) + q * 16;
  const uint8_t* sp = scales + (size_t)nrow * KB;
  const uint16_t* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int xr = mt * 16 + r < M ? mt * 16 + r : M - 1;
    xp[mt] = x + (size_t)xr * K + q * 8;
  }
  const int nchunks = (K + 127) / 128;
  const int c0 = blockIdx.y * chunks_per_split;
  const int c1 = c0 + chunks_per_split < nchunks ? c0 + chunks_per_split : nchunks;
  const bool whole = (KB & 3) == 0;                // K % 128 == 0: a chunk's four scale bytes are one aligned dword
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  for (int c = c0 + wave; c < c1; c += 4) {
    const int kb = c * 128;
    const u32x4 wr = kb + q * 32 < K ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (kb >> 1))) : zero4;
    uint32_t sc4 = 0;
    if (whole) {
      sc4 = *reinterpret_cast<const uint32_t*>(sp + c * 4);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c * 4 + i < KB) sc4 |= (uint32_t)sp[c * 4 + i] << (8 * i);
    }
    s16x8 b[MT][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = kb + i * 32 < K;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) b[mt][i] = ok ? *reinterpret_cast<const s16x8*>(xp[mt] + kb + i * 32) : zero;
    }
    // the 4 x 4 transpose of (q, dword): first bit 1 of q on the pairs (0, 2) and (1, 3), then bit 0 of q on the pairs (0, 1) and (2, 3)
    const u32x2 p02 = __builtin_amdgcn_permlane32_swap(wr.x, wr.z, false, false);
    const u32x2 p13 = __builtin_amdgcn_permlane32_swap(wr.y, wr.w, false, false);
    const u32x2 t01 = __builtin_amdgcn_permlane16_swap(p02.x, p13.x, false, false);
    const u32x2 t23 = __builtin_amdgcn_permlane16_swap(p02.y, p13.y, false, false);
    const uint32_t blk[4] = {t01.x, t01.y, t23.x, t23.y};      // blk[i]: the codes k = 8 q .. 8 q + 7 of block i of the chunk
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const s16x8 a = w4_widen<OT>(blk[i]);
      const float f = kb + i * 32 < K ? mx_scale_f32((sc4 >> (8 * i)) & 0xffu) : 0.f;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const f32x4 d = mfma16<OT>(b[mt][i], a, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[mt][e] = fmaf(d[e], f, acc[mt][e]);
      }
    }
  }
  // D row (m) of acc[e]: 4 q + e ; column (n) = r
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) s_acc[wave][mt * 16 + 4 * q + e][r] = acc[mt][e];
  __syncthreads();
  for (int idx = t; idx < MT * 16 * 16; idx += 256) {
    const int m = idx >> 4, n = n0 + (idx & 15);
    if (m >= M || n >= N) continue;
    const float v = ((s_acc[0][m][idx & 15] + s_acc[1][m][idx & 15]) + s_acc[2][m][idx & 15]) + s_acc[3][m][idx & 15];
    if (part) {
      part[((size_t)blockIdx.y * M + m) * N + n] = v;
    } else {
      gd_store<OT>(gd_epilogue(v, m, n, N, bias, act, res), (int64_t)m * N + n, out_f32, out_h16);
    }
  }
}

template <typename OT>
__global__ __launch_bounds__(256) void gpt_skinny_w4_reduce_kernel(const float* __restrict__ part, int splits, int M, int N, const float* __restrict__ bias,
                                                                   int act, const float* __restrict__ res, float* __restrict__ out_f32,
                                                                   uint16_t* __restrict__ out_h16) {
  gd_reduce_slabs<OT>(part, splits, M, N, bias, act, res, out_f32, out_h16);
}

extern "C" size_t enh_skinny_gemm_w4_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M < 1 || N < 1 || K < 1) return 0;
  int cps, splits;
  w4_gemm_plan(N, K, &cps, &splits);
  return splits > 1 ? (size_t)splits * M * N * sizeof(float) : 0;
}

extern "C" int enh_skinny_gemm_w4(const enh_h16* x, const uint8_t* codes, const uint8_t* scales, int64_t M, int64_t N, int64_t K, const float* bias,
                                  int act, const float* res, float* out_f32, enh_h16* out_h16, void* workspace, size_t workspace_bytes, int dtype,
                                  void* stream) {
  ENH_REQUIRE(x && codes && scales && (out_f32 || out_h16), ENH_E_BADARG, "enh_skinny_gemm_w4: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_skinny_gemm_w4");
  ENH_REQUIRE(M >= 1 && M <= GD_MAX_M, ENH_E_SHAPE, "enh_skinny_gemm_w4: M must be in [1, %d], got %lld", GD_MAX_M, (long long)M);
  ENH_REQUIRE(N >= 8 && K >= MX_BLOCK && N % 8 == 0 && K % MX_BLOCK == 0 && N < (1LL << 30) && K < (1LL << 30), ENH_E_SHAPE,
              "enh_skinny_gemm_w4: N must be a positive multiple of 8 and K of 32, got N=%lld K=%lld", (long long)N, (long long)K);
  ENH_REQUIRE(act == 0 || act == 1, ENH_E_BADARG, "enh_skinny_gemm_w4: act must be 0 (none) or 1 (relu^2), got %d", act);
  ENH_REQUIRE((((uintptr_t)codes | (uintptr_t)x) & 15) == 0 && ((uintptr_t)scales & 3) == 0, ENH_E_BADARG,
              "enh_skinny_gemm_w4: x and codes must be 16-byte aligned, scales 4-byte aligned");
  int cps, splits;
  w4_gemm_plan(N, K, &cps, &splits);
  float* part = nullptr;
  if (splits > 1) {
    ENH_REQUIRE(workspace && workspace_bytes >= enh_skinny_gemm_w4_workspace_bytes(M, N, K), ENH_E_WORKSPACE, "enh_skinny_gemm_w4: workspace too small");
    part = reinterpret_cast<float*>(workspace);
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + 15) / 16), (unsigned)splits);
  // the label is the product kernel's, also when the slab pass follows
#define W4_GEMM_LAUNCH(MT)                                                                                                                          \
  do {                                                                                                                                              \
    enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_skinny_gemm_w4_kernel<F16, " #MT ">" : "gpt_skinny_gemm_w4_kernel<BF16, " #MT ">");            \
    ENH_DT_DISPATCH(dtype, (gpt_skinny_gemm_w4_kernel<OT, MT><<<grid, 256, 0, s>>>(x, codes, scales, (int)M, (int)N, (int)K, cps, bias, act, res,   \
                                                                                   out_f32, out_h16, part)));                                       \
  } while (0)
  if (M <= 16) W4_GEMM_LAUNCH(1);
  else if (M <= 32) W4_GEMM_LAUNCH(2);
  else W4_GEMM_LAUNCH(4);
#undef W4_GEMM_LAUNCH
  if (splits > 1)
    ENH_DT_DISPATCH(dtype, (gpt_skinny_w4_reduce_kernel<OT><<<(unsigned)((M * N + 255) / 256), 256, 0, s>>>(part, splits, (int)M, (int)N, bias, act, res,
                                                                                                           out_f32, out_h16)));
  return enh_check_launch("enh_skinny_gemm_w4");
}
