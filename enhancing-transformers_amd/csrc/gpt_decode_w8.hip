// gpt_decode_w8.hip — stage-2 sampling with MXFP8 weights for gfx950: the weight-only 8-bit form of a decode step's products.  A step streams every
// Block weight once and is bound by those bytes (profiles/gpt_sample.txt); here a weight W [N, K] is one e4m3fn code per element and one E8M0 scale
// per 32 consecutive k of a row (mxfp8.h; include/enh_hip.h states the layout), 1.03 bytes per weight instead of 2.
//
//   enh_mxfp8_quantize    f32 master rows -> (codes, scales), written at a row offset of the operand so that q, k and v land as the row blocks of one
//                         fused [3C, C] operand.  One pass: four lanes hold the 32 values of a block in registers (two 16-byte loads each), the block
//                         maximum crosses them by two shuffles, every lane stores its eight codes as one 8-byte word.
//   enh_skinny_gemm_w8    enh_skinny_gemm_h16's contract (gpt_decode.hip) with W given as (codes, scales): the same workgroup (16 rows of W, four
//                         waves taking the 128-wide K chunks round-robin), the same K slabs (skinny_gemm.h), the same fixed-order sums.  x stays in the
//                         16-bit operand format; the codes are widened to it in registers (v_cvt_scalef32_pk_{f16,bf16}_fp8 at scale 1: exact, e4m3
//                         has 4 significant bits) and v_mfma_f32_16x16x32 multiplies them.
//
// The scale.  An MFMA step is made to cover exactly one 32-wide block, starts from a zero accumulator, and its f32 result is multiplied by the
// block's 2^(s - 127) as it is added to the running sum: a power of two on an f32 partial sum is exact, so the scale costs no accuracy whatever its
// size (folded into an fp16 operand, 2^-28 underflows and 2^10 overflows).  Four v_fma_f32 per MFMA.
//
// The lane mapping.  W is the B operand: lane (r = lane % 16, q = lane / 16) supplies column n = r, and the four D values it holds are rows
// m = 4 q + j of the SAME column n = r.  So a lane needs the scales of the one W row it loads: four bytes per chunk, one dword when K % 128 == 0.
// The k order inside a block is permuted so that loads stay 64 bytes per row and instruction (the 16-bit kernel's finding: 32 bytes per row and
// instruction measured 2 TB/s).  Load j (0, 1) of a chunk: lane (r, q) reads the 16 codes k = 64 j + 16 q .. + 15 of row r, so the four lanes of a
// row read 64 contiguous bytes = blocks 2 j (q = 0, 1) and 2 j + 1 (q = 2, 3).  One v_permlane32_swap per dword pair then hands the upper eight
// codes of lanes q = 0, 1 to lanes q = 2, 3 and the lower eight codes of lanes q = 2, 3 to lanes q = 0, 1: afterwards every lane holds eight codes
// of block 2 j and eight of block 2 j + 1, at k offset 16 (q & 1) + 8 (q >> 1) inside the block, and x is read at the same offsets (a sum over a
// block does not care in which slot a k sits).  Two 16-byte loads of W per lane and chunk, W read exactly once, non-temporal.
// The forms that lost (DESIGN.md §3.13 has the figures): the natural order, lane (r, q) reading the eight codes k = 32 i + 8 q of step i, four 8-byte
// loads per chunk at 32 bytes per row and instruction (1.2 - 1.5 x the time); two or four chunks per wave in flight instead of one (no faster in sum:
// the registers cost occupancy); x rows past M masked off instead of clamped (no difference).
// Every result is the same bits on every run: no atomics, all sums in a fixed order.
#include "common.h"
#include "mxfp8.h"
#include "skinny_gemm.h"

// ---------------------------------------------------------------------------------------------
// quantizer
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpt_mxfp8_quantize_kernel(const float* __restrict__ w, int64_t N, int K, int64_t w_row_stride,
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
  const int X = mx_block_exponent(amax);
  const float inv = mx_inv_scale(X);
  uint32_t c0 = 0, c1 = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    c0 |= (uint32_t)mx_e4m3_rne(v[e] * inv) << (8 * e);
    c1 |= (uint32_t)mx_e4m3_rne(v[4 + e] * inv) << (8 * e);
  }
  *reinterpret_cast<u32x2*>(codes + n * K + (int64_t)g * 8) = u32x2{c0, c1};
  if ((g & 3) == 0) scales[n * (K / MX_BLOCK) + (g >> 2)] = (uint8_t)(X + 127);
}

extern "C" int enh_mxfp8_quantize(const float* w, int64_t N, int64_t K, int64_t w_row_stride, uint8_t* codes, int64_t code_row0, uint8_t* scales,
                                  int64_t scale_row0, void* stream) {
  ENH_REQUIRE(w && codes && scales, ENH_E_BADARG, "enh_mxfp8_quantize: null pointer");
  ENH_REQUIRE(N >= 1 && K >= MX_BLOCK && K % MX_BLOCK == 0 && K < (1LL << 30) && N < (1LL << 30), ENH_E_SHAPE,
              "enh_mxfp8_quantize: K must be a positive multiple of 32 and N positive, got N=%lld K=%lld", (long long)N, (long long)K);
  ENH_REQUIRE(w_row_stride >= K && w_row_stride % 4 == 0 && ((uintptr_t)w & 15) == 0 && code_row0 >= 0 && scale_row0 >= 0, ENH_E_BADARG,
              "enh_mxfp8_quantize: the rows of w must be 16-byte aligned (row stride %lld) and the row offsets non-negative (%lld, %lld)",
              (long long)w_row_stride, (long long)code_row0, (long long)scale_row0);
  ENH_REQUIRE((((uintptr_t)codes + (uintptr_t)(code_row0 * K)) & 7) == 0, ENH_E_BADARG, "enh_mxfp8_quantize: codes must be 8-byte aligned");
  enh_note_kernel_plain("gpt_mxfp8_quantize_kernel");
  const int64_t threads = N * (K / 8);
  gpt_mxfp8_quantize_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, N, (int)K, w_row_stride, codes + code_row0 * K,
                                                                                               scales + scale_row0 * (K / MX_BLOCK));
  return enh_check_launch("enh_mxfp8_quantize");
}

// ---------------------------------------------------------------------------------------------
// skinny GEMM, W in MXFP8
// ---------------------------------------------------------------------------------------------
// eight e4m3 codes (two dwords, k ascending from the low byte) -> eight 16-bit operands; scale 1: exact in either format
template <typename OT>
__device__ __forceinline__ s16x8 w8_widen(uint32_t lo, uint32_t hi) {
  u32x4 r;
  if constexpr (OT::id == 0) {
    r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
    r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
    r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
    r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
  } else {
    r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false));
    r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true));
    r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false));
    r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true));
  }
  return __builtin_bit_cast(s16x8, r);
}

// x rows past M read row M - 1 and W rows past N row N - 1 (memory the caller owns); their rows and columns of D are dropped.  K % 32 == 0, so a
// 16-byte piece of codes and a block of x lie wholly inside K or wholly outside; what lies outside is zero codes, zero x and a zero scale.
template <typename OT, int MT>
__global__ __launch_bounds__(256) void gpt_skinny_gemm_w8_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ codes,
                                                                 const uint8_t* __restrict__ scales, int M, int N, int K, int chunks_per_split,
                                                                 const float* __restrict__ bias, int act, const float* __restrict__ res,
                                                                 float* __restrict__ out_f32, uint16_t* __restrict__ out_h16, float* __restrict__ part) {
  __shared__ float s_acc[4][MT * 16][17];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nrow = n0 + r < N ? n0 + r : N - 1;
  const int KB = K / MX_BLOCK;
  const uint8_t* wp = codes + (size_t)nrow * K + q * 16;
  const uint8_t* sp = scales + (size_t)nrow * KB;
  const int xo = (q & 1) * 16 + (q >> 1) * 8;      // this lane's k offset inside a block, after the swap
  const uint16_t* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int xr = mt * 16 + r < M ? mt * 16 + r : M - 1;
    xp[mt] = x + (size_t)xr * K + xo;
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
    u32x4 wr[2];
    s16x8 b[MT][4];
    uint32_t sc4 = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      wr[j] = kb + 64 * j + q * 16 < K ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + kb + 64 * j)) : zero4;
    if (whole) {
      sc4 = *reinterpret_cast<const uint32_t*>(sp + c * 4);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c * 4 + i < KB) sc4 |= (uint32_t)sp[c * 4 + i] << (8 * i);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = kb + i * 32 < K;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) b[mt][i] = ok ? *reinterpret_cast<const s16x8*>(xp[mt] + kb + i * 32) : zero;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      // (x, y) = this lane's k 0 .. 7 of its 16 codes, (z, w) = k 8 .. 15.  After the swaps (x, y) is block 2 j and (z, w) block 2 j + 1 in every lane.
      const u32x2 s0 = __builtin_amdgcn_permlane32_swap(wr[j].x, wr[j].z, false, false);
      const u32x2 s1 = __builtin_amdgcn_permlane32_swap(wr[j].y, wr[j].w, false, false);
      const s16x8 a0 = w8_widen<OT>(s0.x, s1.x), a1 = w8_widen<OT>(s0.y, s1.y);
      const bool ok0 = kb + (2 * j) * 32 < K, ok1 = kb + (2 * j + 1) * 32 < K;
      const float f0 = ok0 ? mx_scale_f32((sc4 >> (16 * j)) & 0xffu) : 0.f;
      const float f1 = ok1 ? mx_scale_f32((sc4 >> (16 * j + 8)) & 0xffu) : 0.f;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const f32x4 d0 = mfma16<OT>(b[mt][2 * j], a0, f32x4{0.f, 0.f, 0.f, 0.f});
        const f32x4 d1 = mfma16<OT>(b[mt][2 * j + 1], a1, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[mt][e] = fmaf(d1[e], f1, fmaf(d0[e], f0, acc[mt][e]));
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
__global__ __launch_bounds__(256) void gpt_skinny_w8_reduce_kernel(const float* __restrict__ part, int splits, int M, int N, const float* __restrict__ bias,
                                                                   int act, const float* __restrict__ res, float* __restrict__ out_f32,
                                                                   uint16_t* __restrict__ out_h16) {
  gd_reduce_slabs<OT>(part, splits, M, N, bias, act, res, out_f32, out_h16);
}

extern "C" int enh_skinny_gemm_w8(const enh_h16* x, const uint8_t* codes, const uint8_t* scales, int64_t M, int64_t N, int64_t K, const float* bias,
                                  int act, const float* res, float* out_f32, enh_h16* out_h16, void* workspace, size_t workspace_bytes, int dtype,
                                  void* stream) {
  ENH_REQUIRE(x && codes && scales && (out_f32 || out_h16), ENH_E_BADARG, "enh_skinny_gemm_w8: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_skinny_gemm_w8");
  ENH_REQUIRE(M >= 1 && M <= GD_MAX_M, ENH_E_SHAPE, "enh_skinny_gemm_w8: M must be in [1, %d], got %lld", GD_MAX_M, (long long)M);
  ENH_REQUIRE(N >= 8 && K >= MX_BLOCK && N % 8 == 0 && K % MX_BLOCK == 0 && N < (1LL << 30) && K < (1LL << 30), ENH_E_SHAPE,
              "enh_skinny_gemm_w8: N must be a positive multiple of 8 and K of 32, got N=%lld K=%lld", (long long)N, (long long)K);
  ENH_REQUIRE(act == 0 || act == 1, ENH_E_BADARG, "enh_skinny_gemm_w8: act must be 0 (none) or 1 (relu^2), got %d", act);
  ENH_REQUIRE((((uintptr_t)codes | (uintptr_t)x) & 15) == 0 && ((uintptr_t)scales & 3) == 0, ENH_E_BADARG,
              "enh_skinny_gemm_w8: x and codes must be 16-byte aligned, scales 4-byte aligned");
  int cps, splits;
  gd_gemm_plan(N, K, &cps, &splits);
  float* part = nullptr;
  if (splits > 1) {
    ENH_REQUIRE(workspace && workspace_bytes >= enh_skinny_gemm_workspace_bytes(M, N, K), ENH_E_WORKSPACE, "enh_skinny_gemm_w8: workspace too small");
    part = reinterpret_cast<float*>(workspace);
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + 15) / 16), (unsigned)splits);
  // the label is the product kernel's, also when the slab pass follows
#define W8_GEMM_LAUNCH(MT)                                                                                                                          \
  do {                                                                                                                                              \
    enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_skinny_gemm_w8_kernel<F16, " #MT ">" : "gpt_skinny_gemm_w8_kernel<BF16, " #MT ">");            \
    ENH_DT_DISPATCH(dtype, (gpt_skinny_gemm_w8_kernel<OT, MT><<<grid, 256, 0, s>>>(x, codes, scales, (int)M, (int)N, (int)K, cps, bias, act, res,   \
                                                                                   out_f32, out_h16, part)));                                       \
  } while (0)
  if (M <= 16) W8_GEMM_LAUNCH(1);
  else if (M <= 32) W8_GEMM_LAUNCH(2);
  else W8_GEMM_LAUNCH(4);
#undef W8_GEMM_LAUNCH
  if (splits > 1)
    ENH_DT_DISPATCH(dtype, (gpt_skinny_w8_reduce_kernel<OT><<<(unsigned)((M * N + 255) / 256), 256, 0, s>>>(part, splits, (int)M, (int)N, bias, act, res,
                                                                                                           out_f32, out_h16)));
  return enh_check_launch("enh_skinny_gemm_w8");
}
