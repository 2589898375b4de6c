// gpt_decode_w6.hip — stage-2 sampling with MXFP6 weights for gfx950: the weight-only 6-bit form of a decode step's products.  A step streams every
// Block weight once and is bound by those bytes (profiles/gpt_sample.txt); here a weight W [N, K] is one e2m3 code per element, 32 codes to 24 bytes,
// and one E8M0 scale per 32 consecutive k of a row (mxfp6.h; include/enh_hip.h states the layout), 0.78 bytes per weight instead of 2.  Inside a
// block that shares a power-of-two scale e2m3 carries the three mantissa bits of MXFP8's e4m3, so the format is about as accurate at 0.76 of the bytes.
//
//   enh_mxfp6_quantize    f32 master rows -> (codes, scales), written at a row offset of the operand so that q, k and v land as the row blocks of one
//                         fused [3C, C] operand.  One pass: a thread holds the 32 values of one piece of a chunk in registers (eight from each of the
//                         chunk's four blocks), the four block maxima cross the chunk's four lanes by two shuffles each, every lane stores its piece
//                         as one 16-byte and one 8-byte store and one lane per block the scale byte.
//   enh_skinny_gemm_w6    enh_skinny_gemm_w4's contract (gpt_decode_w4.hip) with e2m3 codes: the same workgroup (16 rows of W, four waves taking the K
//                         chunks round-robin), the same fixed-order sums and slab pass (skinny_gemm.h).  x stays in the 16-bit operand format; a lane
//                         widens its whole piece with ONE v_cvt_scalef32_pk32_{f16,bf16}_fp6 at scale 1 (exact: e2m3 has 4 significant bits) and
//                         v_mfma_f32_16x16x32 multiplies.
//
// The scale.  As in the other two quantized kernels an MFMA step covers exactly one 32-wide block, starts from a zero accumulator, and its f32 result
// is multiplied by the block's 2^(s - 127) as it is added to the running sum: exact whatever the scale's size.  The scale byte 0xff widens to
// +infinity, and 0 x infinity makes every result of a row that holds such a block a NaN, which is what the byte says.
//
// The lane mapping.  W is the B operand: lane (r = lane % 16, q = lane / 16) supplies column n = r and, in MFMA step i of a chunk, the eight
// k = 32 i + 8 q .. + 7.  OCP MX fixes the element and the scale, not the memory order of the codes, so the operand is stored in the order the MFMA
// consumes it: piece q of a chunk (mxfp6.h) is those 4 x 8 codes, step-major, 192 bits.  The lane reads it with one aligned 16-byte and one aligned
// 8-byte load (each instruction covers contiguous bytes of a row: 64 and 32), and result registers 4 i .. 4 i + 3 of the one conversion are the
// operand of step i as they stand, opposite the x that the other kernels read at x + kb + 32 i + 8 q.  No lane swaps at all, against four per chunk
// in the 4-bit kernel and two in the 8-bit kernel.
//
// The plan.  A chunk is 128 k, 96 bytes per row; rows are padded to whole chunks, so no weight load is conditional.  The slab count is
// w4_gemm_plan's: a wave keeps at least two chunks (w6_gemm_plan below), which is what the RQ prior's launch-bound position needs (gpt_decode_w4.hip).
// Measured at the shipped shapes: two chunks per loop trip (256 k, both chunks' loads in flight before the first conversion) took
// 0.98 - 1.03 x the time, the same bits: inside the window spread in both directions, so the shorter trip stays.  Longer trips were not tried.
// W is read exactly once, non-temporal.
// Every result is the same bits on every run: no atomics, all sums in a fixed order.
#include "common.h"
#include "mxfp6.h"
#include "skinny_gemm.h"

typedef __attribute__((ext_vector_type(6))) unsigned int u32x6;
typedef __attribute__((ext_vector_type(32))) _Float16 f16x32;
typedef __attribute__((ext_vector_type(32))) __bf16 bf16x32;

// ---------------------------------------------------------------------------------------------
// quantizer
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpt_mxfp6_quantize_kernel(const float* __restrict__ w, int64_t N, int K, int64_t w_row_stride,
                                                                 uint8_t* __restrict__ codes, uint8_t* __restrict__ scales) {
  const int per_row = ((K + MX6_CHUNK_K - 1) / MX6_CHUNK_K) * 4;      // one thread per piece, four threads per chunk (a chunk never straddles waves)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < N * per_row;
  const int64_t n = live ? i / per_row : 0;
  const int g = live ? (int)(i - n * per_row) : 0;
  const int c = g >> 2, q = g & 3;
  const float* p = w + n * w_row_stride + c * MX6_CHUNK_K + q * 8;
  float v[4][8];
  uint32_t amax[4];                                             // magnitudes order like their bit patterns; a NaN sorts above infinity
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const bool in = c * MX6_CHUNK_K + b * MX_BLOCK < K;         // K % 32 == 0: a block lies wholly inside K or wholly outside
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 lo = in ? *reinterpret_cast<const f32x4*>(p + b * MX_BLOCK) : z, hi = in ? *reinterpret_cast<const f32x4*>(p + b * MX_BLOCK + 4) : z;
    v[b][0] = lo.x, v[b][1] = lo.y, v[b][2] = lo.z, v[b][3] = lo.w, v[b][4] = hi.x, v[b][5] = hi.y, v[b][6] = hi.z, v[b][7] = hi.w;
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t a = __builtin_bit_cast(uint32_t, v[b][e]) & 0x7fffffffu;
      m = a > m ? a : m;
    }
    uint32_t o = (uint32_t)__shfl_xor((int)m, 1, 64);
    m = o > m ? o : m;
    o = (uint32_t)__shfl_xor((int)m, 2, 64);
    amax[b] = o > m ? o : m;
  }
  if (!live) return;
  uint8_t code[32];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const bool nan = mx4_block_is_nan(amax[b]);
    const int X = mx4_block_exponent(amax[b]);
    const float inv = mx_inv_scale(X);
#pragma unroll
    for (int e = 0; e < 8; ++e) code[8 * b + e] = nan ? (uint8_t)0 : mx_e2m3_rne(v[b][e] * inv);
    if (b == q && c * MX6_CHUNK_K + b * MX_BLOCK < K) scales[n * (K / MX_BLOCK) + c * 4 + b] = nan ? (uint8_t)MX4_NAN_SCALE : (uint8_t)(X + 127);
  }
  uint32_t d[6];
  mx6_pack_piece(code, d);
  uint8_t* row = codes + n * mx6_row_bytes(K) + (int64_t)c * MX6_CHUNK_BYTES;
  *reinterpret_cast<u32x4*>(row + 16 * q) = u32x4{d[0], d[1], d[2], d[3]};
  *reinterpret_cast<u32x2*>(row + 64 + 8 * q) = u32x2{d[4], d[5]};
}

extern "C" int enh_mxfp6_quantize(const float* w, int64_t N, int64_t K, int64_t w_row_stride, uint8_t* codes, int64_t code_row0, uint8_t* scales,
                                  int64_t scale_row0, void* stream) {
  ENH_REQUIRE(w && codes && scales, ENH_E_BADARG, "enh_mxfp6_quantize: null pointer");
  ENH_REQUIRE(N >= 1 && K >= MX_BLOCK && K % MX_BLOCK == 0 && K < (1LL << 30) && N < (1LL << 30), ENH_E_SHAPE,
              "enh_mxfp6_quantize: K must be a positive multiple of 32 and N positive, got N=%lld K=%lld", (long long)N, (long long)K);
  ENH_REQUIRE(w_row_stride >= K && w_row_stride % 4 == 0 && ((uintptr_t)w & 15) == 0 && code_row0 >= 0 && scale_row0 >= 0, ENH_E_BADARG,
              "enh_mxfp6_quantize: the rows of w must be 16-byte aligned (row stride %lld) and the row offsets non-negative (%lld, %lld)",
              (long long)w_row_stride, (long long)code_row0, (long long)scale_row0);
  ENH_REQUIRE(((uintptr_t)codes & 15) == 0, ENH_E_BADARG, "enh_mxfp6_quantize: codes must be 16-byte aligned");
  enh_note_kernel_plain("gpt_mxfp6_quantize_kernel");
  const int64_t threads = N * ((K + MX6_CHUNK_K - 1) / MX6_CHUNK_K) * 4;
  gpt_mxfp6_quantize_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, N, (int)K, w_row_stride,
                                                                                               codes + code_row0 * mx6_row_bytes(K),
                                                                                               scales + scale_row0 * (K / MX_BLOCK));
  return enh_check_launch("enh_mxfp6_quantize");
}

// ---------------------------------------------------------------------------------------------
// skinny GEMM, W in MXFP6
// ---------------------------------------------------------------------------------------------
// one piece (six dwords, 32 e2m3 codes in position order) -> the four MFMA operands of a chunk, a[i] = positions 8 i .. 8 i + 7; scale 1: exact in
// either format
template <typename OT>
__device__ __forceinline__ void w6_widen(const u32x6 c, s16x8 (&a)[4]) {
  struct quad { s16x8 v[4]; };
  quad r;
  if constexpr (OT::id == 0) {
    r = __builtin_bit_cast(quad, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, 1.0f));
  } else {
    r = __builtin_bit_cast(quad, __builtin_amdgcn_cvt_scalef32_pk32_f16_fp6(c, 1.0f));
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = r.v[i];
}

// K chunks per slab and the slab count, a function of (N, K) alone: w4_gemm_plan's rule, a wave keeps at least TWO chunks
static inline void w6_gemm_plan(int64_t N, int64_t K, int* chunks_per_split, int* splits) {
  const int64_t tiles = (N + 15) / 16, nchunks = (K + MX6_CHUNK_K - 1) / MX6_CHUNK_K;
  int64_t s = 768 / tiles;                // about three 4-wave workgroups per CU
  if (s > nchunks / 8) s = nchunks / 8;   // a chunk is 96 bytes per row here
  if (s > GD_MAX_SPLITS) s = GD_MAX_SPLITS;
  if (s < 1) s = 1;
  const int64_t cps = (nchunks + s - 1) / s;
  *chunks_per_split = (int)cps;
  *splits = (int)((nchunks + cps - 1) / cps);
}

// x rows past M read row M - 1 and W rows past N row N - 1 (memory the caller owns); their rows and columns of D are dropped.  A row of codes is
// whole chunks, so every piece of every chunk is memory of the operand and no weight load is conditional; what lies past K is zero codes, zero x
// and a zero factor.
template <typename OT, int MT>
__global__ __launch_bounds__(256) void gpt_skinny_gemm_w6_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ codes,
                                                                 const uint8_t* __restrict__ scales, int M, int N, int K, int chunks_per_split,
                                                                 const float* __restrict__ bias, int act, const float* __restrict__ res,
                                                                 float* __restrict__ out_f32, uint16_t* __restrict__ out_h16, float* __restrict__ part) {
  __shared__ float s_acc[4][MT * 16][17];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nrow = n0 + r < N ? n0 + r : N - 1;
  const int KB = K / MX_BLOCK;
  const int nchunks = (K + MX6_CHUNK_K - 1) / MX6_CHUNK_K;
  const uint8_t* wlo = codes + (size_t)nrow * nchunks * MX6_CHUNK_BYTES + q * 16;
  const uint8_t* whi = codes + (size_t)nrow * nchunks * MX6_CHUNK_BYTES + 64 + q * 8;
  const uint8_t* sp = scales + (size_t)nrow * KB;
  const uint16_t* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int xr = mt * 16 + r < M ? mt * 16 + r : M - 1;
    xp[mt] = x + (size_t)xr * K + q * 8;
  }
  const int c0 = blockIdx.y * chunks_per_split;
  const int c1 = c0 + chunks_per_split < nchunks ? c0 + chunks_per_split : nchunks;
  const bool whole = (KB & 3) == 0;                // K % 128 == 0: a chunk's four scale bytes are one aligned dword
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = c0 + wave; c < c1; c += 4) {
    const int kb = c * MX6_CHUNK_K;
    const u32x4 lo = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wlo + (size_t)c * MX6_CHUNK_BYTES));
    const u32x2 hi = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(whi + (size_t)c * MX6_CHUNK_BYTES));
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
    s16x8 a[4];                                               // a[i]: the codes k = 8 q .. 8 q + 7 of block i of the chunk, widened
    w6_widen<OT>(u32x6{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y}, a);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float f = kb + i * 32 < K ? mx_scale_f32((sc4 >> (8 * i)) & 0xffu) : 0.f;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const f32x4 d = mfma16<OT>(b[mt][i], a[i], f32x4{0.f, 0.f, 0.f, 0.f});
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
__global__ __launch_bounds__(256) void gpt_skinny_w6_reduce_kernel(const float* __restrict__ part, int splits, int M, int N, const float* __restrict__ bias,
                                                                   int act, const float* __restrict__ res, float* __restrict__ out_f32,
                                                                   uint16_t* __restrict__ out_h16) {
  gd_reduce_slabs<OT>(part, splits, M, N, bias, act, res, out_f32, out_h16);
}

extern "C" size_t enh_skinny_gemm_w6_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M < 1 || N < 1 || K < 1) return 0;
  int cps, splits;
  w6_gemm_plan(N, K, &cps, &splits);
  return splits > 1 ? (size_t)splits * M * N * sizeof(float) : 0;
}

extern "C" int enh_skinny_gemm_w6(const enh_h16* x, const uint8_t* codes, const uint8_t* scales, int64_t M, int64_t N, int64_t K, const float* bias,
                                  int act, const float* res, float* out_f32, enh_h16* out_h16, void* workspace, size_t workspace_bytes, int dtype,
                                  void* stream) {
  ENH_REQUIRE(x && codes && scales && (out_f32 || out_h16), ENH_E_BADARG, "enh_skinny_gemm_w6: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_skinny_gemm_w6");
  ENH_REQUIRE(M >= 1 && M <= GD_MAX_M, ENH_E_SHAPE, "enh_skinny_gemm_w6: M must be in [1, %d], got %lld", GD_MAX_M, (long long)M);
  ENH_REQUIRE(N >= 8 && K >= MX_BLOCK && N % 8 == 0 && K % MX_BLOCK == 0 && N < (1LL << 30) && K < (1LL << 30), ENH_E_SHAPE,
              "enh_skinny_gemm_w6: N must be a positive multiple of 8 and K of 32, got N=%lld K=%lld", (long long)N, (long long)K);
  ENH_REQUIRE(act == 0 || act == 1, ENH_E_BADARG, "enh_skinny_gemm_w6: act must be 0 (none) or 1 (relu^2), got %d", act);
  ENH_REQUIRE((((uintptr_t)codes | (uintptr_t)x) & 15) == 0 && ((uintptr_t)scales & 3) == 0, ENH_E_BADARG,
              "enh_skinny_gemm_w6: x and codes must be 16-byte aligned, scales 4-byte aligned");
  int cps, splits;
  w6_gemm_plan(N, K, &cps, &splits);
  float* part = nullptr;
  if (splits > 1) {
    ENH_REQUIRE(workspace && workspace_bytes >= enh_skinny_gemm_w6_workspace_bytes(M, N, K), ENH_E_WORKSPACE, "enh_skinny_gemm_w6: workspace too small");
    part = reinterpret_cast<float*>(workspace);
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + 15) / 16), (unsigned)splits);
  // the label is the product kernel's, also when the slab pass follows
#define W6_GEMM_LAUNCH(MT)                                                                                                                          \
  do {                                                                                                                                              \
    enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_skinny_gemm_w6_kernel<F16, " #MT ">" : "gpt_skinny_gemm_w6_kernel<BF16, " #MT ">");            \
    ENH_DT_DISPATCH(dtype, (gpt_skinny_gemm_w6_kernel<OT, MT><<<grid, 256, 0, s>>>(x, codes, scales, (int)M, (int)N, (int)K, cps, bias, act, res,   \
                                                                                   out_f32, out_h16, part)));                                       \
  } while (0)
  if (M <= 16) W6_GEMM_LAUNCH(1);
  else if (M <= 32) W6_GEMM_LAUNCH(2);
  else W6_GEMM_LAUNCH(4);
#undef W6_GEMM_LAUNCH
  if (splits > 1)
    ENH_DT_DISPATCH(dtype, (gpt_skinny_w6_reduce_kernel<OT><<<(unsigned)((M * N + 255) / 256), 256, 0, s>>>(part, splits, (int)M, (int)N, bias, act, res,
                                                                                                           out_f32, out_h16)));
  return enh_check_launch("enh_skinny_gemm_w6");
}
