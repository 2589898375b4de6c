// x3_attention.h — the text of the attention forward on split operands (included by x3.hip and x3_tail.hip with ATT_TAIL and ATT_K defined)
#include "attention_tile_loop.h"
// =================================================================================================
// attention forward on split operands.  Same skeleton as attn_fwd_exact (attention_common.h): 128 queries per workgroup, S^T = K Q^T so that a lane owns
// one query column, K / V streamed in 64-key tiles through a two-stage LDS ring — here FOUR tiles per stage (K_hi, K_lo, V_hi, V_lo; 64 KiB of LDS, two
// workgroups per CU).  Per key tile: 24 MFMAs for S (small terms first), exact running maximum, numerators split in registers, 24 MFMAs for O.
// The output row is written as the x3 operand [hi | lo | hi] of to_out (row stride 3 H 64) and, optionally, as the plain bf16 tensor the backward reads.
// This text is compiled twice, as attention_kernels.h is and for the same reason: x3.hip (ATT_TAIL 0) attn_fwd_x3_kernel for N % 64 == 0, x3_tail.hip
// (ATT_TAIL 1) attn_fwd_tail_x3_kernel for any other N — ragged last tile staged with clamped rows and run through a masked instance of the tile body
// behind the loop, query rows clamped for the loads, stores guarded per lane.
// =================================================================================================
#define X3_STAGE_BYTES (4 * ATT_TILE_BYTES)
__global__ __launch_bounds__(256, 2) void ATT_K(fwd, x3_kernel)(const uint16_t* __restrict__ qh, const uint16_t* __restrict__ ql, int B, int N, int H,
                                                             float scale_log2, uint16_t* __restrict__ out3, uint16_t* __restrict__ out16,
                                                             float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2 stages][K_hi | K_lo | V_hi | V_lo]
  int blk, head;
  if (!att_block_coords((N + 127) / 128, B * H, blk, head)) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = head / H, h = head - b * H;
  const int q0 = blk * 128 + wave * 32;
  const int64_t RS = (int64_t)3 * H * ATT_D;
  const int64_t base = (int64_t)b * N * RS + h * ATT_D;
  const uint16_t* Kh = qh + base + H * ATT_D;
  const uint16_t* Kl = ql + base + H * ATT_D;
  const uint16_t* Vh = Kh + H * ATT_D;
  const uint16_t* Vl = Kl + H * ATT_D;

  const bool active = ATT_SEL(q0 + l31 < N, q0 < N);
  const int qrow = ATT_SEL(min(q0 + l31, N - 1), active ? q0 + l31 : l31);
  s16x8 qfh[4], qfl[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    qfh[ds] = *reinterpret_cast<const s16x8*>(qh + base + (int64_t)qrow * RS + ds * 16 + hi * 8);
    qfl[ds] = *reinterpret_cast<const s16x8*>(ql + base + (int64_t)qrow * RS + ds * 16 + hi * 8);
  }
  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  float m_run = -__builtin_inff(), l_part = 0.f;

  const int nt = N / 64;      // full tiles
  u32x4 rkh[2], rkl[2], rvh[2], rvl[2];
#if ATT_TAIL
  if (nt == 0) {
    att_gload_clamped(rkh, Kh, RS, 0, N, t); att_gload_clamped(rkl, Kl, RS, 0, N, t);
    att_gload_clamped(rvh, Vh, RS, 0, N, t); att_gload_clamped(rvl, Vl, RS, 0, N, t);
  } else
#endif
  {
  att_gload(rkh, Kh, RS, 0, t); att_gload(rkl, Kl, RS, 0, t);
  att_gload(rvh, Vh, RS, 0, t); att_gload(rvl, Vl, RS, 0, t);
  }
  att_sstore(rkh, smem, t); att_sstore(rkl, smem + ATT_TILE_BYTES, t);
  att_sstore(rvh, smem + 2 * ATT_TILE_BYTES, t); att_sstore(rvl, smem + 3 * ATT_TILE_BYTES, t);
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) { att_pin(qfh[ds]); att_pin(qfl[ds]); }
  ATT_LOOP_ENTRY();
  __syncthreads();
  ATT_TILES_BEGIN(kt, nt)
    const int st = kt & 1;
#if ATT_TAIL
    if constexpr (LAST) {
    } else if (kt + 1 == nt) {      // the ragged tile is next
      att_gload_clamped(rkh, Kh, RS, (kt + 1) * 64, N, t); att_gload_clamped(rkl, Kl, RS, (kt + 1) * 64, N, t);
      att_gload_clamped(rvh, Vh, RS, (kt + 1) * 64, N, t); att_gload_clamped(rvl, Vl, RS, (kt + 1) * 64, N, t);
    } else
#else
    if (kt + 1 < nt)
#endif
    {
      att_gload(rkh, Kh, RS, (kt + 1) * 64, t); att_gload(rkl, Kl, RS, (kt + 1) * 64, t);
      att_gload(rvh, Vh, RS, (kt + 1) * 64, t); att_gload(rvl, Vl, RS, (kt + 1) * 64, t);
    }
    const unsigned char* kh_ = smem + st * X3_STAGE_BYTES;
    const unsigned char* kl_ = kh_ + ATT_TILE_BYTES;
    const unsigned char* vh_ = kh_ + 2 * ATT_TILE_BYTES;
    const unsigned char* vl_ = kh_ + 3 * ATT_TILE_BYTES;
    // ---- S^T[key][q] = K Q^T : K_lo Q_hi + K_hi Q_lo + K_hi Q_hi ----
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = ATT_SEL(LAST ? att_key_bias(kb, r, hi, N & 63) : 0.f, 0.f);      // (ragged tile: ATT_MASK_BIAS on key rows >= N)
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) {
        const s16x8 fh = att_frag_row(kh_, kb * 32, ds, l31, hi), fl = att_frag_row(kl_, kb * 32, ds, l31, hi);
        s[kb] = MFMA32(fl, qfh[ds], s[kb]);
        s[kb] = MFMA32(fh, qfl[ds], s[kb]);
        s[kb] = MFMA32(fh, qfh[ds], s[kb]);
      }
    }
    // ---- online softmax for this lane's query column (fp32, exact running maximum) ----
    float mx = s[0][0];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx * scale_log2);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    float p[2][16], pl[2][16];
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[kb][r] = __builtin_amdgcn_exp2f(s[kb][r] * scale_log2 - m_new);
        psum += p[kb][r];
      }
    l_part = l_part * alpha + psum;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
    // ---- O^T[d][q] += V^T P^T : V_lo P_hi + V_hi P_lo + V_hi P_hi ----
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const s16x8 pbh = pack8<BF16>(&p[kb][c2 * 8]);
#pragma unroll
        for (int e = 0; e < 8; ++e) pl[kb][c2 * 8 + e] = p[kb][c2 * 8 + e] - bf16_bits_to_f32((uint16_t)pbh[e]);
        const s16x8 pbl = pack8<BF16>(&pl[kb][c2 * 8]);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const s16x8 fvh = att_frag_tr(vh_, kb * 32 + 16 * c2, db, lane), fvl = att_frag_tr(vl_, kb * 32 + 16 * c2, db, lane);
          o[db] = MFMA32(fvl, pbh, o[db]);
          o[db] = MFMA32(fvh, pbl, o[db]);
          o[db] = MFMA32(fvh, pbh, o[db]);
        }
      }
    ATT_UNLESS_LAST {
    if (ATT_SEL(true, kt + 1 < nt)) {
      unsigned char* nx = smem + (st ^ 1) * X3_STAGE_BYTES;
      att_sstore(rkh, nx, t); att_sstore(rkl, nx + ATT_TILE_BYTES, t);
      att_sstore(rvh, nx + 2 * ATT_TILE_BYTES, t); att_sstore(rvl, nx + 3 * ATT_TILE_BYTES, t);
    }
    __syncthreads();
    }
  ATT_TILES_END(kt, nt)
  const float l = l_part + __shfl_xor(l_part, 32, 64);
  const float inv = 1.0f / l;
  if (!active) return;
  const int64_t OS = (int64_t)H * ATT_D;
  uint16_t* op3 = out3 + ((int64_t)b * N + q0 + l31) * (3 * OS) + h * ATT_D;
  uint16_t* op = out16 ? out16 + ((int64_t)b * N + q0 + l31) * OS + h * ATT_D : nullptr;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = db * 32 + 8 * g4 + 4 * hi;
      const float v0 = o[db][g4 * 4 + 0] * inv, v1 = o[db][g4 * 4 + 1] * inv, v2 = o[db][g4 * 4 + 2] * inv, v3 = o[db][g4 * 4 + 3] * inv;
      const u32x2 wh = {pack_bf16x2(v0, v1), pack_bf16x2(v2, v3)};
      const u32x2 wl = {pack_bf16x2(v0 - __builtin_bit_cast(float, wh[0] << 16), v1 - __builtin_bit_cast(float, wh[0] & 0xffff0000u)),
                        pack_bf16x2(v2 - __builtin_bit_cast(float, wh[1] << 16), v3 - __builtin_bit_cast(float, wh[1] & 0xffff0000u))};
      *reinterpret_cast<u32x2*>(op3 + d0) = wh;
      *reinterpret_cast<u32x2*>(op3 + OS + d0) = wl;
      *reinterpret_cast<u32x2*>(op3 + 2 * OS + d0) = wh;
      if (op) *reinterpret_cast<u32x2*>(op + d0) = wh;
    }
  if (hi == 0) lse[((int64_t)b * H + h) * N + q0 + l31] = (m_run + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
}
