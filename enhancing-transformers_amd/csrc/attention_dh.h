// attention_dh.h — the fused attention at head widths D = 32, 96 and 128 (attention_dh.hip; D = 64 stays on the tuned kernels of attention_kernels.h).
//
// One kernel text per pass, a template over <D, OT>, with the arithmetic of the family-1 kernels of attention_kernels.h: v_mfma_f32_32x32x16, the
// swapped product S^T = K Q^T (a lane owns one query column: lane-local softmax statistics), P / dS from accumulator registers to the next MFMA
// unmoved, the raised running reference (rescale only when outgrown by 2^8), max3 / xhalf_*.  What changes with D is counted in AttDh<D>:
//   * the contraction of S / dP over d takes ND = D / 16 MFMAs per 32-key block (2 ND per tile and product);
//   * O / dQ / dK / dV are NB = D / 32 accumulator blocks of 16 registers (P V: 4 NB MFMAs per tile);
//   * a [64][D] tile lives in LDS as NI = ceil(D / 64) of the [64][64] images of attention_common.h (att_off) side by side: att_frag_row / att_frag_tr
//     work unchanged on image d / 64 and stay conflict-free; D = 32 and the second image at D = 96 use chunks 0-3 of a row only.
// Any N >= 1 in the same kernel: EVERY tile is staged through registers with its rows clamped to the image's last row (nothing outside the tensor
// or inside the next image is read, and the LDS image stays finite), key rows >= N get ATT_MASK_BIAS through the C operand of the S products
// (probability exactly 0), query rows >= N of the dK/dV stream get the statistic that makes P exactly 0 and delta 0, every store is guarded per row.
// One wave per SIMD (__launch_bounds__(256)): at D = 128 the dK/dV kernel holds 8 accumulator blocks (128 registers) besides its fragments.
// Not tuned (on purpose): no LDS-DMA, no counted fragment reads, the mask is evaluated in every tile, both q conventions share the general
// arithmetic (exp2(s * scale_log2 - lse), scale_log2 = 1 for pre-scaled q).
#pragma once
#include "attention_common.h"

template <int D>
struct AttDh {
  static_assert(D == 32 || D == 96 || D == 128, "head widths of this family (64: attention_kernels.h)");
  static constexpr int ND = D / 16;               // 32x32x16 steps of a contraction over d
  static constexpr int NB = D / 32;               // 32-wide blocks of d in an output accumulator
  static constexpr int NI = (D + 63) / 64;        // [64][64] LDS images per tile
  static constexpr int CPR = D / 8;               // 16-byte chunks per tile row
  static constexpr int NLD = D / 32;              // 16-byte loads per thread and tile: 64 rows x CPR chunks / 256 threads
  static constexpr int TILE_BYTES = NI * ATT_TILE_BYTES;
};

// rows row0 .. row0 + 63 of a [*][rs] 16-bit matrix, D columns, clamped to row n_rows - 1; chunk q = t + 256 i is chunk q % CPR of tile row q / CPR
template <int D>
__device__ __forceinline__ void dh_gload(u32x4 (&r)[AttDh<D>::NLD], const uint16_t* __restrict__ base, int64_t rs, int row0, int n_rows, int t) {
#pragma unroll
  for (int i = 0; i < AttDh<D>::NLD; ++i) {
    const int q = t + 256 * i, row = q / AttDh<D>::CPR, c = q % AttDh<D>::CPR;
    r[i] = *reinterpret_cast<const u32x4*>(base + (int64_t)min(row0 + row, n_rows - 1) * rs + c * 8);
  }
}
template <int D>
__device__ __forceinline__ void dh_sstore(const u32x4 (&r)[AttDh<D>::NLD], unsigned char* tile, int t) {
#pragma unroll
  for (int i = 0; i < AttDh<D>::NLD; ++i) {
    const int q = t + 256 * i, row = q / AttDh<D>::CPR, c = q % AttDh<D>::CPR;
    *reinterpret_cast<u32x4*>(tile + (c >> 3) * ATT_TILE_BYTES + att_off(row, c & 7)) = r[i];
  }
}
// att_frag_row / att_frag_tr on the image that holds 16-wide step ds / 32-wide block db of d
__device__ __forceinline__ s16x8 dh_frag_row(const unsigned char* tile, int rb, int ds, int l31, int hi) {
  return att_frag_row(tile + (ds >> 2) * ATT_TILE_BYTES, rb, ds & 3, l31, hi);
}
__device__ __forceinline__ s16x8 dh_frag_tr(const unsigned char* tile, int rbase, int db, int lane) {
  return att_frag_tr(tile + (db >> 1) * ATT_TILE_BYTES, rbase, db & 1, lane);
}

// =================================================================================================
// forward: workgroup = 128 queries (4 waves x 32), K / V in 64-key tiles through a 2-stage ring
// =================================================================================================
template <int D, typename OT>
__global__ __launch_bounds__(256) void attn_dh_fwd_kernel(const uint16_t* __restrict__ qkv, int B, int N, int H, float scale_log2, uint16_t* __restrict__ out,
                                                          float* __restrict__ lse) {
  using C = AttDh<D>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][2][C::TILE_BYTES];  // [stage][K | V]
  int blk, head;
  if (!att_block_coords((N + 127) / 128, B * H, blk, head)) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = head / H, h = head - b * H;
  const int q0 = blk * 128 + wave * 32;
  const int64_t RS = (int64_t)3 * H * D;
  const uint16_t* Qp = qkv + (int64_t)b * N * RS + h * D;
  const uint16_t* Kp = Qp + H * D;
  const uint16_t* Vp = Kp + H * D;

  const bool active = q0 + l31 < N;
  const int qrow = min(q0 + l31, N - 1);
  s16x8 qf[C::ND];
#pragma unroll
  for (int ds = 0; ds < C::ND; ++ds) qf[ds] = *reinterpret_cast<const s16x8*>(Qp + (int64_t)qrow * RS + ds * 16 + hi * 8);

  f32x16 o[C::NB];
#pragma unroll
  for (int db = 0; db < C::NB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  float m_run = -__builtin_inff(), l_part = 0.f;

  const int nt = (N + 63) / 64;
  u32x4 rk[C::NLD], rv[C::NLD];
  dh_gload<D>(rk, Kp, RS, 0, N, t);
  dh_gload<D>(rv, Vp, RS, 0, N, t);
  dh_sstore<D>(rk, smem[0][0], t);
  dh_sstore<D>(rv, smem[0][1], t);
  __syncthreads();
  for (int kt = 0; kt < nt; ++kt) {
    const int st = kt & 1;
    if (kt + 1 < nt) {
      dh_gload<D>(rk, Kp, RS, (kt + 1) * 64, N, t);
      dh_gload<D>(rv, Vp, RS, (kt + 1) * 64, N, t);
    }
    const unsigned char* kt_ = smem[st][0];
    const unsigned char* vt_ = smem[st][1];
    const int n_keys = N - kt * 64;      // live keys of this tile (>= 64: all)
    // ---- S^T[key][q] = K Q^T (+ ATT_MASK_BIAS on key rows >= N) ----
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = att_key_bias(kb, r, hi, n_keys);
#pragma unroll
      for (int ds = 0; ds < C::ND; ++ds) s[kb] = MFMA32(dh_frag_row(kt_, kb * 32, ds, l31, hi), qf[ds], s[kb]);
    }
    // ---- online softmax for this lane's query column (attention_kernels.h, family 1) ----
    float mx = max3(s[0][0], s[0][1], s[0][2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) mx = max3(mx, s[0][r], s[0][r + 1]);
    mx = max3(mx, s[0][15], s[1][0]);
#pragma unroll
    for (int r = 1; r < 15; r += 2) mx = max3(mx, s[1][r], s[1][r + 1]);
    mx = xhalf_max(__builtin_fmaxf(mx, s[1][15]));
    const float mt = mx * scale_log2;
    if (kt == 0 || __builtin_amdgcn_ballot_w64(mt - m_run > 8.0f) != 0) {      // wave-uniform: the reference is raised on the first tile and when outgrown by 2^8
      const float m_new = fmaxf(m_run, mt);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_part *= alpha;
#pragma unroll
      for (int db = 0; db < C::NB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
    }
    float p[2][16];
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[kb][r] = __builtin_amdgcn_exp2f(s[kb][r] * scale_log2 - m_run);
        psum += p[kb][r];
      }
    l_part += psum;
    // ---- O^T[d][q] += V^T P^T ----
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const s16x8 pb = pack8<OT>(&p[kb][c2 * 8]);
#pragma unroll
        for (int db = 0; db < C::NB; ++db) o[db] = MFMA32(dh_frag_tr(vt_, kb * 32 + 16 * c2, db, lane), pb, o[db]);
      }
    if (kt + 1 < nt) {
      dh_sstore<D>(rk, smem[st ^ 1][0], t);      // (the other stage is free since the barrier that closed tile kt - 1)
      dh_sstore<D>(rv, smem[st ^ 1][1], t);
    }
    __syncthreads();
  }
  const float l = l_part + __shfl_xor(l_part, 32, 64);
  const float inv = 1.0f / l;
  if (!active) return;
  uint16_t* op = out + ((int64_t)b * N + q0 + l31) * (H * D) + h * D;
#pragma unroll
  for (int db = 0; db < C::NB; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = db * 32 + 8 * g4 + 4 * hi;
      u32x2 w = {pack2<OT>(o[db][g4 * 4 + 0] * inv, o[db][g4 * 4 + 1] * inv), pack2<OT>(o[db][g4 * 4 + 2] * inv, o[db][g4 * 4 + 3] * inv)};
      *reinterpret_cast<u32x2*>(op + d0) = w;
    }
  if (hi == 0) lse[((int64_t)b * H + h) * N + q0 + l31] = (m_run + __builtin_amdgcn_logf(l)) * ATT_LN2;
}

// =================================================================================================
// backward: dQ (the forward's skeleton; the K tile is read both as rows and transposed).  Also writes delta = rowsum(dO o O) for the dK/dV kernel.
// =================================================================================================
template <int D, typename OT>
__global__ __launch_bounds__(256) void attn_dh_bwd_dq_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o, const uint16_t* __restrict__ d_o,
                                                             const float* __restrict__ lse, float* __restrict__ delta, int B, int N, int H, float scale,
                                                             float scale_log2, uint16_t* __restrict__ dqkv) {
  using C = AttDh<D>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][2][C::TILE_BYTES];  // [stage][K | V]
  int blk, head;
  if (!att_block_coords((N + 127) / 128, B * H, blk, head)) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = head / H, h = head - b * H;
  const int q0 = blk * 128 + wave * 32;
  const int64_t RS = (int64_t)3 * H * D;
  const int64_t OS = (int64_t)H * D;
  const uint16_t* Qp = qkv + (int64_t)b * N * RS + h * D;
  const uint16_t* Kp = Qp + H * D;
  const uint16_t* Vp = Kp + H * D;
  const uint16_t* dOp = d_o + (int64_t)b * N * OS + h * D;
  const uint16_t* Op = o + (int64_t)b * N * OS + h * D;

  const bool active = q0 + l31 < N;
  const int qrow = min(q0 + l31, N - 1);
  s16x8 qf[C::ND], dof[C::ND];
  float dpart = 0.f;      // delta[q] = sum_d dO[q][d] O[q][d]: half a row per lane, one cross-half exchange
#pragma unroll
  for (int ds = 0; ds < C::ND; ++ds) {
    qf[ds] = *reinterpret_cast<const s16x8*>(Qp + (int64_t)qrow * RS + ds * 16 + hi * 8);
    dof[ds] = *reinterpret_cast<const s16x8*>(dOp + (int64_t)qrow * OS + ds * 16 + hi * 8);
    const s16x8 of = *reinterpret_cast<const s16x8*>(Op + (int64_t)qrow * OS + ds * 16 + hi * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) dpart += unpack1<OT>((uint16_t)of[k]) * unpack1<OT>((uint16_t)dof[ds][k]);
  }
  const float lse_q = lse[((int64_t)b * H + h) * N + qrow] * ATT_LOG2E;
  const float del_q = dpart + __shfl_xor(dpart, 32, 64);
  if (active && hi == 0) delta[((int64_t)b * H + h) * N + qrow] = del_q;

  f32x16 dq[C::NB];
#pragma unroll
  for (int db = 0; db < C::NB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[db][r] = 0.f;

  const int nt = (N + 63) / 64;
  u32x4 rk[C::NLD], rv[C::NLD];
  dh_gload<D>(rk, Kp, RS, 0, N, t);
  dh_gload<D>(rv, Vp, RS, 0, N, t);
  dh_sstore<D>(rk, smem[0][0], t);
  dh_sstore<D>(rv, smem[0][1], t);
  __syncthreads();
  for (int kt = 0; kt < nt; ++kt) {
    const int st = kt & 1;
    if (kt + 1 < nt) {
      dh_gload<D>(rk, Kp, RS, (kt + 1) * 64, N, t);
      dh_gload<D>(rv, Vp, RS, (kt + 1) * 64, N, t);
    }
    const unsigned char* kt_ = smem[st][0];
    const unsigned char* vt_ = smem[st][1];
    const int n_keys = N - kt * 64;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = att_key_bias(kb, r, hi, n_keys); dp[r] = 0.f; }
#pragma unroll
      for (int ds = 0; ds < C::ND; ++ds) {
        s = MFMA32(dh_frag_row(kt_, kb * 32, ds, l31, hi), qf[ds], s);        // S^T[key][q]
        dp = MFMA32(dh_frag_row(vt_, kb * 32, ds, l31, hi), dof[ds], dp);     // dP^T[key][q] = V dO^T
      }
      float dsv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) dsv[r] = __builtin_amdgcn_exp2f(s[r] * scale_log2 - lse_q) * (dp[r] - del_q);      // (the factor `scale` of dS: once, on the finished dQ)
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const s16x8 dsb = pack8<OT>(&dsv[c2 * 8]);
#pragma unroll
        for (int db = 0; db < C::NB; ++db) dq[db] = MFMA32(dh_frag_tr(kt_, kb * 32 + 16 * c2, db, lane), dsb, dq[db]);      // dQ^T[d][q] += K^T dS^T
      }
    }
    if (kt + 1 < nt) {
      dh_sstore<D>(rk, smem[st ^ 1][0], t);
      dh_sstore<D>(rv, smem[st ^ 1][1], t);
    }
    __syncthreads();
  }
  if (!active) return;
  uint16_t* op = dqkv + ((int64_t)b * N + q0 + l31) * RS + h * D;
#pragma unroll
  for (int db = 0; db < C::NB; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = db * 32 + 8 * g4 + 4 * hi;
      u32x2 w = {pack2<OT>(dq[db][g4 * 4 + 0] * scale, dq[db][g4 * 4 + 1] * scale), pack2<OT>(dq[db][g4 * 4 + 2] * scale, dq[db][g4 * 4 + 3] * scale)};
      *reinterpret_cast<u32x2*>(op + d0) = w;
    }
}

// =================================================================================================
// backward: dK, dV (workgroup owns 128 keys; Q / dO stream through LDS in 64-query tiles).  kscale: the factor of the finished dK (scale, or ln 2 when
// the stored q is pre-scaled by scale * log2e).
// =================================================================================================
template <int D, typename OT>
__global__ __launch_bounds__(256) void attn_dh_bwd_dkv_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ d_o, const float* __restrict__ lse,
                                                              const float* __restrict__ delta, int B, int N, int H, float kscale, float scale_log2,
                                                              uint16_t* __restrict__ dqkv) {
  using C = AttDh<D>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][2][C::TILE_BYTES];  // [stage][Q | dO]
  __shared__ __attribute__((aligned(16))) float s_stat[2][2][64];                   // [stage][lse * log2e | delta]
  int blk, head;
  if (!att_block_coords((N + 127) / 128, B * H, blk, head)) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = head / H, h = head - b * H;
  const int key0 = blk * 128 + wave * 32;
  const int64_t RS = (int64_t)3 * H * D;
  const int64_t OS = (int64_t)H * D;
  const uint16_t* Qp = qkv + (int64_t)b * N * RS + h * D;
  const uint16_t* Kp = Qp + H * D;
  const uint16_t* Vp = Kp + H * D;
  const uint16_t* dOp = d_o + (int64_t)b * N * OS + h * D;
  const float* lsep = lse + ((int64_t)b * H + h) * N;
  const float* delp = delta + ((int64_t)b * H + h) * N;

  const bool active = key0 + l31 < N;
  const int krow = min(key0 + l31, N - 1);
  s16x8 kf[C::ND], vf[C::ND];
#pragma unroll
  for (int ds = 0; ds < C::ND; ++ds) {
    kf[ds] = *reinterpret_cast<const s16x8*>(Kp + (int64_t)krow * RS + ds * 16 + hi * 8);
    vf[ds] = *reinterpret_cast<const s16x8*>(Vp + (int64_t)krow * RS + ds * 16 + hi * 8);
  }
  f32x16 dk[C::NB], dv[C::NB];
#pragma unroll
  for (int db = 0; db < C::NB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[db][r] = 0.f; dv[db][r] = 0.f; }

  const int nt = (N + 63) / 64;
  // statistics of a tile's 64 queries: threads 0-63 fetch lse (kept in the log2 domain), 64-127 delta, through one select-addressed load.  A query row
  // >= N reads the image's last row and is replaced where it is stored: lse = -ATT_MASK_BIAS makes P = exp2(s - lse) exactly 0, delta = 0.
  const float* statp = (t & 64) ? delp : lsep;
  const float stat_mul = (t & 64) ? 1.0f : ATT_LOG2E;
  const float stat_masked = (t & 64) ? 0.f : -ATT_MASK_BIAS;
  u32x4 rq[C::NLD], rdo[C::NLD];
  dh_gload<D>(rq, Qp, RS, 0, N, t);
  dh_gload<D>(rdo, dOp, OS, 0, N, t);
  float rstat = statp[min(t & 63, N - 1)];
  dh_sstore<D>(rq, smem[0][0], t);
  dh_sstore<D>(rdo, smem[0][1], t);
  if (t < 128) s_stat[0][t >> 6][t & 63] = (t & 63) >= N ? stat_masked : rstat * stat_mul;
  __syncthreads();
  for (int qt = 0; qt < nt; ++qt) {
    const int st = qt & 1;
    if (qt + 1 < nt) {
      dh_gload<D>(rq, Qp, RS, (qt + 1) * 64, N, t);
      dh_gload<D>(rdo, dOp, OS, (qt + 1) * 64, N, t);
      rstat = statp[min((qt + 1) * 64 + (t & 63), N - 1)];
    }
    const unsigned char* qt_ = smem[st][0];
    const unsigned char* dot_ = smem[st][1];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      f32x16 s, dp, lrow, drow;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {           // the statistics of the 16 query rows this lane holds (rows 8 g4 + 4 hi + 0..3 of the block)
        const int row0 = qb * 32 + 8 * g4 + 4 * hi;
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(&s_stat[st][0][row0]);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(&s_stat[st][1][row0]);
#pragma unroll
        for (int k = 0; k < 4; ++k) { lrow[g4 * 4 + k] = l4[k]; drow[g4 * 4 + k] = d4[k]; }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int ds = 0; ds < C::ND; ++ds) {
        s = MFMA32(dh_frag_row(qt_, qb * 32, ds, l31, hi), kf[ds], s);        // S[q][key]
        dp = MFMA32(dh_frag_row(dot_, qb * 32, ds, l31, hi), vf[ds], dp);     // dP[q][key] = dO V^T
      }
      float pv[16], dsv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        pv[r] = __builtin_amdgcn_exp2f(s[r] * scale_log2 - lrow[r]);
        dsv[r] = pv[r] * (dp[r] - drow[r]);      // (the factor of dS: once, on the finished dK)
      }
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const s16x8 pa = pack8<OT>(&pv[c2 * 8]);
        const s16x8 dsa = pack8<OT>(&dsv[c2 * 8]);
#pragma unroll
        for (int db = 0; db < C::NB; ++db) {
          dv[db] = MFMA32(dh_frag_tr(dot_, qb * 32 + 16 * c2, db, lane), pa, dv[db]);      // dV^T[d][key] += dO^T P
          dk[db] = MFMA32(dh_frag_tr(qt_, qb * 32 + 16 * c2, db, lane), dsa, dk[db]);      // dK^T[d][key] += Q^T dS
        }
      }
    }
    if (qt + 1 < nt) {
      dh_sstore<D>(rq, smem[st ^ 1][0], t);
      dh_sstore<D>(rdo, smem[st ^ 1][1], t);
      if (t < 128) s_stat[st ^ 1][t >> 6][t & 63] = (qt + 1) * 64 + (t & 63) >= N ? stat_masked : rstat * stat_mul;
    }
    __syncthreads();
  }
  if (!active) return;
  // D^T[d][key]: lane (key = key0 + l31, hi) holds d = db*32 + 8*(r>>2) + 4*hi + (r&3): four consecutive d per register group -> 8-byte stores
  uint16_t* dkp = dqkv + ((int64_t)b * N + key0 + l31) * RS + H * D + h * D;
  uint16_t* dvp = dkp + H * D;
#pragma unroll
  for (int db = 0; db < C::NB; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = db * 32 + 8 * g4 + 4 * hi;
      const u32x2 wk = {pack2<OT>(dk[db][g4 * 4 + 0] * kscale, dk[db][g4 * 4 + 1] * kscale), pack2<OT>(dk[db][g4 * 4 + 2] * kscale, dk[db][g4 * 4 + 3] * kscale)};
      const u32x2 wv = {pack2<OT>(dv[db][g4 * 4 + 0], dv[db][g4 * 4 + 1]), pack2<OT>(dv[db][g4 * 4 + 2], dv[db][g4 * 4 + 3])};
      *reinterpret_cast<u32x2*>(dkp + d0) = wk;
      *reinterpret_cast<u32x2*>(dvp + d0) = wv;
    }
}
