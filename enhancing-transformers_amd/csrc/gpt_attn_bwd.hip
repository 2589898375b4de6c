// gpt_attn_bwd.hip — the backward of the stage-2 GPT's causal attention for gfx950 (forward: gpt_prefill.hip gpt_prefill_causal_kernel).
//
//   enh_causal_attention_backward   dqkv [B,N,3HD] from qkv, the stored out and lse, and dout; head widths D = 64 .. 384 in steps of 64, any N >= 1
//
// Flash-style: no N x N matrix in memory.  P is recomputed from lse, delta = rowsum(dO o O) is taken on the STORED out (the 16-bit values the
// forward wrote: what proj consumed).  Two kernels on v_mfma_f32_32x32x16 with the arithmetic of attention_dh.h's attn_dh_bwd_dq_kernel /
// attn_dh_bwd_dkv_kernel and the causal structure of gpt_prefill_causal_kernel: tiles wholly on the masked side of the diagonal are neither loaded
// nor computed, masked entries get ATT_MASK_BIAS through the C operand (P exactly 0), rows are clamped, stores guarded, longest blocks first.
// No float atomics; every sum runs in a fixed order: the same bits on every run.
#include "attention_dh.h"

// The budget (one wave per SIMD: 512 registers per lane; 160 KB LDS).  Both kernels contract the scores AND dP over the full D, so each holds two
// fragment sets of D / 16 x 4 registers (Q and dO, or K and V: 192 at D = 384) besides its accumulators.  Above D = 128 a workgroup therefore owns
// a slice of DS <= 128 OUTPUT columns (grid.y = NS slices) and contracts S and dP over the full D:
//   dQ      DS = 64, 128, 96, 128, 128, 128 at D = 64 .. 384: at most 64 accumulator registers;
//   dK/dV   DS = 64, 128, 96,  64,  64,  64: two outputs, so twice the accumulators of dQ per column.  With DS = 128 the compiler left 43 / 108 / 209
//           registers in scratch at D = 256 / 320 / 384 (-Rpass-analysis=kernel-resource-usage); with 64 every width is free of scratch.
// D = 320 in the dQ kernel is three slices of 128 whose last one owns 64 live columns: its two dead accumulator blocks repeat the last live block
// and are never stored.  A [64][D] tile pair is D x 256 bytes: two ring stages up to D = 256 (128 KB), one above (80 / 96 KB: request, wait, compute).
// The price is the S / dP products computed NS times.  MFMAs per 32 x 32 block with ND = D / 16, unsplit: dQ 2 ND + ND, dK/dV 2 ND + 2 ND; sliced:
// dQ NS 2 ND + NS DS / 16 and dK/dV NS 2 ND + 2 NS DS / 16.  Both kernels together, against the unsplit 7 ND: 1.00, 1.00, 1.57, 2.14, 2.74, 3.00 x
// at D = 64 .. 384.
template <int D, bool DKV>
struct GbAtt {
  static_assert(D % 64 == 0 && D >= 64 && D <= 384, "head widths of the stage-2 GPT");
  static constexpr int DS = DKV && D >= 256 ? 64 : (D <= 128 ? D : (D == 192 ? 96 : 128));   // output columns of one workgroup
  static constexpr int NS = (D + DS - 1) / DS;                      // workgroups (grid.y) per block
  static constexpr int ND = D / 16;                                 // 32x32x16 steps of a contraction over d
  static constexpr int NB = DS / 32;                                // accumulator blocks of one output
  static constexpr int NBT = D / 32;                                // 32-column blocks of the head
  static constexpr int TILE_BYTES = (D / 64) * ATT_TILE_BYTES;
  static constexpr int NSTG = 4 * TILE_BYTES <= 128 * 1024 ? 2 : 1;
};

// a [64][D] tile by LDS-DMA (attention_common.h att_dma_tile_clamped: one [64][64] image per 64 columns, rows clamped to n_rows - 1): no staging registers
template <int D>
__device__ __forceinline__ void gb_dma(const uint16_t* __restrict__ p, int64_t rs, int row0, int n_rows, unsigned char* tile, int wave, int lane) {
#pragma unroll
  for (int im = 0; im < D / 64; ++im) att_dma_tile_clamped(p + im * 64, rs, row0, n_rows, tile + im * ATT_TILE_BYTES, wave, lane);
}
#define GB_DMA_LANDED() __builtin_amdgcn_s_waitcnt(0x0070)      // vmcnt(0) (and lgkmcnt(0)): in front of the barrier that publishes a DMA-written tile

// =================================================================================================
// dQ: workgroup = 128 queries (4 waves x 32) of one (batch, head) and one slice of dQ's columns; K / V in 64-key tiles 0 .. (last query) / 64.
// Also writes delta = rowsum(dO o O) for the dK/dV kernel (slice 0).  Query 0 sees one key: P = 1 and dS = 0 whatever the values, so its row of
// dQ is written as exact zeros (its statistic is replaced by one that makes P exactly 0) instead of the rounding residue of dP - delta.
// =================================================================================================
template <int D, typename OT>
__global__ __launch_bounds__(256) void gpt_causal_bwd_dq_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o, const uint16_t* __restrict__ d_o,
                                                                const float* __restrict__ lse, float* __restrict__ delta, int B, int N, int H, float scale,
                                                                float scale_log2, uint16_t* __restrict__ dqkv) {
  using C = GbAtt<D, false>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[C::NSTG][2][C::TILE_BYTES];  // [stage][K | V]
  const int nblk = (N + 127) / 128, heads = B * H, ngroups = (heads + 7) / 8;
  const int Lid = blockIdx.x, r8 = Lid >> 3;
  const int blk = nblk - 1 - r8 / ngroups;      // last block first: it has the most key tiles
  const int head = (r8 % ngroups) * 8 + (Lid & 7);
  if (head >= heads) return;
  const int z = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
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

  const bool wave_live = q0 < N;
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
  const float lse_q = qrow == 0 ? -ATT_MASK_BIAS : lse[((int64_t)b * H + h) * N + qrow] * ATT_LOG2E;
  const float del_q = dpart + __shfl_xor(dpart, 32, 64);
  if (active && hi == 0 && z == 0) delta[((int64_t)b * H + h) * N + qrow] = del_q;

  f32x16 dq[C::NB];
#pragma unroll
  for (int db = 0; db < C::NB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[db][r] = 0.f;

  const int nt = min(blk * 128 + 127, N - 1) / 64 + 1;      // tiles whose first key is not past the block's last query
  gb_dma<D>(Kp, RS, 0, N, smem[0][0], wave, lane);
  gb_dma<D>(Vp, RS, 0, N, smem[0][1], wave, lane);
  GB_DMA_LANDED();
  __syncthreads();
  int st = 0;
  for (int kt = 0; kt < nt; ++kt) {
    const bool more = kt + 1 < nt;
    if (C::NSTG == 2 && more) {      // (the other stage is free since the barrier that closed tile kt - 1)
      gb_dma<D>(Kp, RS, (kt + 1) * 64, N, smem[st ^ 1][0], wave, lane);
      gb_dma<D>(Vp, RS, (kt + 1) * 64, N, smem[st ^ 1][1], wave, lane);
    }
    if (wave_live && kt * 64 <= q0) {      // wave-uniform: tiles wholly above this wave's diagonal are skipped
      const unsigned char* kt_ = smem[st][0];
      const unsigned char* vt_ = smem[st][1];
      const int k_live = qrow - kt * 64;      // this lane's query sees tile keys 0 .. k_live
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = kb * 32 + 8 * (r >> 2) + 4 * hi + (r & 3) <= k_live ? 0.f : ATT_MASK_BIAS; dp[r] = 0.f; }
#pragma unroll
        for (int ds = 0; ds < C::ND; ++ds) {
          s = MFMA32(dh_frag_row(kt_, kb * 32, ds, l31, hi), qf[ds], s);        // S^T[key][q]
          dp = MFMA32(dh_frag_row(vt_, kb * 32, ds, l31, hi), dof[ds], dp);     // dP^T[key][q] = V dO^T
          if ((ds & 3) == 3) ATT_FENCE();      // (keeps the fragment reads of later steps behind these products: hoisted, they cost D / 2 registers)
        }
        ATT_FENCE();
        float dsv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) dsv[r] = __builtin_amdgcn_exp2f(s[r] * scale_log2 - lse_q) * (dp[r] - del_q);      // (the factor `scale` of dS: once, on the finished dQ)
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
          const s16x8 dsb = pack8<OT>(&dsv[c2 * 8]);
#pragma unroll
          for (int db = 0; db < C::NB; ++db)      // dQ^T[d][q] += K^T dS^T over this workgroup's columns
            dq[db] = MFMA32(dh_frag_tr(kt_, kb * 32 + 16 * c2, min(z * C::NB + db, C::NBT - 1), lane), dsb, dq[db]);
          ATT_FENCE();
        }
      }
    }
    if (C::NSTG == 1) {
      __syncthreads();      // every wave is done with the only stage
      if (more) {
        gb_dma<D>(Kp, RS, (kt + 1) * 64, N, smem[0][0], wave, lane);
        gb_dma<D>(Vp, RS, (kt + 1) * 64, N, smem[0][1], wave, lane);
      }
    } else {
      st ^= 1;
    }
    GB_DMA_LANDED();
    __syncthreads();
  }
  if (!active) return;
  uint16_t* op = dqkv + ((int64_t)b * N + q0 + l31) * RS + h * D;
#pragma unroll
  for (int db = 0; db < C::NB; ++db) {
    if (z * C::NB + db >= C::NBT) continue;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = (z * C::NB + db) * 32 + 8 * g4 + 4 * hi;
      u32x2 w = {pack2<OT>(dq[db][g4 * 4 + 0] * scale, dq[db][g4 * 4 + 1] * scale), pack2<OT>(dq[db][g4 * 4 + 2] * scale, dq[db][g4 * 4 + 3] * scale)};
      *reinterpret_cast<u32x2*>(op + d0) = w;
    }
  }
}

// =================================================================================================
// dK, dV: workgroup = 128 keys (4 waves x 32) and one slice of dK's / dV's columns; Q / dO stream through LDS in 64-query tiles from the tile that
// holds the block's first key to the last.  Query rows >= N get the statistic that makes P exactly 0; queries before the key get ATT_MASK_BIAS.
// =================================================================================================
template <int D, typename OT>
__global__ __launch_bounds__(256) void gpt_causal_bwd_dkv_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ d_o, const float* __restrict__ lse,
                                                                 const float* __restrict__ delta, int B, int N, int H, float scale, float scale_log2,
                                                                 uint16_t* __restrict__ dqkv) {
  using C = GbAtt<D, true>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[C::NSTG][2][C::TILE_BYTES];  // [stage][Q | dO]
  __shared__ __attribute__((aligned(16))) float s_stat[C::NSTG][2][64];                   // [stage][lse * log2e | delta]
  const int nblk = (N + 127) / 128, heads = B * H, ngroups = (heads + 7) / 8;
  const int Lid = blockIdx.x, r8 = Lid >> 3;
  const int blk = r8 / ngroups;      // first block first: every query tile from its diagonal on
  const int head = (r8 % ngroups) * 8 + (Lid & 7);
  if (head >= heads || blk >= nblk) return;
  const int z = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
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

  const bool wave_live = key0 < N;
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

  const int qt0 = blk * 2, ntq = (N + 63) / 64;      // query tiles qt0 .. ntq - 1 (blk < nblk: qt0 < ntq)
  // statistics of a tile's 64 queries: threads 0-63 fetch lse (kept in the log2 domain), 64-127 delta.  A query row >= N reads the last row and is
  // replaced where it is stored: lse = -ATT_MASK_BIAS makes P = exp2(s - lse) exactly 0, delta = 0.
  const float* statp = (t & 64) ? delp : lsep;
  const float stat_mul = (t & 64) ? 1.0f : ATT_LOG2E;
  const float stat_masked = (t & 64) ? 0.f : -ATT_MASK_BIAS;
  gb_dma<D>(Qp, RS, qt0 * 64, N, smem[0][0], wave, lane);
  gb_dma<D>(dOp, OS, qt0 * 64, N, smem[0][1], wave, lane);
  float rstat = statp[min(qt0 * 64 + (t & 63), N - 1)];
  if (t < 128) s_stat[0][t >> 6][t & 63] = qt0 * 64 + (t & 63) >= N ? stat_masked : rstat * stat_mul;
  GB_DMA_LANDED();
  __syncthreads();
  int st = 0;
  for (int qt = qt0; qt < ntq; ++qt) {
    const bool more = qt + 1 < ntq;
    if (C::NSTG == 2 && more) {
      gb_dma<D>(Qp, RS, (qt + 1) * 64, N, smem[st ^ 1][0], wave, lane);
      gb_dma<D>(dOp, OS, (qt + 1) * 64, N, smem[st ^ 1][1], wave, lane);
      rstat = statp[min((qt + 1) * 64 + (t & 63), N - 1)];
    }
    if (wave_live && qt * 64 + 63 >= key0) {      // wave-uniform: tiles wholly before this wave's first key are skipped
      const unsigned char* qt_ = smem[st][0];
      const unsigned char* dot_ = smem[st][1];
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        const int q_rel = qt * 64 + qb * 32 + 4 * hi - krow;      // (query of accumulator register 0) - (this lane's key)
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = q_rel + 8 * (r >> 2) + (r & 3) >= 0 ? 0.f : ATT_MASK_BIAS; dp[r] = 0.f; }
#pragma unroll
        for (int ds = 0; ds < C::ND; ++ds) {
          s = MFMA32(dh_frag_row(qt_, qb * 32, ds, l31, hi), kf[ds], s);        // S[q][key]
          dp = MFMA32(dh_frag_row(dot_, qb * 32, ds, l31, hi), vf[ds], dp);     // dP[q][key] = dO V^T
          if ((ds & 3) == 3) ATT_FENCE();
        }
        ATT_FENCE();
        float pv[16], dsv[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {           // the statistics of the 16 query rows this lane holds (rows 8 g4 + 4 hi + 0..3 of the block)
          const int row0 = qb * 32 + 8 * g4 + 4 * hi;
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(&s_stat[st][0][row0]);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(&s_stat[st][1][row0]);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int r = g4 * 4 + k;
            pv[r] = __builtin_amdgcn_exp2f(s[r] * scale_log2 - l4[k]);
            dsv[r] = pv[r] * (dp[r] - d4[k]);      // (the factor of dS: once, on the finished dK)
          }
        }
        if (qt == 0 && qb == 0 && hi == 0) dsv[0] = 0.f;      // query 0 sees one key: dS = 0 whatever the values (see the dQ kernel)
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
          const s16x8 pa = pack8<OT>(&pv[c2 * 8]);
          const s16x8 dsa = pack8<OT>(&dsv[c2 * 8]);
#pragma unroll
          for (int db = 0; db < C::NB; ++db) {
            const int dbg = min(z * C::NB + db, C::NBT - 1);
            dv[db] = MFMA32(dh_frag_tr(dot_, qb * 32 + 16 * c2, dbg, lane), pa, dv[db]);      // dV^T[d][key] += dO^T P
            dk[db] = MFMA32(dh_frag_tr(qt_, qb * 32 + 16 * c2, dbg, lane), dsa, dk[db]);      // dK^T[d][key] += Q^T dS
          }
          ATT_FENCE();
        }
      }
    }
    int sn = st ^ 1;
    if (C::NSTG == 1) {
      sn = 0;
      __syncthreads();      // every wave is done with the only stage
      if (more) {
        gb_dma<D>(Qp, RS, (qt + 1) * 64, N, smem[0][0], wave, lane);
        gb_dma<D>(dOp, OS, (qt + 1) * 64, N, smem[0][1], wave, lane);
        rstat = statp[min((qt + 1) * 64 + (t & 63), N - 1)];
      }
    }
    if (more && t < 128) s_stat[sn][t >> 6][t & 63] = (qt + 1) * 64 + (t & 63) >= N ? stat_masked : rstat * stat_mul;
    if (C::NSTG == 2) st ^= 1;
    GB_DMA_LANDED();
    __syncthreads();
  }
  if (!active) return;
  // D^T[d][key]: lane (key = key0 + l31, hi) holds d = db*32 + 8*(r>>2) + 4*hi + (r&3): four consecutive d per register group -> 8-byte stores
  uint16_t* dkp = dqkv + ((int64_t)b * N + key0 + l31) * RS + H * D + h * D;
  uint16_t* dvp = dkp + H * D;
#pragma unroll
  for (int db = 0; db < C::NB; ++db) {
    if (z * C::NB + db >= C::NBT) continue;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = (z * C::NB + db) * 32 + 8 * g4 + 4 * hi;
      const u32x2 wk = {pack2<OT>(dk[db][g4 * 4 + 0] * scale, dk[db][g4 * 4 + 1] * scale), pack2<OT>(dk[db][g4 * 4 + 2] * scale, dk[db][g4 * 4 + 3] * scale)};
      const u32x2 wv = {pack2<OT>(dv[db][g4 * 4 + 0], dv[db][g4 * 4 + 1]), pack2<OT>(dv[db][g4 * 4 + 2], dv[db][g4 * 4 + 3])};
      *reinterpret_cast<u32x2*>(dkp + d0) = wk;
      *reinterpret_cast<u32x2*>(dvp + d0) = wv;
    }
  }
}

#define GB_D_DISPATCH(D, dtype, CALL)                                               \
  do {                                                                              \
    if ((D) == 64) { constexpr int DH = 64; ENH_DT_DISPATCH(dtype, CALL); }         \
    else if ((D) == 128) { constexpr int DH = 128; ENH_DT_DISPATCH(dtype, CALL); }  \
    else if ((D) == 192) { constexpr int DH = 192; ENH_DT_DISPATCH(dtype, CALL); }  \
    else if ((D) == 256) { constexpr int DH = 256; ENH_DT_DISPATCH(dtype, CALL); }  \
    else if ((D) == 320) { constexpr int DH = 320; ENH_DT_DISPATCH(dtype, CALL); }  \
    else { constexpr int DH = 384; ENH_DT_DISPATCH(dtype, CALL); }                  \
  } while (0)

extern "C" size_t enh_causal_attention_backward_workspace_bytes(int B, int N, int H) {
  return B > 0 && N > 0 && H > 0 ? (size_t)B * H * N * sizeof(float) : 0;      // delta [B, H, N]
}

extern "C" int enh_causal_attention_backward(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse, int B, int N, int H, int D,
                                             float scale, enh_h16* dqkv, void* ws, size_t ws_bytes, int dtype, void* stream) {
  ENH_REQUIRE(D >= 64 && D <= 384 && D % 64 == 0, ENH_E_SHAPE, "enh_causal_attention_backward: dim_head must be a multiple of 64 up to 384, got %d", D);
  ENH_REQUIRE_DT(dtype, "enh_causal_attention_backward");
  ENH_REQUIRE(qkv && out && dout && lse && dqkv, ENH_E_BADARG, "enh_causal_attention_backward: null pointer");
  ENH_REQUIRE(B > 0 && H > 0 && N > 0, ENH_E_SHAPE, "enh_causal_attention_backward: need positive B, N, H (B=%d N=%d H=%d)", B, N, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_causal_attention_backward: scale must be positive");
  ENH_REQUIRE(ws && ws_bytes >= enh_causal_attention_backward_workspace_bytes(B, N, H), ENH_E_WORKSPACE,
              "enh_causal_attention_backward: workspace too small (%zu bytes)", ws_bytes);
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H, wgs = ((heads + 7) / 8) * 8 * nblk;
  ENH_REQUIRE(wgs <= 2147483647LL, ENH_E_SHAPE, "enh_causal_attention_backward: too many workgroups (B=%d N=%d H=%d)", B, N, H);
  float* delta = (float*)ws;
  hipStream_t s = (hipStream_t)stream;
  GB_D_DISPATCH(D, dtype, (gpt_causal_bwd_dq_kernel<DH, OT><<<dim3((unsigned)wgs, GbAtt<DH, false>::NS), 256, 0, s>>>(qkv, out, dout, lse, delta, B, N, H, scale, scale * ATT_LOG2E, dqkv)));
  enh_note_kernel_dh("gpt_causal_bwd_dkv_kernel", D, dtype);
  GB_D_DISPATCH(D, dtype, (gpt_causal_bwd_dkv_kernel<DH, OT><<<dim3((unsigned)wgs, GbAtt<DH, true>::NS), 256, 0, s>>>(qkv, dout, lse, delta, B, N, H, scale, scale * ATT_LOG2E, dqkv)));
  return enh_check_launch("enh_causal_attention_backward");
}
