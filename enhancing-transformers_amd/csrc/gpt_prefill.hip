// gpt_prefill.hip — the causal attention of the stage-2 GPT's teacher-forced forward for gfx950 (reference enhancing/modules/stage2/layers.py:
// MultiHeadSelfAttention.forward 57-97 with cond_num_tokens == 1).  Where gpt_decode.hip sees one token per batch row and step, the forward sees
// M = B S token rows at once: the wide GEMMs are enh_gemm_h16's, the row kernels between them are gpt_rows.hip's, and the attention is here.
//
//   enh_causal_attention_forward   causal flash attention, head widths D = 64 .. 384 in steps of 64, on v_mfma_f32_32x32x16 (gpt_prefill_causal_kernel<D, OT>
//                                  below: the arithmetic of attention_dh.h, tiles above the diagonal neither loaded nor computed)
//   enh_causal_attention_forward_f32  the exact mode's form on the vector ALU: a parity instrument
// No float atomics; every sum runs in a fixed order: the same bits on every run.
#include "attention_dh.h"

#define PF_F32_ATT_MAX_N 8192

// ---------------------------------------------------------------------------------------------
// causal attention
// ---------------------------------------------------------------------------------------------
// The budget at D = 384 (one wave per SIMD, 512 registers per lane, 160 KB LDS): a lane's output accumulators would be D / 32 x 16 = 192 registers
// besides D / 16 x 4 = 96 of Q fragments, and a 64-key K + V tile pair is 96 KB, so no two-stage ring.  Above D = 128 a workgroup therefore owns
// HALF of V's width (DV = D / 2; grid.y = 2): it contracts the scores over the full D (K tile [64][D]) and accumulates O over its DV columns only
// (V tile [64][DV]).  At D = 384 that is 96 accumulator registers and a stage of 48 + 24 = 72 KB: the two-stage ring of attention_dh.h fits
// (144 KB) and the kernel keeps its structure.  The price is the score product computed twice: (D + DV) 2 / (2 D) = 1.5 x the MFMA work of an
// unsplit kernel.  In the GPT the attention is ~1.4 % of a layer's FLOPs (4 N^2 D H / 2 against 24 N C^2 at N = 1024, C = 6144).
template <int D>
struct PfAtt {
  static_assert(D % 64 == 0 && D >= 64 && D <= 384, "head widths of the stage-2 GPT");
  static constexpr int DV = D <= 128 ? D : D / 2;   // V / O columns of one workgroup: 64, 128, 96, 128, 160, 192
  static constexpr int NS = D / DV;                 // workgroups (grid.y) per query block
  static constexpr int ND = D / 16;                 // 32x32x16 steps of the score contraction
  static constexpr int NB = DV / 32;                // accumulator blocks of O
  static constexpr int K_BYTES = ((D + 63) / 64) * ATT_TILE_BYTES;
  static constexpr int V_BYTES = ((DV + 63) / 64) * ATT_TILE_BYTES;
};

// dh_gload / dh_sstore of attention_dh.h for a [64][W] tile, W a multiple of 32: rows clamped to n_rows - 1, chunk q = t + 256 i
template <int W>
__device__ __forceinline__ void pf_gload(u32x4 (&r)[W / 32], const uint16_t* __restrict__ base, int64_t rs, int row0, int n_rows, int t) {
#pragma unroll
  for (int i = 0; i < W / 32; ++i) {
    const int q = t + 256 * i, row = q / (W / 8), c = q % (W / 8);
    r[i] = *reinterpret_cast<const u32x4*>(base + (int64_t)min(row0 + row, n_rows - 1) * rs + c * 8);
  }
}
template <int W>
__device__ __forceinline__ void pf_sstore(const u32x4 (&r)[W / 32], unsigned char* tile, int t) {
#pragma unroll
  for (int i = 0; i < W / 32; ++i) {
    const int q = t + 256 * i, row = q / (W / 8), c = q % (W / 8);
    *reinterpret_cast<u32x4*>(tile + (c >> 3) * ATT_TILE_BYTES + att_off(row, c & 7)) = r[i];
  }
}

// the K tile [64][D] by LDS-DMA (attention_common.h att_dma_tile_clamped, one [64][64] image per 64 columns): no staging registers — at D = 384 the
// K tile staged through registers (48 per lane) beside 96 of Q fragments and 96 of accumulators went to scratch.  The V slice keeps the register path:
// its width need not be whole images (DV = 96, 160), and a whole image would read past the head's columns.
template <int D>
__device__ __forceinline__ void pf_dma_k(const uint16_t* __restrict__ Kp, int64_t rs, int row0, int n_rows, unsigned char* tile, int wave, int lane) {
#pragma unroll
  for (int im = 0; im < D / 64; ++im) att_dma_tile_clamped(Kp + im * 64, rs, row0, n_rows, tile + im * ATT_TILE_BYTES, wave, lane);
}
#define PF_DMA_LANDED() __builtin_amdgcn_s_waitcnt(0x0070)      // vmcnt(0) (and lgkmcnt(0)): in front of the barrier that publishes a DMA-written tile

// Workgroup = 128 queries (4 waves x 32) of one (batch, head) and one V slice; K / V in 64-key tiles 0 .. (last query of the block) / 64 through
// a two-stage ring.  A wave skips the tiles wholly above ITS diagonal (first key > its last query; it still stages and meets the barriers); in
// every tile it computes, key 64 kt <= q0 is live for all of its lanes, so no row is ever all-masked.  Keys > query and keys >= N get
// ATT_MASK_BIAS through the C operand (probability exactly 0).
// Workgroup order: the work of a block grows with its position, so the blocks are dispatched LAST BLOCK FIRST across all heads (longest
// processing time first): the workgroups that start when the chip drains are the one-tile blocks at the top of the triangle.  The heads of one
// dispatch round keep att_block_coords' XCD rule (ids congruent mod 8 share a head's K / V in one L2).
template <int D, typename OT>
__global__ __launch_bounds__(256) void gpt_prefill_causal_kernel(const uint16_t* __restrict__ qkv, int B, int N, int H, float scale_log2,
                                                                 uint16_t* __restrict__ out, float* __restrict__ lse) {
  using C = PfAtt<D>;
  constexpr int DV = C::DV;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][C::K_BYTES + C::V_BYTES];  // [stage][K | V slice]
  const int nblk = (N + 127) / 128, heads = B * H, ngroups = (heads + 7) / 8;
  const int Lid = blockIdx.x, r8 = Lid >> 3;
  const int blk = nblk - 1 - r8 / ngroups;
  const int head = (r8 % ngroups) * 8 + (Lid & 7);
  if (head >= heads) return;
  const int z = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = head / H, h = head - b * H;
  const int q0 = blk * 128 + wave * 32;
  const int64_t RS = (int64_t)3 * H * D;
  const uint16_t* Qp = qkv + (int64_t)b * N * RS + h * D;
  const uint16_t* Kp = Qp + H * D;
  const uint16_t* Vp = Kp + H * D + z * DV;

  const bool wave_live = q0 < N;
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

  const int nt = min(blk * 128 + 127, N - 1) / 64 + 1;      // tiles whose first key is not past the block's last query
  u32x4 rv[DV / 32];
  pf_dma_k<D>(Kp, RS, 0, N, smem[0], wave, lane);
  pf_gload<DV>(rv, Vp, RS, 0, N, t);
  pf_sstore<DV>(rv, smem[0] + C::K_BYTES, t);
  PF_DMA_LANDED();
  __syncthreads();
  for (int kt = 0; kt < nt; ++kt) {
    const int st = kt & 1;
    if (kt + 1 < nt) {
      pf_dma_k<D>(Kp, RS, (kt + 1) * 64, N, smem[st ^ 1], wave, lane);      // (the other stage is free since the barrier that closed tile kt - 1)
      pf_gload<DV>(rv, Vp, RS, (kt + 1) * 64, N, t);
    }
    if (wave_live && kt * 64 <= q0) {      // wave-uniform
      const unsigned char* kt_ = smem[st];
      const unsigned char* vt_ = smem[st] + C::K_BYTES;
      const int k_live = qrow - kt * 64;      // this lane's query sees tile keys 0 .. k_live (qrow <= N - 1: the sequence's end bounds it too)
      // ---- S^T[key][q] = K Q^T (+ ATT_MASK_BIAS on keys past the query or the sequence) ----
      f32x16 s[2];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kb][r] = kb * 32 + 8 * (r >> 2) + 4 * hi + (r & 3) <= k_live ? 0.f : ATT_MASK_BIAS;
#pragma unroll
        for (int ds = 0; ds < C::ND; ++ds) s[kb] = MFMA32(dh_frag_row(kt_, kb * 32, ds, l31, hi), qf[ds], s[kb]);
        ATT_FENCE();      // (keeps the next block's fragment reads behind this block's products: hoisted, they cost D / 4 registers per block)
      }
      // ---- online softmax for this lane's query column (attention_dh.h's lane-local statistics) ----
      float mx = max3(s[0][0], s[0][1], s[0][2]);
#pragma unroll
      for (int r = 3; r < 15; r += 2) mx = max3(mx, s[0][r], s[0][r + 1]);
      mx = max3(mx, s[0][15], s[1][0]);
#pragma unroll
      for (int r = 1; r < 15; r += 2) mx = max3(mx, s[1][r], s[1][r + 1]);
      mx = xhalf_max(__builtin_fmaxf(mx, s[1][15]));
      const float mt = mx * scale_log2;
      // The reference is the EXACT running maximum (raised whenever a lane's maximum grows; wave-uniform branch), not attention_dh.h's reference
      // that lags by up to 2^8: a row's largest numerator is then exactly 1, as in the rounding model.  Early causal rows have few keys and one
      // of them often carries the row, so its rounding error showed: with the lagging reference the worst row was 1.4 - 2.1 x the model's.
      if (kt == 0 || __builtin_amdgcn_ballot_w64(mt > m_run) != 0) {
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
      ATT_FENCE();
      // ---- O^T[d][q] += V^T P^T over this workgroup's DV columns ----
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
          const s16x8 pb = pack8<OT>(&p[kb][c2 * 8]);
#pragma unroll
          for (int db = 0; db < C::NB; ++db) o[db] = MFMA32(dh_frag_tr(vt_, kb * 32 + 16 * c2, db, lane), pb, o[db]);
          ATT_FENCE();
        }
    }
    if (kt + 1 < nt) pf_sstore<DV>(rv, smem[st ^ 1] + C::K_BYTES, t);
    PF_DMA_LANDED();
    __syncthreads();
  }
  const float l = l_part + __shfl_xor(l_part, 32, 64);
  const float inv = 1.0f / l;
  if (!active) return;
  uint16_t* op = out + ((int64_t)b * N + q0 + l31) * (H * D) + h * D + z * DV;
#pragma unroll
  for (int db = 0; db < C::NB; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = db * 32 + 8 * g4 + 4 * hi;
      u32x2 w = {pack2<OT>(o[db][g4 * 4 + 0] * inv, o[db][g4 * 4 + 1] * inv), pack2<OT>(o[db][g4 * 4 + 2] * inv, o[db][g4 * 4 + 3] * inv)};
      *reinterpret_cast<u32x2*>(op + d0) = w;
    }
  if (lse && z == 0 && hi == 0) lse[((int64_t)b * H + h) * N + q0 + l31] = (m_run + __builtin_amdgcn_logf(l)) * ATT_LN2;
}

#define PF_D_DISPATCH(D, dtype, CALL)                                               \
  do {                                                                              \
    if ((D) == 64) { constexpr int DH = 64; ENH_DT_DISPATCH(dtype, CALL); }         \
    else if ((D) == 128) { constexpr int DH = 128; ENH_DT_DISPATCH(dtype, CALL); }  \
    else if ((D) == 192) { constexpr int DH = 192; ENH_DT_DISPATCH(dtype, CALL); }  \
    else if ((D) == 256) { constexpr int DH = 256; ENH_DT_DISPATCH(dtype, CALL); }  \
    else if ((D) == 320) { constexpr int DH = 320; ENH_DT_DISPATCH(dtype, CALL); }  \
    else { constexpr int DH = 384; ENH_DT_DISPATCH(dtype, CALL); }                  \
  } while (0)

extern "C" int enh_causal_attention_forward(const enh_h16* qkv, int B, int N, int H, int D, float scale, enh_h16* out, float* lse, int dtype, void* stream) {
  ENH_REQUIRE(D >= 64 && D <= 384 && D % 64 == 0, ENH_E_SHAPE, "enh_causal_attention_forward: dim_head must be a multiple of 64 up to 384, got %d", D);
  ENH_REQUIRE_DT(dtype, "enh_causal_attention_forward");
  ENH_REQUIRE(qkv && out, ENH_E_BADARG, "enh_causal_attention_forward: null pointer");
  ENH_REQUIRE(B > 0 && H > 0 && N > 0, ENH_E_SHAPE, "enh_causal_attention_forward: need positive B, N, H (B=%d N=%d H=%d)", B, N, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_causal_attention_forward: scale must be positive");
  const int64_t nblk = (N + 127) / 128, heads = (int64_t)B * H, wgs = ((heads + 7) / 8) * 8 * nblk;
  ENH_REQUIRE(wgs <= 2147483647LL, ENH_E_SHAPE, "enh_causal_attention_forward: too many workgroups (B=%d N=%d H=%d)", B, N, H);
  const dim3 grid((unsigned)wgs, (unsigned)(D <= 128 ? 1 : 2));
  enh_note_kernel_dh("gpt_prefill_causal_kernel", D, dtype);
  PF_D_DISPATCH(D, dtype, (gpt_prefill_causal_kernel<DH, OT><<<grid, 256, 0, (hipStream_t)stream>>>(qkv, B, N, H, scale * ATT_LOG2E, out, lse)));
  return enh_check_launch("enh_causal_attention_forward");
}

// exact mode: one workgroup per (batch, head, query).  Scores of keys 0 .. q into LDS (a thread per key, the D products of a score added in
// ascending d), softmax over them, then a thread per output column adds p_j V[j][d] in ascending j.  A parity instrument.
__global__ __launch_bounds__(256) void gpt_prefill_causal_f32_kernel(const float* __restrict__ qkv, int N, int H, int D, float scale,
                                                                     float* __restrict__ out, float* __restrict__ lse) {
  __shared__ float s_p[PF_F32_ATT_MAX_N];
  __shared__ float s_red[4];
  const int t = threadIdx.x;
  const int q = blockIdx.x % N, bh = blockIdx.x / N, b = bh / H, h = bh - b * H;
  const int64_t RS = (int64_t)3 * H * D;
  const float* Qr = qkv + ((int64_t)b * N + q) * RS + h * D;
  const float* Kb = qkv + (int64_t)b * N * RS + H * D + h * D;
  const float* Vb = Kb + H * D;
  float mx = -__builtin_inff();
  for (int j = t; j <= q; j += 256) {
    const float* kr = Kb + (int64_t)j * RS;
    float dot = 0.f;
    for (int d = 0; d < D; d += 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(Qr + d), k4 = *reinterpret_cast<const f32x4*>(kr + d);
      dot = fmaf(a.w, k4.w, fmaf(a.z, k4.z, fmaf(a.y, k4.y, fmaf(a.x, k4.x, dot))));
    }
    dot *= scale;
    s_p[j] = dot;
    mx = fmaxf(mx, dot);
  }
  mx = block_max<4>(mx, s_red);
  float ps = 0.f;
  for (int j = t; j <= q; j += 256) {
    const float e = expf(s_p[j] - mx);
    s_p[j] = e;
    ps += e;
  }
  const float l = block_sum<4>(ps, s_red);      // (its barriers publish s_p)
  for (int d = t; d < D; d += 256) {
    float acc = 0.f;
    for (int j = 0; j <= q; ++j) acc = fmaf(s_p[j], Vb[(int64_t)j * RS + d], acc);
    out[((int64_t)b * N + q) * (H * D) + h * D + d] = acc / l;
  }
  if (lse && t == 0) lse[((int64_t)b * H + h) * N + q] = mx + logf(l);
}

extern "C" int enh_causal_attention_forward_f32(const float* qkv, int B, int N, int H, int D, float scale, float* out, float* lse, void* stream) {
  ENH_REQUIRE(D >= 64 && D <= 384 && D % 64 == 0, ENH_E_SHAPE, "enh_causal_attention_forward_f32: dim_head must be a multiple of 64 up to 384, got %d", D);
  ENH_REQUIRE(qkv && out, ENH_E_BADARG, "enh_causal_attention_forward_f32: null pointer");
  ENH_REQUIRE(B > 0 && H > 0 && N > 0 && N <= PF_F32_ATT_MAX_N && (int64_t)B * H * N <= 2147483647LL, ENH_E_SHAPE,
              "enh_causal_attention_forward_f32: need positive B, H and N in [1, %d] (B=%d N=%d H=%d)", PF_F32_ATT_MAX_N, B, N, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_causal_attention_forward_f32: scale must be positive");
  enh_note_kernel_plain("gpt_prefill_causal_f32_kernel");
  gpt_prefill_causal_f32_kernel<<<(unsigned)(B * H * N), 256, 0, (hipStream_t)stream>>>(qkv, N, H, D, scale, out, lse);
  return enh_check_launch("enh_causal_attention_forward_f32");
}
