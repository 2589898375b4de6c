// attention_kernels.h — the text of the attention kernels, compiled twice:
//   attention.hip       ATT_TAIL 0: the aligned kernels (N % 64 == 0)  attn_fwd_kernel, attn_fwd_pre_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel;
//   attention_tail.hip  ATT_TAIL 1: their tail forms (any other N)     attn_fwd_tail_kernel, attn_fwd_tail_pre_kernel, attn_bwd_tail_dq_kernel, attn_bwd_tail_dkv_kernel.
// One text, two translation units, and the PREPROCESSOR (ATT_SEL, #if ATT_TAIL) rather than a template parameter.  The aligned kernels have to stay the
// instruction streams they were tuned as (tools/isa_lint.py --diff against the previous library), and that was lost by everything milder: an aligned
// kernel that calls an inlined body function, a tile body behind a lambda, a discarded `if constexpr` inside the generic lambdas of the fragment
// stream, even a tail kernel compiled in the same translation unit each changed the aligned kernels' register allocation and schedule.  With ATT_TAIL 0 this
// file preprocesses to the token stream the aligned kernels always had.
//
// Tail form — an (image, head) still attends over its own keys 0 .. N-1 and nothing else:
//   * the last, ragged tile is staged with its rows clamped to the image's last row (attention_common.h, att_dma_tile_clamped / att_gload_clamped):
//     nothing outside the tensor or inside the next image is read, and the LDS image stays finite;
//   * forward and dQ process it in a second, MASKED instance of the tile body behind the tile loop (ATT_TILES_BEGIN / ATT_TILES_END; LAST names that
//     instance): the loop is the aligned loop, and no branch stands between a counted fragment read and its wait.  ATT_MASK_BIAS rides in the C operand
//     of the S products of key rows >= N: probability exactly 0, out of the row maximum and the row sum;
//   * dK/dV streams QUERY tiles, so its ragged tile runs through the same tile body: query rows >= N are given the statistic that makes
//     P = exp2(s - lse) exactly 0, and delta 0 — dV += dO^T 0 and dK += Q^T (0 x dP) add nothing and the MFMA stream is untouched;
//   * query / key rows are clamped for the prologue's fragment loads, and every store is guarded per lane (a wave may own 1 - 31 live rows).
#ifndef ATT_TAIL
#error "attention_kernels.h is included with ATT_TAIL (0 | 1) and ATT_K (the kernel names) defined"
#endif
#include "attention_tile_loop.h"

// The round-1/2 forward pass of one 128-query block (exact running maximum, O rescaled every tile): the body of attn_fwd_kernel.  smem: [2][2][ATT_TILE_BYTES] ([stage][K | V]).
template <typename OT>
__device__ __forceinline__ void ATT_K(fwd, exact)(const uint16_t* __restrict__ qkv, int B, int N, int H, float scale_log2, uint16_t* __restrict__ out,
                                               float* __restrict__ lse, unsigned char (*smem)[2][ATT_TILE_BYTES], int blk, int head) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = head / H, h = head - b * H;
  const int q0 = blk * 128 + wave * 32;
  const int64_t RS = (int64_t)3 * H * ATT_D;
  const uint16_t* Qp = qkv + (int64_t)b * N * RS + h * ATT_D;
  const uint16_t* Kp = Qp + H * ATT_D;
  const uint16_t* Vp = Kp + H * ATT_D;

  const bool active = ATT_SEL(q0 + l31 < N, q0 < N);  // N % 64 == 0: a wave's 32 queries are all in or all out; tail form: per lane
  const int qrow = ATT_SEL(min(q0 + l31, N - 1), active ? q0 + l31 : l31);
  s16x8 qf[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) qf[ds] = *reinterpret_cast<const s16x8*>(Qp + (int64_t)qrow * RS + ds * 16 + hi * 8);

  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  float m_run = -__builtin_inff(), l_part = 0.f;

  const int nt = N / 64;      // full tiles
  u32x4 rk[2], rv[2];
#if ATT_TAIL
  if (nt == 0) {
    att_gload_clamped(rk, Kp, RS, 0, N, t);
    att_gload_clamped(rv, Vp, RS, 0, N, t);
  } else
#endif
  {
  att_gload(rk, Kp, RS, 0, t);
  att_gload(rv, Vp, RS, 0, t);
  }
  att_sstore(rk, smem[0][0], t);
  att_sstore(rv, smem[0][1], t);
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) att_pin(qf[ds]);
  ATT_LOOP_ENTRY();
  __syncthreads();
  ATT_TILES_BEGIN(kt, nt)
    const int st = kt & 1;
#if ATT_TAIL
    if constexpr (LAST) {
    } else if (kt + 1 == nt) {      // the ragged tile is next
      att_gload_clamped(rk, Kp, RS, (kt + 1) * 64, N, t);
      att_gload_clamped(rv, Vp, RS, (kt + 1) * 64, N, t);
    } else
#else
    if (kt + 1 < nt)
#endif
    {
      att_gload(rk, Kp, RS, (kt + 1) * 64, t);
      att_gload(rv, Vp, RS, (kt + 1) * 64, t);
    }
    const unsigned char* kt_ = smem[st][0];
    const unsigned char* vt_ = smem[st][1];
    // ---- S^T[key][q] = K Q^T ----
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = ATT_SEL(LAST ? att_key_bias(kb, r, hi, N & 63) : 0.f, 0.f);      // (ragged tile: ATT_MASK_BIAS on key rows >= N)
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) s[kb] = MFMA32(att_frag_row(kt_, kb * 32, ds, l31, hi), qf[ds], s[kb]);
    }
    // ---- online softmax for this lane's query column ----
    // Round 4 (the kernel runs at the speed of its VECTOR instruction stream, profiles/r04_attention_lab.txt): the row maximum through v_max3 (16
    // instructions instead of 32 v_max + canonicalisations) and one v_permlane32_swap instead of an LDS round trip; and the running maximum is a
    // REFERENCE that is raised — O and l rescaled, a wave-uniform branch — only on the first tile and when some row's tile maximum exceeds it by more
    // than 2^8: the 32 multiplies of O per tile are gone in all but a handful of tiles (numerators stay below 2^8; bf16's relative precision does not
    // depend on that scale, lse = m + log2(l) is exact either way; cdna_hip_programming.md T13: no product is pending across the rescale here).
    float mx = max3(s[0][0], s[0][1], s[0][2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) mx = max3(mx, s[0][r], s[0][r + 1]);
    mx = max3(mx, s[0][15], s[1][0]);
#pragma unroll
    for (int r = 1; r < 15; r += 2) mx = max3(mx, s[1][r], s[1][r + 1]);
    mx = xhalf_max(__builtin_fmaxf(mx, s[1][15]));
    const float mt = mx * scale_log2;
    if (kt == 0 || __builtin_amdgcn_ballot_w64(mt - m_run > 8.0f) != 0) {
      const float m_new = fmaxf(m_run, mt);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_part *= alpha;
#pragma unroll
      for (int db = 0; db < 2; ++db)
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
        for (int db = 0; db < 2; ++db) o[db] = MFMA32(att_frag_tr(vt_, kb * 32 + 16 * c2, db, lane), pb, o[db]);
      }
    ATT_UNLESS_LAST {
    if (ATT_SEL(true, kt + 1 < nt)) {
      att_sstore(rk, smem[st ^ 1][0], t);
      att_sstore(rv, smem[st ^ 1][1], t);
    }
    __syncthreads();
    }
  ATT_TILES_END(kt, nt)
  const float l = l_part + __shfl_xor(l_part, 32, 64);
  const float inv = 1.0f / l;
  if (!active) return;
  uint16_t* op = out + ((int64_t)b * N + q0 + l31) * (H * ATT_D) + h * ATT_D;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = db * 32 + 8 * g4 + 4 * hi;
      u32x2 w = {pack2<OT>(o[db][g4 * 4 + 0] * inv, o[db][g4 * 4 + 1] * inv), pack2<OT>(o[db][g4 * 4 + 2] * inv, o[db][g4 * 4 + 3] * inv)};
      *reinterpret_cast<u32x2*>(op + d0) = w;
    }
  if (hi == 0) lse[((int64_t)b * H + h) * N + q0 + l31] = (m_run + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
}

// ---- the fragment stream of a tile (LDS-DMA kernels) ----------------------------------------------------------------------------------------------
// A tile's MFMAs take their operand fragments from a stream of counted reads (attention_common.h, att_req_* / att_take_*): fragment I feeds MFMA I.
// The stream repeats with period P; the first 8 fragments of a period are row fragments (one ds_read_b128), the rest transpose fragments (two
// ds_read_b64_tr_b16).  A fragment is requested ATT_PF MFMAs ahead of the one that consumes it (4 registers per level), inside RUNS: the first ATT_PF
// fragments of a run are requested together where it starts — the one place where an MFMA waits for a read issued just in front of it.  A run is the
// whole tile (WHOLE: fragments are also held across the exponentials between two phases; dQ and dK/dV, three waves per SIMD) or one phase — the row
// fragments of a block | its transpose fragments (the forward: 126 registers so, 128 = the end of its four-wave class with WHOLE; measured the same).
// Two levels measured the same as one on dQ (profiles/r07_attention_pipeline.txt).
#define ATT_PF 1
__host__ __device__ constexpr bool att_run_start(int k, int P, bool WHOLE) { return k == 0 || (!WHOLE && (k % P == 0 || k % P == 8)); }
__host__ __device__ constexpr int att_run_end(int I, int NF, int P, bool WHOLE) {
  int e = I + 1;
  while (e < NF && !att_run_start(e, P, WHOLE)) ++e;
  return e;
}
// LDS operations the kernel has issued behind fragment I's own when MFMA I takes it
__host__ __device__ constexpr int att_pending(int I, int NF, int P, bool WHOLE) {
  int n = 0;
  for (int k = I + 1; k <= I + ATT_PF && k < att_run_end(I, NF, P, WHOLE); ++k) n += (k % P < 8) ? 1 : 2;
  return n;
}
// what MFMA I requests before it takes its own fragment.  req(integral_constant<int, K>) requests fragment K.
template <int I, int NF, int P, bool WHOLE, typename REQ>
__device__ __forceinline__ void att_stream_request(REQ& req) {
  constexpr int E = att_run_end(I, NF, P, WHOLE);
  if constexpr (att_run_start(I, P, WHOLE)) att_static_for<I, (I + ATT_PF < E ? I + ATT_PF : E)>(req);
  if constexpr (I + ATT_PF < E) req(std::integral_constant<int, I + ATT_PF>{});
}

// =================================================================================================
// forward
// =================================================================================================
template <typename OT>
__global__ __launch_bounds__(256, 2) void ATT_K(fwd, kernel)(const uint16_t* __restrict__ qkv, int B, int N, int H, float scale_log2,
                                                          uint16_t* __restrict__ out, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][2][ATT_TILE_BYTES];  // [stage][K | V]
  int blk, head;
  if (!att_block_coords((N + 127) / 128, B * H, blk, head)) return;
  ATT_K(fwd, exact)<OT>(qkv, B, N, H, scale_log2, out, lse, smem, blk, head);
}

// Round 5 — the forward for PRE-SCALED q (the training path's convention: the products are log2-domain scores), with the vector stream cut where the
// round-4 anatomy says the kernel's time is (profiles/r04_attention_lab.txt: it runs at the speed of its vector instructions):
//   * -m_ref rides in the MFMA C operand of the first S product (a lane owns ONE query column, so -m_ref is a per-lane constant in a 16-register block,
//     rewritten only when the reference is raised — a handful of tiles per row): the exponential reads the accumulator directly, the 32 multiply-subtracts
//     per tile are gone (what the dQ / dK/dV kernels do with -lse);
//   * the row sum runs on float pairs (16 v_pk_add_f32 per tile instead of 32 adds), still exact f32: lse keeps its 5e-8.  (Summing the PACKED bf16
//     numerators with v_dot2c_f32_bf16 against (1, 1) — also 16 instructions — measured the same time and moved lse to 2e-5: not adopted.)
// Same skeleton, LDS images and results layout as attn_fwd_exact; the exact running-reference semantics are kept (no fallback path).
__device__ __forceinline__ float dot2_ones(uint32_t pk, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, pk), __builtin_bit_cast(bf16x2_t, 0x3f803f80u), acc, false);
}
template <typename OT>
__global__ __launch_bounds__(256, 2) void ATT_K(fwd, pre_kernel)(const uint16_t* __restrict__ qkv, int B, int N, int H, uint16_t* __restrict__ out, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][2][ATT_TILE_BYTES];  // [stage][K | V]
  int blk, head;
  if (!att_block_coords((N + 127) / 128, B * H, blk, head)) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int b = head / H, h = head - b * H;
  const int q0 = blk * 128 + wave * 32;
  const int64_t RS = (int64_t)3 * H * ATT_D;
  const uint16_t* Qp = qkv + (int64_t)b * N * RS + h * ATT_D;
  const uint16_t* Kp = Qp + H * ATT_D;
  const uint16_t* Vp = Kp + H * ATT_D;
  const bool active = ATT_SEL(q0 + l31 < N, q0 < N);
  const int qrow = ATT_SEL(min(q0 + l31, N - 1), active ? q0 + l31 : l31);
  s16x8 qf[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) qf[ds] = *reinterpret_cast<const s16x8*>(Qp + (int64_t)qrow * RS + ds * 16 + hi * 8);
  f32x16 o[2], negm;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o[0][r] = 0.f; o[1][r] = 0.f; negm[r] = 0.f; }
  float m_ref = 0.f;                   // the first tile's scores are taken against 0 and re-based below (kt == 0)
  f32x2 l2[2] = {{0.f, 0.f}, {0.f, 0.f}};

  const int nt = N / 64;      // full tiles
  // K / V tiles by LDS-DMA (round 5): no staging registers, no ds_write pass; the next tile is requested at the top of a tile into the stage the last barrier freed
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const unsigned ko0 = att_dma_lane_off((int)RS, lane, 0), ko1 = att_dma_lane_off((int)RS, lane, 1);
#if ATT_TAIL
  if (nt == 0) {
    att_dma_tile_clamped(Kp, RS, 0, N, smem[0][0], wave_u, lane);
    att_dma_tile_clamped(Vp, RS, 0, N, smem[0][1], wave_u, lane);
  } else
#endif
  {
  att_dma_tile(Kp, RS, 0, smem[0][0], wave_u, ko0, ko1);
  att_dma_tile(Vp, RS, 0, smem[0][1], wave_u, ko0, ko1);
  }
  unsigned ra[4], ta[2][2];      // this lane's fragment addresses in the stage being read
  att_ring_addresses(ra, ta, &smem[0][0][0], lane);
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) att_pin(qf[ds]);
  ATT_LOOP_ENTRY();
  __syncthreads();
  ATT_TILES_BEGIN(kt, nt)
    const int st = kt & 1;
#if ATT_TAIL
    if constexpr (LAST) {
    } else if (kt + 1 == nt) {      // the ragged tile is next
      att_dma_tile_clamped(Kp, RS, (kt + 1) * 64, N, smem[st ^ 1][0], wave_u, lane);
      att_dma_tile_clamped(Vp, RS, (kt + 1) * 64, N, smem[st ^ 1][1], wave_u, lane);
    } else
#else
    if (kt + 1 < nt)
#endif
    {
      att_dma_tile(Kp, RS, (kt + 1) * 64, smem[st ^ 1][0], wave_u, ko0, ko1);
      att_dma_tile(Vp, RS, (kt + 1) * 64, smem[st ^ 1][1], wave_u, ko0, ko1);
    }
    // (Round 5: issuing the tile's fragment reads ahead of their use in a fenced order — all eight K fragments at once, one V fragment behind every S
    // product, counted lgkmcnt waits instead of the compiler's read / wait(0) / MFMA chains — needs 168 registers (three waves per SIMD instead of four)
    // and measured no faster than the round-4 kernel: profiles/r05_attention_lab.txt §6.  The stream below holds ATT_PF + 1 fragments, not eight.)
    // Fragment I of the tile's 16 (see "the fragment stream of a tile" above): I < 8: row fragment ds = I % 4 of K, key block kb = I / 4 (-> S);
    // else transpose fragment (kb, c2, db) = ((I - 8) / 4, ((I - 8) / 2) % 2, I % 2) of V (-> O).
    constexpr int NF = 16;
    u32x4 fr[ATT_PF + 1];
    att_u64 tl[ATT_PF + 1], th[ATT_PF + 1];
    auto req = [&](auto ic) {
      constexpr int I = decltype(ic)::value, B = I % (ATT_PF + 1);
      if constexpr (I < 8) att_req_row<(I >> 2) * 32 * 128>(fr[B], ra[I & 3]);
      else att_req_tr<ATT_TILE_BYTES + (((I - 8) >> 2) * 32 + 16 * (((I - 8) >> 1) & 1)) * 128>(tl[B], th[B], ta[I & 1][0], ta[I & 1][1]);
    };
    f32x16 s[2];
    att_static_for<0, 8>([&](auto ic) {
      constexpr int I = decltype(ic)::value, kb = I >> 2, ds = I & 3, B = I % (ATT_PF + 1);
      att_stream_request<I, NF, 16, false>(req);
#if ATT_TAIL
      if constexpr (LAST && ds == 0) {       // the ragged tile: ATT_MASK_BIAS joins -m_ref in the C operand of key rows >= N
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kb][r] = negm[r] + att_key_bias(kb, r, hi, N & 63);
      }
#endif
      s[kb] = MFMA32(att_take_row<att_pending(I, NF, 16, false)>(fr[B]), qf[ds], ATT_SEL(ds == 0 && !LAST, ds == 0) ? negm : s[kb]);   // S^T[key][q] - m_ref[q]
    });
    // four independent v_max3 chains of depth 4 (one dependent chain of 16 leaves the in-order wave waiting on its own previous instruction)
    float mq[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const f32x16& sv = s[c >> 1];
      const int r0 = (c & 1) * 8;
      mq[c] = max3(sv[r0], sv[r0 + 1], sv[r0 + 2]);
      mq[c] = max3(mq[c], sv[r0 + 3], sv[r0 + 4]);
      mq[c] = max3(mq[c], sv[r0 + 5], sv[r0 + 6]);
    }
    float mx = max3(mq[0], mq[1], s[0][7]);
    mx = max3(mx, mq[2], s[0][15]);
    mx = max3(mx, mq[3], s[1][7]);
    mx = xhalf_max(__builtin_fmaxf(mx, s[1][15]));       // this tile's row maximum RELATIVE to the reference
    if (kt == 0 || __builtin_amdgcn_ballot_w64(mx > 8.0f) != 0) {   // wave-uniform: the reference is raised on the first tile and when outgrown by 2^8
      const float delta = kt == 0 ? mx : __builtin_fmaxf(mx, 0.f);
      if (kt != 0) {
        const float alpha = __builtin_amdgcn_exp2f(-delta);
        l2[0] *= alpha; l2[1] *= alpha;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      }
      m_ref += delta;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[0][r] -= delta; s[1][r] -= delta; negm[r] = -m_ref; }
    }
    // ---- numerators, packed; row sum of the packed values; O^T[d][q] += V^T P^T ----
    s16x8 pb;
    att_static_for<8, 16>([&](auto ic) {
      constexpr int I = decltype(ic)::value, kb = (I - 8) >> 2, c2 = ((I - 8) >> 1) & 1, db = I & 1, B = I % (ATT_PF + 1);
      att_stream_request<I, NF, 16, false>(req);
      if constexpr (db == 0) {
        float p8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) p8[j] = __builtin_amdgcn_exp2f(s[kb][c2 * 8 + j]);
        const u32x4 pk = {pack2<OT>(p8[0], p8[1]), pack2<OT>(p8[2], p8[3]), pack2<OT>(p8[4], p8[5]), pack2<OT>(p8[6], p8[7])};
#pragma unroll
        for (int j = 0; j < 4; ++j) l2[j & 1] += (f32x2){p8[2 * j], p8[2 * j + 1]};      // exact f32 row sum, two lanes of one v_pk_add_f32 (lse stays exact to f32), two chains
        pb = __builtin_bit_cast(s16x8, pk);
      }
      o[db] = MFMA32(att_take_tr<att_pending(I, NF, 16, false)>(tl[B], th[B]), pb, o[db]);
    });
    ATT_UNLESS_LAST {
    att_ring_advance(ra, ta, st);
    ATT_FENCE();                             // (every MFMA of the tile is issued before the wave parks)
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): this wave's share of the next tile has landed
    __syncthreads();
    }
  ATT_TILES_END(kt, nt)
  const float l_part = (l2[0][0] + l2[1][0]) + (l2[0][1] + l2[1][1]);
  const float l = l_part + __shfl_xor(l_part, 32, 64);
  const float inv = 1.0f / l;
  if (!active) return;
  uint16_t* op = out + ((int64_t)b * N + q0 + l31) * (H * ATT_D) + h * ATT_D;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = db * 32 + 8 * g4 + 4 * hi;
      u32x2 w = {pack2<OT>(o[db][g4 * 4 + 0] * inv, o[db][g4 * 4 + 1] * inv), pack2<OT>(o[db][g4 * 4 + 2] * inv, o[db][g4 * 4 + 3] * inv)};
      *reinterpret_cast<u32x2*>(op + d0) = w;
    }
  if (hi == 0) lse[((int64_t)b * H + h) * N + q0 + l31] = (m_ref + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
}

// =================================================================================================
// backward: dQ  (same skeleton as forward; K tile is read both as rows and transposed)
// =================================================================================================
// MODE 0: the round-2 arithmetic.  MODE 1: -delta enters as the C operand of the first dP product (a lane owns ONE query column, so -delta_q is a
// per-lane constant kept in a 16-register block; D = A B + C with D != C): 32 subtractions per tile gone.  MODE 2 (q pre-scaled by scale*log2e, i.e.
// the products are already log2-domain scores): -lse enters the S product the same way and the exponential reads the accumulator directly — no
// vector arithmetic left but exp, the P o dP' multiply and the bf16 packing.  The kernels are vector-ISSUE bound (profiles/r03_attention_lab.txt).
template <int MODE, typename OT>
__global__ __launch_bounds__(256, 3) void ATT_K(bwd, dq_kernel)(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o, const uint16_t* __restrict__ d_o,
                                                             const float* __restrict__ lse, float* __restrict__ delta, int B, int N,
                                                             int H, float scale, float scale_log2, uint16_t* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][2][ATT_TILE_BYTES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  int blk, head;
  if (!att_block_coords((N + 127) / 128, B * H, blk, head)) return;
  const int b = head / H, h = head - b * H;
  const int q0 = blk * 128 + wave * 32;
  const int64_t RS = (int64_t)3 * H * ATT_D;
  const uint16_t* Qp = qkv + (int64_t)b * N * RS + h * ATT_D;
  const uint16_t* Kp = Qp + H * ATT_D;
  const uint16_t* Vp = Kp + H * ATT_D;
  const uint16_t* dOp = d_o + (int64_t)b * N * (H * ATT_D) + h * ATT_D;

  const bool active = ATT_SEL(q0 + l31 < N, q0 < N);
  const int qrow = ATT_SEL(min(q0 + l31, N - 1), active ? q0 + l31 : l31);
  s16x8 qf[4], dof[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    qf[ds] = *reinterpret_cast<const s16x8*>(Qp + (int64_t)qrow * RS + ds * 16 + hi * 8);
    dof[ds] = *reinterpret_cast<const s16x8*>(dOp + (int64_t)qrow * (H * ATT_D) + ds * 16 + hi * 8);
  }
  const float lse_q = lse[((int64_t)b * H + h) * N + qrow] * 1.4426950408889634f;
  // delta[q] = sum_d dO[q][d] * O[q][d]: a lane already holds half of its query's dO row as MFMA fragments, so the row dot product is 32 products per
  // lane and one cross-half exchange here — and is WRITTEN for the dK/dV kernel that runs next (this replaced a separate pass over O and dO per layer)
  float dpart = 0.f;
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    const s16x8 of = *reinterpret_cast<const s16x8*>(o + ((int64_t)b * N + qrow) * (H * ATT_D) + h * ATT_D + ds * 16 + hi * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) dpart += unpack1<OT>((uint16_t)of[k]) * unpack1<OT>((uint16_t)dof[ds][k]);
  }
  const float del_q = dpart + __shfl_xor(dpart, 32, 64);
  if (active && hi == 0) delta[((int64_t)b * H + h) * N + qrow] = del_q;
  f32x16 negd, negl;
#pragma unroll
  for (int r = 0; r < 16; ++r) { negd[r] = MODE >= 1 ? -del_q : 0.f; negl[r] = MODE == 2 ? -lse_q : 0.f; }

  f32x16 dq[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[db][r] = 0.f;

  const int nt = N / 64;      // full tiles
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);      // K / V tiles by LDS-DMA (see attn_fwd_pre_kernel)
  const unsigned ko0 = att_dma_lane_off((int)RS, lane, 0), ko1 = att_dma_lane_off((int)RS, lane, 1);
#if ATT_TAIL
  if (nt == 0) {
    att_dma_tile_clamped(Kp, RS, 0, N, smem[0][0], wave_u, lane);
    att_dma_tile_clamped(Vp, RS, 0, N, smem[0][1], wave_u, lane);
  } else
#endif
  {
  att_dma_tile(Kp, RS, 0, smem[0][0], wave_u, ko0, ko1);
  att_dma_tile(Vp, RS, 0, smem[0][1], wave_u, ko0, ko1);
  }
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) { att_pin(qf[ds]); att_pin(dof[ds]); }
  ATT_LOOP_ENTRY();
  __syncthreads();
  // The tile's 24 MFMAs take their fragments from a stream of 24 counted reads (attention_common.h, att_req_* / att_take_*), requested ATT_PF
  // fragments ahead of the MFMA that consumes them — also across the exponentials between the S / dP products and the dQ products and from one key block
  // to the next; only the first ATT_PF fragments of a tile, behind the barrier that publishes the stage, are awaited with nothing to do.
  // Fragment I: key block kb = I / 12; j = I % 12 < 8: row fragment ds = j / 2 of K (j even, -> S) or V (j odd, -> dP); else transpose fragment
  // (c2, db) = ((j - 8) / 2, (j - 8) % 2) of K (-> dQ).  Same products, same order per accumulator as the serial form: the same bits.
  unsigned ra[4], ta[2][2];      // this lane's fragment addresses in the stage being read
  att_ring_addresses(ra, ta, &smem[0][0][0], lane);
  ATT_TILES_BEGIN(kt, nt)
    const int st = kt & 1;
#if ATT_TAIL
    if constexpr (LAST) {
    } else if (kt + 1 == nt) {      // the ragged tile is next
      att_dma_tile_clamped(Kp, RS, (kt + 1) * 64, N, smem[st ^ 1][0], wave_u, lane);
      att_dma_tile_clamped(Vp, RS, (kt + 1) * 64, N, smem[st ^ 1][1], wave_u, lane);
    } else
#else
    if (kt + 1 < nt)
#endif
    {
      att_dma_tile(Kp, RS, (kt + 1) * 64, smem[st ^ 1][0], wave_u, ko0, ko1);
      att_dma_tile(Vp, RS, (kt + 1) * 64, smem[st ^ 1][1], wave_u, ko0, ko1);
    }
    constexpr int NF = 24;
    u32x4 fr[ATT_PF + 1];
    att_u64 tl[ATT_PF + 1], th[ATT_PF + 1];
    auto req = [&](auto ic) {
      constexpr int I = decltype(ic)::value, kb = I / 12, j = I % 12, B = I % (ATT_PF + 1);
      if constexpr (j < 8) att_req_row<(j & 1) * ATT_TILE_BYTES + kb * 32 * 128>(fr[B], ra[j >> 1]);
      else att_req_tr<(kb * 32 + 16 * ((j - 8) >> 1)) * 128>(tl[B], th[B], ta[j & 1][0], ta[j & 1][1]);
    };
    f32x16 s, dp;
    float dsv[16];
    s16x8 dsb;
    att_static_for<0, NF>([&](auto ic) {
      constexpr int I = decltype(ic)::value, j = I % 12, B = I % (ATT_PF + 1);
      att_stream_request<I, NF, 12, true>(req);
      constexpr int PEND = att_pending(I, NF, 12, true);
      if constexpr (j < 8) {
        constexpr int ds = j >> 1;
        const s16x8 f = att_take_row<PEND>(fr[B]);
#if ATT_TAIL
        if constexpr (LAST && j == 0) {     // the ragged tile: ATT_MASK_BIAS joins -lse in the C operand of key rows >= N
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = negl[r] + att_key_bias(I / 12, r, hi, N & 63);
        }
#endif
        if constexpr ((j & 1) == 0) s = MFMA32(f, qf[ds], ATT_SEL(ds == 0 && !LAST, ds == 0) ? negl : s);     // S^T[key][q]  (- lse[q] in MODE 2)
        else dp = MFMA32(f, dof[ds], ds == 0 ? negd : dp);                         // dP^T[key][q] = V dO^T  (- delta[q] in MODE >= 1)
        if constexpr (j == 7) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float pr = MODE == 2 ? __builtin_amdgcn_exp2f(s[r]) : __builtin_amdgcn_exp2f(s[r] * scale_log2 - lse_q);
            dsv[r] = MODE >= 1 ? pr * dp[r] : pr * (dp[r] - del_q);     // (the factor `scale` of dS is applied once to the finished dQ)
          }
        }
      } else {
        constexpr int c2 = (j - 8) >> 1, db = j & 1;
        if constexpr (db == 0) dsb = pack8<OT>(&dsv[c2 * 8]);
        dq[db] = MFMA32(att_take_tr<PEND>(tl[B], th[B]), dsb, dq[db]);              // dQ^T[d][q] += K^T dS^T
      }
    });
    ATT_UNLESS_LAST {
    att_ring_advance(ra, ta, st);
    ATT_FENCE();                             // (every MFMA of the tile is issued before the wave parks)
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): this wave's share of the next tile has landed
    __syncthreads();
    }
  ATT_TILES_END(kt, nt)
  if (!active) return;
  uint16_t* op = dqkv + ((int64_t)b * N + q0 + l31) * RS + h * ATT_D;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = db * 32 + 8 * g4 + 4 * hi;
      u32x2 w = {pack2<OT>(dq[db][g4 * 4 + 0] * scale, dq[db][g4 * 4 + 1] * scale), pack2<OT>(dq[db][g4 * 4 + 2] * scale, dq[db][g4 * 4 + 3] * scale)};
      *reinterpret_cast<u32x2*>(op + d0) = w;
    }
}

// =================================================================================================
// backward: dK, dV  (workgroup owns 128 keys; Q / dO tiles stream through LDS)
// =================================================================================================
// CINIT: -delta (and, with PRE — q pre-scaled by scale*log2e — also -lse) enter as the C operands of the first dP / S products: the statistics are
// loaded from LDS straight into the accumulator registers (the same four 16-byte reads per block as before, no extra registers), which removes the
// per-element subtraction (and the scale-and-subtract before the exponential).  kscale: the factor of the finished dK (scale, or ln 2 with PRE).
template <bool CINIT, bool PRE, typename OT>
#ifndef ATT_DKV_OCC
#define ATT_DKV_OCC 2
#endif
// (round 5: forcing three waves per SIMD here — __launch_bounds__(256, 3), 168 registers — spills 18 registers into the tile loop and costs +20 % on the backward;
// four waves on the forward, 38 spills, doubles its time: profiles/r05_attention_lab.txt §5.  The occupancy these kernels have is the one their live set allows.)
__global__ __launch_bounds__(256, ATT_DKV_OCC) void ATT_K(bwd, dkv_kernel)(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ d_o,
                                                              const float* __restrict__ lse, const float* __restrict__ delta, int B, int N,
                                                              int H, float scale, float scale_log2, uint16_t* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][2][ATT_TILE_BYTES];  // [stage][Q | dO]
  __shared__ __attribute__((aligned(16))) float s_stat[2][2][64];                   // [stage][lse*log2e | delta]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  int blk, head;
  if (!att_block_coords((N + 127) / 128, B * H, blk, head)) return;
  const int b = head / H, h = head - b * H;
  const int key0 = blk * 128 + wave * 32;
  const int64_t RS = (int64_t)3 * H * ATT_D;
  const int64_t OS = (int64_t)H * ATT_D;
  const uint16_t* Qp = qkv + (int64_t)b * N * RS + h * ATT_D;
  const uint16_t* Kp = Qp + H * ATT_D;
  const uint16_t* Vp = Kp + H * ATT_D;
  const uint16_t* dOp = d_o + (int64_t)b * N * OS + h * ATT_D;
  const float* lsep = lse + ((int64_t)b * H + h) * N;
  const float* delp = delta + ((int64_t)b * H + h) * N;

  const bool active = ATT_SEL(key0 + l31 < N, key0 < N);
  const int krow = ATT_SEL(min(key0 + l31, N - 1), active ? key0 + l31 : l31);
  s16x8 kf[4], vf[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
    kf[ds] = *reinterpret_cast<const s16x8*>(Kp + (int64_t)krow * RS + ds * 16 + hi * 8);
    vf[ds] = *reinterpret_cast<const s16x8*>(Vp + (int64_t)krow * RS + ds * 16 + hi * 8);
  }
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[db][r] = 0.f; dv[db][r] = 0.f; }

  const int nt = ATT_SEL(N / 64 + 1, N / 64);      // (the ragged tile runs through the same tile body: see the head of this file)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);      // Q / dO tiles by LDS-DMA (see attn_fwd_pre_kernel)
  const unsigned qo0 = att_dma_lane_off((int)RS, lane, 0), qo1 = att_dma_lane_off((int)RS, lane, 1);
  const unsigned do0 = att_dma_lane_off((int)OS, lane, 0), do1 = att_dma_lane_off((int)OS, lane, 1);
  float rstat = 0.f;
#if ATT_TAIL
  if (nt == 1) {
    att_dma_tile_clamped(Qp, RS, 0, N, smem[0][0], wave_u, lane);
    att_dma_tile_clamped(dOp, OS, 0, N, smem[0][1], wave_u, lane);
  } else
#endif
  {
  att_dma_tile(Qp, RS, 0, smem[0][0], wave_u, qo0, qo1);
  att_dma_tile(dOp, OS, 0, smem[0][1], wave_u, do0, do1);
  }
  unsigned ra[4], ta[2][2];      // this lane's fragment addresses in the stage being read
  att_ring_addresses(ra, ta, &smem[0][0][0], lane);
  // statistics of the 64 queries of a tile: threads 0-63 fetch lse (kept in the log2 domain), 64-127 delta — through ONE select-addressed load in the
  // straight-line code.  The former `if (t < 64) .. else if (t < 128) ..` put each load in its own divergent block, and the wait-count pass closed
  // that block with s_waitcnt vmcnt(0): every iteration waited for the Q / dO prefetch issued just before it (found in the ISA, round 3).
  const float* statp = ((t & 64) ? delp : lsep) + (t & 63);
  const float stat_mul = (t & 64) ? (CINIT ? -1.0f : 1.0f) : ((CINIT && PRE) ? -1.4426950408889634f : 1.4426950408889634f);   // stored negated where they are C operands
#if ATT_TAIL
  // the statistic of a query row >= N is read from the image's last row and replaced where it is stored: P = exp2(s - lse) = 0, delta = 0
  const float stat_masked = (t & 64) ? 0.f : ((CINIT && PRE) ? ATT_MASK_BIAS : -ATT_MASK_BIAS);
#endif
  rstat = statp[ATT_SEL(min(0, N - 1 - (t & 63)), 0)];
  if (t < 128) s_stat[0][t >> 6][t & 63] = ATT_SEL((t & 63) >= N ? stat_masked :, ) rstat * stat_mul;
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) { att_pin(kf[ds]); att_pin(vf[ds]); }
  ATT_LOOP_ENTRY();
  __syncthreads();
  for (int qt = 0; qt < nt; ++qt) {
    const int st = qt & 1;
#if ATT_TAIL
    if (qt + 2 == nt) {      // the ragged tile is next
      att_dma_tile_clamped(Qp, RS, (qt + 1) * 64, N, smem[st ^ 1][0], wave_u, lane);
      att_dma_tile_clamped(dOp, OS, (qt + 1) * 64, N, smem[st ^ 1][1], wave_u, lane);
      rstat = statp[min((qt + 1) * 64, N - 1 - (t & 63))];
    }
#endif
    if (qt + 1 < ATT_SEL(nt - 1, nt)) {
      att_dma_tile(Qp, RS, (qt + 1) * 64, smem[st ^ 1][0], wave_u, qo0, qo1);      // the other stage is free since the barrier that closed tile qt - 1
      att_dma_tile(dOp, OS, (qt + 1) * 64, smem[st ^ 1][1], wave_u, do0, do1);
      rstat = statp[(qt + 1) * 64];                 // (scaled when it is stored, after the tile's arithmetic: nothing here waits for the load)
    }
    // The tile's 32 MFMAs take their fragments from a stream of 32 counted reads, requested ATT_PF fragments ahead (see attn_bwd_dq_kernel).  Fragment I:
    // query block qb = I / 16; j = I % 16 < 8: row fragment ds = j / 2 of Q (j even, -> S) or dO (j odd, -> dP); else transpose fragment
    // (c2, db) = ((j - 8) / 4, ((j - 8) / 2) % 2) of dO (j even, -> dV) or Q (j odd, -> dK).  The statistics stay plain reads of s_stat, which the LDS-DMA does not write.
    constexpr int NF = 32;
    u32x4 fr[ATT_PF + 1];
    att_u64 tl[ATT_PF + 1], th[ATT_PF + 1];
    auto req = [&](auto ic) {
      constexpr int I = decltype(ic)::value, qb = I / 16, j = I % 16, B = I % (ATT_PF + 1);
      if constexpr (j < 8) att_req_row<(j & 1) * ATT_TILE_BYTES + qb * 32 * 128>(fr[B], ra[j >> 1]);
      else att_req_tr<((j & 1) ^ 1) * ATT_TILE_BYTES + (qb * 32 + 16 * ((j - 8) >> 2)) * 128>(tl[B], th[B], ta[(j >> 1) & 1][0], ta[(j >> 1) & 1][1]);
    };
    f32x16 s, dp, lrow, drow;
    float pv[16], dsv[16];
    s16x8 pa, dsa;
    att_static_for<0, NF>([&](auto ic) {
      constexpr int I = decltype(ic)::value, qb = I / 16, j = I % 16, B = I % (ATT_PF + 1);
      att_stream_request<I, NF, 16, true>(req);
      constexpr int PEND = att_pending(I, NF, 16, true);
      if constexpr (j == 0) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {           // the statistics of the 16 query rows this lane holds (rows 8 g4 + 4 hi + 0..3 of the block)
          const int row0 = qb * 32 + 8 * g4 + 4 * hi;
          const f32x4 l4 = *reinterpret_cast<const f32x4*>(&s_stat[st][0][row0]);
          const f32x4 d4 = *reinterpret_cast<const f32x4*>(&s_stat[st][1][row0]);
#pragma unroll
          for (int k = 0; k < 4; ++k) { lrow[g4 * 4 + k] = l4[k]; dp[g4 * 4 + k] = d4[k]; }
        }
        drow = dp;
        if (!(CINIT && PRE)) {
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = 0.f;
        } else {
          s = lrow;                               // -lse (log2 domain) as the C operand
        }
        if (!CINIT) {
#pragma unroll
          for (int r = 0; r < 16; ++r) dp[r] = 0.f;
        }
      }
      if constexpr (j < 8) {
        constexpr int ds = j >> 1;
        const s16x8 f = att_take_row<PEND>(fr[B]);
        if constexpr ((j & 1) == 0) s = MFMA32(f, kf[ds], s);      // S[q][key]  (- lse[q])
        else dp = MFMA32(f, vf[ds], dp);                           // dP[q][key] = dO V^T  (- delta[q])
        if constexpr (j == 7) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            pv[r] = (CINIT && PRE) ? __builtin_amdgcn_exp2f(s[r]) : __builtin_amdgcn_exp2f(s[r] * scale_log2 - lrow[r]);
            dsv[r] = CINIT ? pv[r] * dp[r] : pv[r] * (dp[r] - drow[r]);      // the factor of dS is applied once to the finished dK
          }
        }
      } else {
        constexpr int c2 = (j - 8) >> 2, db = (j >> 1) & 1;
        if constexpr (((j - 8) & 3) == 0) { pa = pack8<OT>(&pv[c2 * 8]); dsa = pack8<OT>(&dsv[c2 * 8]); }
        const s16x8 f = att_take_tr<PEND>(tl[B], th[B]);
        if constexpr ((j & 1) == 0) dv[db] = MFMA32(f, pa, dv[db]);  // dV^T[d][key] += dO^T P
        else dk[db] = MFMA32(f, dsa, dk[db]);                        // dK^T[d][key] += Q^T dS
      }
    });
    att_ring_advance(ra, ta, st);
    // ONE wait for everything this wave has asked global memory for — its share of the next tile and the statistic it stores below — behind the tile's last MFMA
    ATT_FENCE();
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0)
    if (qt + 1 < nt && t < 128) s_stat[st ^ 1][t >> 6][t & 63] = ATT_SEL((qt + 1) * 64 + (t & 63) >= N ? stat_masked :, ) rstat * stat_mul;
    __syncthreads();
  }
  if (!active) return;
  // D^T[d][key]: lane (key = key0 + l31, hi) holds d = db*32 + 8*(r>>2) + 4*hi + (r&3): four consecutive d per register group -> 8-byte stores
  uint16_t* dkp = dqkv + ((int64_t)b * N + key0 + l31) * RS + H * ATT_D + h * ATT_D;
  uint16_t* dvp = dkp + H * ATT_D;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d0 = db * 32 + 8 * g4 + 4 * hi;
      const u32x2 wk = {pack2<OT>(dk[db][g4 * 4 + 0] * scale, dk[db][g4 * 4 + 1] * scale), pack2<OT>(dk[db][g4 * 4 + 2] * scale, dk[db][g4 * 4 + 3] * scale)};
      const u32x2 wv = {pack2<OT>(dv[db][g4 * 4 + 0], dv[db][g4 * 4 + 1]), pack2<OT>(dv[db][g4 * 4 + 2], dv[db][g4 * 4 + 3])};
      *reinterpret_cast<u32x2*>(dkp + d0) = wk;
      *reinterpret_cast<u32x2*>(dvp + d0) = wv;
    }
}
