// rq_backward.hip — what the backward of the stage-2 RQTransformer's teacher-forced loss needs beyond the GPT's kernels, for gfx950.  The Blocks of both
// stacks run the GPT's backward launches (gpt_rows.hip, gpt_attn_bwd.hip, enh_gemm_h16) over two row counts; the RQ topology adds
//
//   enh_short_causal_attention_backward   dqkv of rq_prefill.hip's rq_short_causal_kernel: NSEQ sequences of L <= 8 tokens, 32 (sequence, head) pairs
//                                         per workgroup, one group of eight lanes writes all of dq, dk and dv of its pair
//   enh_rq_embed_seq_backward             the gradients of the five embedding tables from the gradients of the spatial and the depth stream's inputs
//   (enh_ln_rows_strided_backward, the backward of ln_spatial through slot 0 of the depth sequences, shares its body with the LayerNorm backward of
//    gpt_rows.hip and is defined there)
// No float atomics; every sum runs in a fixed order: the same bits on every run.
#include "common.h"

#define RQ_MAX_DEPTH 8
#define RQ_EMB_MAX_C 8192
#define RQ_LOG2E 1.4426950408889634f

// ---------------------------------------------------------------------------------------------
// short-sequence causal attention, backward
// ---------------------------------------------------------------------------------------------
// The ownership of rq_short_causal_kernel: eight lanes own one (sequence, head) pair, lane g columns 64 c + 8 g .. + 7 of every 64-column chunk c; a
// per-pair scalar is the xor-butterfly sum of the eight lanes' partial sums, the same bits in every lane.  The arithmetic contract of
// gpt_attn_bwd.hip: P = exp2(s scale log2(e) - lse log2(e)) from the stored lse, delta = rowsum(dO o O) on the stored 16-bit out, P rounded to the
// format before P^T dO, P o (dP - delta) rounded to the format before the dQ / dK products, one rounding of dq, dk and dv.  Query 0 sees one key
// (P = 1, dS = 0 whatever the values): its dQ row is written as exact zeros and entry (0, 0) adds nothing to dK.
// Three passes over the chunks of the head, so that the unpacked rows of one operand pair at a time live beside the two triangles:
//   1  s over q and k                          (L (L + 1) / 2 partial sums)
//   2  dP over dO and v, delta over dO and out (the same, and L)
//   -  butterflies; P and dS, rounded, replace s and dP
//   3  per chunk: dv from P and dO, dq from dS and k, dk from dS and q; 16-byte stores, every element written once
template <int L, typename OT>
__global__ __launch_bounds__(256) void rq_short_causal_bwd_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ out,
                                                                  const uint16_t* __restrict__ dout, const float* __restrict__ lse, int64_t npairs, int H, int D,
                                                                  float scale, float scale_log2, uint16_t* __restrict__ dqkv) {
  const int64_t pair = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  if (pair >= npairs) return;      // uniform over the group's eight lanes: the butterflies below stay inside a group
  const int g = threadIdx.x & 7;
  const int64_t seq = pair / H;
  const int h = (int)(pair - seq * H);
  const int64_t RS = (int64_t)3 * H * D, HD = (int64_t)H * D;
  const int64_t qoff = seq * L * RS + (int64_t)h * D + g * 8, ooff = seq * L * HD + (int64_t)h * D + g * 8;
  const uint16_t* Qp = qkv + qoff;
  const uint16_t* Kp = Qp + HD;
  const uint16_t* Vp = Kp + HD;
  const uint16_t* Op = out + ooff;
  const uint16_t* Gp = dout + ooff;

  float p[L][L], ds[L][L], delta[L];
#pragma unroll
  for (int i = 0; i < L; ++i) {
    delta[i] = 0.f;
#pragma unroll
    for (int j = 0; j < L; ++j) { p[i][j] = 0.f; ds[i][j] = 0.f; }
  }
  // pass 1: s
  for (int c = 0; c < D; c += 64) {
    u32x4 qr[L], kr[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
      qr[i] = *reinterpret_cast<const u32x4*>(Qp + i * RS + c);
      kr[i] = *reinterpret_cast<const u32x4*>(Kp + i * RS + c);
    }
#pragma unroll
    for (int j = 0; j < L; ++j) {
      float k[8];
      unpack8<OT>(kr[j], k);
#pragma unroll
      for (int i = j; i < L; ++i) {
        float q[8];
        unpack8<OT>(qr[i], q);
#pragma unroll
        for (int e = 0; e < 8; ++e) p[i][j] = fmaf(q[e], k[e], p[i][j]);
      }
    }
  }
  // pass 2: dP and delta
  for (int c = 0; c < D; c += 64) {
    u32x4 gr[L], vr[L], orw[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
      gr[i] = *reinterpret_cast<const u32x4*>(Gp + i * HD + c);
      vr[i] = *reinterpret_cast<const u32x4*>(Vp + i * RS + c);
      orw[i] = *reinterpret_cast<const u32x4*>(Op + i * HD + c);
    }
#pragma unroll
    for (int i = 0; i < L; ++i) {
      float d[8], o[8];
      unpack8<OT>(gr[i], d);
      unpack8<OT>(orw[i], o);
#pragma unroll
      for (int e = 0; e < 8; ++e) delta[i] = fmaf(d[e], o[e], delta[i]);
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        float v[8];
        unpack8<OT>(vr[j], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) ds[i][j] = fmaf(d[e], v[e], ds[i][j]);
      }
    }
  }
  // the group's sums; P and dS in the operand format
#pragma unroll
  for (int i = 0; i < L; ++i) {
    float dl = delta[i];
    dl += __shfl_xor(dl, 1, 64);
    dl += __shfl_xor(dl, 2, 64);
    dl += __shfl_xor(dl, 4, 64);
    const float lse2 = lse[pair * L + i] * RQ_LOG2E;
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      float s = p[i][j], dp = ds[i][j];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      dp += __shfl_xor(dp, 1, 64);
      dp += __shfl_xor(dp, 2, 64);
      dp += __shfl_xor(dp, 4, 64);
      const float pe = __builtin_amdgcn_exp2f(s * scale_log2 - lse2);
      p[i][j] = unpack1<OT>(pack1<OT>(pe));
      ds[i][j] = i == 0 ? 0.f : unpack1<OT>(pack1<OT>(pe * (dp - dl)));
    }
  }
  // pass 3: the three outputs, chunk by chunk
  uint16_t* dQp = dqkv + qoff;
  uint16_t* dKp = dQp + HD;
  uint16_t* dVp = dKp + HD;
  for (int c = 0; c < D; c += 64) {
    {      // dv[j] = sum_{i >= j} P[i][j] dO[i], ascending i
      u32x4 gr[L];
#pragma unroll
      for (int i = 0; i < L; ++i) gr[i] = *reinterpret_cast<const u32x4*>(Gp + i * HD + c);
#pragma unroll
      for (int j = 0; j < L; ++j) {
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
#pragma unroll
        for (int i = j; i < L; ++i) {
          float d[8];
          unpack8<OT>(gr[i], d);
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = fmaf(p[i][j], d[e], a[e]);
        }
        const u32x4 pk = {pack2<OT>(a[0], a[1]), pack2<OT>(a[2], a[3]), pack2<OT>(a[4], a[5]), pack2<OT>(a[6], a[7])};
        *reinterpret_cast<u32x4*>(dVp + j * RS + c) = pk;
      }
    }
    {      // dq[i] = scale sum_{j <= i} dS[i][j] k[j], ascending j; row 0 is zero
      u32x4 kr[L];
#pragma unroll
      for (int j = 0; j < L; ++j) kr[j] = *reinterpret_cast<const u32x4*>(Kp + j * RS + c);
      const u32x4 zero = {0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(dQp + c) = zero;
#pragma unroll
      for (int i = 1; i < L; ++i) {
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          float k[8];
          unpack8<OT>(kr[j], k);
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = fmaf(ds[i][j], k[e], a[e]);
        }
        const u32x4 pk = {pack2<OT>(a[0] * scale, a[1] * scale), pack2<OT>(a[2] * scale, a[3] * scale), pack2<OT>(a[4] * scale, a[5] * scale),
                          pack2<OT>(a[6] * scale, a[7] * scale)};
        *reinterpret_cast<u32x4*>(dQp + i * RS + c) = pk;
      }
    }
    {      // dk[j] = scale sum_{i >= j} dS[i][j] q[i], ascending i
      u32x4 qr[L];
#pragma unroll
      for (int i = 0; i < L; ++i) qr[i] = *reinterpret_cast<const u32x4*>(Qp + i * RS + c);
#pragma unroll
      for (int j = 0; j < L; ++j) {
        float a[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = 0.f;
#pragma unroll
        for (int i = j; i < L; ++i) {
          float q[8];
          unpack8<OT>(qr[i], q);
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = fmaf(ds[i][j], q[e], a[e]);
        }
        const u32x4 pk = {pack2<OT>(a[0] * scale, a[1] * scale), pack2<OT>(a[2] * scale, a[3] * scale), pack2<OT>(a[4] * scale, a[5] * scale),
                          pack2<OT>(a[6] * scale, a[7] * scale)};
        *reinterpret_cast<u32x4*>(dKp + j * RS + c) = pk;
      }
    }
  }
}

#define RQ_LB_CASE(LL)                                                                                                                                  \
  case LL:                                                                                                                                              \
    ENH_DT_DISPATCH(dtype, (rq_short_causal_bwd_kernel<LL, OT><<<grid, 256, 0, (hipStream_t)stream>>>(qkv, out, dout, lse, npairs, H, D, scale,       \
                                                                                                       scale * RQ_LOG2E, dqkv)));                       \
    break

extern "C" int enh_short_causal_attention_backward(const enh_h16* qkv, const enh_h16* out, const enh_h16* dout, const float* lse, int NSEQ, int L, int H, int D,
                                                   float scale, enh_h16* dqkv, int dtype, void* stream) {
  ENH_REQUIRE(L >= 1 && L <= RQ_MAX_DEPTH, ENH_E_SHAPE, "enh_short_causal_attention_backward: the sequence length must be in [1, %d], got %d", RQ_MAX_DEPTH, L);
  ENH_REQUIRE(D >= 64 && D <= 384 && D % 64 == 0, ENH_E_SHAPE, "enh_short_causal_attention_backward: dim_head must be a multiple of 64 up to 384, got %d", D);
  ENH_REQUIRE_DT(dtype, "enh_short_causal_attention_backward");
  ENH_REQUIRE(qkv && out && dout && lse && dqkv, ENH_E_BADARG, "enh_short_causal_attention_backward: null pointer");
  ENH_REQUIRE(NSEQ > 0 && H > 0, ENH_E_SHAPE, "enh_short_causal_attention_backward: need positive NSEQ, H (NSEQ=%d H=%d)", NSEQ, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_short_causal_attention_backward: scale must be positive");
  const int64_t npairs = (int64_t)NSEQ * H, wgs = (npairs + 31) / 32;
  ENH_REQUIRE(wgs <= 2147483647LL, ENH_E_SHAPE, "enh_short_causal_attention_backward: too many workgroups (NSEQ=%d H=%d)", NSEQ, H);
  const unsigned grid = (unsigned)wgs;
  enh_note_kernel_dh("rq_short_causal_bwd_kernel", L, dtype);
  switch (L) {
    RQ_LB_CASE(1); RQ_LB_CASE(2); RQ_LB_CASE(3); RQ_LB_CASE(4); RQ_LB_CASE(5); RQ_LB_CASE(6); RQ_LB_CASE(7); RQ_LB_CASE(8);
  }
  return enh_check_launch("enh_short_causal_attention_backward");
}

// ---------------------------------------------------------------------------------------------
// embedding backward
// ---------------------------------------------------------------------------------------------
// The scheme of gpt_rows.hip's gpt_embed_seq_bwd_kernel: one workgroup per table row with all of its columns in registers (a thread holds
// C / 1024 <= 8 float4 sums).  blockIdx.x walks the rows of tok_code [V], tok_cond [Vc], pos_code [P], pos_depth [Dp - 1] and pos_cond [1].
// A row of tok_code scans the B T Dp codes, 256 per round (the four waves publish their match ballots), and adds for every match (b, t, j), in
// ascending (b, t, j) order, what that occurrence of the code fed: spatial row t + 1 (while t <= T - 2), then slots d = j + 1 .. Dp - 1 of depth
// sequence (b, t), d ascending.  Code (b, T - 1, Dp - 1) is fed to nothing and never matches.  Ids are clamped as the forward clamps them, never
// followed.  A row without a match is written as zeros, or left alone under `accumulate`.  pos_code[t] = sum_b gs[b, t + 1] for t <= T - 2 and
// zero beyond; pos_depth[d - 1] = sum over (b, t) ascending of gd[(b, t), d]; pos_cond = sum_b gs[b, 0].  Slot 0 of gd is never read.
__global__ __launch_bounds__(256) void rq_embed_seq_bwd_kernel(const float* __restrict__ gs, const float* __restrict__ gd, const int64_t* __restrict__ conds,
                                                               const int64_t* __restrict__ codes, int B, int T, int Dp, int C, int Vc, int V, int P,
                                                               float* __restrict__ dtok_cond, float* __restrict__ dpos_cond, float* __restrict__ dtok_code,
                                                               float* __restrict__ dpos_code, float* __restrict__ dpos_depth, int accumulate) {
  __shared__ unsigned long long s_mask[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nv = C >> 2;
  int row = blockIdx.x;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = zero;
  auto add_row = [&](const float* __restrict__ gr) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (t + 256 * k < nv) acc[k] = acc[k] + *reinterpret_cast<const f32x4*>(gr + 4 * (t + 256 * k));
  };
  float* out;
  bool any = true;      // workgroup-uniform: whether the row received a term
  if (row < V + Vc) {
    const bool is_code = row < V;
    const int id = is_code ? row : row - V;
    const int64_t n_ids = is_code ? (int64_t)B * T * Dp : (int64_t)B;
    const int64_t top = is_code ? V - 1 : Vc - 1;
    out = (is_code ? dtok_code : dtok_cond) + (int64_t)id * C;
    any = false;
    for (int64_t base = 0; base < n_ids; base += 256) {
      const int64_t i = base + t;
      bool match = false;
      if (i < n_ids) {
        int64_t v = is_code ? codes[i] : conds[i];
        v = v < 0 ? 0 : (v > top ? top : v);
        match = v == id;
        if (is_code) {
          const int64_t m = i / Dp;
          match = match && !((int)(i - m * Dp) == Dp - 1 && (int)(m % T) == T - 1);
        }
      }
      const unsigned long long mk = __ballot(match);
      if (lane == 0) s_mask[wave] = mk;
      __syncthreads();
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        unsigned long long mm = s_mask[ww];
        any = any || mm != 0ull;
        while (mm) {
          const int jb = __builtin_ctzll(mm);
          mm &= mm - 1;
          const int64_t i2 = base + ww * 64 + jb;
          if (is_code) {
            const int64_t m = i2 / Dp;
            const int j = (int)(i2 - m * Dp);
            if ((int)(m % T) < T - 1) add_row(gs + (m + 1) * C);
            for (int d = j + 1; d < Dp; ++d) add_row(gd + (m * Dp + d) * C);
          } else {
            add_row(gs + i2 * T * C);
          }
        }
      }
      __syncthreads();
    }
  } else {
    row -= V + Vc;
    if (row < P) {
      out = dpos_code + (int64_t)row * C;
      any = row < T - 1;
      if (any)
        for (int bb = 0; bb < B; ++bb) add_row(gs + ((int64_t)bb * T + row + 1) * C);
    } else if (row < P + Dp - 1) {
      const int d = row - P + 1;
      out = dpos_depth + (int64_t)(d - 1) * C;
      const int64_t n = (int64_t)B * T;
#pragma unroll 4
      for (int64_t m = 0; m < n; ++m) add_row(gd + (m * Dp + d) * C);
    } else {
      out = dpos_cond;
      for (int bb = 0; bb < B; ++bb) add_row(gs + (int64_t)bb * T * C);
    }
  }
  if (accumulate && !any) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = 4 * (t + 256 * k);
    if (c >= C) continue;
    f32x4 r = acc[k];
    if (accumulate) r = r + *reinterpret_cast<const f32x4*>(out + c);
    *reinterpret_cast<f32x4*>(out + c) = r;
  }
}

extern "C" int enh_rq_embed_seq_backward(const float* gs, const float* gd, const int64_t* conds, const int64_t* codes, int B, int T, int Dp, int C, int Vc, int V,
                                         int P, float* dtok_cond, float* dpos_cond, float* dtok_code, float* dpos_code, float* dpos_depth, int accumulate,
                                         void* stream) {
  ENH_REQUIRE(gs && gd && conds && codes && dtok_cond && dpos_cond && dtok_code && dpos_code && dpos_depth, ENH_E_BADARG, "enh_rq_embed_seq_backward: null pointer");
  ENH_REQUIRE(B >= 1 && T >= 1 && Vc >= 1 && V >= 1 && P >= T - 1 && P >= 0 && (int64_t)B * T * RQ_MAX_DEPTH <= 2147483647LL &&
                  (int64_t)V + Vc + P + RQ_MAX_DEPTH <= 2147483647LL, ENH_E_BADARG, "enh_rq_embed_seq_backward: B=%d T=%d Vc=%d V=%d P=%d", B, T, Vc, V, P);
  ENH_REQUIRE(Dp >= 2 && Dp <= RQ_MAX_DEPTH, ENH_E_SHAPE, "enh_rq_embed_seq_backward: the depth must be in [2, %d], got %d", RQ_MAX_DEPTH, Dp);
  ENH_REQUIRE(C >= 4 && C % 4 == 0 && C <= RQ_EMB_MAX_C, ENH_E_SHAPE, "enh_rq_embed_seq_backward: C must be a multiple of 4 in [4, %d], got %d", RQ_EMB_MAX_C, C);
  enh_note_kernel_plain("rq_embed_seq_bwd_kernel");
  rq_embed_seq_bwd_kernel<<<(unsigned)(V + Vc + P + Dp), 256, 0, (hipStream_t)stream>>>(gs, gd, conds, codes, B, T, Dp, C, Vc, V, P, dtok_cond, dpos_cond, dtok_code,
                                                                                       dpos_code, dpos_depth, accumulate);
  return enh_check_launch("enh_rq_embed_seq_backward");
}
