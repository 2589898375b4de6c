// rq_prefill.hip — what the stage-2 RQTransformer's teacher-forced forward needs beyond the GPT's kernels, for gfx950 (reference
// enhancing/modules/stage2/layers.py: RQTransformer.forward 370-395).  The spatial transformer is the GPT's launch sequence over [B, T] rows; the depth
// transformer runs B T sequences of D <= 8 slots, and around it are:
//
//   enh_rq_embed_seq                     the whole embedding stage in one launch: the spatial stream [B, T, C] (the condition row, then the sum over depth of
//                                        every position's D code embeddings) and slots 1 .. D - 1 of the depth stream [B T, D, C] (the running sums)
//   enh_ln_rows_strided                  LayerNorm of [M, C] rows written with an output row stride: ln_spatial into slot 0 of every depth sequence
//   enh_short_causal_attention_forward   causal attention of NSEQ sequences of L <= 8 tokens, 32 (sequence, head) pairs per workgroup
// No float atomics; every sum runs in a fixed order: the same bits on every run.
#include "common.h"

#define RQ_MAX_DEPTH 8
#define RQ_LN_MAX_D 8192
#define RQ_LOG2E 1.4426950408889634f
#define RQ_LN2 0.6931471805599453f

// ---------------------------------------------------------------------------------------------
// embedding
// ---------------------------------------------------------------------------------------------
// One workgroup per position (b, t); a thread owns float4 columns c, c + 1024, ...  It reads the position's embedding rows once, in ascending depth,
// and keeps the running sum in registers: after rows 0 .. d - 1 the sum (+ pos_depth[d - 1]) is slot d of depth sequence b T + t, after all D rows
// the sum (+ pos_code[t]) is spatial row t + 1.  The spatial stream has S = T rows: position T - 1 has no spatial row (the causal mask keeps it from
// every logit), so its last embedding row is not read.  The workgroup of t == 0 also writes the condition row.  Slot 0 of the depth stream is
// enh_ln_rows_strided's.  One rounding per addition: the bits of the same sums in that order anywhere.  An id outside its table is clamped, never followed.
__global__ __launch_bounds__(256) void rq_embed_seq_kernel(const int64_t* __restrict__ conds, const int64_t* __restrict__ codes, const float* __restrict__ tok_cond,
                                                           const float* __restrict__ pos_cond, const float* __restrict__ tok_code,
                                                           const float* __restrict__ pos_code, const float* __restrict__ pos_depth, int T, int Dp, int C,
                                                           int Vc, int V, float* __restrict__ spatial, float* __restrict__ depth) {
  const int64_t m = blockIdx.x;
  const int64_t b = m / T;
  const int t = (int)(m - b * T);
  const bool has_row = t + 1 < T;      // workgroup-uniform
  const int n_read = has_row ? Dp : Dp - 1;
  const float* rows[RQ_MAX_DEPTH];
#pragma unroll
  for (int j = 0; j < RQ_MAX_DEPTH; ++j) {
    int64_t id = j < n_read ? codes[m * Dp + j] : 0;
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    rows[j] = tok_code + id * C;
  }
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    if (t == 0) {
      int64_t id = conds[b];
      id = id < 0 ? 0 : (id >= Vc ? Vc - 1 : id);
      *reinterpret_cast<f32x4*>(spatial + m * C + c) = *reinterpret_cast<const f32x4*>(tok_cond + id * C + c) + *reinterpret_cast<const f32x4*>(pos_cond + c);
    }
    f32x4 run = *reinterpret_cast<const f32x4*>(rows[0] + c);
#pragma unroll
    for (int d = 1; d < RQ_MAX_DEPTH; ++d) {
      if (d < Dp) {
        *reinterpret_cast<f32x4*>(depth + (m * Dp + d) * C + c) = run + *reinterpret_cast<const f32x4*>(pos_depth + (int64_t)(d - 1) * C + c);
        if (d < n_read) run = run + *reinterpret_cast<const f32x4*>(rows[d] + c);
      }
    }
    if (has_row) *reinterpret_cast<f32x4*>(spatial + (m + 1) * C + c) = run + *reinterpret_cast<const f32x4*>(pos_code + (int64_t)t * C + c);
  }
}

extern "C" int enh_rq_embed_seq(const int64_t* conds, const int64_t* codes, const float* tok_cond, const float* pos_cond, const float* tok_code,
                                const float* pos_code, const float* pos_depth, int B, int T, int Dp, int C, int Vc, int V, float* spatial, float* depth,
                                void* stream) {
  ENH_REQUIRE(conds && codes && tok_cond && pos_cond && tok_code && pos_code && pos_depth && spatial && depth, ENH_E_BADARG, "enh_rq_embed_seq: null pointer");
  ENH_REQUIRE(B >= 1 && T >= 1 && Vc >= 1 && V >= 1 && (int64_t)B * T <= 2147483647LL, ENH_E_BADARG, "enh_rq_embed_seq: B=%d T=%d Vc=%d V=%d", B, T, Vc, V);
  ENH_REQUIRE(Dp >= 2 && Dp <= RQ_MAX_DEPTH, ENH_E_SHAPE, "enh_rq_embed_seq: the depth must be in [2, %d], got %d", RQ_MAX_DEPTH, Dp);
  ENH_REQUIRE(C >= 4 && C % 4 == 0, ENH_E_SHAPE, "enh_rq_embed_seq: C must be a positive multiple of 4, got %d", C);
  enh_note_kernel_plain("rq_embed_seq_kernel");
  rq_embed_seq_kernel<<<(unsigned)(B * T), 256, 0, (hipStream_t)stream>>>(conds, codes, tok_cond, pos_cond, tok_code, pos_code, pos_depth, T, Dp, C, Vc, V, spatial,
                                                                          depth);
  return enh_check_launch("enh_rq_embed_seq");
}

// ---------------------------------------------------------------------------------------------
// LayerNorm with an output row stride
// ---------------------------------------------------------------------------------------------
// One workgroup per row, the row in registers (8 x float4 per thread: D <= 8192), mean and variance in two passes over them: the arithmetic of
// gpt_rows.hip's gpt_prefill_ln_kernel without a column scale or a shifted term.  Row m of the f32 output starts at out + m out_stride.
__global__ __launch_bounds__(256) void rq_ln_strided_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int D, float eps,
                                                            float* __restrict__ out, int64_t out_stride) {
  __shared__ float s_red[4];
  const int t = threadIdx.x;
  const int64_t m = blockIdx.x;
  const int nv = D >> 2;
  const float* xr = x + m * D;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 v[8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = t + 256 * i;
    v[i] = c < nv ? *reinterpret_cast<const f32x4*>(xr + 4 * c) : zero;
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float mean = block_sum<4>(s, s_red) / (float)D;
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (t + 256 * i < nv) {
      const f32x4 d = v[i] - mean;
      s2 += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    }
  }
  const float rstd = 1.0f / sqrtf(block_sum<4>(s2, s_red) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = t + 256 * i;
    if (c >= nv) continue;
    const f32x4 g = *reinterpret_cast<const f32x4*>(w + 4 * c), bb = *reinterpret_cast<const f32x4*>(bias + 4 * c);
    *reinterpret_cast<f32x4*>(out + m * out_stride + 4 * c) = (v[i] - mean) * rstd * g + bb;
  }
}

extern "C" int enh_ln_rows_strided(const float* x, const float* w, const float* b, int64_t M, int D, float eps, float* out, int64_t out_stride, void* stream) {
  ENH_REQUIRE(x && w && b && out, ENH_E_BADARG, "enh_ln_rows_strided: null pointer");
  ENH_REQUIRE(M >= 1 && M <= 2147483647LL, ENH_E_SHAPE, "enh_ln_rows_strided: M=%lld", (long long)M);
  ENH_REQUIRE(D >= 8 && D <= RQ_LN_MAX_D && D % 8 == 0, ENH_E_SHAPE, "enh_ln_rows_strided: D must be a multiple of 8 in [8, %d], got %d", RQ_LN_MAX_D, D);
  ENH_REQUIRE(out_stride >= D && out_stride % 4 == 0, ENH_E_SHAPE, "enh_ln_rows_strided: the output row stride must be a multiple of 4 that is at least D=%d, got %lld",
              D, (long long)out_stride);
  enh_note_kernel_plain("rq_ln_strided_kernel");
  rq_ln_strided_kernel<<<(unsigned)M, 256, 0, (hipStream_t)stream>>>(x, w, b, D, eps, out, out_stride);
  return enh_check_launch("enh_ln_rows_strided");
}

// ---------------------------------------------------------------------------------------------
// short-sequence causal attention
// ---------------------------------------------------------------------------------------------
// Eight lanes own one (sequence, head) pair; a workgroup of 256 threads holds 32 pairs, neighbouring groups the neighbouring heads of a sequence.  Lane g of
// a group owns columns 64 c + 8 g .. + 7 of every 64-column chunk c of the head: one 16-byte load per row and chunk, and the eight lanes of a group
// read one whole 128-byte line.  q, k and v are each read once and out is written once (8 H Dh bytes per token row); nothing goes through LDS.
//   scores   a lane adds the products of its columns of q_i and k_j for the L (L + 1) / 2 pairs j <= i in f32 (fmaf, ascending column), chunk after
//            chunk; an xor butterfly over the group's eight lanes adds the partial sums, so every lane of the group holds the same bits
//   softmax  t_j = s_ij scale log2(e) as a rounded product of its own (never fused into the subtraction: the largest numerator is exactly 1, as in
//            gpt_prefill_causal_kernel), e_j = exp2(t_j - max), l = sum of the unrounded e_j in ascending j
//   P V      e_j rounded to the operand format, times v_j in f32, added in ascending j; out = sum / l, rounded once
// The loops over L are unrolled (a kernel per L): scores and probabilities stay in registers, and keys above the diagonal are never touched.
template <int L, typename OT>
__global__ __launch_bounds__(256) void rq_short_causal_kernel(const uint16_t* __restrict__ qkv, int64_t npairs, int H, int D, float scale_log2,
                                                              uint16_t* __restrict__ out, float* __restrict__ lse) {
  const int64_t pair = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  if (pair >= npairs) return;      // uniform over the group's eight lanes: the butterfly below stays inside a group
  const int g = threadIdx.x & 7;
  const int64_t seq = pair / H;
  const int h = (int)(pair - seq * H);
  const int64_t RS = (int64_t)3 * H * D, HD = (int64_t)H * D;
  const uint16_t* Qp = qkv + seq * L * RS + (int64_t)h * D + g * 8;
  const uint16_t* Kp = Qp + HD;
  const uint16_t* Vp = Kp + HD;

  float s[L][L];
#pragma unroll
  for (int i = 0; i < L; ++i)
#pragma unroll
    for (int j = 0; j < L; ++j) s[i][j] = 0.f;
  for (int c = 0; c < D; c += 64) {
    u32x4 qr[L], kr[L];
#pragma unroll
    for (int i = 0; i < L; ++i) {
      qr[i] = *reinterpret_cast<const u32x4*>(Qp + i * RS + c);
      kr[i] = *reinterpret_cast<const u32x4*>(Kp + i * RS + c);
    }
    float k[L][8];
#pragma unroll
    for (int j = 0; j < L; ++j) unpack8<OT>(kr[j], k[j]);
#pragma unroll
    for (int i = 0; i < L; ++i) {
      float q[8];
      unpack8<OT>(qr[i], q);
#pragma unroll
      for (int j = 0; j <= i; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) s[i][j] = fmaf(q[e], k[j][e], s[i][j]);
    }
  }
  float inv[L];
#pragma unroll
  for (int i = 0; i < L; ++i) {
    float mx = -__builtin_inff();
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      float v = s[i][j];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      s[i][j] = __fmul_rn(v, scale_log2);
      mx = fmaxf(mx, s[i][j]);
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const float e = __builtin_amdgcn_exp2f(s[i][j] - mx);
      l += e;
      s[i][j] = unpack1<OT>(pack1<OT>(e));
    }
    inv[i] = 1.0f / l;
    if (lse && g == 0) lse[pair * L + i] = (mx + __builtin_amdgcn_logf(l)) * RQ_LN2;
  }
  uint16_t* Op = out + seq * L * HD + (int64_t)h * D + g * 8;
  for (int c = 0; c < D; c += 64) {
    float v[L][8];
#pragma unroll
    for (int j = 0; j < L; ++j) unpack8<OT>(*reinterpret_cast<const u32x4*>(Vp + j * RS + c), v[j]);
#pragma unroll
    for (int i = 0; i < L; ++i) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j <= i; ++j) acc = fmaf(s[i][j], v[j][e], acc);
        o[e] = acc * inv[i];
      }
      const u32x4 pk = {pack2<OT>(o[0], o[1]), pack2<OT>(o[2], o[3]), pack2<OT>(o[4], o[5]), pack2<OT>(o[6], o[7])};
      *reinterpret_cast<u32x4*>(Op + i * HD + c) = pk;
    }
  }
}

#define RQ_L_CASE(LL) \
  case LL: ENH_DT_DISPATCH(dtype, (rq_short_causal_kernel<LL, OT><<<grid, 256, 0, (hipStream_t)stream>>>(qkv, npairs, H, D, scale * RQ_LOG2E, out, lse))); break

extern "C" int enh_short_causal_attention_forward(const enh_h16* qkv, int NSEQ, int L, int H, int D, float scale, enh_h16* out, float* lse, int dtype, void* stream) {
  ENH_REQUIRE(L >= 1 && L <= RQ_MAX_DEPTH, ENH_E_SHAPE, "enh_short_causal_attention_forward: the sequence length must be in [1, %d], got %d", RQ_MAX_DEPTH, L);
  ENH_REQUIRE(D >= 64 && D <= 384 && D % 64 == 0, ENH_E_SHAPE, "enh_short_causal_attention_forward: dim_head must be a multiple of 64 up to 384, got %d", D);
  ENH_REQUIRE_DT(dtype, "enh_short_causal_attention_forward");
  ENH_REQUIRE(qkv && out, ENH_E_BADARG, "enh_short_causal_attention_forward: null pointer");
  ENH_REQUIRE(NSEQ > 0 && H > 0, ENH_E_SHAPE, "enh_short_causal_attention_forward: need positive NSEQ, H (NSEQ=%d H=%d)", NSEQ, H);
  ENH_REQUIRE(scale > 0.f, ENH_E_BADARG, "enh_short_causal_attention_forward: scale must be positive");
  const int64_t npairs = (int64_t)NSEQ * H, wgs = (npairs + 31) / 32;
  ENH_REQUIRE(wgs <= 2147483647LL, ENH_E_SHAPE, "enh_short_causal_attention_forward: too many workgroups (NSEQ=%d H=%d)", NSEQ, H);
  const unsigned grid = (unsigned)wgs;
  enh_note_kernel_dh("rq_short_causal_kernel", L, dtype);
  switch (L) {
    RQ_L_CASE(1); RQ_L_CASE(2); RQ_L_CASE(3); RQ_L_CASE(4); RQ_L_CASE(5); RQ_L_CASE(6); RQ_L_CASE(7); RQ_L_CASE(8);
  }
  return enh_check_launch("enh_short_causal_attention_forward");
}
