// gpt_rows.hip — the row kernels of the stage-2 GPT for gfx950: what both of its paths run between their GEMMs and attentions (reference
// enhancing/modules/stage2/layers.py: Block.forward 146-163, FFN 132-136, GPT.forward 193-211, GPT.sample 213-266, cond_num_tokens == 1).
// Sampling (gpt_decode.hip) sees one token per batch row and step, the teacher-forced forward (gpt_prefill.hip) M = B S token rows at once.
//
//   enh_ln_timeshift         LayerNorm of [B S, D] rows with f32 statistics, D % 8 == 0 up to 8192, times an optional per-column vector tm, and the
//                            time-shift mix  ln(x[b,s]) tm + ln(x[b,s-1]) (1 - tm)  with ln(x[b,-1]) = 0
//   enh_row_ln_scale         the same function of a decode step's <= 64 rows (S = 1: no shifted term), in a kernel of its own: see gpt_row_ln_kernel
//   enh_gpt_embed            x[b] = table[id[b]] + pos[row], ids read from device memory (a strided column): a decode step
//   enh_gpt_embed_seq        the whole [B, S, C] residual stream in one launch
//   enh_relu_sq_h16          square(relu(.)) of the p0 GEMM's f32 output into the 16-bit operand of p1 (or in place; dtype f32: the exact mode)
//   enh_cross_entropy_rows   nll[m] = logsumexp(row m) - row[m][target[m]] and, in a second fixed-order pass, the mean
//   enh_mean_f32             that second pass alone
// and, in the second half of the file, their backward twins for GPT.forward_backward (enh_cross_entropy_backward, enh_relu_sq_backward,
// enh_ln_timeshift_backward, enh_gpt_embed_seq_backward).
// No float atomics; every sum runs in a fixed order (common.h block_sum / block_max): the same bits on every run.
#include "common.h"

#define GR_LN_MAX_D 8192
#define GR_LN_DECODE_MAX_M 64      // rows of one decode step (gpt_decode.hip GD_MAX_M)
#define GR_CE_MAX_V 16384

// ---------------------------------------------------------------------------------------------
// LayerNorm (+ time shift)
// ---------------------------------------------------------------------------------------------
// one workgroup per row; the row is held in registers (8 x float4 per thread: D <= 8192).  mean / rstd in two passes over them.
__device__ __forceinline__ void gpt_ln_row(const float* __restrict__ xr, int nv, int D, float eps, f32x4 (&v)[8], float& mean, float& rstd, float* s_red) {
  const int t = threadIdx.x;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = t + 256 * i;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    v[i] = c < nv ? *reinterpret_cast<const f32x4*>(xr + 4 * c) : zero;
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  mean = block_sum<4>(s, s_red) / (float)D;
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (t + 256 * i < nv) {
      const f32x4 d = v[i] - mean;
      s2 += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    }
  }
  rstd = 1.0f / sqrtf(block_sum<4>(s2, s_red) / (float)D + eps);
}

// row m = (b, s = m % S).  With colscale (time_mix): y = ln(x[m]) tm + ln(x[m - 1]) (1 - tm) for s > 0 and ln(x[m]) tm for s == 0: the shifted term
// of a batch element's first row is zero and never the previous element's last row.  The previous row's LayerNorm is recomputed here (one more
// read of a row that the neighbouring workgroup has just brought into L2) instead of being passed through memory.
template <typename OT>
__global__ __launch_bounds__(256) void gpt_prefill_ln_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             const float* __restrict__ colscale, int S, int D, float eps, float* __restrict__ out_f32,
                                                             uint16_t* __restrict__ out_h16) {
  __shared__ float s_red[4];
  const int t = threadIdx.x;
  const int64_t m = blockIdx.x;
  const int nv = D >> 2;
  const bool shifted = colscale && (m % S) != 0;      // workgroup-uniform
  f32x4 v[8], vp[8];
  float mean, rstd, meanp = 0.f, rstdp = 0.f;
  gpt_ln_row(x + m * D, nv, D, eps, v, mean, rstd, s_red);
  if (shifted) gpt_ln_row(x + (m - 1) * D, nv, D, eps, vp, meanp, rstdp, s_red);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = t + 256 * i;
    if (c >= nv) continue;
    const f32x4 g = *reinterpret_cast<const f32x4*>(w + 4 * c), bb = *reinterpret_cast<const f32x4*>(bias + 4 * c);
    f32x4 y = (v[i] - mean) * rstd * g + bb;
    if (colscale) {
      const f32x4 tm = *reinterpret_cast<const f32x4*>(colscale + 4 * c);
      y = y * tm;
      if (shifted) y = y + ((vp[i] - meanp) * rstdp * g + bb) * (1.0f - tm);
    }
    const int64_t o = m * D + 4 * c;
    if (out_f32) *reinterpret_cast<f32x4*>(out_f32 + o) = y;
    if (out_h16) {
      const u32x2 pk = {pack2<OT>(y.x, y.y), pack2<OT>(y.z, y.w)};
      *reinterpret_cast<u32x2*>(out_h16 + o) = pk;
    }
  }
}

extern "C" int enh_ln_timeshift(const float* x, const float* w, const float* b, const float* colscale, int64_t M, int S, int D, float eps, float* out_f32,
                                enh_h16* out_h16, int dtype, void* stream) {
  ENH_REQUIRE(x && w && b && (out_f32 || out_h16), ENH_E_BADARG, "enh_ln_timeshift: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_ln_timeshift");
  ENH_REQUIRE(M >= 1 && M <= 2147483647LL && S >= 1 && M % S == 0, ENH_E_SHAPE, "enh_ln_timeshift: M=%lld rows must be whole sequences of S=%d", (long long)M, S);
  ENH_REQUIRE(D >= 8 && D <= GR_LN_MAX_D && D % 8 == 0, ENH_E_SHAPE, "enh_ln_timeshift: D must be a multiple of 8 in [8, %d], got %d", GR_LN_MAX_D, D);
  enh_note_kernel("gpt_prefill_ln_kernel", dtype);
  ENH_DT_DISPATCH(dtype, (gpt_prefill_ln_kernel<OT><<<(unsigned)M, 256, 0, (hipStream_t)stream>>>(x, w, b, colscale, S, D, eps, out_f32, out_h16)));
  return enh_check_launch("enh_ln_timeshift");
}

// A decode step's rows: what gpt_prefill_ln_kernel computes at S = 1, and NOT the same bits.  The compiler fuses the variance pass of gpt_ln_row into
// multiply-adds (d.x d.x + d.y d.y becomes one fma) and packs this kernel's into v_pk_mul_f32 / v_pk_add_f32 with every product rounded: on the
// rows of a sampling step the two differ by an ulp of the statistics (measured: 120 of 256 outputs of one LayerNorm of the `tiny` test model, up to
// 2.4e-7; its exact-mode logits then differ by up to 1.2e-6).  Sampling's logits are pinned bit for bit, so the decode path keeps this kernel.
template <typename OT>
__global__ __launch_bounds__(256) void gpt_row_ln_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ colscale, int D, float eps, float* __restrict__ out_f32,
                                                         uint16_t* __restrict__ out_h16) {
  __shared__ float s_red[4];
  const int t = threadIdx.x;
  const float* xr = x + (size_t)blockIdx.x * D;
  const int nv = D >> 2;      // float4 pieces of the row (<= 2048)
  f32x4 v[8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = t + 256 * i;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
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
    f32x4 y = (v[i] - mean) * rstd * g + bb;
    if (colscale) y = y * *reinterpret_cast<const f32x4*>(colscale + 4 * c);
    const size_t o = (size_t)blockIdx.x * D + 4 * c;
    if (out_f32) *reinterpret_cast<f32x4*>(out_f32 + o) = y;
    if (out_h16) {
      const u32x2 pk = {pack2<OT>(y.x, y.y), pack2<OT>(y.z, y.w)};
      *reinterpret_cast<u32x2*>(out_h16 + o) = pk;
    }
  }
}

extern "C" int enh_row_ln_scale(const float* x, const float* w, const float* b, const float* colscale, int M, int D, float eps, float* out_f32,
                                enh_h16* out_h16, int dtype, void* stream) {
  ENH_REQUIRE(x && w && b && (out_f32 || out_h16), ENH_E_BADARG, "enh_row_ln_scale: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_row_ln_scale");
  ENH_REQUIRE(M >= 1 && M <= GR_LN_DECODE_MAX_M, ENH_E_SHAPE, "enh_row_ln_scale: M must be in [1, %d], got %d", GR_LN_DECODE_MAX_M, M);
  ENH_REQUIRE(D >= 8 && D <= GR_LN_MAX_D && D % 8 == 0, ENH_E_SHAPE, "enh_row_ln_scale: D must be a multiple of 8 in [8, %d], got %d", GR_LN_MAX_D, D);
  enh_note_kernel("gpt_row_ln_kernel", dtype);
  ENH_DT_DISPATCH(dtype, (gpt_row_ln_kernel<OT><<<(unsigned)M, 256, 0, (hipStream_t)stream>>>(x, w, b, colscale, D, eps, out_f32, out_h16)));
  return enh_check_launch("enh_row_ln_scale");
}

// ---------------------------------------------------------------------------------------------
// embedding: one row per decode step, or the whole sequence
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gpt_embed_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids, int64_t id_stride,
                                                        const float* __restrict__ pos_row, int C, int V, float* __restrict__ out) {
  int64_t id = ids[(int64_t)blockIdx.x * id_stride];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);      // an id outside the table cannot come from the sampler; a caller's is clamped, never followed
  const float* row = table + (size_t)id * C;
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(row + c), p = *reinterpret_cast<const f32x4*>(pos_row + c);
    *reinterpret_cast<f32x4*>(out + (size_t)blockIdx.x * C + c) = a + p;
  }
}

extern "C" int enh_gpt_embed(const float* table, const int64_t* ids, int64_t id_stride, const float* pos_row, int B, int C, int V, float* out, void* stream) {
  ENH_REQUIRE(table && ids && pos_row && out, ENH_E_BADARG, "enh_gpt_embed: null pointer");
  ENH_REQUIRE(B >= 1 && V >= 1 && id_stride >= 1, ENH_E_BADARG, "enh_gpt_embed: B=%d V=%d id_stride=%lld", B, V, (long long)id_stride);
  ENH_REQUIRE(C >= 4 && C % 4 == 0, ENH_E_SHAPE, "enh_gpt_embed: C must be a positive multiple of 4, got %d", C);
  enh_note_kernel_plain("gpt_embed_kernel");
  gpt_embed_kernel<<<(unsigned)B, 256, 0, (hipStream_t)stream>>>(table, ids, id_stride, pos_row, C, V, out);
  return enh_check_launch("enh_gpt_embed");
}

// row (b, s): s == 0 the condition (tok_cond[conds[b]] + pos_cond), else code s - 1 of the row (tok_code[codes[b][s - 1]] + pos_code[s - 1]).
// An id outside its table is clamped, never followed (the Python side refuses such codes before the launch).
__global__ __launch_bounds__(256) void gpt_prefill_embed_kernel(const int64_t* __restrict__ conds, const int64_t* __restrict__ codes, int64_t code_stride,
                                                                const float* __restrict__ tok_cond, const float* __restrict__ pos_cond,
                                                                const float* __restrict__ tok_code, const float* __restrict__ pos_code, int S, int C,
                                                                int Vc, int V, float* __restrict__ out) {
  const int64_t m = blockIdx.x;
  const int64_t b = m / S;
  const int s = (int)(m - b * S);
  const float *row, *pos;
  if (s == 0) {
    int64_t id = conds[b];
    id = id < 0 ? 0 : (id >= Vc ? Vc - 1 : id);
    row = tok_cond + id * C;
    pos = pos_cond;
  } else {
    int64_t id = codes[b * code_stride + s - 1];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    row = tok_code + id * C;
    pos = pos_code + (int64_t)(s - 1) * C;
  }
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(row + c), p = *reinterpret_cast<const f32x4*>(pos + c);
    *reinterpret_cast<f32x4*>(out + m * C + c) = a + p;
  }
}

extern "C" int enh_gpt_embed_seq(const int64_t* conds, const int64_t* codes, int64_t code_stride, const float* tok_cond, const float* pos_cond,
                                 const float* tok_code, const float* pos_code, int B, int S, int C, int Vc, int V, float* out, void* stream) {
  ENH_REQUIRE(conds && tok_cond && pos_cond && out && (S == 1 || (codes && tok_code && pos_code)), ENH_E_BADARG, "enh_gpt_embed_seq: null pointer");
  ENH_REQUIRE(B >= 1 && S >= 1 && Vc >= 1 && V >= 1 && code_stride >= S - 1 && (int64_t)B * S <= 2147483647LL, ENH_E_BADARG,
              "enh_gpt_embed_seq: B=%d S=%d Vc=%d V=%d code_stride=%lld", B, S, Vc, V, (long long)code_stride);
  ENH_REQUIRE(C >= 4 && C % 4 == 0, ENH_E_SHAPE, "enh_gpt_embed_seq: C must be a positive multiple of 4, got %d", C);
  enh_note_kernel_plain("gpt_prefill_embed_kernel");
  gpt_prefill_embed_kernel<<<(unsigned)(B * S), 256, 0, (hipStream_t)stream>>>(conds, codes, code_stride, tok_cond, pos_cond, tok_code, pos_code, S, C, Vc, V, out);
  return enh_check_launch("enh_gpt_embed_seq");
}

// ---------------------------------------------------------------------------------------------
// relu^2, cross-entropy
// ---------------------------------------------------------------------------------------------
// y = square(relu(x)), eight elements per thread.  X32: the source is f32 (x), else the 16-bit y itself (in place).  Y32: y is f32.
template <typename OT, bool X32, bool Y32>
__global__ __launch_bounds__(256) void gpt_prefill_relu_sq_kernel(const float* __restrict__ x, void* __restrict__ y_, int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float f[8];
  if constexpr (X32) {
    const f32x4 a = reinterpret_cast<const f32x4*>(x)[2 * i], c = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = c.x; f[5] = c.y; f[6] = c.z; f[7] = c.w;
  } else {
    unpack8<OT>(reinterpret_cast<const u32x4*>(y_)[i], f);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) { f[k] = f[k] < 0.f ? 0.f : f[k]; f[k] = f[k] * f[k]; }      // (not fmaxf: fmaxf(NaN, 0) is 0, and a NaN of the fp16 forward must reach the loss)
  if constexpr (Y32) {
    const f32x4 a = {f[0], f[1], f[2], f[3]}, c = {f[4], f[5], f[6], f[7]};
    reinterpret_cast<f32x4*>(y_)[2 * i] = a;
    reinterpret_cast<f32x4*>(y_)[2 * i + 1] = c;
  } else {
    const u32x4 pk = {pack2<OT>(f[0], f[1]), pack2<OT>(f[2], f[3]), pack2<OT>(f[4], f[5]), pack2<OT>(f[6], f[7])};
    reinterpret_cast<u32x4*>(y_)[i] = pk;
  }
}

extern "C" int enh_relu_sq_h16(const float* x, void* y, int64_t n, int dtype, void* stream) {
  ENH_REQUIRE(y, ENH_E_BADARG, "enh_relu_sq_h16: null pointer");
  ENH_REQUIRE(dtype == ENH_DT_BF16 || dtype == ENH_DT_F16 || dtype == ENH_DT_F32, ENH_E_BADARG, "enh_relu_sq_h16: dtype must be 0, 1 or 2, got %d", dtype);
  ENH_REQUIRE(n >= 8 && n % 8 == 0 && n / 8 <= 2147483647LL * 256, ENH_E_SHAPE, "enh_relu_sq_h16: n must be a positive multiple of 8, got %lld", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n8 = n / 8;
  const unsigned grid = (unsigned)((n8 + 255) / 256);
  if (dtype == ENH_DT_F32) {      // the exact mode: f32 in place (x == NULL or x == y) or from x
    enh_note_kernel_plain("gpt_prefill_relu_sq_kernel<BF16, true, true>");
    gpt_prefill_relu_sq_kernel<BF16, true, true><<<grid, 256, 0, s>>>(x ? x : reinterpret_cast<const float*>(y), y, n8);
  } else if (x) {
    enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_prefill_relu_sq_kernel<F16, true, false>" : "gpt_prefill_relu_sq_kernel<BF16, true, false>");
    ENH_DT_DISPATCH(dtype, (gpt_prefill_relu_sq_kernel<OT, true, false><<<grid, 256, 0, s>>>(x, y, n8)));
  } else {
    enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_prefill_relu_sq_kernel<F16, false, false>" : "gpt_prefill_relu_sq_kernel<BF16, false, false>");
    ENH_DT_DISPATCH(dtype, (gpt_prefill_relu_sq_kernel<OT, false, false><<<grid, 256, 0, s>>>(nullptr, y, n8)));
  }
  return enh_check_launch("enh_relu_sq_h16");
}

// one workgroup per row: nll = log(sum_i exp(x_i - max)) - (x_target - max).  A thread adds its V / 256 terms in ascending index order, the
// workgroup adds the threads in a fixed tree.  A target outside [0, V) is clamped, never followed.
__global__ __launch_bounds__(256) void gpt_prefill_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int V, float* __restrict__ nll) {
  __shared__ float s_red[4];
  const int t = threadIdx.x;
  const float* row = logits + (int64_t)blockIdx.x * V;
  float mx = -__builtin_inff();
  for (int i = t; i < V; i += 256) mx = fmaxf(mx, row[i]);
  mx = block_max<4>(mx, s_red);
  float ps = 0.f;
  for (int i = t; i < V; i += 256) ps += expf(row[i] - mx);
  const float l = block_sum<4>(ps, s_red);
  if (t == 0) {
    int64_t y = target[blockIdx.x];
    y = y < 0 ? 0 : (y >= V ? V - 1 : y);
    nll[blockIdx.x] = logf(l) - (row[y] - mx);
  }
}
// mean of M values by one workgroup: a thread adds every 256th value in ascending order, then the fixed tree
__global__ __launch_bounds__(256) void gpt_prefill_mean_kernel(const float* __restrict__ v, int64_t M, float* __restrict__ mean) {
  __shared__ float s_red[4];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < M; i += 256) s += v[i];
  const float tot = block_sum<4>(s, s_red);
  if (threadIdx.x == 0) mean[0] = tot / (float)M;
}

extern "C" int enh_cross_entropy_rows(const float* logits, const int64_t* target, int64_t M, int V, float* nll, float* mean, void* stream) {
  ENH_REQUIRE(logits && target && nll, ENH_E_BADARG, "enh_cross_entropy_rows: null pointer");
  ENH_REQUIRE(M >= 1 && M <= 2147483647LL, ENH_E_SHAPE, "enh_cross_entropy_rows: M=%lld", (long long)M);
  ENH_REQUIRE(V >= 1 && V <= GR_CE_MAX_V, ENH_E_SHAPE, "enh_cross_entropy_rows: V must be in [1, %d], got %d", GR_CE_MAX_V, V);
  enh_note_kernel_plain("gpt_prefill_ce_kernel");
  gpt_prefill_ce_kernel<<<(unsigned)M, 256, 0, (hipStream_t)stream>>>(logits, target, V, nll);
  if (mean) gpt_prefill_mean_kernel<<<1, 256, 0, (hipStream_t)stream>>>(nll, M, mean);
  return enh_check_launch("enh_cross_entropy_rows");
}

extern "C" int enh_mean_f32(const float* v, int64_t M, float* mean, void* stream) {
  ENH_REQUIRE(v && mean && M >= 1, ENH_E_BADARG, "enh_mean_f32: null pointer or M=%lld", (long long)M);
  enh_note_kernel_plain("gpt_prefill_mean_kernel");
  gpt_prefill_mean_kernel<<<1, 256, 0, (hipStream_t)stream>>>(v, M, mean);
  return enh_check_launch("enh_mean_f32");
}

// =============================================================================================
// backward of the teacher-forced forward: the row kernels between the gradient GEMMs and the attention backward (gpt_attn_bwd.hip)
//
//   enh_cross_entropy_backward    nll as enh_cross_entropy_rows (the same bits) and dlogits = (softmax - onehot) gscale in the operand format: one read of the logits
//   enh_relu_sq_backward          dx = dy 2 relu(h) with relu(h) = sqrt(y) taken from the stored 16-bit y = relu(h)^2 (p1's operand: nothing else is saved)
//   enh_ln_timeshift_backward     gradients of enh_ln_timeshift: dx (+ dres), dw, db, d colscale; row statistics recomputed from x
//   enh_gpt_embed_seq_backward    gradients of enh_gpt_embed_seq's four tables
// =============================================================================================
// One workgroup per row.  The row is read once, 16 bytes per lane, into LDS; the maximum and the sum then run in gpt_prefill_ce_kernel's order
// (thread t adds columns t, t + 256, ... ascending, the workgroup adds the threads in the fixed tree): nll has that kernel's bits.
template <typename OT>
__global__ __launch_bounds__(256) void gpt_ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, int V, float gscale,
                                                         float* __restrict__ nll, uint16_t* __restrict__ dlogits, const float* __restrict__ gscale_dev) {
  __shared__ __attribute__((aligned(16))) float s_row[GR_CE_MAX_V];
  if (gscale_dev) gscale *= *gscale_dev;      // the device loss scale (a power of two: exact)
  __shared__ float s_red[4];
  const int t = threadIdx.x;
  const float* row = logits + (int64_t)blockIdx.x * V;
  for (int c = t; c < (V >> 2); c += 256) *reinterpret_cast<f32x4*>(s_row + 4 * c) = *reinterpret_cast<const f32x4*>(row + 4 * c);
  __syncthreads();
  float mx = -__builtin_inff();
  for (int i = t; i < V; i += 256) mx = fmaxf(mx, s_row[i]);
  mx = block_max<4>(mx, s_red);
  float ps = 0.f;
  for (int i = t; i < V; i += 256) ps += expf(s_row[i] - mx);
  const float l = block_sum<4>(ps, s_red);
  int64_t y = target[blockIdx.x];
  y = y < 0 ? 0 : (y >= V ? V - 1 : y);
  if (t == 0) nll[blockIdx.x] = logf(l) - (s_row[y] - mx);
  const float inv = 1.0f / l;
  uint16_t* drow = dlogits + (int64_t)blockIdx.x * V;
  for (int c = t; c < (V >> 3); c += 256) {
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = (expf(s_row[8 * c + k] - mx) * inv - (8 * c + k == (int)y ? 1.0f : 0.f)) * gscale;
    const u32x4 pk = {pack2<OT>(f[0], f[1]), pack2<OT>(f[2], f[3]), pack2<OT>(f[4], f[5]), pack2<OT>(f[6], f[7])};
    *reinterpret_cast<u32x4*>(drow + 8 * c) = pk;
  }
}

extern "C" int enh_cross_entropy_backward(const float* logits, const int64_t* target, int64_t M, int V, float gscale, float* nll, enh_h16* dlogits, int dtype,
                                          const float* gscale_dev, void* stream) {
  ENH_REQUIRE(logits && target && nll && dlogits, ENH_E_BADARG, "enh_cross_entropy_backward: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_cross_entropy_backward");
  ENH_REQUIRE(M >= 1 && M <= 2147483647LL, ENH_E_SHAPE, "enh_cross_entropy_backward: M=%lld", (long long)M);
  ENH_REQUIRE(V >= 8 && V <= GR_CE_MAX_V && V % 8 == 0, ENH_E_SHAPE, "enh_cross_entropy_backward: V must be a multiple of 8 in [8, %d], got %d", GR_CE_MAX_V, V);
  enh_note_kernel("gpt_ce_bwd_kernel", dtype);
  ENH_DT_DISPATCH(dtype, (gpt_ce_bwd_kernel<OT><<<(unsigned)M, 256, 0, (hipStream_t)stream>>>(logits, target, V, gscale, nll, dlogits, gscale_dev)));
  return enh_check_launch("enh_cross_entropy_backward");
}

// dx = dy 2 relu(h), eight elements per thread.  y = relu(h)^2 in the operand format is what the forward kept (p1's input), so relu(h) = sqrt(y):
// half of y's relative rounding error, and no second copy of the [M, 4C] hidden activation.
template <typename OT>
__global__ __launch_bounds__(256) void gpt_relu_sq_bwd_kernel(const float* __restrict__ dy, const uint16_t* __restrict__ y, uint16_t* __restrict__ dx, int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const f32x4 a = reinterpret_cast<const f32x4*>(dy)[2 * i], c = reinterpret_cast<const f32x4*>(dy)[2 * i + 1];
  const float g[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
  float f[8];
  unpack8<OT>(reinterpret_cast<const u32x4*>(y)[i], f);
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = g[k] * (2.0f * sqrtf(f[k]));
  const u32x4 pk = {pack2<OT>(f[0], f[1]), pack2<OT>(f[2], f[3]), pack2<OT>(f[4], f[5]), pack2<OT>(f[6], f[7])};
  reinterpret_cast<u32x4*>(dx)[i] = pk;
}

extern "C" int enh_relu_sq_backward(const float* dy, const enh_h16* y, enh_h16* dx, int64_t n, int dtype, void* stream) {
  ENH_REQUIRE(dy && y && dx, ENH_E_BADARG, "enh_relu_sq_backward: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_relu_sq_backward");
  ENH_REQUIRE(n >= 8 && n % 8 == 0 && n / 8 <= 2147483647LL * 256, ENH_E_SHAPE, "enh_relu_sq_backward: n must be a positive multiple of 8, got %lld", (long long)n);
  const int64_t n8 = n / 8;
  enh_note_kernel("gpt_relu_sq_bwd_kernel", dtype);
  ENH_DT_DISPATCH(dtype, (gpt_relu_sq_bwd_kernel<OT><<<(unsigned)((n8 + 255) / 256), 256, 0, (hipStream_t)stream>>>(dy, y, dx, n8)));
  return enh_check_launch("enh_relu_sq_backward");
}

// ---------------------------------------------------------------------------------------------
// LayerNorm (+ time shift) backward
// ---------------------------------------------------------------------------------------------
// y[m] = ln[m] tm + ln[m - 1] (1 - tm), ln[m] = xhat[m] w + b.  The gradient reaching ln[m] is g = dy[m] tm + dy[m + 1] (1 - tm), the second term
// only while row m + 1 belongs to the same sequence; d tm = sum_m dy[m] (ln[m] - ln[m - 1]) = sum_m ln[m] (dy[m] - dy[m + 1]) with the same
// condition, so a row needs its own statistics only (recomputed from x, as the forward recomputes its neighbour's).  Without colscale g = dy.
// A workgroup walks GR_LNB_ROWS consecutive rows, one at a time as gpt_prefill_ln_kernel holds a row, and keeps its column sums of dw, db and
// d tm in registers; they go to part[block][3][D], which gpt_ln_bwd_reduce_kernel adds in ascending block order.
// Row m of dy starts at dy + m dys (dys = D: contiguous rows; rq_ln_strided_bwd_kernel below passes the stride of slot 0 of the depth sequences);
// x, dres, dx and dx16 are contiguous [M, D].
#define GR_LNB_ROWS 8
template <typename OT>
__device__ __forceinline__ void gpt_ln_bwd_rows(const float* __restrict__ dy, int64_t dys, const float* __restrict__ x, const float* __restrict__ w,
                                                const float* __restrict__ bias, const float* __restrict__ colscale, const float* __restrict__ dres, int64_t M,
                                                int S, int D, float eps, float* __restrict__ dx, uint16_t* __restrict__ dx16, float* __restrict__ part,
                                                float* s_red) {
  const int t = threadIdx.x;
  const int nv = D >> 2;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 aw[8], ab[8], at[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { aw[i] = zero; ab[i] = zero; at[i] = zero; }
  const int64_t m0 = (int64_t)blockIdx.x * GR_LNB_ROWS;
  const int64_t m1 = m0 + GR_LNB_ROWS < M ? m0 + GR_LNB_ROWS : M;
  for (int64_t m = m0; m < m1; ++m) {
    f32x4 v[8];
    float mean, rstd;
    gpt_ln_row(x + m * D, nv, D, eps, v, mean, rstd, s_red);
    const bool has_next = colscale && (m % S) != S - 1;      // workgroup-uniform
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = t + 256 * i;
      if (c >= nv) continue;
      const f32x4 gw = *reinterpret_cast<const f32x4*>(w + 4 * c);
      f32x4 g = *reinterpret_cast<const f32x4*>(dy + m * dys + 4 * c);
      const f32x4 xh = (v[i] - mean) * rstd;
      if (colscale) {
        const f32x4 tm = *reinterpret_cast<const f32x4*>(colscale + 4 * c), bb = *reinterpret_cast<const f32x4*>(bias + 4 * c);
        const f32x4 gn = has_next ? *reinterpret_cast<const f32x4*>(dy + (m + 1) * dys + 4 * c) : zero;
        at[i] = at[i] + (xh * gw + bb) * (g - gn);
        g = g * tm + gn * (1.0f - tm);
      }
      aw[i] = aw[i] + g * xh;
      ab[i] = ab[i] + g;
      g = g * gw;
      s1 += (g.x + g.y) + (g.z + g.w);
      s2 += (g.x * xh.x + g.y * xh.y) + (g.z * xh.z + g.w * xh.w);
      v[i] = g;      // (the row's registers now hold g w; xhat is rebuilt below from x, which L1 still has)
    }
    const float c1 = block_sum<4>(s1, s_red) / (float)D;
    const float c2 = block_sum<4>(s2, s_red) / (float)D;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = t + 256 * i;
      if (c >= nv) continue;
      const f32x4 xh = (*reinterpret_cast<const f32x4*>(x + m * D + 4 * c) - mean) * rstd;
      f32x4 d = (v[i] - c1 - xh * c2) * rstd;
      const int64_t o = m * D + 4 * c;
      if (dres) d = d + *reinterpret_cast<const f32x4*>(dres + o);
      *reinterpret_cast<f32x4*>(dx + o) = d;
      if (dx16) {
        const u32x2 pk = {pack2<OT>(d.x, d.y), pack2<OT>(d.z, d.w)};
        *reinterpret_cast<u32x2*>(dx16 + o) = pk;
      }
    }
  }
  float* p = part + (int64_t)blockIdx.x * 3 * D;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = t + 256 * i;
    if (c >= nv) continue;
    *reinterpret_cast<f32x4*>(p + 4 * c) = aw[i];
    *reinterpret_cast<f32x4*>(p + D + 4 * c) = ab[i];
    *reinterpret_cast<f32x4*>(p + 2 * D + 4 * c) = at[i];
  }
}

template <typename OT>
__global__ __launch_bounds__(256) void gpt_ln_timeshift_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, const float* __restrict__ colscale,
                                                                   const float* __restrict__ dres, int64_t M, int S, int D, float eps,
                                                                   float* __restrict__ dx, uint16_t* __restrict__ dx16, float* __restrict__ part) {
  __shared__ float s_red[4];
  gpt_ln_bwd_rows<OT>(dy, (int64_t)D, x, w, bias, colscale, dres, M, S, D, eps, dx, dx16, part, s_red);
}

// The backward of rq_prefill.hip's rq_ln_strided_kernel (ln_spatial, whose output is slot 0 of every depth sequence): the same body over a strided dy
// with the colscale / dres arguments passed as null pointers at run time, so the arithmetic is the instruction sequence of the kernel above.
template <typename OT>
__global__ __launch_bounds__(256) void rq_ln_strided_bwd_kernel(const float* __restrict__ dy, int64_t dys, const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, const float* __restrict__ colscale,
                                                                const float* __restrict__ dres, int64_t M, int D, float eps, float* __restrict__ dx,
                                                                uint16_t* __restrict__ dx16, float* __restrict__ part) {
  __shared__ float s_red[4];
  gpt_ln_bwd_rows<OT>(dy, dys, x, w, bias, colscale, dres, M, 1, D, eps, dx, dx16, part, s_red);
}

// out_k[c] (+)= sum over blocks of part[block][k][c], ascending; blockIdx.y = k (0 dw, 1 db, 2 d colscale)
__global__ __launch_bounds__(256) void gpt_ln_bwd_reduce_kernel(const float* __restrict__ part, int nblk, int D, float* __restrict__ dw, float* __restrict__ db,
                                                                float* __restrict__ dcs, int accumulate) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  float* out = k == 0 ? dw : (k == 1 ? db : dcs);
  if (c >= D || !out) return;
  const float* p = part + (int64_t)k * D + c;
  float s = 0.f;
#pragma unroll 8
  for (int j = 0; j < nblk; ++j) s += p[(int64_t)j * 3 * D];
  out[c] = accumulate ? out[c] + s : s;
}

extern "C" size_t enh_ln_timeshift_backward_workspace_bytes(int64_t M, int D) {
  return M > 0 && D > 0 ? (size_t)((M + GR_LNB_ROWS - 1) / GR_LNB_ROWS) * 3 * D * sizeof(float) : 0;
}

extern "C" int enh_ln_timeshift_backward(const float* dy, const float* x, const float* w, const float* b, const float* colscale, const float* dres, int64_t M,
                                         int S, int D, float eps, float* dx, enh_h16* dx16, float* dw, float* db, float* dcolscale, int accumulate, void* ws,
                                         size_t ws_bytes, int dtype, void* stream) {
  ENH_REQUIRE(dy && x && w && dx && dw && db && (!colscale || (b && dcolscale)), ENH_E_BADARG, "enh_ln_timeshift_backward: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_ln_timeshift_backward");
  ENH_REQUIRE(M >= 1 && M <= 2147483647LL && S >= 1 && M % S == 0, ENH_E_SHAPE, "enh_ln_timeshift_backward: M=%lld rows must be whole sequences of S=%d", (long long)M, S);
  ENH_REQUIRE(D >= 8 && D <= GR_LN_MAX_D && D % 8 == 0, ENH_E_SHAPE, "enh_ln_timeshift_backward: D must be a multiple of 8 in [8, %d], got %d", GR_LN_MAX_D, D);
  ENH_REQUIRE(ws && ws_bytes >= enh_ln_timeshift_backward_workspace_bytes(M, D), ENH_E_WORKSPACE, "enh_ln_timeshift_backward: workspace too small (%zu bytes)", ws_bytes);
  const int nblk = (int)((M + GR_LNB_ROWS - 1) / GR_LNB_ROWS);
  hipStream_t s = (hipStream_t)stream;
  enh_note_kernel("gpt_ln_timeshift_bwd_kernel", dtype);
  ENH_DT_DISPATCH(dtype, (gpt_ln_timeshift_bwd_kernel<OT><<<(unsigned)nblk, 256, 0, s>>>(dy, x, w, b, colscale, dres, M, S, D, eps, dx, dx16, (float*)ws)));
  gpt_ln_bwd_reduce_kernel<<<dim3((unsigned)((D + 255) / 256), colscale ? 3 : 2), 256, 0, s>>>((const float*)ws, nblk, D, dw, db, colscale ? dcolscale : nullptr, accumulate);
  return enh_check_launch("enh_ln_timeshift_backward");
}

extern "C" int enh_ln_rows_strided_backward(const float* dy, int64_t dy_stride, const float* x, const float* w, int64_t M, int D, float eps, float* dx,
                                            enh_h16* dx16, float* dw, float* db, int accumulate, void* ws, size_t ws_bytes, int dtype, void* stream) {
  ENH_REQUIRE(dy && x && w && dx && dw && db, ENH_E_BADARG, "enh_ln_rows_strided_backward: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_ln_rows_strided_backward");
  ENH_REQUIRE(M >= 1 && M <= 2147483647LL, ENH_E_SHAPE, "enh_ln_rows_strided_backward: M=%lld", (long long)M);
  ENH_REQUIRE(D >= 8 && D <= GR_LN_MAX_D && D % 8 == 0, ENH_E_SHAPE, "enh_ln_rows_strided_backward: D must be a multiple of 8 in [8, %d], got %d", GR_LN_MAX_D, D);
  ENH_REQUIRE(dy_stride >= D && dy_stride % 4 == 0, ENH_E_SHAPE, "enh_ln_rows_strided_backward: the row stride of dy must be a multiple of 4 that is at least D=%d, got %lld",
              D, (long long)dy_stride);
  ENH_REQUIRE(ws && ws_bytes >= enh_ln_timeshift_backward_workspace_bytes(M, D), ENH_E_WORKSPACE, "enh_ln_rows_strided_backward: workspace too small (%zu bytes)", ws_bytes);
  const int nblk = (int)((M + GR_LNB_ROWS - 1) / GR_LNB_ROWS);
  hipStream_t s = (hipStream_t)stream;
  const float* none = nullptr;
  enh_note_kernel("rq_ln_strided_bwd_kernel", dtype);
  ENH_DT_DISPATCH(dtype, (rq_ln_strided_bwd_kernel<OT><<<(unsigned)nblk, 256, 0, s>>>(dy, dy_stride, x, w, none, none, none, M, D, eps, dx, dx16, (float*)ws)));
  gpt_ln_bwd_reduce_kernel<<<dim3((unsigned)((D + 255) / 256), 2), 256, 0, s>>>((const float*)ws, nblk, D, dw, db, nullptr, accumulate);
  return enh_check_launch("enh_ln_rows_strided_backward");
}

// ---------------------------------------------------------------------------------------------
// embedding backward
// ---------------------------------------------------------------------------------------------
// One workgroup per table row, all of its columns (a thread holds C / 1024 <= 8 float4 sums: the id list is scanned once per row, not once per
// column block).  blockIdx.x walks the rows of tok_code [V], tok_cond [Vc], pos_code [P] and pos_cond [1].
// A token row scans the fed ids (codes 0 .. S - 2 of every sequence: the last code is never fed; conds), 256 per round: the four waves publish
// their match ballots, then every thread adds the matching rows of g in ascending (b, s) order.  No sort, no atomics; a row without a match is
// written as zeros (or left, under accumulate).  pos_code[p] = sum_b g[b, p + 1] for p < S - 1 and zero beyond; pos_cond = sum_b g[b, 0].
#define GR_EMB_MAX_C 8192
__global__ __launch_bounds__(256) void gpt_embed_seq_bwd_kernel(const float* __restrict__ g, const int64_t* __restrict__ conds, const int64_t* __restrict__ codes,
                                                                int64_t code_stride, int B, int S, int C, int Vc, int V, int P, float* __restrict__ dtok_cond,
                                                                float* __restrict__ dpos_cond, float* __restrict__ dtok_code, float* __restrict__ dpos_code,
                                                                int accumulate) {
  __shared__ unsigned long long s_mask[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nv = C >> 2;
  int row = blockIdx.x;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = zero;
  float* out;
  if (row < V + Vc) {
    const bool is_code = row < V;
    const int id = is_code ? row : row - V;
    const int per = is_code ? S - 1 : 1;      // fed ids per sequence
    const int64_t n_ids = (int64_t)B * per;
    out = (is_code ? dtok_code : dtok_cond) + (int64_t)id * C;
    for (int64_t base = 0; base < n_ids; base += 256) {
      const int64_t i = base + t;
      bool match = false;
      if (i < n_ids) {
        const int64_t bb = i / per, p = i - bb * per;
        match = (is_code ? codes[bb * code_stride + p] : conds[bb]) == id;
      }
      const unsigned long long mk = __ballot(match);
      if (lane == 0) s_mask[wave] = mk;
      __syncthreads();
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        unsigned long long m = s_mask[ww];
        while (m) {
          const int j = __builtin_ctzll(m);
          m &= m - 1;
          const int64_t i2 = base + ww * 64 + j;
          const int64_t bb = i2 / per, p = i2 - bb * per;
          const float* gr = g + (bb * S + (is_code ? p + 1 : 0)) * C;
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (t + 256 * k < nv) acc[k] = acc[k] + *reinterpret_cast<const f32x4*>(gr + 4 * (t + 256 * k));
        }
      }
      __syncthreads();
    }
  } else {
    row -= V + Vc;
    const bool is_code = row < P;
    out = is_code ? dpos_code + (int64_t)row * C : dpos_cond;
    const int s = is_code ? row + 1 : 0;
    if (s < S)
      for (int bb = 0; bb < B; ++bb) {
        const float* gr = g + ((int64_t)bb * S + s) * C;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (t + 256 * k < nv) acc[k] = acc[k] + *reinterpret_cast<const f32x4*>(gr + 4 * (t + 256 * k));
      }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = 4 * (t + 256 * k);
    if (c >= C) continue;
    f32x4 r = acc[k];
    if (accumulate) r = r + *reinterpret_cast<const f32x4*>(out + c);
    *reinterpret_cast<f32x4*>(out + c) = r;
  }
}

extern "C" int enh_gpt_embed_seq_backward(const float* g, const int64_t* conds, const int64_t* codes, int64_t code_stride, int B, int S, int C, int Vc, int V,
                                          int P, float* dtok_cond, float* dpos_cond, float* dtok_code, float* dpos_code, int accumulate, void* stream) {
  ENH_REQUIRE(g && conds && dtok_cond && dpos_cond && dtok_code && dpos_code && (S == 1 || codes), ENH_E_BADARG, "enh_gpt_embed_seq_backward: null pointer");
  ENH_REQUIRE(B >= 1 && S >= 1 && Vc >= 1 && V >= 1 && P >= S - 1 && code_stride >= S - 1 && (int64_t)B * S <= 2147483647LL &&
                  (int64_t)V + Vc + P + 1 <= 2147483647LL, ENH_E_BADARG,
              "enh_gpt_embed_seq_backward: B=%d S=%d Vc=%d V=%d P=%d code_stride=%lld", B, S, Vc, V, P, (long long)code_stride);
  ENH_REQUIRE(C >= 4 && C % 4 == 0 && C <= GR_EMB_MAX_C, ENH_E_SHAPE, "enh_gpt_embed_seq_backward: C must be a multiple of 4 in [4, %d], got %d", GR_EMB_MAX_C, C);
  enh_note_kernel_plain("gpt_embed_seq_bwd_kernel");
  gpt_embed_seq_bwd_kernel<<<(unsigned)(V + Vc + P + 1), 256, 0, (hipStream_t)stream>>>(
      g, conds, codes, code_stride, B, S, C, Vc, V, P, dtok_cond, dpos_cond, dtok_code, dpos_code, accumulate);
  return enh_check_launch("enh_gpt_embed_seq_backward");
}
