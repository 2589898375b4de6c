// gumbel.hip — fused Gumbel-softmax quantizer for gfx950: one level of GumbelQuantizer.quantize (reference
// enhancing/modules/stage1/quantizers.py:103-126) and its backward WITHOUT any [M,K] buffer.
//
//   zn = n(z), en = n(E)                      l_k = (2 zn.en_k - |zn|^2) - |en_k|^2
//   y  = softmax((l + g) / tau)               z_q = y @ en   (hard: en[idx])
//   p  = softmax(l)                           loss_tok = sum_k p_k (log p_k + log K)
//   idx = argmax_k (l_k + g_k), lowest index on ties
//
// This is flash attention with Q = zn, K = V = en and two softmaxes over the same scores.  The skeleton is vq.hip's vq_nn_kernel: one wave = 32 tokens
// held as the B operand of v_mfma_f32_32x32x2_f32 (exact f32: idx must be the reference's fp32 argmax), a 256-thread workgroup streams the
// pre-normalised codebook through LDS in 128-code tiles, and each D[32 codes x 32 tokens] tile leaves a lane with 16 codes of ONE token, so both
// online softmaxes are lane-local (the two half-waves of a token share their running maxima: one exchange per 32 codes).  The probabilities
// are then already the B operand of z_q^T += en^T y^T (k-pair of MFMA step j = the codes of accumulator register j in the two half-waves).
//
// The noise g is a pure function of (seed, call, token, code) — gb_noise4 below, Philox4x32-10 — so the backward regenerates it; the forward
// saves five floats per token (max and sum of both softmaxes, loss_tok).  The backward is two kernels in the shape of the attention backward:
// a token-owner kernel (dz; tokens in registers, codes through LDS) and a code-owner kernel (dE; 32 codes per wave in registers, tokens through
// LDS in slabs) whose slab partials are added in a fixed order: no float atomics, the same bits on every run.
//
// Widths: d % 8 == 0, 8 <= d <= 32, on the width-32 form with zero padding (loads and stores masked to d columns), as vq.hip.
// Compiled with -ffp-contract=off: the three kernels must recompute bit-identical scores.
#include "common.h"

#define GB_D 32
#define GB_TILE 128
#define GB_PITCH 36   // floats per staged row (144 B: 16-B aligned, off the 128-B bank period)
#define GB_NSTAT 5    // per-token statistics, [GB_NSTAT][M]: m1, s1 (softmax of l), m2, s2 (softmax of (l+g)/tau), loss_tok
#define GB_NEG (-1.0e30f)   // running maximum before the first code (finite: (m_old - m_new) * 0 must be 0)

// ---------------------------------------------------------------------------------------------
// noise.  g(seed, call, m, k) = -log(-log(u)),  u = (x >> 9) * 2^-23 + 2^-24  in [2^-24, 1 - 2^-24]  (23 bits: exact in f32, open at both ends),
// x = word (k & 3) of Philox4x32-10 with key = (seed low, seed high) and counter = (k >> 2, m low, m high, call).
// One call yields the four codes 4*(k>>2) .. 4*(k>>2)+3 of token m.  Nothing else enters: not M, K, the grid or the caller.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float gb_gumbel(uint32_t x) {
  const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f;
  const float e = fmaxf(-0.69314718056f * __builtin_amdgcn_logf(u), 5.0e-8f);   // -ln u >= -ln(1 - 2^-24) = 5.96e-8
  return -0.69314718056f * __builtin_amdgcn_logf(e);
}
__device__ __forceinline__ void gb_noise4(uint64_t seed, uint32_t call, uint64_t m, uint32_t k4, float (&g)[4]) {
  const u32x4 x = philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), u32x4{k4, (uint32_t)m, (uint32_t)(m >> 32), call});
  g[0] = gb_gumbel(x.x); g[1] = gb_gumbel(x.y); g[2] = gb_gumbel(x.z); g[3] = gb_gumbel(x.w);
}

__global__ void gumbel_noise_kernel(uint64_t seed, uint32_t call, int64_t M, int K, float* __restrict__ out) {
  const int k4n = (K + 3) / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * k4n) return;
  const int64_t m = i / k4n;
  const int k4 = (int)(i - m * k4n);
  float g[4];
  gb_noise4(seed, call, (uint64_t)m, (uint32_t)k4, g);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (k4 * 4 + q < K) out[m * K + k4 * 4 + q] = g[q];
}

// ---------------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float gb_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504089f); }
__device__ __forceinline__ float gb_chain16_sq(const float* x) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) s = fmaf(x[j], x[j], s);
  return s;
}
// 16 consecutive floats of a row of width d starting at column `off`, columns >= d read as zero (d % 8 == 0)
__device__ __forceinline__ void gb_load16(float (&x)[16], const float* __restrict__ row, int off, int d) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = off + 4 * q < d ? *reinterpret_cast<const float4*>(row + off + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    x[q * 4 + 0] = v.x; x[q * 4 + 1] = v.y; x[q * 4 + 2] = v.z; x[q * 4 + 3] = v.w;
  }
}
// The 16 values a lane holds of an MFMA D tile are rows (r & 3) + 8 (r >> 2) + 4 hi: four runs of four consecutive rows.  When the rows are the
// columns of a [*, d] matrix (z_q^T, dz^T) run g is the float4 at column 8 g + 4 hi.
__device__ __forceinline__ void gb_loadD(float (&x)[16], const float* __restrict__ row, int hi, int d) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 v = 8 * g < d ? *reinterpret_cast<const float4*>(row + 8 * g + 4 * hi) : make_float4(0.f, 0.f, 0.f, 0.f);
    x[g * 4 + 0] = v.x; x[g * 4 + 1] = v.y; x[g * 4 + 2] = v.z; x[g * 4 + 3] = v.w;
  }
}
__device__ __forceinline__ void gb_storeD(float* __restrict__ row, const float (&x)[16], int hi, int d) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    if (8 * g < d) *reinterpret_cast<float4*>(row + 8 * g + 4 * hi) = make_float4(x[g * 4], x[g * 4 + 1], x[g * 4 + 2], x[g * 4 + 3]);
}

// codebook preparation (quantizers.py:104-105): en = n(E) at the padded width 32 (rows >= K zero), ee = |en|^2, enrm = max(|E|, 1e-12)
__global__ void gumbel_prep_kernel(const float* __restrict__ E, float* __restrict__ en, float* __restrict__ ee, float* __restrict__ enrm,
                                   int K, int Kpad, int d, int use_norm) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Kpad) return;
  float x[2][16];
  float den = 1.f, s2 = 0.f;
  if (k < K) {
    gb_load16(x[0], E + (size_t)k * d, 0, d);
    gb_load16(x[1], E + (size_t)k * d, 16, d);
    if (use_norm) {
      den = fmaxf(sqrtf(gb_chain16_sq(x[0]) + gb_chain16_sq(x[1])), 1e-12f);
#pragma unroll
      for (int j = 0; j < 16; ++j) { x[0][j] = x[0][j] / den; x[1][j] = x[1][j] / den; }
    }
    s2 = gb_chain16_sq(x[0]) + gb_chain16_sq(x[1]);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) x[0][j] = x[1][j] = 0.f;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(en + (size_t)k * GB_D + h * 16 + q * 4) = make_float4(x[h][q * 4], x[h][q * 4 + 1], x[h][q * 4 + 2], x[h][q * 4 + 3]);
  ee[k] = s2;
  enrm[k] = den;
}

// tile staging: 128 rows x 32 floats (16 KB), 4 x 16 B per thread, fully coalesced; rows >= nrows read as zero
__device__ __forceinline__ void gb_tile_gload(f32x4 (&pre)[4], const float* __restrict__ src, int64_t row0, int64_t nrows, int d, int t) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = t + 256 * i;
    const int64_t row = row0 + (id >> 3);
    const int c = (id & 7) * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    pre[i] = (row < nrows && c < d) ? *reinterpret_cast<const f32x4*>(src + (size_t)row * d + c) : zero;
  }
}
__device__ __forceinline__ void gb_tile_sstore(const f32x4 (&pre)[4], float* tile, int t) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = t + 256 * i;
    *reinterpret_cast<f32x4*>(&tile[(id >> 3) * GB_PITCH + (id & 7) * 4]) = pre[i];
  }
}
// A operand of the 16 score MFMAs of one 32-row sub-tile: row (sub*32 + col), columns hi*16 .. hi*16+15
__device__ __forceinline__ void gb_read_a(float (&a)[16], const float* tile, int sub, int col, int hi) {
  const float4* ap = reinterpret_cast<const float4*>(&tile[(sub * 32 + col) * GB_PITCH + hi * 16]);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float4 v = ap[c];
    a[c * 4 + 0] = v.x; a[c * 4 + 1] = v.y; a[c * 4 + 2] = v.z; a[c * 4 + 3] = v.w;
  }
}
// acc += X^T P: MFMA step j contracts the two rows (j & 3) + 8 (j >> 2) + 4 hi of the sub-tile (the rows of accumulator register j in the two
// half-waves) — A[i = col][k = hi] = tile[row][col], B or A = the register itself.
#define GB_ROW(sub, j, hi) ((sub) * 32 + ((j) & 3) + 8 * ((j) >> 2) + 4 * (hi))

// normalise this lane's 16 columns of a token row (two half-waves per token)
__device__ __forceinline__ float gb_normalise(float (&zn)[16], const float (&z0)[16], int use_norm) {
  float den = 1.f;
  if (use_norm) {
    const float sp = gb_chain16_sq(z0);
    den = fmaxf(sqrtf(sp + __shfl_xor(sp, 32, 64)), 1e-12f);
#pragma unroll
    for (int j = 0; j < 16; ++j) zn[j] = z0[j] / den;
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) zn[j] = z0[j];
  }
  return den;
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gumbel_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ en, const float* __restrict__ ee, int64_t M, int d, int K, int Kpad, int use_norm,
    float inv_tau, float logK, int hard, uint64_t seed, uint32_t call, float* __restrict__ zq_out, float* __restrict__ zq_soft,
    int64_t* __restrict__ idx_out, float* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) float s_tile[2][GB_TILE * GB_PITCH];
  __shared__ __attribute__((aligned(16))) float s_ee[2][GB_TILE];

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int col = lane & 31, hi = lane >> 5;
  const int64_t tok = ((int64_t)blockIdx.x * 4 + wave) * 32 + col;
  const bool live = tok < M;
  const int ntiles = Kpad / GB_TILE;

  float z0[16], zn[16];
  gb_load16(z0, z + (size_t)(live ? tok : 0) * d, hi * 16, live ? d : 0);
  gb_normalise(zn, z0, use_norm);
  const float zzp = gb_chain16_sq(zn);
  const float zz = zzp + __shfl_xor(zzp, 32, 64);

  float m1 = GB_NEG, s1 = 0.f, t1 = 0.f, m2 = GB_NEG, s2 = 0.f;
  float best_v = -__builtin_inff();
  int best_i = 0;
  f32x16 zq;
#pragma unroll
  for (int q = 0; q < 16; ++q) zq[q] = 0.f;

  f32x4 pre[4];
  float pre_ee = 0.f;
  gb_tile_gload(pre, en, 0, Kpad, GB_D, t);
  if (t < GB_TILE) pre_ee = ee[t];
  gb_tile_sstore(pre, s_tile[0], t);
  if (t < GB_TILE) s_ee[0][t] = pre_ee;
  __syncthreads();
  for (int kt = 0; kt < ntiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < ntiles) {
      gb_tile_gload(pre, en, (int64_t)(kt + 1) * GB_TILE, Kpad, GB_D, t);
      if (t < GB_TILE) pre_ee = ee[(size_t)(kt + 1) * GB_TILE + t];
    }
#pragma unroll 1
    for (int sub = 0; sub < 4; ++sub) {
      if (kt * GB_TILE + sub * 32 >= K) break;   // codes >= K of the padded codebook contribute nothing
      float a[16];
      gb_read_a(a, s_tile[buf], sub, col, hi);
      f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], zn[kk], acc, 0, 0, 0);
      // D row (code) of acc[j]: (j&3) + 8*(j>>2) + 4*hi ; column = this lane's token
      float l[16], a2[16];
      float mx1 = -__builtin_inff(), mx2 = -__builtin_inff();
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int row0 = sub * 32 + 8 * g4 + 4 * hi;
        const int code0 = kt * GB_TILE + row0;
        float gn[4];
        gb_noise4(seed, call, (uint64_t)tok, (uint32_t)(code0 >> 2), gn);
        const float4 e4 = *reinterpret_cast<const float4*>(&s_ee[buf][row0]);
        const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = g4 * 4 + q;
          const bool ok = code0 + q < K;
          const float lv = (2.0f * acc[j] - zz) - ev[q];
          const float sv = lv + gn[q];
          if (ok && sv > best_v) { best_v = sv; best_i = code0 + q; }
          l[j] = ok ? lv : -__builtin_inff();
          a2[j] = ok ? sv * inv_tau : -__builtin_inff();
          mx1 = fmaxf(mx1, l[j]);
          mx2 = fmaxf(mx2, a2[j]);
        }
      }
      mx1 = fmaxf(mx1, __shfl_xor(mx1, 32, 64));
      mx2 = fmaxf(mx2, __shfl_xor(mx2, 32, 64));
      const float n1 = fmaxf(m1, mx1), n2 = fmaxf(m2, mx2);
      const float c1 = gb_exp(m1 - n1), c2 = gb_exp(m2 - n2);
      t1 = c1 * (t1 + (m1 - n1) * s1);   // sum e^(l-m) (l-m) under the new maximum
      s1 = c1 * s1;
      s2 = c2 * s2;
      m1 = n1;
      m2 = n2;
      float p[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float x = l[j] - n1;
        const float e = gb_exp(x);
        s1 = s1 + e;
        t1 = t1 + (l[j] > -__builtin_inff() ? e * x : 0.f);
        p[j] = gb_exp(a2[j] - n2);
        s2 = s2 + p[j];
        zq[j] = zq[j] * c2;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j)
        zq = __builtin_amdgcn_mfma_f32_32x32x2f32(s_tile[buf][GB_ROW(sub, j, hi) * GB_PITCH + col], p[j], zq, 0, 0, 0);
    }
    if (kt + 1 < ntiles) {
      gb_tile_sstore(pre, s_tile[buf ^ 1], t);
      if (t < GB_TILE) s_ee[buf ^ 1][t] = pre_ee;
    }
    __syncthreads();
  }
  // ---- merge the two half-waves (same token, same maxima) ----
  s1 = s1 + __shfl_xor(s1, 32, 64);
  t1 = t1 + __shfl_xor(t1, 32, 64);
  s2 = s2 + __shfl_xor(s2, 32, 64);
  {
    const float ov = __shfl_xor(best_v, 32, 64);
    const int oi = __shfl_xor(best_i, 32, 64);
    if (ov > best_v || (ov == best_v && oi < best_i)) { best_v = ov; best_i = oi; }
  }
  if (!live) return;
  const float loss_tok = (t1 / s1 - logf(s1)) + logK;
  if (hi == 0) {
    idx_out[tok] = (int64_t)best_i;
    stats[0 * M + tok] = m1;
    stats[1 * M + tok] = s1;
    stats[2 * M + tok] = m2;
    stats[3 * M + tok] = s2;
    stats[4 * M + tok] = loss_tok;
  }
  float o[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) o[j] = zq[j] / s2;
  if (hard) {
    if (zq_soft) gb_storeD(zq_soft + (size_t)tok * d, o, hi, d);
    gb_loadD(o, en + (size_t)best_i * GB_D, hi, GB_D);
  }
  gb_storeD(zq_out + (size_t)tok * d, o, hi, d);
}

// loss = mean over the M tokens of loss_tok (quantizers.py:121-122), fixed order
__global__ void gumbel_loss_kernel(const float* __restrict__ loss_tok, int64_t M, float* __restrict__ loss_out) {
  __shared__ double s_acc[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < M; i += 256) a += (double)loss_tok[i];
  s_acc[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_acc[threadIdx.x] += s_acc[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_out[0] = (float)(s_acc[0] / (double)M);
}

// ---------------------------------------------------------------------------------------------
// backward.  dl_mk = y (dy - delta) / tau + gL p (log p + log K - loss_tok),  dy = g_zq.en_k,  delta = g_zq.z_q(soft),  gL = g_loss / M
// ---------------------------------------------------------------------------------------------
struct GbTok { float m1, is1, ls1, m2, is2, lt, delta, zz; };
__device__ __forceinline__ void gb_dl(float acc, float dy, float ee_k, float gn, const GbTok& s, float inv_tau, float logK, float gL, bool ok,
                                      float& dl, float& y) {
  const float lv = (2.0f * acc - s.zz) - ee_k;
  const float x = lv - s.m1;
  const float p = gb_exp(x) * s.is1;
  y = gb_exp((lv + gn) * inv_tau - s.m2) * s.is2;
  dl = y * (dy - s.delta) * inv_tau + gL * (p * (((x - s.ls1) + logK) - s.lt));
  if (!ok) { dl = 0.f; y = 0.f; }
}

// token owner: dz.  Also leaves zn (padded width 32), |zn|^2 and delta of every token in the workspace for the code owner.
__global__ __launch_bounds__(256) void gumbel_bwd_dz_kernel(
    const float* __restrict__ z, const float* __restrict__ en, const float* __restrict__ ee, const float* __restrict__ g_zq,
    const float* __restrict__ zq_soft, const float* __restrict__ stats, float g_loss, const float* __restrict__ g_loss_dev, int64_t M, int d,
    int K, int Kpad, int use_norm, float inv_tau, float logK, uint64_t seed, uint32_t call, float* __restrict__ dz, float* __restrict__ zn_ws,
    float* __restrict__ zz_ws, float* __restrict__ delta_ws) {
  __shared__ __attribute__((aligned(16))) float s_tile[2][GB_TILE * GB_PITCH];
  __shared__ __attribute__((aligned(16))) float s_ee[2][GB_TILE];

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int col = lane & 31, hi = lane >> 5;
  const int64_t tok = ((int64_t)blockIdx.x * 4 + wave) * 32 + col;
  const bool live = tok < M;
  const int64_t tk = live ? tok : 0;
  const int ntiles = Kpad / GB_TILE;
  const float gL = g_loss * (g_loss_dev ? g_loss_dev[0] : 1.f) / (float)M;

  float z0[16], zn[16], gq[16];
  gb_load16(z0, z + (size_t)tk * d, hi * 16, live ? d : 0);
  const float den = gb_normalise(zn, z0, use_norm);
  const float zzp = gb_chain16_sq(zn);
  GbTok s;
  s.zz = zzp + __shfl_xor(zzp, 32, 64);
  gb_load16(gq, g_zq + (size_t)tk * d, hi * 16, live ? d : 0);
  {
    float zs[16], dp = 0.f;
    gb_load16(zs, zq_soft + (size_t)tk * d, hi * 16, live ? d : 0);
#pragma unroll
    for (int j = 0; j < 16; ++j) dp = fmaf(gq[j], zs[j], dp);
    s.delta = dp + __shfl_xor(dp, 32, 64);
  }
  s.m1 = stats[0 * M + tk];
  const float s1 = stats[1 * M + tk];
  s.m2 = stats[2 * M + tk];
  s.is1 = 1.0f / s1;
  s.ls1 = logf(s1);
  s.is2 = 1.0f / stats[3 * M + tk];
  s.lt = stats[4 * M + tk];
  if (live) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(zn_ws + (size_t)tok * GB_D + hi * 16 + q * 4) = make_float4(zn[q * 4], zn[q * 4 + 1], zn[q * 4 + 2], zn[q * 4 + 3]);
    if (hi == 0) { zz_ws[tok] = s.zz; delta_ws[tok] = s.delta; }
  }

  f32x16 dzn;
#pragma unroll
  for (int q = 0; q < 16; ++q) dzn[q] = 0.f;

  f32x4 pre[4];
  float pre_ee = 0.f;
  gb_tile_gload(pre, en, 0, Kpad, GB_D, t);
  if (t < GB_TILE) pre_ee = ee[t];
  gb_tile_sstore(pre, s_tile[0], t);
  if (t < GB_TILE) s_ee[0][t] = pre_ee;
  __syncthreads();
  for (int kt = 0; kt < ntiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < ntiles) {
      gb_tile_gload(pre, en, (int64_t)(kt + 1) * GB_TILE, Kpad, GB_D, t);
      if (t < GB_TILE) pre_ee = ee[(size_t)(kt + 1) * GB_TILE + t];
    }
#pragma unroll 1
    for (int sub = 0; sub < 4; ++sub) {
      if (kt * GB_TILE + sub * 32 >= K) break;
      float a[16];
      gb_read_a(a, s_tile[buf], sub, col, hi);
      f32x16 acc, accd;
#pragma unroll
      for (int q = 0; q < 16; ++q) { acc[q] = 0.f; accd[q] = 0.f; }
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], zn[kk], acc, 0, 0, 0);
        accd = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], gq[kk], accd, 0, 0, 0);
      }
      float dl[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int row0 = sub * 32 + 8 * g4 + 4 * hi;
        const int code0 = kt * GB_TILE + row0;
        float gn[4];
        gb_noise4(seed, call, (uint64_t)tok, (uint32_t)(code0 >> 2), gn);
        const float4 e4 = *reinterpret_cast<const float4*>(&s_ee[buf][row0]);
        const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = g4 * 4 + q;
          float y;
          gb_dl(acc[j], accd[j], ev[q], gn[q], s, inv_tau, logK, gL, code0 + q < K, dl[j], y);
        }
      }
#pragma unroll
      for (int j = 0; j < 16; ++j)
        dzn = __builtin_amdgcn_mfma_f32_32x32x2f32(s_tile[buf][GB_ROW(sub, j, hi) * GB_PITCH + col], dl[j], dzn, 0, 0, 0);
    }
    if (kt + 1 < ntiles) {
      gb_tile_sstore(pre, s_tile[buf ^ 1], t);
      if (t < GB_TILE) s_ee[buf ^ 1][t] = pre_ee;
    }
    __syncthreads();
  }
  // dzn = 2 sum_k dl_k en_k (sum_k dl_k = 0: the |zn|^2 term gives nothing), then the normalise Jacobian (quantizers.py:104)
  float o[16], znD[16];
  gb_loadD(znD, z + (size_t)tk * d, hi, live ? d : 0);
  float dp = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    o[j] = 2.0f * dzn[j];
    if (use_norm) znD[j] = znD[j] / den;
    dp = fmaf(znD[j], o[j], dp);
  }
  const float dot = dp + __shfl_xor(dp, 32, 64);
  if (use_norm) {
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j] = (o[j] - znD[j] * dot) / den;
  }
  if (live) gb_storeD(dz + (size_t)tok * d, o, hi, d);
}

// code owner: one wave = 32 codes (B operand of the score products, in registers), the workgroup's 128 codes sweep the tokens of one slab
// through LDS in 128-token tiles.  Scores and dy come out as D[32 tokens x 32 codes]: a lane holds 16 tokens of ONE code, and dl / y are
// already the A operand of  acc1[code][dim] += dl^T zn  and  acc2[code][dim] += y^T g_zq.  The noise of a (4 tokens x 4 codes) patch is four
// Philox calls, one per lane of the quad of codes, exchanged inside the quad.
// part[slab][code][dim] = 2 acc1 + acc2 - 2 en_k sum_m dl_mk     (hard: acc2 += y_hard^T g_zq, y_hard the one-hot of idx)
template <bool HARD>
__global__ __launch_bounds__(256) void gumbel_bwd_de_kernel(
    const float* __restrict__ zn_ws, const float* __restrict__ zz_ws, const float* __restrict__ delta_ws, const float* __restrict__ en,
    const float* __restrict__ ee, const float* __restrict__ g_zq, const float* __restrict__ stats, float g_loss,
    const float* __restrict__ g_loss_dev, const int64_t* __restrict__ idx_hard, int64_t M, int d, int K, int Kpad, int tiles_per_slab, float inv_tau,
    float logK, uint64_t seed, uint32_t call, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_zn[2][GB_TILE * GB_PITCH];
  __shared__ __attribute__((aligned(16))) float s_gq[2][GB_TILE * GB_PITCH];
  __shared__ float s_st[2][8][GB_TILE];
  __shared__ int s_idx[HARD ? 2 : 1][HARD ? GB_TILE : 1];   // hard mode: the token's chosen code (the soft instantiation never touches it)

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int col = lane & 31, hi = lane >> 5;
  const int code = blockIdx.x * GB_TILE + wave * 32 + col;   // < Kpad
  const bool cok = code < K;
  const float gL = g_loss * (g_loss_dev ? g_loss_dev[0] : 1.f) / (float)M;
  const int64_t ntt = (M + GB_TILE - 1) / GB_TILE;
  const int64_t tt0 = (int64_t)blockIdx.y * tiles_per_slab;
  const int64_t tt1 = tt0 + tiles_per_slab < ntt ? tt0 + tiles_per_slab : ntt;

  float e[16];
  gb_load16(e, en + (size_t)code * GB_D, hi * 16, GB_D);
  const float ee_k = ee[code];
  const int cq = col & 3;

  f32x16 acc1, acc2;
#pragma unroll
  for (int q = 0; q < 16; ++q) { acc1[q] = 0.f; acc2[q] = 0.f; }
  float rs = 0.f;

  f32x4 pre_z[4], pre_g[4];
  float pre_s[4] = {0.f, 0.f, 0.f, 0.f};
  int pre_i = -1;
  // per-token statistics of a tile: 8 rows of 128, two threads per token, four values each
  const int st_tok = t & 127, st_half = t >> 7;
  auto gload = [&](int64_t tt) {
    gb_tile_gload(pre_z, zn_ws, tt * GB_TILE, M, GB_D, t);
    gb_tile_gload(pre_g, g_zq, tt * GB_TILE, M, d, t);
    const int64_t m = tt * GB_TILE + st_tok;
    const bool ok = m < M;
    const int64_t mk = ok ? m : 0;
    if (st_half == 0) {
      const float s1 = stats[1 * M + mk];
      pre_s[0] = stats[0 * M + mk];
      pre_s[1] = 1.0f / s1;
      pre_s[2] = logf(s1);
      pre_s[3] = stats[2 * M + mk];
    } else {
      pre_s[0] = 1.0f / stats[3 * M + mk];
      pre_s[1] = stats[4 * M + mk];
      pre_s[2] = delta_ws[mk];
      pre_s[3] = zz_ws[mk];
      if constexpr (HARD) pre_i = ok ? (int)idx_hard[mk] : -1;
    }
  };
  auto sstore = [&](int buf) {
    gb_tile_sstore(pre_z, s_zn[buf], t);
    gb_tile_sstore(pre_g, s_gq[buf], t);
#pragma unroll
    for (int q = 0; q < 4; ++q) s_st[buf][st_half * 4 + q][st_tok] = pre_s[q];
    if constexpr (HARD) { if (st_half == 1) s_idx[buf][st_tok] = pre_i; }
  };
  gload(tt0);
  sstore(0);
  __syncthreads();
  for (int64_t tt = tt0; tt < tt1; ++tt) {
    const int buf = (int)(tt - tt0) & 1;
    if (tt + 1 < tt1) gload(tt + 1);
#pragma unroll 1
    for (int sub = 0; sub < 4; ++sub) {
      const int64_t m0 = tt * GB_TILE + sub * 32;
      if (m0 >= M) break;
      float az[16], ag[16];
      gb_read_a(az, s_zn[buf], sub, col, hi);
      gb_read_a(ag, s_gq[buf], sub, col, hi);
      f32x16 acc, accd;
#pragma unroll
      for (int q = 0; q < 16; ++q) { acc[q] = 0.f; accd[q] = 0.f; }
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(az[kk], e[kk], acc, 0, 0, 0);
        accd = __builtin_amdgcn_mfma_f32_32x32x2f32(ag[kk], e[kk], accd, 0, 0, 0);
      }
      // D row (token) of acc[j]: (j&3) + 8*(j>>2) + 4*hi ; column = this lane's code
      float dl[16], y[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int row0 = sub * 32 + 8 * g4 + 4 * hi;
        // this lane draws the four codes of its quad for token row0 + (col & 3); lane ^ k then holds the draw for token row0 + ((col & 3) ^ k)
        float gn[4], gx[4];
        gb_noise4(seed, call, (uint64_t)(tt * GB_TILE + row0 + cq), (uint32_t)(code >> 2), gn);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int w = cq ^ k;
          const float send = w == 0 ? gn[0] : w == 1 ? gn[1] : w == 2 ? gn[2] : gn[3];
          gx[k] = k == 0 ? send : __shfl_xor(send, k, 64);   // = noise(token row0 + (cq ^ k), this code)
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = g4 * 4 + q;
          const int k = q ^ cq;
          const float g = k == 0 ? gx[0] : k == 1 ? gx[1] : k == 2 ? gx[2] : gx[3];
          const int r = row0 + q;
          GbTok s;
          s.m1 = s_st[buf][0][r]; s.is1 = s_st[buf][1][r]; s.ls1 = s_st[buf][2][r]; s.m2 = s_st[buf][3][r];
          s.is2 = s_st[buf][4][r]; s.lt = s_st[buf][5][r]; s.delta = s_st[buf][6][r]; s.zz = s_st[buf][7][r];
          gb_dl(acc[j], accd[j], ee_k, g, s, inv_tau, logK, gL, cok && tt * GB_TILE + r < M, dl[j], y[j]);
          rs = rs + dl[j];
          // hard: z_q = y_st @ en carries the one-hot VALUE, so en's own gradient takes y_hard^T g_zq (the path through y stays the soft one)
          if constexpr (HARD) y[j] = s_idx[buf][r] == code ? 1.f : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int r = GB_ROW(sub, j, hi);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(dl[j], s_zn[buf][r * GB_PITCH + col], acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(y[j], s_gq[buf][r * GB_PITCH + col], acc2, 0, 0, 0);
      }
    }
    if (tt + 1 < tt1) sstore(buf ^ 1);
    __syncthreads();
  }
  rs = rs + __shfl_xor(rs, 32, 64);   // sum_m dl_mk of code `col` of this wave, on both half-waves
  // acc1 / acc2 register j: code row (j&3) + 8*(j>>2) + 4*hi of this wave, dim = col
  const int cbase = blockIdx.x * GB_TILE + wave * 32;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int r = (j & 3) + 8 * (j >> 2) + 4 * hi;
    const float rsr = __shfl(rs, r, 64);
    const float ev = en[(size_t)(cbase + r) * GB_D + col];
    part[((size_t)blockIdx.y * Kpad + cbase + r) * GB_D + col] = (2.0f * acc1[j] + acc2[j]) - 2.0f * ev * rsr;
  }
}

// dE[k] += J^T(E_k) [ sum over the slabs, ascending ]  — the l2-normalise Jacobian of quantizers.py:105.  32 lanes per code, one column each.
__global__ __launch_bounds__(256) void gumbel_de_finalize_kernel(const float* __restrict__ part, int nslabs, const float* __restrict__ en,
                                                                 const float* __restrict__ enrm, int K, int Kpad, int d, int use_norm,
                                                                 float* __restrict__ dE) {
  const int k = blockIdx.x * 8 + (threadIdx.x >> 5), c = threadIdx.x & 31;
  const int kk = k < K ? k : K - 1;   // whole-wave shuffles below: dead codes compute on a live one and store nothing
  float s = part[(size_t)kk * GB_D + c];
  for (int r = 1; r < nslabs; ++r) s += part[((size_t)r * Kpad + kk) * GB_D + c];
  if (use_norm) {
    const float ev = en[(size_t)kk * GB_D + c];
    float dot = ev * s;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    s = (s - ev * dot) / enrm[kk];
  }
  if (k < K && c < d) dE[(size_t)k * d + c] += s;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
#define GB_MAX_GRID 2147483647LL   // workgroups along x of one launch
static inline int gb_kpad(int K) { return (K + GB_TILE - 1) / GB_TILE * GB_TILE; }
static inline int64_t gb_nblocks(int64_t M) { return (M + GB_TILE - 1) / GB_TILE; }
static inline bool gb_dim_ok(int d) { return d >= 8 && d <= GB_D && d % 8 == 0; }
// token tiles per slab of the code-owner kernel: about 1024 workgroups in all, at most 64 slabs; a function of (M, K) only
static inline int gb_tiles_per_slab(int64_t M, int K) {
  const int64_t ntt = gb_nblocks(M), nct = gb_kpad(K) / GB_TILE;
  int64_t ns = (1024 + nct - 1) / nct;
  if (ns > 64) ns = 64;
  if (ns > ntt) ns = ntt;
  return (int)((ntt + ns - 1) / ns);
}
static inline int gb_nslabs(int64_t M, int K) {
  const int64_t tps = gb_tiles_per_slab(M, K);
  return (int)((gb_nblocks(M) + tps - 1) / tps);
}

struct GbWs { float *en, *ee, *enrm, *zn, *zz, *delta, *part; };
static GbWs gb_carve(void* ws, int64_t M, int K) {
  const size_t kp = (size_t)gb_kpad(K), mp = ((size_t)M + 3) / 4 * 4;
  GbWs w;
  w.en = reinterpret_cast<float*>(ws);
  w.ee = w.en + kp * GB_D;
  w.enrm = w.ee + kp;
  w.zn = w.enrm + kp;
  w.zz = w.zn + mp * GB_D;
  w.delta = w.zz + mp;
  w.part = w.delta + mp;
  return w;
}

extern "C" size_t enh_gumbel_workspace_bytes(int64_t M, int n_embed, int embed_dim) {
  (void)embed_dim;
  if (M < 1 || n_embed < 1) return 0;
  const size_t kp = (size_t)gb_kpad(n_embed), mp = ((size_t)M + 3) / 4 * 4;
  return (kp * GB_D + 2 * kp + mp * GB_D + 2 * mp + (size_t)gb_nslabs(M, n_embed) * kp * GB_D) * sizeof(float) + 256;
}

extern "C" int enh_gumbel_forward(const float* z, const float* codebook, int64_t M, int n_embed, int embed_dim, float tau, int hard,
                                  int use_norm, uint64_t seed, uint32_t call, float* zq_out, float* zq_soft, int64_t* idx_out,
                                  float* loss_out, float* stats_out, void* workspace, size_t workspace_bytes, void* stream) {
  ENH_REQUIRE(z && codebook && zq_out && idx_out && loss_out && stats_out && workspace, ENH_E_BADARG, "enh_gumbel_forward: null pointer");
  ENH_REQUIRE(M > 0 && n_embed > 0 && tau > 0.f, ENH_E_BADARG, "enh_gumbel_forward: M=%lld n_embed=%d tau=%g", (long long)M, n_embed, (double)tau);
  ENH_REQUIRE(gb_dim_ok(embed_dim), ENH_E_SHAPE, "enh_gumbel_forward: embed_dim must be a multiple of 8 in [8, 32], got %d", embed_dim);
  ENH_REQUIRE(gb_nblocks(M) <= GB_MAX_GRID, ENH_E_SHAPE, "enh_gumbel_forward: M=%lld needs more than 2^31-1 workgroups", (long long)M);
  ENH_REQUIRE(workspace_bytes >= enh_gumbel_workspace_bytes(M, n_embed, embed_dim), ENH_E_WORKSPACE, "enh_gumbel_forward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int kp = gb_kpad(n_embed);
  GbWs w = gb_carve(workspace, M, n_embed);
  gumbel_prep_kernel<<<(unsigned)((kp + 255) / 256), 256, 0, s>>>(codebook, w.en, w.ee, w.enrm, n_embed, kp, embed_dim, use_norm);
  gumbel_fwd_kernel<<<(unsigned)gb_nblocks(M), 256, 0, s>>>(z, w.en, w.ee, M, embed_dim, n_embed, kp, use_norm, 1.0f / tau, logf((float)n_embed),
                                                            hard, seed, call, zq_out, zq_soft, idx_out, stats_out);
  gumbel_loss_kernel<<<1, 256, 0, s>>>(stats_out + 4 * M, M, loss_out);
  return enh_check_launch("enh_gumbel_forward");
}

extern "C" int enh_gumbel_backward(const float* z, const float* codebook, const float* zq_soft, const float* stats, const float* g_zq,
                                   float g_loss, const float* g_loss_dev, int64_t M, int n_embed, int embed_dim, float tau, int hard,
                                   const int64_t* idx, int use_norm, uint64_t seed, uint32_t call, float* dz, float* d_codebook,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  ENH_REQUIRE(z && codebook && zq_soft && stats && g_zq && dz && d_codebook && workspace && (idx || !hard), ENH_E_BADARG, "enh_gumbel_backward: null pointer");
  ENH_REQUIRE(M > 0 && n_embed > 0 && tau > 0.f, ENH_E_BADARG, "enh_gumbel_backward: M=%lld n_embed=%d tau=%g", (long long)M, n_embed, (double)tau);
  ENH_REQUIRE(gb_dim_ok(embed_dim), ENH_E_SHAPE, "enh_gumbel_backward: embed_dim must be a multiple of 8 in [8, 32], got %d", embed_dim);
  ENH_REQUIRE(gb_nblocks(M) <= GB_MAX_GRID, ENH_E_SHAPE, "enh_gumbel_backward: M=%lld needs more than 2^31-1 workgroups", (long long)M);
  ENH_REQUIRE(workspace_bytes >= enh_gumbel_workspace_bytes(M, n_embed, embed_dim), ENH_E_WORKSPACE, "enh_gumbel_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int kp = gb_kpad(n_embed), d = embed_dim;
  const float inv_tau = 1.0f / tau, logK = logf((float)n_embed);
  GbWs w = gb_carve(workspace, M, n_embed);
  gumbel_prep_kernel<<<(unsigned)((kp + 255) / 256), 256, 0, s>>>(codebook, w.en, w.ee, w.enrm, n_embed, kp, d, use_norm);
  gumbel_bwd_dz_kernel<<<(unsigned)gb_nblocks(M), 256, 0, s>>>(z, w.en, w.ee, g_zq, zq_soft, stats, g_loss, g_loss_dev, M, d, n_embed, kp, use_norm,
                                                               inv_tau, logK, seed, call, dz, w.zn, w.zz, w.delta);
  const int tps = gb_tiles_per_slab(M, n_embed), ns = gb_nslabs(M, n_embed);
  const dim3 dg((unsigned)(kp / GB_TILE), (unsigned)ns);
  if (hard)
    gumbel_bwd_de_kernel<true><<<dg, 256, 0, s>>>(w.zn, w.zz, w.delta, w.en, w.ee, g_zq, stats, g_loss, g_loss_dev, idx, M,
                                                                                    d, n_embed, kp, tps, inv_tau, logK, seed, call, w.part);
  else
    gumbel_bwd_de_kernel<false><<<dg, 256, 0, s>>>(w.zn, w.zz, w.delta, w.en, w.ee, g_zq, stats, g_loss, g_loss_dev, idx, M,
                                                                                    d, n_embed, kp, tps, inv_tau, logK, seed, call, w.part);
  gumbel_de_finalize_kernel<<<(unsigned)((n_embed + 7) / 8), 256, 0, s>>>(w.part, ns, w.en, w.enrm, n_embed, kp, d, use_norm, d_codebook);
  return enh_check_launch("enh_gumbel_backward");
}

extern "C" int enh_gumbel_noise(uint64_t seed, uint32_t call, int64_t M, int n_embed, float* out, void* stream) {
  ENH_REQUIRE(out, ENH_E_BADARG, "enh_gumbel_noise: null pointer");
  ENH_REQUIRE(M > 0 && n_embed > 0, ENH_E_BADARG, "enh_gumbel_noise: M=%lld n_embed=%d", (long long)M, n_embed);
  const int64_t n = M * ((n_embed + 3) / 4);
  ENH_REQUIRE((n + 255) / 256 <= GB_MAX_GRID, ENH_E_SHAPE, "enh_gumbel_noise: M=%lld x n_embed=%d needs more than 2^31-1 workgroups", (long long)M, n_embed);
  gumbel_noise_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(seed, call, M, n_embed, out);
  return enh_check_launch("enh_gumbel_noise");
}
