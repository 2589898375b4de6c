// gpt_decode.hip — the decode-shaped kernels of stage-2 sampling for gfx950 (reference enhancing/modules/stage2/layers.py: GPT.sample / sample_step
// with cond_num_tokens == 1: every step is ONE token per batch row, so the block sees T == 1, time_shift(x) == 0 and the mix is ln1(x) * time_mix).
//
//   enh_skinny_gemm_h16   y[M,N] = act(x[M,K] W[N,K]^T + bias) (+ res), M <= 64: a weight-streaming kernel.  One workgroup owns 16 rows of W; its four
//                         waves take the 128-wide K chunks of the workgroup's K slice round-robin, every lane loads its W fragment straight into
//                         registers (non-temporal 16-byte loads, W is read exactly once) and the x fragment from L2 (x is at most 64 x K: it stays on
//                         chip), and v_mfma_f32_16x16x32 accumulates D[16 n x 16 m] tiles in f32.  The four waves' accumulators are added in wave order
//                         through LDS.  When N / 16 workgroups cannot fill the chip the K chunks are also split across workgroups (grid.y): slabs in
//                         the caller's workspace, added in ascending slab order by a second pass that also runs the epilogue.  No float atomics.
//   enh_decode_attention  one new token per (batch, head) against a cache [B, H, Tmax, hs]: appends k / v at slot t and returns
//                         softmax(q K[0..t]^T / sqrt(hs)) V[0..t].  Slot t is taken from the step's qkv row, never read back from the cache; slots > t
//                         are never touched.  The cache length is cut into pieces of at most 256 slots (grid.y); partial (max, sum, out) triples are
//                         merged in ascending piece order by a second kernel (the plan and the merge: decode_attn.h, shared with the MXFP8-cache
//                         form of gpt_decode_kv8.hip).
//   enh_sample_logits     temperature, top-k, softmax, top-p and an inverse-CDF draw of one row per workgroup (GPT.sample lines 233-258).
//   enh_skinny_gemm_f32   the exact mode's form of the product: f32 operands, vector ALU, tree-ordered sums.
// The step's LayerNorm and embedding are row kernels and stand beside the teacher-forced forward's: gpt_rows.hip (enh_row_ln_scale, enh_gpt_embed).
// Every result is the same bits on every run: all sums run in a fixed order.
//
// The cursor forms (enh_cursor_advance, enh_decode_attention_at, enh_embed_step_at, enh_sample_logits_at) take the loop's position from one int32 in
// device memory instead of from their arguments, so the launches of one position, captured into a HIP graph, can be replayed for the next one.
// Each is a kernel of its own name around the __device__ body of its by-value sibling: the same arithmetic, the same bits.
#include "common.h"
#include "decode_attn.h"
#include "embed_row.h"
#include "skinny_gemm.h"
#include <type_traits>

#define GD_SAMPLE_MAX_V 16384
#define GD_SAMPLE_PER 16      // logits per thread of the sampler (1024 threads)

// ---------------------------------------------------------------------------------------------
// skinny GEMM
// ---------------------------------------------------------------------------------------------
// One workgroup = 16 rows of W; wave w takes the 128-wide K chunks w, w + 4, ... of the workgroup's K slice.  v_mfma_f32_16x16x32: lane (r = lane % 16,
// q = lane / 16) supplies row r, k = 8 q .. 8 q + 7 of a 32-wide step, so ONE load instruction reads 64 contiguous bytes of each of the 16 rows
// (whole 64-byte sectors: a 32-row fragment of the 32x32x16 form reads 32 bytes per row and instruction and measured 2 TB/s), four are in flight
// per wave and chunk.  x rows past M read row M - 1 (memory the caller owns); their columns are dropped.
template <typename OT, int MT>
__global__ __launch_bounds__(256) void gpt_skinny_gemm_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ W, int M, int N, int K,
                                                              int chunks_per_split, const float* __restrict__ bias, int act,
                                                              const float* __restrict__ res, float* __restrict__ out_f32,
                                                              uint16_t* __restrict__ out_h16, float* __restrict__ part) {
  __shared__ float s_acc[4][MT * 16][17];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nrow = n0 + r < N ? n0 + r : N - 1;
  const uint16_t* wp = W + (size_t)nrow * K + q * 8;
  const uint16_t* xp[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int xr = mt * 16 + r < M ? mt * 16 + r : M - 1;
    xp[mt] = x + (size_t)xr * K + q * 8;
  }
  const int nchunks = (K + 127) / 128;
  const int c0 = blockIdx.y * chunks_per_split;
  const int c1 = c0 + chunks_per_split < nchunks ? c0 + chunks_per_split : nchunks;
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = c0 + wave; c < c1; c += 4) {
    const int kb = c * 128;
    s16x8 a[4], b[MT][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = kb + i * 32;
      const bool ok = k + q * 8 < K;
      a[i] = ok ? __builtin_nontemporal_load(reinterpret_cast<const s16x8*>(wp + k)) : zero;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) b[mt][i] = ok ? *reinterpret_cast<const s16x8*>(xp[mt] + k) : zero;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16<OT>(a[i], b[mt][i], acc[mt]);
  }
  // D row (n) of acc[j]: 4 q + j ; column (m) = r
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < 4; ++j) s_acc[wave][mt * 16 + r][4 * q + j] = acc[mt][j];
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
__global__ __launch_bounds__(256) void gpt_skinny_reduce_kernel(const float* __restrict__ part, int splits, int M, int N, const float* __restrict__ bias,
                                                                int act, const float* __restrict__ res, float* __restrict__ out_f32,
                                                                uint16_t* __restrict__ out_h16) {
  gd_reduce_slabs<OT>(part, splits, M, N, bias, act, res, out_f32, out_h16);
}

extern "C" size_t enh_skinny_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M < 1 || N < 1 || K < 1) return 0;
  int cps, splits;
  gd_gemm_plan(N, K, &cps, &splits);
  return splits > 1 ? (size_t)splits * M * N * sizeof(float) : 0;
}

extern "C" int enh_skinny_gemm_h16(const enh_h16* x, const enh_h16* W, int64_t M, int64_t N, int64_t K, const float* bias, int act, const float* res,
                                   float* out_f32, enh_h16* out_h16, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  ENH_REQUIRE(x && W && (out_f32 || out_h16), ENH_E_BADARG, "enh_skinny_gemm_h16: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_skinny_gemm_h16");
  ENH_REQUIRE(M >= 1 && M <= GD_MAX_M, ENH_E_SHAPE, "enh_skinny_gemm_h16: M must be in [1, %d], got %lld", GD_MAX_M, (long long)M);
  ENH_REQUIRE(N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0 && N < (1LL << 30) && K < (1LL << 30), ENH_E_SHAPE,
              "enh_skinny_gemm_h16: N and K must be positive multiples of 8, got N=%lld K=%lld", (long long)N, (long long)K);
  ENH_REQUIRE(act == 0 || act == 1, ENH_E_BADARG, "enh_skinny_gemm_h16: act must be 0 (none) or 1 (relu^2), got %d", act);
  int cps, splits;
  gd_gemm_plan(N, K, &cps, &splits);
  float* part = nullptr;
  if (splits > 1) {
    ENH_REQUIRE(workspace && workspace_bytes >= enh_skinny_gemm_workspace_bytes(M, N, K), ENH_E_WORKSPACE, "enh_skinny_gemm_h16: workspace too small");
    part = reinterpret_cast<float*>(workspace);
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + 15) / 16), (unsigned)splits);
  // the label is the product kernel's, also when the slab pass follows
#define GD_GEMM_LAUNCH(MT)                                                                                                                        \
  do {                                                                                                                                            \
    enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_skinny_gemm_kernel<F16, " #MT ">" : "gpt_skinny_gemm_kernel<BF16, " #MT ">");                \
    ENH_DT_DISPATCH(dtype, (gpt_skinny_gemm_kernel<OT, MT><<<grid, 256, 0, s>>>(x, W, (int)M, (int)N, (int)K, cps, bias, act, res, out_f32,       \
                                                                                out_h16, part)));                                                 \
  } while (0)
  if (M <= 16) GD_GEMM_LAUNCH(1);
  else if (M <= 32) GD_GEMM_LAUNCH(2);
  else GD_GEMM_LAUNCH(4);
#undef GD_GEMM_LAUNCH
  if (splits > 1)
    ENH_DT_DISPATCH(dtype, (gpt_skinny_reduce_kernel<OT><<<(unsigned)((M * N + 255) / 256), 256, 0, s>>>(part, splits, (int)M, (int)N, bias, act, res,
                                                                                                        out_f32, out_h16)));
  return enh_check_launch("enh_skinny_gemm_h16");
}

// ---------------------------------------------------------------------------------------------
// decode attention
// ---------------------------------------------------------------------------------------------
template <typename OT, bool F32>
__device__ __forceinline__ void gd_load8(const void* p, float (&f)[8]) {
  if constexpr (F32) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    unpack8<OT>(*reinterpret_cast<const u32x4*>(p), f);
  }
}

// one piece (blockIdx.y) of one (batch, head) pair (blockIdx.x): the body of gpt_decode_attn_kernel and of its cursor form gpt_decode_attn_at_kernel
template <typename OT, bool F32>
__device__ __forceinline__ void gd_attn_piece(const void* __restrict__ qkv_, void* __restrict__ Kc_, void* __restrict__ Vc_, int H, int hs, int Tmax, int t,
                                              int nsplit, int split_len, float scale, void* __restrict__ out_, float* __restrict__ part) {
  typedef typename std::conditional<F32, float, uint16_t>::type CT;
  __shared__ float s_p[GD_ATT_PIECE];
  __shared__ float s_mx[4], s_sm[4];
  __shared__ float s_o[2048];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H, sp = blockIdx.y;
  const int C = H * hs;
  const int j0 = sp * split_len;
  const int j1 = j0 + split_len < t + 1 ? j0 + split_len : t + 1;
  const CT* qb = reinterpret_cast<const CT*>(qkv_) + (size_t)b * 3 * C + (size_t)h * hs;
  const CT* knew = qb + C;
  const CT* vnew = qb + 2 * C;
  CT* Kb = reinterpret_cast<CT*>(Kc_) + (size_t)bh * Tmax * hs;
  CT* Vb = reinterpret_cast<CT*>(Vc_) + (size_t)bh * Tmax * hs;
  const int nq = hs >> 6;   // 64-wide pieces of a head row (<= 6)

  // ---- scores: eight lanes per cache slot, 32 slots per pass ----
  const int g8 = tid & 7, slot = tid >> 3;
  float q[6][8];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    if (i < nq) gd_load8<OT, F32>(qb + i * 64 + g8 * 8, q[i]);
    else
#pragma unroll
      for (int e = 0; e < 8; ++e) q[i][e] = 0.f;
  }
  for (int base = j0; base < j1; base += 32) {
    const int j = base + slot;
    const bool valid = j < j1;
    float dot = 0.f;
    if (valid) {
      const CT* row = j == t ? knew : Kb + (size_t)j * hs;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        if (i < nq) {
          float k[8];
          gd_load8<OT, F32>(row + i * 64 + g8 * 8, k);
#pragma unroll
          for (int e = 0; e < 8; ++e) dot = fmaf(q[i][e], k[e], dot);
        }
      }
    }
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    dot += __shfl_xor(dot, 4, 64);
    if (valid && g8 == 0) s_p[j - j0] = dot * scale;
  }
  __syncthreads();
  // ---- softmax numerators of this piece ----
  const int n = j1 - j0;
  const float sv = tid < n ? s_p[tid] : -__builtin_inff();
  float mx = sv;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) s_mx[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
  const float e = tid < n ? expf(sv - mx) : 0.f;
  if (tid < n) s_p[tid] = e;
  const float ws = wave_sum(e);
  if (lane == 0) s_sm[wave] = ws;
  __syncthreads();
  const float l = ((s_sm[0] + s_sm[1]) + s_sm[2]) + s_sm[3];
  // ---- out = sum_j p_j V_j: hs / 8 threads per row, 256 / (hs / 8) rows in flight ----
  const int tpr = hs >> 3, ng = 256 / tpr;
  const int g = tid / tpr, c = tid - g * tpr;
  if (g < ng) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = j0 + g; j < j1; j += ng) {
      const CT* row = j == t ? vnew : Vb + (size_t)j * hs;
      float v[8];
      gd_load8<OT, F32>(row + c * 8, v);
      const float p = s_p[j - j0];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = fmaf(p, v[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) s_o[g * hs + c * 8 + k] = acc[k];
  }
  __syncthreads();
  for (int d = tid; d < hs; d += 256) {
    float o = s_o[d];
    for (int gg = 1; gg < ng; ++gg) o += s_o[gg * hs + d];
    if (nsplit == 1) {
      const float y = o / l;
      CT* out = reinterpret_cast<CT*>(out_) + (size_t)b * C + (size_t)h * hs;
      if constexpr (F32) out[d] = y;
      else out[d] = pack1<OT>(y);
    } else {
      part[((size_t)bh * nsplit + sp) * (hs + 2) + d] = o;
    }
    // the piece that holds slot t appends the step's k and v
    if (t >= j0 && t < j1) {
      Kb[(size_t)t * hs + d] = knew[d];
      Vb[(size_t)t * hs + d] = vnew[d];
    }
  }
  if (nsplit > 1 && tid == 0) {
    part[((size_t)bh * nsplit + sp) * (hs + 2) + hs] = mx;
    part[((size_t)bh * nsplit + sp) * (hs + 2) + hs + 1] = l;
  }
}

template <typename OT, bool F32>
__global__ __launch_bounds__(256) void gpt_decode_attn_kernel(const void* __restrict__ qkv_, void* __restrict__ Kc_, void* __restrict__ Vc_, int H, int hs,
                                                              int Tmax, int t, int nsplit, int split_len, float scale, void* __restrict__ out_,
                                                              float* __restrict__ part) {
  gd_attn_piece<OT, F32>(qkv_, Kc_, Vc_, H, hs, Tmax, t, nsplit, split_len, scale, out_, part);
}

// the pieces in ascending order (decode_attn.h gd_attn_merge, as the cursor form below)
template <typename OT, bool F32>
__global__ __launch_bounds__(128) void gpt_decode_attn_merge_kernel(const float* __restrict__ part, int H, int hs, int nsplit, void* __restrict__ out_) {
  gd_attn_merge<OT, F32>(part, H, hs, nsplit, out_);
}

extern "C" size_t enh_decode_attention_workspace_bytes(int B, int H, int hs, int Tmax) {
  if (B < 1 || H < 1 || hs < 1 || Tmax < 1) return 0;
  const size_t most = (size_t)(Tmax + 63) / 64;     // gd_att_plan never makes more pieces than 64-slot ones
  return (size_t)B * H * most * (hs + 2) * sizeof(float);
}

extern "C" int enh_decode_attention(const void* qkv, void* k_cache, void* v_cache, int B, int H, int hs, int Tmax, int t, void* out, void* workspace,
                                    size_t workspace_bytes, int dtype, void* stream) {
  ENH_REQUIRE(qkv && k_cache && v_cache && out, ENH_E_BADARG, "enh_decode_attention: null pointer");
  ENH_REQUIRE(dtype == ENH_DT_BF16 || dtype == ENH_DT_F16 || dtype == ENH_DT_F32, ENH_E_BADARG, "enh_decode_attention: dtype must be 0, 1 or 2, got %d", dtype);
  ENH_REQUIRE(B >= 1 && H >= 1 && (int64_t)B * H <= 2147483647LL, ENH_E_BADARG, "enh_decode_attention: B=%d H=%d", B, H);
  ENH_REQUIRE(hs >= 64 && hs <= 384 && hs % 64 == 0, ENH_E_SHAPE, "enh_decode_attention: head size must be a multiple of 64 up to 384, got %d", hs);
  ENH_REQUIRE(Tmax >= 1 && Tmax <= GD_ATT_MAX_T, ENH_E_SHAPE, "enh_decode_attention: cache length must be in [1, %d], got %d", GD_ATT_MAX_T, Tmax);
  ENH_REQUIRE(t >= 0 && t < Tmax, ENH_E_BADARG, "enh_decode_attention: step %d outside the cache of %d slots", t, Tmax);
  int nsplit, split_len;
  gd_att_plan((int64_t)B * H, t + 1, &nsplit, &split_len);
  float* part = nullptr;
  if (nsplit > 1) {
    ENH_REQUIRE(workspace && workspace_bytes >= (size_t)B * H * nsplit * (hs + 2) * sizeof(float), ENH_E_WORKSPACE,
                "enh_decode_attention: workspace too small");
    part = reinterpret_cast<float*>(workspace);
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * H), (unsigned)nsplit);
  const float scale = 1.0f / sqrtf((float)hs);
  if (dtype == ENH_DT_F32) {
    enh_note_kernel_plain("gpt_decode_attn_kernel<BF16, true>");
    gpt_decode_attn_kernel<BF16, true><<<grid, 256, 0, s>>>(qkv, k_cache, v_cache, H, hs, Tmax, t, nsplit, split_len, scale, out, part);
    if (nsplit > 1) gpt_decode_attn_merge_kernel<BF16, true><<<(unsigned)(B * H), 128, 0, s>>>(part, H, hs, nsplit, out);
  } else {
    enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_decode_attn_kernel<F16, false>" : "gpt_decode_attn_kernel<BF16, false>");
    ENH_DT_DISPATCH(dtype, (gpt_decode_attn_kernel<OT, false><<<grid, 256, 0, s>>>(qkv, k_cache, v_cache, H, hs, Tmax, t, nsplit, split_len, scale, out, part)));
    if (nsplit > 1) ENH_DT_DISPATCH(dtype, (gpt_decode_attn_merge_kernel<OT, false><<<(unsigned)(B * H), 128, 0, s>>>(part, H, hs, nsplit, out)));
  }
  return enh_check_launch("enh_decode_attention");
}

// ---------------------------------------------------------------------------------------------
// the cursor forms: the position t of the sampling loop is one int32 in device memory, so a captured launch sequence can be replayed for the
// next position.  Nothing that depends on t is a kernel argument: the slot, the split plan and the grid's live part are worked out on the device.
// ---------------------------------------------------------------------------------------------
__global__ void gpt_cursor_advance_kernel(int* __restrict__ cursor) { *cursor += 1; }

extern "C" int enh_cursor_advance(int* cursor, void* stream) {
  ENH_REQUIRE(cursor, ENH_E_BADARG, "enh_cursor_advance: null pointer");
  enh_note_kernel_plain("gpt_cursor_advance_kernel");
  gpt_cursor_advance_kernel<<<1, 1, 0, (hipStream_t)stream>>>(cursor);
  return enh_check_launch("enh_cursor_advance");
}

// gpt_decode_attn_kernel under a grid sized for the whole cache (gridDim.y = (Tmax + 63) / 64 >= every plan's nsplit): the pieces past the plan return
template <typename OT, bool F32>
__global__ __launch_bounds__(256) void gpt_decode_attn_at_kernel(const void* __restrict__ qkv_, void* __restrict__ Kc_, void* __restrict__ Vc_, int H, int hs,
                                                                 int Tmax, const int* __restrict__ cursor, int t_offset, float scale,
                                                                 void* __restrict__ out_, float* __restrict__ part) {
  const int t = gd_cursor_step(cursor, t_offset, Tmax);
  if (t < 0) return;
  int nsplit, split_len;
  gd_att_plan((int64_t)gridDim.x, t + 1, &nsplit, &split_len);
  if ((int)blockIdx.y >= nsplit) return;
  gd_attn_piece<OT, F32>(qkv_, Kc_, Vc_, H, hs, Tmax, t, nsplit, split_len, scale, out_, part);
}

// always launched: under a plan of one piece the main kernel has written out itself
template <typename OT, bool F32>
__global__ __launch_bounds__(128) void gpt_decode_attn_merge_at_kernel(const float* __restrict__ part, int H, int hs, int Tmax,
                                                                       const int* __restrict__ cursor, int t_offset, void* __restrict__ out_) {
  const int t = gd_cursor_step(cursor, t_offset, Tmax);
  if (t < 0) return;
  int nsplit, split_len;
  gd_att_plan((int64_t)gridDim.x, t + 1, &nsplit, &split_len);
  if (nsplit == 1) return;
  gd_attn_merge<OT, F32>(part, H, hs, nsplit, out_);
}

extern "C" int enh_decode_attention_at(const void* qkv, void* k_cache, void* v_cache, int B, int H, int hs, int Tmax, const int* cursor, int t_offset,
                                       void* out, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  ENH_REQUIRE(qkv && k_cache && v_cache && out && cursor, ENH_E_BADARG, "enh_decode_attention_at: null pointer");
  ENH_REQUIRE(dtype == ENH_DT_BF16 || dtype == ENH_DT_F16 || dtype == ENH_DT_F32, ENH_E_BADARG, "enh_decode_attention_at: dtype must be 0, 1 or 2, got %d", dtype);
  ENH_REQUIRE(B >= 1 && H >= 1 && (int64_t)B * H <= 2147483647LL, ENH_E_BADARG, "enh_decode_attention_at: B=%d H=%d", B, H);
  ENH_REQUIRE(hs >= 64 && hs <= 384 && hs % 64 == 0, ENH_E_SHAPE, "enh_decode_attention_at: head size must be a multiple of 64 up to 384, got %d", hs);
  ENH_REQUIRE(Tmax >= 1 && Tmax <= GD_ATT_MAX_T, ENH_E_SHAPE, "enh_decode_attention_at: cache length must be in [1, %d], got %d", GD_ATT_MAX_T, Tmax);
  // the plan is not known here: the workspace holds the most pieces any position of the cache can have
  ENH_REQUIRE(workspace && workspace_bytes >= enh_decode_attention_workspace_bytes(B, H, hs, Tmax), ENH_E_WORKSPACE,
              "enh_decode_attention_at: workspace too small");
  float* part = reinterpret_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * H), (unsigned)((Tmax + 63) / 64));
  const float scale = 1.0f / sqrtf((float)hs);
  if (dtype == ENH_DT_F32) {
    enh_note_kernel_plain("gpt_decode_attn_at_kernel<BF16, true>");
    gpt_decode_attn_at_kernel<BF16, true><<<grid, 256, 0, s>>>(qkv, k_cache, v_cache, H, hs, Tmax, cursor, t_offset, scale, out, part);
    gpt_decode_attn_merge_at_kernel<BF16, true><<<(unsigned)(B * H), 128, 0, s>>>(part, H, hs, Tmax, cursor, t_offset, out);
  } else {
    enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_decode_attn_at_kernel<F16, false>" : "gpt_decode_attn_at_kernel<BF16, false>");
    ENH_DT_DISPATCH(dtype, (gpt_decode_attn_at_kernel<OT, false><<<grid, 256, 0, s>>>(qkv, k_cache, v_cache, H, hs, Tmax, cursor, t_offset, scale, out, part)));
    ENH_DT_DISPATCH(dtype, (gpt_decode_attn_merge_at_kernel<OT, false><<<(unsigned)(B * H), 128, 0, s>>>(part, H, hs, Tmax, cursor, t_offset, out)));
  }
  return enh_check_launch("enh_decode_attention_at");
}

// The step's input row at t = *cursor: row b sums the n ids at ids_base[b id_row_stride + t id_t_stride + id_offset ..] in ascending order and adds
// the position row at pos_base + t pos_t_stride + pos_offset (embed_row.h: rq_embed_step_kernel's body; at n == 1 the row is table[id] + pos, the
// bits of gpt_embed_kernel).  A position outside [t_lo, t_hi) reads and writes nothing.
__global__ __launch_bounds__(256) void gpt_embed_at_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids_base, int64_t id_row_stride,
                                                           int64_t id_t_stride, int64_t id_offset, int n, const float* __restrict__ pos_base,
                                                           int64_t pos_t_stride, int64_t pos_offset, const int* __restrict__ cursor, int t_lo, int t_hi,
                                                           int C, int V, float* __restrict__ out) {
  const int64_t t = *cursor;
  if (t < t_lo || t >= t_hi) return;
  const int64_t b = blockIdx.x;
  rq_embed_row(table, ids_base + b * id_row_stride + t * id_t_stride + id_offset, n, pos_base + t * pos_t_stride + pos_offset, C, V, out + b * C);
}

extern "C" int enh_embed_step_at(const float* table, const int64_t* ids_base, int64_t id_row_stride, int64_t id_t_stride, int64_t id_offset, int n,
                                 const float* pos_base, int64_t pos_t_stride, int64_t pos_offset, const int* cursor, int t_lo, int t_hi, int B, int C,
                                 int V, float* out, void* stream) {
  ENH_REQUIRE(n >= 1 && n <= RQ_MAX_DEPTH, ENH_E_SHAPE, "enh_embed_step_at: the number of summed codes must be in [1, %d], got %d", RQ_MAX_DEPTH, n);
  ENH_REQUIRE(table && ids_base && pos_base && cursor && out, ENH_E_BADARG, "enh_embed_step_at: null pointer");
  ENH_REQUIRE(B >= 1 && V >= 1 && t_lo >= 0 && t_hi > t_lo, ENH_E_BADARG, "enh_embed_step_at: B=%d V=%d positions [%d, %d)", B, V, t_lo, t_hi);
  // the first and the last position's ids and position row must lie at or behind the bases (the caller owns what follows them)
  ENH_REQUIRE(t_lo * id_t_stride + id_offset >= 0 && (t_hi - 1) * id_t_stride + id_offset >= 0 && t_lo * pos_t_stride + pos_offset >= 0 &&
                  (t_hi - 1) * pos_t_stride + pos_offset >= 0 && id_row_stride >= 0 && pos_offset % 4 == 0 && pos_t_stride % 4 == 0,
              ENH_E_BADARG, "enh_embed_step_at: strides %lld %lld %lld / %lld %lld reach in front of a base or break the 16-byte alignment",
              (long long)id_row_stride, (long long)id_t_stride, (long long)id_offset, (long long)pos_t_stride, (long long)pos_offset);
  ENH_REQUIRE(C >= 4 && C % 4 == 0, ENH_E_SHAPE, "enh_embed_step_at: C must be a positive multiple of 4, got %d", C);
  enh_note_kernel_plain("gpt_embed_at_kernel");
  gpt_embed_at_kernel<<<(unsigned)B, 256, 0, (hipStream_t)stream>>>(table, ids_base, id_row_stride, id_t_stride, id_offset, n, pos_base, pos_t_stride,
                                                                    pos_offset, cursor, t_lo, t_hi, C, V, out);
  return enh_check_launch("enh_embed_step_at");
}

// ---------------------------------------------------------------------------------------------
// exact-mode product
// ---------------------------------------------------------------------------------------------
// exact mode: the same product with f32 operands on the vector ALU.  One wave per row of W, the lanes share K (a lane adds K / 64 products,
// then a 6-level tree over the lanes), eight rows of x at a time.  A parity instrument: W is re-read through L2 once per eight rows.
__global__ __launch_bounds__(256) void gpt_skinny_gemm_f32_kernel(const float* __restrict__ x, const float* __restrict__ W, int M, int N, int K,
                                                                  const float* __restrict__ bias, int act, const float* __restrict__ res,
                                                                  float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* wr = W + (size_t)n * K;
  for (int m0 = 0; m0 < M; m0 += 8) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = lane * 4; k < K; k += 256) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + k);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (m0 + j < M) {
          const f32x4 x4 = *reinterpret_cast<const f32x4*>(x + (size_t)(m0 + j) * K + k);
          acc[j] = fmaf(x4.w, w4.w, fmaf(x4.z, w4.z, fmaf(x4.y, w4.y, fmaf(x4.x, w4.x, acc[j]))));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = wave_sum(acc[j]);
      if (lane == 0 && m0 + j < M) out[(size_t)(m0 + j) * N + n] = gd_epilogue(v, m0 + j, n, N, bias, act, res);
    }
  }
}

extern "C" int enh_skinny_gemm_f32(const float* x, const float* W, int64_t M, int64_t N, int64_t K, const float* bias, int act, const float* res,
                                   float* out, void* stream) {
  ENH_REQUIRE(x && W && out, ENH_E_BADARG, "enh_skinny_gemm_f32: null pointer");
  ENH_REQUIRE(M >= 1 && M <= GD_MAX_M, ENH_E_SHAPE, "enh_skinny_gemm_f32: M must be in [1, %d], got %lld", GD_MAX_M, (long long)M);
  ENH_REQUIRE(N >= 1 && K >= 8 && K % 8 == 0 && N < (1LL << 30) && K < (1LL << 30), ENH_E_SHAPE,
              "enh_skinny_gemm_f32: K must be a positive multiple of 8, got N=%lld K=%lld", (long long)N, (long long)K);
  ENH_REQUIRE(act == 0 || act == 1, ENH_E_BADARG, "enh_skinny_gemm_f32: act must be 0 (none) or 1 (relu^2), got %d", act);
  enh_note_kernel_plain("gpt_skinny_gemm_f32_kernel");
  gpt_skinny_gemm_f32_kernel<<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(x, W, (int)M, (int)N, (int)K, bias, act, res, out);
  return enh_check_launch("enh_skinny_gemm_f32");
}

// ---------------------------------------------------------------------------------------------
// sampler.  One workgroup of 1024 threads per row; thread t holds the 16 logits t * 16 .. t * 16 + 15 in registers, so the draw walks the row
// in index order.  The k-th largest logit and the top-p cut are found by a bitwise threshold search on the order-preserving integer image
// of a float (32 counting / summing passes over registers), not by a sort.
// ---------------------------------------------------------------------------------------------
// word 0 of Philox4x32-10 (common.h) with key = seed and counter = (row low, row high, step, call)
__device__ __forceinline__ float gd_uniform(uint64_t seed, uint32_t call, uint32_t step, uint64_t row) {
  const uint32_t c0 = philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), u32x4{(uint32_t)row, (uint32_t)(row >> 32), step, call}).x;
  return (float)(c0 >> 9) * 1.1920928955078125e-07f + 5.9604644775390625e-08f;   // 23 bits: (c0 >> 9) 2^-23 + 2^-24 in [2^-24, 1 - 2^-24], every step exact
}
__device__ __forceinline__ uint32_t gd_key(float x) {   // a < b  <=>  key(a) < key(b)
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// one row (blockIdx.x): the body of gpt_sample_kernel and of its cursor form gpt_sample_at_kernel
__device__ __forceinline__ void gd_sample_row(const float* __restrict__ logits, int V, float temperature, int top_k, float top_p,
                                              const float* __restrict__ uniforms, uint64_t seed, uint32_t call, uint32_t step, int64_t row0,
                                              int64_t* __restrict__ codes, int64_t code_stride, float* __restrict__ logits_out,
                                              int64_t logits_out_stride, uint8_t* __restrict__ mask_out, float* __restrict__ probs_out) {
  __shared__ float s_f[16];
  __shared__ int s_i[16];
  __shared__ int s_pick, s_last;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row = blockIdx.x;
  const float* lr = logits + (size_t)row * V;
  const int i0 = t * GD_SAMPLE_PER;
  const float NEG = -__builtin_inff();
  float x[GD_SAMPLE_PER];
#pragma unroll
  for (int i = 0; i < GD_SAMPLE_PER; ++i) x[i] = i0 + i < V ? lr[i0 + i] / temperature : NEG;
  if (t == 0) { s_pick = 0x7fffffff; s_last = -1; }
  // ---- top-k: T = the k-th largest logit; everything below it becomes -inf (ties with it stay: the reference masks with `<`) ----
  if (top_k > 0 && top_k < V) {
    uint32_t T = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = T | (1u << bit);
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < GD_SAMPLE_PER; ++i) cnt += (i0 + i < V && gd_key(x[i]) >= cand) ? 1 : 0;
      if (block_count<16>(cnt, s_i) >= top_k) T = cand;
    }
#pragma unroll
    for (int i = 0; i < GD_SAMPLE_PER; ++i)
      if (gd_key(x[i]) < T) x[i] = NEG;
  }
  if (logits_out) {
#pragma unroll
    for (int i = 0; i < GD_SAMPLE_PER; ++i)
      if (i0 + i < V) logits_out[(size_t)row * logits_out_stride + i0 + i] = x[i];
  }
  // ---- softmax ----
  float mx = NEG;
#pragma unroll
  for (int i = 0; i < GD_SAMPLE_PER; ++i) mx = fmaxf(mx, x[i]);
  mx = block_max<16>(mx, s_f);
  float p[GD_SAMPLE_PER];
  float ps = 0.f;
#pragma unroll
  for (int i = 0; i < GD_SAMPLE_PER; ++i) {
    p[i] = i0 + i < V ? expf(x[i] - mx) : 0.f;
    ps += p[i];
  }
  const float tot = block_sum<16>(ps, s_f);
#pragma unroll
  for (int i = 0; i < GD_SAMPLE_PER; ++i) p[i] = p[i] / tot;
  // ---- top-p: in descending order entry j >= 1 goes when the probability in front of it is >= top_p, i.e. an entry stays iff the sum of the
  // strictly larger probabilities is < top_p.  F(T) = sum of p > T falls as T rises: the cut is the smallest T with F(T) < top_p (probabilities
  // are non-negative floats, whose bit patterns order like integers).  The largest entry always stays. ----
  uint32_t cut = 0;
  if (top_p >= 0.f) {
    float pm = 0.f;
#pragma unroll
    for (int i = 0; i < GD_SAMPLE_PER; ++i) pm = fmaxf(pm, p[i]);
    pm = block_max<16>(pm, s_f);
    float f = 0.f;
#pragma unroll
    for (int i = 0; i < GD_SAMPLE_PER; ++i) f += p[i] > 0.f ? p[i] : 0.f;
    if (!(block_sum<16>(f, s_f) < top_p)) {
      uint32_t Tn = 0;      // the largest T with F(T) >= top_p
      for (int bit = 30; bit >= 0; --bit) {
        const uint32_t cand = Tn | (1u << bit);
        float fs = 0.f;
#pragma unroll
        for (int i = 0; i < GD_SAMPLE_PER; ++i) fs += __builtin_bit_cast(uint32_t, p[i]) > cand ? p[i] : 0.f;
        if (!(block_sum<16>(fs, s_f) < top_p)) Tn = cand;
      }
      cut = Tn + 1;
    }
    const uint32_t pmk = __builtin_bit_cast(uint32_t, pm);
    if (cut > pmk) cut = pmk;
  }
  bool keep[GD_SAMPLE_PER];
  float ks = 0.f;
#pragma unroll
  for (int i = 0; i < GD_SAMPLE_PER; ++i) {
    keep[i] = i0 + i < V && x[i] != NEG && __builtin_bit_cast(uint32_t, p[i]) >= cut;
    if (!keep[i]) p[i] = 0.f;
    ks += p[i];
  }
  if (top_p >= 0.f) {
    const float kt = block_sum<16>(ks, s_f);
    ks = 0.f;
#pragma unroll
    for (int i = 0; i < GD_SAMPLE_PER; ++i) { p[i] = p[i] / kt; ks += p[i]; }
  }
  if (mask_out || probs_out) {
#pragma unroll
    for (int i = 0; i < GD_SAMPLE_PER; ++i) {
      if (i0 + i >= V) continue;
      if (mask_out) mask_out[(size_t)row * V + i0 + i] = keep[i] ? 1 : 0;
      if (probs_out) probs_out[(size_t)row * V + i0 + i] = p[i];
    }
  }
  // ---- draw: the first index whose running sum exceeds u * total ----
  // exclusive prefix of the threads' sums: inside the wave by shuffles, across waves in wave order
  float inc = ks;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();
  if (lane == 63) s_f[wave] = inc;
  __syncthreads();
  float base = 0.f, total = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i < wave) base += s_f[i];
    total += s_f[i];
  }
  const float u = uniforms ? uniforms[row] : gd_uniform(seed, call, step, (uint64_t)(row0 + row));
  const float target = u * total;
  float run = base + (inc - ks);
  int pick = 0x7fffffff, last = -1;
#pragma unroll
  for (int i = 0; i < GD_SAMPLE_PER; ++i) {
    run += p[i];
    if (p[i] > 0.f) {
      last = i0 + i;
      if (run > target && pick == 0x7fffffff) pick = i0 + i;
    }
  }
  if (pick != 0x7fffffff) atomicMin(&s_pick, pick);
  if (last >= 0) atomicMax(&s_last, last);
  __syncthreads();
  if (t == 0) {
    int c = s_pick != 0x7fffffff ? s_pick : s_last;      // u * total rounded up to the total itself: the last kept entry
    if (c < 0) c = 0;
    codes[(int64_t)row * code_stride] = (int64_t)c;
  }
}

__global__ __launch_bounds__(1024) void gpt_sample_kernel(const float* __restrict__ logits, int V, float temperature, int top_k, float top_p,
                                                          const float* __restrict__ uniforms, uint64_t seed, uint32_t call, uint32_t step,
                                                          int64_t row0, int64_t* __restrict__ codes, int64_t code_stride,
                                                          float* __restrict__ logits_out, int64_t logits_out_stride, uint8_t* __restrict__ mask_out,
                                                          float* __restrict__ probs_out) {
  gd_sample_row(logits, V, temperature, top_k, top_p, uniforms, seed, call, step, row0, codes, code_stride, logits_out, logits_out_stride, mask_out,
                probs_out);
}

extern "C" int enh_sample_logits(const float* logits, int B, int V, float temperature, int top_k, float top_p, const float* uniforms, uint64_t seed,
                                 uint32_t call, uint32_t step, int64_t row0, int64_t* codes, int64_t code_stride, float* logits_out,
                                 int64_t logits_out_stride, uint8_t* mask_out, float* probs_out, void* stream) {
  ENH_REQUIRE(logits && codes, ENH_E_BADARG, "enh_sample_logits: null pointer");
  ENH_REQUIRE(B >= 1 && code_stride >= 1 && row0 >= 0 && (!logits_out || logits_out_stride >= V), ENH_E_BADARG, "enh_sample_logits: B=%d strides %lld %lld",
              B, (long long)code_stride, (long long)logits_out_stride);
  ENH_REQUIRE(V >= 1 && V <= GD_SAMPLE_MAX_V, ENH_E_SHAPE, "enh_sample_logits: V must be in [1, %d], got %d", GD_SAMPLE_MAX_V, V);
  ENH_REQUIRE(temperature > 0.f, ENH_E_BADARG, "enh_sample_logits: temperature must be positive, got %g", (double)temperature);
  enh_note_kernel_plain("gpt_sample_kernel");
  gpt_sample_kernel<<<(unsigned)B, 1024, 0, (hipStream_t)stream>>>(logits, V, temperature, top_k, top_p, uniforms, seed, call, step, row0, codes,
                                                                   code_stride, logits_out, logits_out_stride, mask_out, probs_out);
  return enh_check_launch("enh_sample_logits");
}

// the cursor form: step = *cursor * step_mul + step_add selects the draw's uniform, the column of the codes and the row of logits_out.  A step
// outside [0, n_steps) (a replay too many) writes nothing.
__global__ __launch_bounds__(1024) void gpt_sample_at_kernel(const float* __restrict__ logits, int V, float temperature, int top_k, float top_p,
                                                             uint64_t seed, uint32_t call, const int* __restrict__ cursor, int step_mul, int step_add,
                                                             int n_steps, int64_t row0, int64_t* __restrict__ codes_base, int64_t code_row_stride,
                                                             float* __restrict__ logits_base, int64_t logits_row_stride) {
  const int64_t step = (int64_t)*cursor * step_mul + step_add;
  if (step < 0 || step >= n_steps) return;
  gd_sample_row(logits, V, temperature, top_k, top_p, nullptr, seed, call, (uint32_t)step, row0, codes_base + step, code_row_stride,
                logits_base ? logits_base + step * V : nullptr, logits_row_stride, nullptr, nullptr);
}

extern "C" int enh_sample_logits_at(const float* logits, int B, int V, float temperature, int top_k, float top_p, uint64_t seed, uint32_t call,
                                    const int* cursor, int step_mul, int step_add, int n_steps, int64_t row0, int64_t* codes_base,
                                    int64_t code_row_stride, float* logits_base, int64_t logits_row_stride, void* stream) {
  ENH_REQUIRE(logits && codes_base && cursor, ENH_E_BADARG, "enh_sample_logits_at: null pointer");
  ENH_REQUIRE(B >= 1 && n_steps >= 1 && row0 >= 0 && code_row_stride >= n_steps && (!logits_base || logits_row_stride >= (int64_t)n_steps * V), ENH_E_BADARG,
              "enh_sample_logits_at: B=%d n_steps=%d strides %lld %lld", B, n_steps, (long long)code_row_stride, (long long)logits_row_stride);
  ENH_REQUIRE(V >= 1 && V <= GD_SAMPLE_MAX_V, ENH_E_SHAPE, "enh_sample_logits_at: V must be in [1, %d], got %d", GD_SAMPLE_MAX_V, V);
  ENH_REQUIRE(temperature > 0.f, ENH_E_BADARG, "enh_sample_logits_at: temperature must be positive, got %g", (double)temperature);
  enh_note_kernel_plain("gpt_sample_at_kernel");
  gpt_sample_at_kernel<<<(unsigned)B, 1024, 0, (hipStream_t)stream>>>(logits, V, temperature, top_k, top_p, seed, call, cursor, step_mul, step_add, n_steps,
                                                                      row0, codes_base, code_row_stride, logits_base, logits_row_stride);
  return enh_check_launch("enh_sample_logits_at");
}
