// gpt_decode_kv8.hip — the decode attention of stage-2 sampling over an MXFP8 k / v cache for gfx950.  At batch 64 a step reads 38.7 GB of 16-bit
// cache against 11.3 GB of MXFP8 weights; here a cache entry is one e4m3fn code per element and one E8M0 scale per 32 consecutive
// elements of a head row (mxfp8.h; include/enh_hip.h states the layout), 1 + 1/32 bytes per element instead of 2.
//
//   enh_decode_attention_kv8     enh_decode_attention's contract (gpt_decode.hip) with each cache given as (codes [B, H, Tmax, hs], scales
//                                [B, H, Tmax, hs / 32]): quantizes the step's k and v rows (the 16-bit values of the qkv row, widened to f32, with
//                                enh_mxfp8_quantize's rounding), appends them at slot t and returns softmax(q K[0..t]^T / sqrt(hs)) V[0..t] over the
//                                DEQUANTIZED cache, slot t included: a slot contributes the same k / v to every step that reads it.
//   enh_decode_attention_kv8_at  the cursor form: t = *cursor + t_offset read on the device, the same __device__ body, the same bits.
//
// The pieces, their (out, max, sum) records and the ascending merge are the 16-bit kernel's (decode_attn.h).  Per piece, as there: a score pass into
// LDS, the piece's max / sum, P V with a fixed-order reduction; the piece that holds slot t quantizes the step's rows into LDS first, reads slot t from
// there (never from the cache) and writes its codes and scales.
// The lanes.  A lane reads 16 codes (one 16-byte load) and the one scale byte of their half block.  Scores: four lanes per slot take the 64-wide
// chunks of a head row, so a load instruction reads 64 contiguous bytes per slot and 64 slots are in flight per pass; q is f32 in registers.  A
// chunk's sum of q * code products (two chains of packed f32 FMAs, even and odd elements, added once) starts from zero and is multiplied by the
// block's 2^(s - 127) as it is added to the lane's score: a 16-bit q times a code is exact in f32 and a power of two on an f32 partial sum is
// exact, so the scale costs no accuracy.  P V: hs / 16 lanes per slot, eight rows requested before the first is used (a row at a time left every
// lane waiting one memory latency per slot: 1.2 - 1.3 x the time at batch 64); the weight p_j 2^(s - 127) is formed once per lane and slot (exact)
// and multiplies the 16 codes.  Packed FMAs alone changed nothing: the kernel waits for memory, not for the vector ALU.
// q stays 16-bit; scores, softmax and P V accumulate in f32.  No atomics, all sums in a fixed order: the same bits on every run.
#include "common.h"
#include "decode_attn.h"
#include "mxfp8.h"

#define KV8_MAX_HS 384
#define KV8_PV_UNROLL 8     // cache rows of P V a lane has in flight

// 16 e4m3fn codes (four dwords, ascending from the low byte) -> eight f32 pairs; scale 1: exact
__device__ __forceinline__ void kv8_widen16(const u32x4 c, f32x2 (&f)[8]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    f[2 * w] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c[w], 1.0f, false);
    f[2 * w + 1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c[w], 1.0f, true);
  }
}

// one piece (blockIdx.y) of one (batch, head) pair (blockIdx.x): the body of gpt_decode_attn_kv8_kernel and of its cursor form
template <typename OT>
__device__ __forceinline__ void kv8_attn_piece(const uint16_t* __restrict__ qkv, uint8_t* __restrict__ Kc, uint8_t* __restrict__ Ks,
                                               uint8_t* __restrict__ Vc, uint8_t* __restrict__ Vs, int H, int hs, int Tmax, int t, int nsplit,
                                               int split_len, float scale, uint16_t* __restrict__ out_, float* __restrict__ part) {
  __shared__ float s_p[GD_ATT_PIECE];
  __shared__ float s_mx[4], s_sm[4];
  __shared__ float s_o[4096];                                   // (256 / (hs / 16)) rows of hs partial sums: at most 64 x 64
  __shared__ __attribute__((aligned(16))) uint8_t s_code[2 * KV8_MAX_HS];   // slot t: the k row's codes, then the v row's
  __shared__ uint8_t s_scale[2 * KV8_MAX_HS / MX_BLOCK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H, sp = blockIdx.y;
  const int C = H * hs, nb = hs / MX_BLOCK;
  const int j0 = sp * split_len;
  const int j1 = j0 + split_len < t + 1 ? j0 + split_len : t + 1;
  const bool holds_t = t >= j0 && t < j1;
  const uint16_t* qb = qkv + (size_t)b * 3 * C + (size_t)h * hs;
  uint8_t* Kcb = Kc + (size_t)bh * Tmax * hs;
  uint8_t* Vcb = Vc + (size_t)bh * Tmax * hs;
  uint8_t* Ksb = Ks + (size_t)bh * Tmax * nb;
  uint8_t* Vsb = Vs + (size_t)bh * Tmax * nb;
  const int nq = hs >> 6;   // 64-wide chunks of a head row (<= 6)

  // ---- slot t: quantize the step's k and v rows, one element per thread and turn; the 32 lanes of a half wave hold a block (2 hs % 64 == 0:
  // a turn is whole waves), its maximum crosses them by five shuffles ----
  if (holds_t) {
    for (int idx = tid; idx < 2 * hs; idx += 256) {
      const int d = idx < hs ? idx : idx - hs;
      const float v = unpack1<OT>(qb[(idx < hs ? C : 2 * C) + d]);
      uint32_t amax = __builtin_bit_cast(uint32_t, v) & 0x7fffffffu;
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)amax, o, 64);
        amax = other > amax ? other : amax;
      }
      const int X = mx_block_exponent(amax);
      s_code[idx] = mx_e4m3_rne(v * mx_inv_scale(X));
      if ((lane & 31) == 0) s_scale[idx >> 5] = (uint8_t)(X + 127);
    }
    __syncthreads();
    // append: 16 codes per thread, then the scale bytes
    for (int i = tid; i < hs >> 3; i += 256) {
      const bool is_v = i >= hs >> 4;
      const int o = (is_v ? i - (hs >> 4) : i) * 16;
      *reinterpret_cast<u32x4*>((is_v ? Vcb : Kcb) + (size_t)t * hs + o) = *reinterpret_cast<const u32x4*>(s_code + (is_v ? hs : 0) + o);
    }
    if (tid < 2 * nb) {
      const bool is_v = tid >= nb;
      (is_v ? Vsb : Ksb)[(size_t)t * nb + (is_v ? tid - nb : tid)] = s_scale[tid];
    }
  }

  // ---- scores: four lanes per cache slot, 64 slots per pass; lane g4 takes codes 64 i + 16 g4 .. + 15 of a row, half of block 2 i + g4 / 2 ----
  const int g4 = tid & 3, slot = tid >> 2;
  f32x2 q[6][8];   // pairs of neighbours: the products of a chunk run as packed f32 FMAs (v_pk_fma_f32), even and odd elements in two chains
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    if (i < nq) {
      float lo[8], hi[8];
      unpack8<OT>(*reinterpret_cast<const u32x4*>(qb + i * 64 + g4 * 16), lo);
      unpack8<OT>(*reinterpret_cast<const u32x4*>(qb + i * 64 + g4 * 16 + 8), hi);
#pragma unroll
      for (int e = 0; e < 4; ++e) { q[i][e] = f32x2{lo[2 * e], lo[2 * e + 1]}; q[i][4 + e] = f32x2{hi[2 * e], hi[2 * e + 1]}; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) q[i][e] = f32x2{0.f, 0.f};
    }
  }
  for (int base = j0; base < j1; base += 64) {
    const int j = base + slot;
    const bool valid = j < j1;
    float dot = 0.f;
    if (valid) {
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        if (i < nq) {
          u32x4 c;
          uint32_t sb;
          if (j == t) {
            c = *reinterpret_cast<const u32x4*>(s_code + i * 64 + g4 * 16);
            sb = s_scale[2 * i + (g4 >> 1)];
          } else {
            c = *reinterpret_cast<const u32x4*>(Kcb + (size_t)j * hs + i * 64 + g4 * 16);
            sb = Ksb[(size_t)j * nb + 2 * i + (g4 >> 1)];
          }
          f32x2 k[8];
          kv8_widen16(c, k);
          f32x2 blk = {0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 8; ++e) blk = __builtin_elementwise_fma(q[i][e], k[e], blk);
          dot = fmaf(blk.x + blk.y, mx_scale_f32(sb), dot);
        }
      }
    }
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    if (valid && g4 == 0) s_p[j - j0] = dot * scale;
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
  // ---- out = sum_j p_j V_j: hs / 16 threads per row, 256 / (hs / 16) rows in flight; thread c of a row takes codes 16 c .. + 15, half of block c / 2 ----
  const int tpr = hs >> 4, ng = 256 / tpr;
  const int g = tid / tpr, c = tid - g * tpr;
  if (g < ng) {
    f32x2 acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = f32x2{0.f, 0.f};
    // slot t, when this piece holds it, is its last slot (j1 == t + 1): the slots in front of it come from the cache, KV8_PV_UNROLL rows requested
    // before the first is used (one 16-byte request per lane and row: a row at a time leaves the lane waiting a memory latency per slot); the
    // rows are added in ascending order either way
    const int jend = holds_t ? t : j1;
    const auto add_row = [&](const u32x4 cw, const uint32_t sb, const int j) {
      f32x2 v[8];
      kv8_widen16(cw, v);
      const float w = s_p[j - j0] * mx_scale_f32(sb);
      const f32x2 w2 = {w, w};
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = __builtin_elementwise_fma(w2, v[k], acc[k]);
    };
    int j = j0 + g;
    for (; j + (KV8_PV_UNROLL - 1) * ng < jend; j += KV8_PV_UNROLL * ng) {
      u32x4 cw[KV8_PV_UNROLL];
      uint32_t sb[KV8_PV_UNROLL];
#pragma unroll
      for (int u = 0; u < KV8_PV_UNROLL; ++u) {
        cw[u] = *reinterpret_cast<const u32x4*>(Vcb + (size_t)(j + u * ng) * hs + c * 16);
        sb[u] = Vsb[(size_t)(j + u * ng) * nb + (c >> 1)];
      }
#pragma unroll
      for (int u = 0; u < KV8_PV_UNROLL; ++u) add_row(cw[u], sb[u], j + u * ng);
    }
    for (; j < jend; j += ng) add_row(*reinterpret_cast<const u32x4*>(Vcb + (size_t)j * hs + c * 16), Vsb[(size_t)j * nb + (c >> 1)], j);
    if (holds_t && j == t) add_row(*reinterpret_cast<const u32x4*>(s_code + hs + c * 16), s_scale[nb + (c >> 1)], t);
#pragma unroll
    for (int k = 0; k < 8; ++k) { s_o[g * hs + c * 16 + 2 * k] = acc[k].x; s_o[g * hs + c * 16 + 2 * k + 1] = acc[k].y; }
  }
  __syncthreads();
  for (int d = tid; d < hs; d += 256) {
    float o = s_o[d];
    for (int gg = 1; gg < ng; ++gg) o += s_o[gg * hs + d];
    if (nsplit == 1) out_[(size_t)b * C + (size_t)h * hs + d] = pack1<OT>(o / l);
    else part[((size_t)bh * nsplit + sp) * (hs + 2) + d] = o;
  }
  if (nsplit > 1 && tid == 0) {
    part[((size_t)bh * nsplit + sp) * (hs + 2) + hs] = mx;
    part[((size_t)bh * nsplit + sp) * (hs + 2) + hs + 1] = l;
  }
}

template <typename OT>
__global__ __launch_bounds__(256) void gpt_decode_attn_kv8_kernel(const uint16_t* __restrict__ qkv, uint8_t* __restrict__ Kc, uint8_t* __restrict__ Ks,
                                                                  uint8_t* __restrict__ Vc, uint8_t* __restrict__ Vs, int H, int hs, int Tmax, int t,
                                                                  int nsplit, int split_len, float scale, uint16_t* __restrict__ out,
                                                                  float* __restrict__ part) {
  kv8_attn_piece<OT>(qkv, Kc, Ks, Vc, Vs, H, hs, Tmax, t, nsplit, split_len, scale, out, part);
}

template <typename OT>
__global__ __launch_bounds__(128) void gpt_decode_attn_kv8_merge_kernel(const float* __restrict__ part, int H, int hs, int nsplit, void* __restrict__ out) {
  gd_attn_merge<OT, false>(part, H, hs, nsplit, out);
}

// the cursor forms: a grid sized for the whole cache (gridDim.y = (Tmax + 63) / 64 >= every plan's nsplit), the pieces past the plan return
template <typename OT>
__global__ __launch_bounds__(256) void gpt_decode_attn_kv8_at_kernel(const uint16_t* __restrict__ qkv, uint8_t* __restrict__ Kc, uint8_t* __restrict__ Ks,
                                                                     uint8_t* __restrict__ Vc, uint8_t* __restrict__ Vs, int H, int hs, int Tmax,
                                                                     const int* __restrict__ cursor, int t_offset, float scale,
                                                                     uint16_t* __restrict__ out, float* __restrict__ part) {
  const int t = gd_cursor_step(cursor, t_offset, Tmax);
  if (t < 0) return;
  int nsplit, split_len;
  gd_att_plan((int64_t)gridDim.x, t + 1, &nsplit, &split_len);
  if ((int)blockIdx.y >= nsplit) return;
  kv8_attn_piece<OT>(qkv, Kc, Ks, Vc, Vs, H, hs, Tmax, t, nsplit, split_len, scale, out, part);
}

// always launched: under a plan of one piece the main kernel has written out itself
template <typename OT>
__global__ __launch_bounds__(128) void gpt_decode_attn_kv8_merge_at_kernel(const float* __restrict__ part, int H, int hs, int Tmax,
                                                                           const int* __restrict__ cursor, int t_offset, void* __restrict__ out) {
  const int t = gd_cursor_step(cursor, t_offset, Tmax);
  if (t < 0) return;
  int nsplit, split_len;
  gd_att_plan((int64_t)gridDim.x, t + 1, &nsplit, &split_len);
  if (nsplit == 1) return;
  gd_attn_merge<OT, false>(part, H, hs, nsplit, out);
}

// what both entries check; `who` names the entry in the message
static int kv8_check(const char* who, const void* qkv, const uint8_t* k_codes, const uint8_t* k_scales, const uint8_t* v_codes, const uint8_t* v_scales,
                     int B, int H, int hs, int Tmax, const void* out, int dtype) {
  ENH_REQUIRE(qkv && k_codes && k_scales && v_codes && v_scales && out, ENH_E_BADARG, "%s: null pointer", who);
  ENH_REQUIRE(dtype == ENH_DT_BF16 || dtype == ENH_DT_F16, ENH_E_BADARG, "%s: dtype must be ENH_DT_BF16 (0) or ENH_DT_F16 (1), got %d", who, dtype);
  ENH_REQUIRE(B >= 1 && H >= 1 && (int64_t)B * H <= 2147483647LL, ENH_E_BADARG, "%s: B=%d H=%d", who, B, H);
  ENH_REQUIRE(hs >= 64 && hs <= KV8_MAX_HS && hs % 64 == 0, ENH_E_SHAPE, "%s: head size must be a multiple of 64 up to 384, got %d", who, hs);
  ENH_REQUIRE(Tmax >= 1 && Tmax <= GD_ATT_MAX_T, ENH_E_SHAPE, "%s: cache length must be in [1, %d], got %d", who, GD_ATT_MAX_T, Tmax);
  ENH_REQUIRE((((uintptr_t)qkv | (uintptr_t)k_codes | (uintptr_t)v_codes) & 15) == 0, ENH_E_BADARG, "%s: qkv and the code tensors must be 16-byte aligned", who);
  return ENH_OK;
}

extern "C" int enh_decode_attention_kv8(const void* qkv, uint8_t* k_codes, uint8_t* k_scales, uint8_t* v_codes, uint8_t* v_scales, int B, int H, int hs,
                                        int Tmax, int t, void* out, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  const int rc = kv8_check("enh_decode_attention_kv8", qkv, k_codes, k_scales, v_codes, v_scales, B, H, hs, Tmax, out, dtype);
  if (rc != ENH_OK) return rc;
  ENH_REQUIRE(t >= 0 && t < Tmax, ENH_E_BADARG, "enh_decode_attention_kv8: step %d outside the cache of %d slots", t, Tmax);
  int nsplit, split_len;
  gd_att_plan((int64_t)B * H, t + 1, &nsplit, &split_len);
  float* part = nullptr;
  if (nsplit > 1) {
    ENH_REQUIRE(workspace && workspace_bytes >= (size_t)B * H * nsplit * (hs + 2) * sizeof(float), ENH_E_WORKSPACE,
                "enh_decode_attention_kv8: workspace too small");
    part = reinterpret_cast<float*>(workspace);
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * H), (unsigned)nsplit);
  const float scale = 1.0f / sqrtf((float)hs);
  const uint16_t* q = reinterpret_cast<const uint16_t*>(qkv);
  uint16_t* o = reinterpret_cast<uint16_t*>(out);
  enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_decode_attn_kv8_kernel<F16>" : "gpt_decode_attn_kv8_kernel<BF16>");
  ENH_DT_DISPATCH(dtype, (gpt_decode_attn_kv8_kernel<OT><<<grid, 256, 0, s>>>(q, k_codes, k_scales, v_codes, v_scales, H, hs, Tmax, t, nsplit, split_len,
                                                                            scale, o, part)));
  if (nsplit > 1) ENH_DT_DISPATCH(dtype, (gpt_decode_attn_kv8_merge_kernel<OT><<<(unsigned)(B * H), 128, 0, s>>>(part, H, hs, nsplit, out)));
  return enh_check_launch("enh_decode_attention_kv8");
}

extern "C" int enh_decode_attention_kv8_at(const void* qkv, uint8_t* k_codes, uint8_t* k_scales, uint8_t* v_codes, uint8_t* v_scales, int B, int H, int hs,
                                           int Tmax, const int* cursor, int t_offset, void* out, void* workspace, size_t workspace_bytes, int dtype,
                                           void* stream) {
  const int rc = kv8_check("enh_decode_attention_kv8_at", qkv, k_codes, k_scales, v_codes, v_scales, B, H, hs, Tmax, out, dtype);
  if (rc != ENH_OK) return rc;
  ENH_REQUIRE(cursor, ENH_E_BADARG, "enh_decode_attention_kv8_at: null pointer");
  // the plan is not known here: the workspace holds the most pieces any position of the cache can have
  ENH_REQUIRE(workspace && workspace_bytes >= enh_decode_attention_workspace_bytes(B, H, hs, Tmax), ENH_E_WORKSPACE,
              "enh_decode_attention_kv8_at: workspace too small");
  float* part = reinterpret_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * H), (unsigned)((Tmax + 63) / 64));
  const float scale = 1.0f / sqrtf((float)hs);
  const uint16_t* q = reinterpret_cast<const uint16_t*>(qkv);
  uint16_t* o = reinterpret_cast<uint16_t*>(out);
  enh_note_kernel_plain(dtype == ENH_DT_F16 ? "gpt_decode_attn_kv8_at_kernel<F16>" : "gpt_decode_attn_kv8_at_kernel<BF16>");
  ENH_DT_DISPATCH(dtype, (gpt_decode_attn_kv8_at_kernel<OT><<<grid, 256, 0, s>>>(q, k_codes, k_scales, v_codes, v_scales, H, hs, Tmax, cursor, t_offset,
                                                                               scale, o, part)));
  ENH_DT_DISPATCH(dtype, (gpt_decode_attn_kv8_merge_at_kernel<OT><<<(unsigned)(B * H), 128, 0, s>>>(part, H, hs, Tmax, cursor, t_offset, out)));
  return enh_check_launch("enh_decode_attention_kv8_at");
}
