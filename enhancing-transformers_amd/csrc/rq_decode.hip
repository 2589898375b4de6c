// rq_decode.hip — what the stage-2 RQTransformer's sampling loop needs beyond the GPT's decode kernels, for gfx950 (reference
// enhancing/modules/stage2/layers.py: RQTransformer.sample / sample_spatial_step / sample_depth_step 397-547 with one condition token).  Every step of
// either transformer is ONE row per batch element: the Blocks run GPT's decode launches (gpt_decode.hip, gpt_rows.hip), and around them are:
//
//   enh_rq_embed_step             the input row of a step built from codes that are already on the device: the sum of n <= 8 embedding rows in
//                                 ascending depth plus one position row (the spatial input: all D codes of the position before; depth slot d >= 1:
//                                 codes 0 .. d - 1 of this position)
//   enh_short_decode_attention    enh_decode_attention for a cache of Tmax <= 8 slots (the depth transformer's): eight lanes per (row, head) pair,
//                                 32 pairs per workgroup, nothing staged in LDS
// No float atomics; every sum runs in a fixed order: the same bits on every run.
#include "common.h"
#include "embed_row.h"
#include <type_traits>

// ---------------------------------------------------------------------------------------------
// embedding of one step
// ---------------------------------------------------------------------------------------------
// One workgroup per row b.  The row's n ids are read from device memory (ids + b id_stride: a strided view of the [B, T, D] codes the sampler writes, so
// the step follows the draws without a host read) and their embedding rows are added in ascending depth, one rounding per addition, then the position
// row (embed_row.h): the bits of rq_embed_seq_kernel's row for the same codes.  An id outside the table is clamped, never followed.
__global__ __launch_bounds__(256) void rq_embed_step_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids, int64_t id_stride, int n,
                                                            const float* __restrict__ pos_row, int C, int V, float* __restrict__ out) {
  const int64_t b = blockIdx.x;
  rq_embed_row(table, ids + b * id_stride, n, pos_row, C, V, out + b * C);
}

extern "C" int enh_rq_embed_step(const float* table, const int64_t* ids, int64_t id_stride, int n, const float* pos_row, int B, int C, int V, float* out,
                                 void* stream) {
  ENH_REQUIRE(n >= 1 && n <= RQ_MAX_DEPTH, ENH_E_SHAPE, "enh_rq_embed_step: the number of summed codes must be in [1, %d], got %d", RQ_MAX_DEPTH, n);
  ENH_REQUIRE(table && ids && pos_row && out, ENH_E_BADARG, "enh_rq_embed_step: null pointer");
  ENH_REQUIRE(B >= 1 && V >= 1 && id_stride >= n, ENH_E_BADARG, "enh_rq_embed_step: B=%d V=%d id_stride=%lld n=%d", B, V, (long long)id_stride, n);
  ENH_REQUIRE(C >= 4 && C % 4 == 0, ENH_E_SHAPE, "enh_rq_embed_step: C must be a positive multiple of 4, got %d", C);
  enh_note_kernel_plain("rq_embed_step_kernel");
  rq_embed_step_kernel<<<(unsigned)B, 256, 0, (hipStream_t)stream>>>(table, ids, id_stride, n, pos_row, C, V, out);
  return enh_check_launch("enh_rq_embed_step");
}

// ---------------------------------------------------------------------------------------------
// decode attention over a short cache
// ---------------------------------------------------------------------------------------------
template <typename OT, bool F32>
__device__ __forceinline__ void rd_load8(const void* p, float (&f)[8]) {
  if constexpr (F32) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    unpack8<OT>(*reinterpret_cast<const u32x4*>(p), f);
  }
}
template <typename OT, bool F32>
__device__ __forceinline__ void rd_copy8(void* dst, const void* src) {      // the eight elements as they are stored
  if constexpr (F32) {
    reinterpret_cast<f32x4*>(dst)[0] = reinterpret_cast<const f32x4*>(src)[0];
    reinterpret_cast<f32x4*>(dst)[1] = reinterpret_cast<const f32x4*>(src)[1];
  } else {
    *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
  }
}

// The launch shape of rq_short_causal_kernel (rq_prefill.hip) with the arithmetic contract of gpt_decode_attn_kernel.  Eight lanes own one (row, head)
// pair; a workgroup of 256 threads holds 32 pairs, neighbouring groups the neighbouring heads of a row.  Lane g of a group owns columns 64 c + 8 g .. + 7
// of every 64-column chunk c of the head: 16-byte loads (two per chunk in the f32 format), and the eight lanes of a group read whole lines.
//   scores   q . k_j for the slots j <= t in f32 (fmaf, ascending column, chunk after chunk), an xor butterfly over the group's eight lanes, times
//            1 / sqrt(hs); slot t is the step's own k from qkv, never read back from the cache
//   softmax  e_j = expf(s_j - max), kept in f32 (not rounded to the format), l = their sum in ascending j
//   P V      e_j times v_j in f32 (fmaf, ascending j), out = sum / l, rounded once
// The step's k and v are appended at slot t by the lanes that hold them; slots > t are neither read nor written.  The loops over the slots are unrolled
// under a predicate on t, so scores and numerators stay in registers.
template <typename OT, bool F32>
__global__ __launch_bounds__(256) void rq_short_decode_attn_kernel(const void* __restrict__ qkv_, void* __restrict__ Kc_, void* __restrict__ Vc_,
                                                                   int64_t npairs, int H, int hs, int Tmax, int t, float scale, void* __restrict__ out_) {
  typedef typename std::conditional<F32, float, uint16_t>::type CT;
  const int64_t pair = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  if (pair >= npairs) return;      // uniform over the group's eight lanes: the butterfly below stays inside a group
  const int g = threadIdx.x & 7;
  const int64_t b = pair / H;
  const int h = (int)(pair - b * H);
  const int64_t C = (int64_t)H * hs;
  const CT* qp = reinterpret_cast<const CT*>(qkv_) + b * 3 * C + (int64_t)h * hs + g * 8;
  const CT* knew = qp + C;
  const CT* vnew = knew + C;
  CT* Kb = reinterpret_cast<CT*>(Kc_) + pair * Tmax * hs + g * 8;
  CT* Vb = reinterpret_cast<CT*>(Vc_) + pair * Tmax * hs + g * 8;

  float s[RQ_MAX_DEPTH];
#pragma unroll
  for (int j = 0; j < RQ_MAX_DEPTH; ++j) s[j] = 0.f;
  for (int c = 0; c < hs; c += 64) {
    float q[8];
    rd_load8<OT, F32>(qp + c, q);
#pragma unroll
    for (int j = 0; j < RQ_MAX_DEPTH; ++j) {
      if (j <= t) {
        const CT* row = j == t ? knew + c : Kb + (int64_t)j * hs + c;
        float k[8];
        rd_load8<OT, F32>(row, k);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[j] = fmaf(q[e], k[e], s[j]);
      }
    }
    rd_copy8<OT, F32>(Kb + (int64_t)t * hs + c, knew + c);
  }
  float mx = -__builtin_inff();
#pragma unroll
  for (int j = 0; j < RQ_MAX_DEPTH; ++j) {
    if (j <= t) {
      float v = s[j];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      s[j] = v * scale;
      mx = fmaxf(mx, s[j]);
    }
  }
  float l = 0.f;
#pragma unroll
  for (int j = 0; j < RQ_MAX_DEPTH; ++j) {
    if (j <= t) {
      s[j] = expf(s[j] - mx);
      l += s[j];
    }
  }
  CT* op = reinterpret_cast<CT*>(out_) + b * C + (int64_t)h * hs + g * 8;
  for (int c = 0; c < hs; c += 64) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < RQ_MAX_DEPTH; ++j) {
      if (j <= t) {
        const CT* row = j == t ? vnew + c : Vb + (int64_t)j * hs + c;
        float v[8];
        rd_load8<OT, F32>(row, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(s[j], v[e], acc[e]);
      }
    }
    rd_copy8<OT, F32>(Vb + (int64_t)t * hs + c, vnew + c);
    if constexpr (F32) {
      reinterpret_cast<f32x4*>(op + c)[0] = f32x4{acc[0] / l, acc[1] / l, acc[2] / l, acc[3] / l};
      reinterpret_cast<f32x4*>(op + c)[1] = f32x4{acc[4] / l, acc[5] / l, acc[6] / l, acc[7] / l};
    } else {
      const u32x4 pk = {pack2<OT>(acc[0] / l, acc[1] / l), pack2<OT>(acc[2] / l, acc[3] / l), pack2<OT>(acc[4] / l, acc[5] / l),
                        pack2<OT>(acc[6] / l, acc[7] / l)};
      *reinterpret_cast<u32x4*>(op + c) = pk;
    }
  }
}

extern "C" int enh_short_decode_attention(const void* qkv, void* k_cache, void* v_cache, int B, int H, int hs, int Tmax, int t, void* out, int dtype,
                                          void* stream) {
  ENH_REQUIRE(qkv && k_cache && v_cache && out, ENH_E_BADARG, "enh_short_decode_attention: null pointer");
  ENH_REQUIRE(dtype == ENH_DT_BF16 || dtype == ENH_DT_F16 || dtype == ENH_DT_F32, ENH_E_BADARG, "enh_short_decode_attention: dtype must be 0, 1 or 2, got %d",
              dtype);
  ENH_REQUIRE(B >= 1 && H >= 1 && (int64_t)B * H <= 2147483647LL, ENH_E_BADARG, "enh_short_decode_attention: B=%d H=%d", B, H);
  ENH_REQUIRE(hs >= 64 && hs <= 384 && hs % 64 == 0, ENH_E_SHAPE, "enh_short_decode_attention: head size must be a multiple of 64 up to 384, got %d", hs);
  ENH_REQUIRE(Tmax >= 1 && Tmax <= RQ_MAX_DEPTH, ENH_E_SHAPE, "enh_short_decode_attention: cache length must be in [1, %d], got %d", RQ_MAX_DEPTH, Tmax);
  ENH_REQUIRE(t >= 0 && t < Tmax, ENH_E_BADARG, "enh_short_decode_attention: step %d outside the cache of %d slots", t, Tmax);
  const int64_t npairs = (int64_t)B * H;
  const unsigned grid = (unsigned)((npairs + 31) / 32);
  const float scale = 1.0f / sqrtf((float)hs);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == ENH_DT_F32) {
    enh_note_kernel_plain("rq_short_decode_attn_kernel<BF16, true>");
    rq_short_decode_attn_kernel<BF16, true><<<grid, 256, 0, s>>>(qkv, k_cache, v_cache, npairs, H, hs, Tmax, t, scale, out);
  } else {
    enh_note_kernel_plain(dtype == ENH_DT_F16 ? "rq_short_decode_attn_kernel<F16, false>" : "rq_short_decode_attn_kernel<BF16, false>");
    ENH_DT_DISPATCH(dtype, (rq_short_decode_attn_kernel<OT, false><<<grid, 256, 0, s>>>(qkv, k_cache, v_cache, npairs, H, hs, Tmax, t, scale, out)));
  }
  return enh_check_launch("enh_short_decode_attention");
}
