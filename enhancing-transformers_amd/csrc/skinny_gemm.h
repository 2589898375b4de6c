// skinny_gemm.h — what the weight-streaming products of a decode step share, whatever format W is stored in (gpt_decode.hip: 16-bit W,
// gpt_decode_w8.hip: MXFP8 W): the limits, the epilogue, the K-slab plan and the body of the slab pass.  Each file wraps the slab pass in a kernel
// of its own name.
#pragma once
#include "common.h"

#define GD_MAX_M 64
#define GD_MAX_SPLITS 32

__device__ __forceinline__ float gd_epilogue(float v, int64_t m, int64_t n, int64_t N, const float* __restrict__ bias, int act, const float* __restrict__ res) {
  if (bias) v += bias[n];
  if (act) { v = fmaxf(v, 0.f); v = v * v; }
  if (res) v += res[m * N + n];
  return v;
}
template <typename OT>
__device__ __forceinline__ void gd_store(float v, int64_t i, float* __restrict__ out_f32, uint16_t* __restrict__ out_h16) {
  if (out_f32) out_f32[i] = v;
  if (out_h16) out_h16[i] = pack1<OT>(v);
}

// the slab pass: element i of the result is the slabs' partial sums added in ascending slab order, then the epilogue
template <typename OT>
__device__ __forceinline__ void gd_reduce_slabs(const float* __restrict__ part, int splits, int M, int N, const float* __restrict__ bias, int act,
                                                const float* __restrict__ res, float* __restrict__ out_f32, uint16_t* __restrict__ out_h16) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t MN = (int64_t)M * N;
  if (i >= MN) return;
  float v = part[i];
  for (int s = 1; s < splits; ++s) v += part[(int64_t)s * MN + i];
  const int64_t m = i / N, n = i - m * N;
  gd_store<OT>(gd_epilogue(v, m, n, N, bias, act, res), i, out_f32, out_h16);
}

// K chunks per slab and the slab count: a function of (N, K) alone
static inline void gd_gemm_plan(int64_t N, int64_t K, int* chunks_per_split, int* splits) {
  const int64_t tiles = (N + 15) / 16, nchunks = (K + 127) / 128;
  int64_t s = 768 / tiles;                // about three 4-wave workgroups per CU
  if (s > nchunks / 4) s = nchunks / 4;   // a wave keeps at least one chunk
  if (s > GD_MAX_SPLITS) s = GD_MAX_SPLITS;
  if (s < 1) s = 1;
  const int64_t cps = (nchunks + s - 1) / s;
  *chunks_per_split = (int)cps;
  *splits = (int)((nchunks + cps - 1) / cps);
}
