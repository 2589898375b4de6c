// embed_row.h — the input row of one sampling step from ids that are already on the device: the body of rq_embed_step_kernel (rq_decode.hip) and of
// its cursor form gpt_embed_at_kernel (gpt_decode.hip), stated once so that the two give the same bits.
#pragma once
#include "common.h"

#define RQ_MAX_DEPTH 8

// One workgroup of 256 threads per row; a thread owns float4 columns c, c + 1024, ...  The n <= 8 embedding rows are added in ascending depth, one
// rounding per addition, then the position row.  An id outside the table is clamped, never followed.
__device__ __forceinline__ void rq_embed_row(const float* __restrict__ table, const int64_t* __restrict__ ids, int n, const float* __restrict__ pos_row, int C,
                                             int V, float* __restrict__ out) {
  const float* rows[RQ_MAX_DEPTH];
#pragma unroll
  for (int j = 0; j < RQ_MAX_DEPTH; ++j) {
    int64_t id = j < n ? ids[j] : 0;
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    rows[j] = table + id * C;
  }
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    f32x4 run = *reinterpret_cast<const f32x4*>(rows[0] + c);
#pragma unroll
    for (int j = 1; j < RQ_MAX_DEPTH; ++j)
      if (j < n) run = run + *reinterpret_cast<const f32x4*>(rows[j] + c);
    *reinterpret_cast<f32x4*>(out + c) = run + *reinterpret_cast<const f32x4*>(pos_row + c);
  }
}
