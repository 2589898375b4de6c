// decode_attn.h — what the decode attentions over a long cache share, stated once: gpt_decode.hip (16-bit and f32 caches) and gpt_decode_kv8.hip
// (MXFP8 caches) cut the cache into the same pieces (gd_att_plan), leave the same (out, max, sum) triples per piece in the workspace and merge them
// with the same body in ascending piece order (gd_attn_merge); their cursor forms read the step the same way (gd_cursor_step).
#pragma once
#include "common.h"
#include <type_traits>

#define GD_ATT_PIECE 256      // cache slots per workgroup of the decode attention (its scores live in LDS)
#define GD_ATT_MAX_T 8192

// pieces of a cache of `len` slots: at most GD_ATT_PIECE slots each, and more, down to 64 slots, while B * H workgroups leave the chip idle.
// Host and device: the cursor kernels plan on the device from the position they read there, with the integers of the host's plan.
__host__ __device__ static inline void gd_att_plan(int64_t BH, int len, int* nsplit, int* split_len) {
  int64_t by_len = (len + GD_ATT_PIECE - 1) / GD_ATT_PIECE;
  int64_t want = (512 + BH - 1) / BH;
  const int64_t most = (len + 63) / 64;
  if (want > most) want = most;
  int64_t ns = by_len > want ? by_len : want;
  if (ns < 1) ns = 1;
  int64_t sl = (len + ns - 1) / ns;
  sl = (sl + 31) / 32 * 32;
  *split_len = (int)sl;
  *nsplit = (int)((len + sl - 1) / sl);
}

// pieces in ascending order under the common maximum: the body of the merge kernels.  part: per (batch, head) pair nsplit records of hs + 2 floats
// (the piece's unnormalised out, its maximum, its sum)
template <typename OT, bool F32>
__device__ __forceinline__ void gd_attn_merge(const float* __restrict__ part, int H, int hs, int nsplit, void* __restrict__ out_) {
  typedef typename std::conditional<F32, float, uint16_t>::type CT;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const float* pp = part + (size_t)bh * nsplit * (hs + 2);
  float mx = -__builtin_inff();
  for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, pp[(size_t)s * (hs + 2) + hs]);
  float l = 0.f;
  for (int s = 0; s < nsplit; ++s) l += pp[(size_t)s * (hs + 2) + hs + 1] * expf(pp[(size_t)s * (hs + 2) + hs] - mx);
  CT* out = reinterpret_cast<CT*>(out_) + (size_t)b * H * hs + (size_t)h * hs;
  for (int d = threadIdx.x; d < hs; d += 128) {
    float o = 0.f;
    for (int s = 0; s < nsplit; ++s) o += pp[(size_t)s * (hs + 2) + d] * expf(pp[(size_t)s * (hs + 2) + hs] - mx);
    const float y = o / l;
    if constexpr (F32) out[d] = y;
    else out[d] = pack1<OT>(y);
  }
}

// the step t = *cursor + t_offset, or -1 when it lies outside the cache: then no workgroup reads or writes anything
__device__ __forceinline__ int gd_cursor_step(const int* __restrict__ cursor, int t_offset, int Tmax) {
  const int64_t t = (int64_t)*cursor + t_offset;
  return t >= 0 && t < Tmax ? (int)t : -1;
}
