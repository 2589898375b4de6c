// gpt_adam.hip — the optimizer step of the stage-2 GPT (reference modules/stage2/transformer.py:132-194): torch.optim.Adam(betas = (0.9, 0.96)) with two
// parameter groups (L2 weight decay 0.01 on the Linear weights, none elsewhere) over ONE flat f32 buffer, in one launch, driven by a device segment table.
//
//   enh_adam_step_segments       the step: p, m, v updated in place, the new p also written in the 16-bit operand format into an operand arena
//   enh_adam_step_segments_s16   the same step with m and v held as bf16 and stored with stochastic rounding: 22 bytes per element (see below)
//
// Per element, in f32 (gscale = grad_scale / *loss_scale * *clip_coef, formed once per thread):
//   gg = g gscale;  gg = clamp(gg, +-clip_value) if clip_value > 0;  gg += wd_seg p                      (L2 decay: part of the gradient, unlike AdamW)
//   m  = m + (gg - m) (1 - b1)                                                                           (torch's exp_avg.lerp_(grad, 1 - beta1))
//   v  = v b2 + (gg gg) (1 - b2)
//   p  = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))                                                (true divisions, as torch's addcdiv_)
// 1 - b1 and 1 - b2 are formed in double on the host and passed as floats.  bc1 = 1 - b1^t and bc2 = 1 - b2^t come from DEVICE state {t, b1^t, b2^t}
// (doubles): a one-workgroup launch advances it only when the step is not dropped (found_inf == 0), the way torch.cuda.amp.GradScaler leaves the
// optimizer's step count alone when it skips — the host never learns of a skip, so it cannot count.  A dropped step writes nothing at all.
//
// Segment table: `nseg` entries {begin, end, dst16, wd} sorted by begin, disjoint, every bound a multiple of 64 elements (GPT._flat_grads' layout), so
// the 4 consecutive elements one thread handles (and the 8 of a lane pair) never straddle two segments; a workgroup's tile and a wave may.  Elements
// outside every segment (padding) are never written.  dst16 >= 0: element e of the segment is also written, rounded to nearest even, to arena[dst16 + e - begin] (query, key and value
// land as the rows of one [3C, C] operand this way); arena elements that are no destination are never written.
//
// One launch whatever the number of parameters: a fixed grid of workgroups in a grid-stride loop over 4096-element tiles (adjacent workgroups stream
// adjacent tiles; a thread's four 16-byte groups of a tile are 4 KiB apart, so every wave access is one contiguous KiB).  A thread finds the
// segment of its first group by one binary search (the same for the whole workgroup: scalar loads) and then keeps the segment in registers — its groups
// ascend, so it only ever moves the cursor forward, one table entry per crossing: at most nseg entries per thread in the whole launch (~340 against
// ~1300 tiles per workgroup at the shipped size).
//
// Memory: 30 bytes per element, every byte touched once per step and far more of them than any cache holds -> 16-byte non-temporal loads and stores,
// the policy the MI355X guides give for streamed-once data (nt weight streams 6.5-6.8 TB/s against 6.4 default), confirmed on this kernel at 1.07 G
// elements (profiles/gpt_train.txt): plain / plain 5.82 ms, nt loads 5.91, nt stores 5.76, both 5.44.  The 16-bit image is written with 16-byte
// stores as well: two neighbouring lanes exchange their packed halves.  int64 element indices throughout.  No atomics.
//
// bf16 moments (the kernel is one template over the moments' type; the f32 instantiation is bit for bit what it was): the old moments are widened
// exactly, gg, m, v and p are computed as above — p from the UNROUNDED new moments — and only the stored m16 / v16 are rounded, stochastically, with
// one Philox4x32-10 call per 4-element group keyed by the caller's seed and counted by (group, applied steps): include/enh_hip.h has the rule.  A
// group's moments are one 8-byte non-temporal access per array; 16-byte accesses through the lane-pair exchange measured the same
// (profiles/gpt_train_adam16.txt: 42.14 against 42.25 ms at 10.7 G elements), so the simpler form is the one kept.
#include "common.h"
#include <math.h>

#define GA_THREADS 256
#define GA_VEC 4                                          // elements per thread and group: one 16-byte access per f32 array, perfectly coalesced
#define GA_UNROLL 4                                       // groups per thread and tile, all of their loads in flight before the first use
#define GA_TILE (GA_THREADS * GA_VEC * GA_UNROLL)         // 4096 elements
#define GA_WG_PER_CU 8

struct ga_seg { int64_t begin, end, dst16; float wd; int32_t pad; };      // 32 bytes: what enhancing/_C.py adam_segment_table packs

__global__ void gpt_adam_advance_kernel(double* __restrict__ state, const float* __restrict__ found_inf, double b1, double b2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (found_inf && *found_inf != 0.f) return;
  state[0] += 1.0; state[1] *= b1; state[2] *= b2;
}

__device__ __forceinline__ f32x4 ga_load(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
__device__ __forceinline__ void ga_store(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }

// ---- bf16 moments (enh_adam_step_segments_s16): a group's four moments are one 8-byte access; widened exactly, stored with stochastic rounding ----
__device__ __forceinline__ f32x4 ga_load(const uint16_t* p) {
  const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
  return f32x4{__builtin_bit_cast(float, w[0] << 16), __builtin_bit_cast(float, w[0] & 0xffff0000u), __builtin_bit_cast(float, w[1] << 16),
               __builtin_bit_cast(float, w[1] & 0xffff0000u)};
}
// the stored rounding of include/enh_hip.h: (u + r) >> 16 on the f32 bits, r a 16-bit word; a carry into the exponent's all-ones stops at the largest
// finite bf16; an inf is truncated (exact), a nan is truncated with its quiet bit set.  Integer arithmetic only: the same through subnormals.
__device__ __forceinline__ uint32_t ga_round16(float x, uint32_t r) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x), a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) return (u >> 16) | (a > 0x7f800000u ? 0x40u : 0u);
  const uint32_t h = (u + r) >> 16;      // a + r < 0x7f810000: the sign bit is never reached
  return (h & 0x7fffu) >= 0x7f80u ? (h & 0x8000u) | 0x7f7fu : h;
}
// r: word k serves element k of the group, its low half (k = 0: m) or high half (k = 1: v)
template <int HALF>
__device__ __forceinline__ void ga_store(uint16_t* p, f32x4 x, u32x4 r) {
  uint32_t h[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = ga_round16(x[k], HALF ? r[k] >> 16 : r[k] & 0xffffu);
  __builtin_nontemporal_store(u32x2{h[0] | (h[1] << 16), h[2] | (h[3] << 16)}, reinterpret_cast<u32x2*>(p));
}

// ST: the moments' type.  float: enh_adam_step_segments (sr_seed, sr_words unused).  uint16_t: bf16 bits, enh_adam_step_segments_s16.
template <typename OT, typename ST>
__global__ __launch_bounds__(GA_THREADS) void gpt_adam_segments_kernel(float* __restrict__ p, const float* __restrict__ g, ST* __restrict__ m,
                                                                       ST* __restrict__ v, int64_t n, uint16_t* __restrict__ arena, int64_t arena_n,
                                                                       const ga_seg* __restrict__ seg, int nseg, const double* __restrict__ state,
                                                                       int64_t ntiles, float lr, float omb1, float b2, float omb2, float eps,
                                                                       float gscale, const float* __restrict__ skip, const float* __restrict__ loss_scale,
                                                                       const float* __restrict__ clip_coef, float clip_value, uint64_t sr_seed,
                                                                       const uint32_t* __restrict__ sr_words) {
  constexpr bool S16 = sizeof(ST) == 2;
  if (skip && *skip != 0.f) return;
  if ((int64_t)blockIdx.x >= ntiles) return;
  const float step_size = (float)((double)lr / (1.0 - state[1]));
  const float bc2_sqrt = (float)sqrt(1.0 - state[2]);
  if (loss_scale) gscale /= *loss_scale;      // GradScaler's unscale (a power of two: exact)
  if (clip_coef) gscale *= *clip_coef;
  const bool odd = threadIdx.x & 1;

  // the first segment that ends behind the workgroup's first element: one search per launch, the same for the whole workgroup
  const int64_t e0 = (int64_t)blockIdx.x * GA_TILE;
  int lo = 0, hi = nseg;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid].end > e0) hi = mid; else lo = mid + 1;
  }
  int si = lo;
  const int64_t NONE = 0x7fffffffffffffffLL;
  int64_t cb = NONE, ce = NONE, cd = -1;
  float cw = 0.f;
  if (si < nseg) { const ga_seg s = seg[si]; cb = s.begin; ce = s.end; cd = s.dst16; cw = s.wd; }

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {      // adjacent workgroups stream adjacent tiles
    int64_t e[GA_UNROLL];
    f32x4 pv[GA_UNROLL], gv[GA_UNROLL], mv[GA_UNROLL], vv[GA_UNROLL];
    bool in[GA_UNROLL];
#pragma unroll
    for (int u = 0; u < GA_UNROLL; ++u) {
      e[u] = tile * GA_TILE + ((int64_t)u * GA_THREADS + threadIdx.x) * GA_VEC;
      in[u] = e[u] + GA_VEC <= n;
      pv[u] = gv[u] = mv[u] = vv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (in[u]) { pv[u] = ga_load(p + e[u]); gv[u] = ga_load(g + e[u]); mv[u] = ga_load(m + e[u]); vv[u] = ga_load(v + e[u]); }
    }
    u32x2 pk[GA_UNROLL];
    int64_t dst[GA_UNROLL];
#pragma unroll
    for (int u = 0; u < GA_UNROLL; ++u) {
      while (si < nseg && e[u] >= ce) {      // forward only: this thread's groups ascend; at most nseg entries are read in the whole launch
        ++si;
        if (si < nseg) { const ga_seg s = seg[si]; cb = s.begin; ce = s.end; cd = s.dst16; cw = s.wd; }
        else { cb = NONE; ce = NONE; cd = -1; }
      }
      const bool live = in[u] && e[u] >= cb && e[u] + GA_VEC <= ce;      // else padding, or behind the last segment: nothing is written
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pp = pv[u][k], mm = mv[u][k], sq = vv[u][k];
        float gg = gv[u][k] * gscale;
        if (clip_value > 0.f) gg = gg > clip_value ? clip_value : (gg < -clip_value ? -clip_value : gg);      // a nan stays a nan
        gg = gg + cw * pp;
        mm = mm + (gg - mm) * omb1;
        sq = sq * b2 + (gg * gg) * omb2;
        const float denom = sqrtf(sq) / bc2_sqrt + eps;
        pp = pp - step_size * (mm / denom);
        pv[u][k] = pp; mv[u][k] = mm; vv[u][k] = sq;
      }
      if constexpr (S16) {
        if (live) {      // p came from the unrounded moments above; only what the next step reads is rounded.  One Philox call per 4-element group
          const uint64_t G = (uint64_t)e[u] / GA_VEC, t = (uint64_t)state[0];
          const u32x4 r = sr_words ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(sr_words + e[u]))
                                   : philox4x32_10((uint32_t)sr_seed, (uint32_t)(sr_seed >> 32),
                                                   u32x4{(uint32_t)G, (uint32_t)(G >> 32), (uint32_t)t, (uint32_t)(t >> 32)});
          ga_store(p + e[u], pv[u]); ga_store<0>(m + e[u], mv[u], r); ga_store<1>(v + e[u], vv[u], r);
        }
      } else {
        if (live) { ga_store(p + e[u], pv[u]); ga_store(m + e[u], mv[u]); ga_store(v + e[u], vv[u]); }
      }
      pk[u] = u32x2{pack2<OT>(pv[u][0], pv[u][1]), pack2<OT>(pv[u][2], pv[u][3])};
      dst[u] = live && cd >= 0 ? cd + (e[u] - cb) : -1;
    }
    // 16-bit image: lanes 2k and 2k + 1 hold 8 consecutive elements of one segment (bounds are multiples of 64).  They swap halves so that the even lane
    // writes the 16 bytes of group 2q and the odd lane those of group 2q + 1: 16-byte stores, every lane in both exchanges
#pragma unroll
    for (int q = 0; q < GA_UNROLL / 2; ++q) {
      const u32x2 a = pk[2 * q], b = pk[2 * q + 1];
      const u32x2 send = odd ? a : b;
      const u32x2 recv = {(unsigned)__shfl_xor((int)send[0], 1, 64), (unsigned)__shfl_xor((int)send[1], 1, 64)};
      const int64_t d = odd ? dst[2 * q + 1] - GA_VEC : dst[2 * q];      // the 8-element group begins at the even lane's element
      const bool wr = odd ? dst[2 * q + 1] >= 0 : dst[2 * q] >= 0;
      if (wr && d >= 0 && d + 2 * GA_VEC <= arena_n) {
        const u32x4 out = odd ? u32x4{recv[0], recv[1], b[0], b[1]} : u32x4{a[0], a[1], recv[0], recv[1]};
        __builtin_nontemporal_store(out, reinterpret_cast<u32x4*>(arena + d));
      }
    }
  }
}

template <typename ST>
static int ga_launch(const char* what, float* p, const float* g, ST* m, ST* v, int64_t n, enh_h16* arena, int64_t arena_n, const void* segments, int nseg,
                     double* state, float lr, double beta1, double beta2, float eps, float grad_scale, const float* skip_flag,
                     const float* loss_scale_dev, const float* clip_coef_dev, float clip_value, uint64_t sr_seed, const uint32_t* sr_words, int dtype,
                     void* stream) {
  ENH_REQUIRE(dtype == ENH_DT_BF16 || dtype == ENH_DT_F16, ENH_E_BADARG, "%s: dtype must be ENH_DT_BF16 (0) or ENH_DT_F16 (1), got %d", what, dtype);
  ENH_REQUIRE(p && g && m && v && segments && state && n > 0 && nseg >= 1 && arena_n >= 0 && (arena || arena_n == 0) && clip_value >= 0.f, ENH_E_BADARG,
              "%s: bad argument", what);
  ENH_REQUIRE(n % 64 == 0 && arena_n % 8 == 0, ENH_E_SHAPE, "%s: n must be a multiple of 64 and arena_n of 8 (n=%lld arena_n=%lld)", what, (long long)n,
              (long long)arena_n);
  ENH_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)arena | (uintptr_t)segments | (uintptr_t)sr_words) & 15) == 0 &&
                  ((uintptr_t)state & 7) == 0,
              ENH_E_BADARG, "%s: p, g, m, v, arena, the segment table and the injected words must be 16-byte aligned", what);
  ENH_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.f, ENH_E_BADARG, "%s: betas in [0, 1), eps >= 0", what);
  hipStream_t s = (hipStream_t)stream;
  const int64_t ntiles = (n + GA_TILE - 1) / GA_TILE;
  const int64_t want = (int64_t)enh_cu_budget() * GA_WG_PER_CU;
  const int64_t grid = ntiles < want ? ntiles : want;
  gpt_adam_advance_kernel<<<1, 64, 0, s>>>(state, skip_flag, beta1, beta2);
  enh_note_kernel(sizeof(ST) == 2 ? "gpt_adam_segments_s16_kernel" : "gpt_adam_segments_kernel", dtype);
  ENH_DT_DISPATCH(dtype, (gpt_adam_segments_kernel<OT, ST><<<(unsigned)grid, GA_THREADS, 0, s>>>(
      p, g, m, v, n, (uint16_t*)arena, arena_n, (const ga_seg*)segments, nseg, state, ntiles, lr, (float)(1.0 - beta1), (float)beta2,
      (float)(1.0 - beta2), eps, grad_scale, skip_flag, loss_scale_dev, clip_coef_dev, clip_value, sr_seed, sr_words)));
  return enh_check_launch(what);
}

extern "C" int enh_adam_step_segments(float* p, const float* g, float* m, float* v, int64_t n, enh_h16* arena, int64_t arena_n, const void* segments,
                                      int nseg, double* state, float lr, double beta1, double beta2, float eps, float grad_scale,
                                      const float* skip_flag, const float* loss_scale_dev, const float* clip_coef_dev, float clip_value, int dtype,
                                      void* stream) {
  return ga_launch<float>("enh_adam_step_segments", p, g, m, v, n, arena, arena_n, segments, nseg, state, lr, beta1, beta2, eps, grad_scale, skip_flag,
                          loss_scale_dev, clip_coef_dev, clip_value, 0, nullptr, dtype, stream);
}

extern "C" int enh_adam_step_segments_s16(float* p, const float* g, uint16_t* m16, uint16_t* v16, int64_t n, enh_h16* arena, int64_t arena_n,
                                          const void* segments, int nseg, double* state, float lr, double beta1, double beta2, float eps,
                                          float grad_scale, const float* skip_flag, const float* loss_scale_dev, const float* clip_coef_dev,
                                          float clip_value, uint64_t sr_seed, const uint32_t* sr_words, int dtype, void* stream) {
  return ga_launch<uint16_t>("enh_adam_step_segments_s16", p, g, m16, v16, n, arena, arena_n, segments, nseg, state, lr, beta1, beta2, eps, grad_scale,
                             skip_flag, loss_scale_dev, clip_coef_dev, clip_value, sr_seed, sr_words, dtype, stream);
}
