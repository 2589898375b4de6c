// gpt_prefill_cache.hip — what the prefill of stage-2 sampling (sample(prefix_codes=)) needs beyond the kernels of the
// teacher-forced forward: the k / v rows of whole sequences put into the caches of the decode attention, for gfx950.
//
//   enh_kv_cache_fill      the k and v columns of row (b, s) of the packed qkv [B S, 3 H hs] copied bit for bit to slot slot0 + s of
//                          k_cache / v_cache [B, H, Tmax, hs]: what S successive enh_decode_attention calls append, in one launch.
//   enh_kv_cache_fill_kv8  the same rows quantized into an MXFP8 cache with the rounding of enh_decode_attention_kv8's append (mxfp8.h: blocks of 32
//                          along hs), and the DEQUANTIZED values written back over the k and v columns of qkv in the operand format, so that the
//                          prefill's own attention reads what every later step reads from the slot.
//
// Both are copies: a lane moves 16 bytes per request, the 64-bit offsets are formed per lane, nothing is staged, no atomics, no workspace.  The
// kv8 form: a lane owns 16 elements (two 16-byte loads), the two lanes of a block of 32 exchange their maxima by one shuffle; a lane stores its 16
// codes as one 16-byte request and its 16 dequantized values as two, the even lane of a pair the scale byte.
#include "common.h"
#include "mxfp8.h"

#define KF_MAX_HS 384

// item i of the flat grid: 16 bytes of the k | v columns of one row.  vpr: 16-byte vectors per row (2 C es / 16), epv: elements per vector
__global__ __launch_bounds__(256) void kv_cache_fill_kernel(const u32x4* __restrict__ qkv, int64_t total, int vpr, int epv, int S, int H, int hs, int Tmax,
                                                            int slot0, u32x4* __restrict__ Kc, u32x4* __restrict__ Vc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t r = i / vpr;
  const int j = (int)(i - r * vpr);
  const int C = H * hs;
  const int e = j * epv;
  const bool is_v = e >= C;
  const int col = is_v ? e - C : e;
  const int h = col / hs, d = col - h * hs;
  const int64_t b = r / S;
  const int s = (int)(r - b * S);
  const int64_t src = (r * 3 * C + C + e) / epv;
  const int64_t dst = (((b * H + h) * Tmax + slot0 + s) * hs + d) / epv;
  (is_v ? Vc : Kc)[dst] = qkv[src];
}

// item i of the flat grid: 16 elements (half a block of 32) of the k | v columns of one row
template <typename OT>
__global__ __launch_bounds__(256) void kv_cache_fill_kv8_kernel(uint16_t* __restrict__ qkv, int64_t total, int S, int H, int hs, int Tmax, int slot0,
                                                                uint8_t* __restrict__ Kc, uint8_t* __restrict__ Ks, uint8_t* __restrict__ Vc,
                                                                uint8_t* __restrict__ Vs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;      // total is even and a pair starts at an even lane: both lanes of a pair leave or stay
  const int C = H * hs, ipr = C >> 3;      // items per row: 2 C / 16
  const int64_t r = i / ipr;
  const int e = (int)(i - r * ipr) * 16;
  const bool is_v = e >= C;
  const int col = is_v ? e - C : e;
  const int h = col / hs, d = col - h * hs;
  const int64_t b = r / S;
  const int s = (int)(r - b * S);
  uint16_t* src = qkv + r * 3 * C + C + e;
  float f[16];
  {
    float lo[8], hi[8];
    unpack8<OT>(*reinterpret_cast<const u32x4*>(src), lo);
    unpack8<OT>(*reinterpret_cast<const u32x4*>(src + 8), hi);
#pragma unroll
    for (int k = 0; k < 8; ++k) { f[k] = lo[k]; f[8 + k] = hi[k]; }
  }
  uint32_t amax = 0;      // magnitudes order like their bit patterns; a NaN sorts above infinity
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t a = __builtin_bit_cast(uint32_t, f[k]) & 0x7fffffffu;
    amax = a > amax ? a : amax;
  }
  {
    const uint32_t other = (uint32_t)__shfl_xor((int)amax, 1, 64);
    amax = other > amax ? other : amax;
  }
  const int X = mx_block_exponent(amax);
  const uint32_t sb = amax >= 0x7f800000u ? 0xffu : (uint32_t)(X + 127);      // a block that holds an infinity or a NaN: the format's NaN scale
  const float inv = mx_inv_scale(X), sc = mx_scale_f32(sb);
  uint32_t cw[4] = {0u, 0u, 0u, 0u};
  uint32_t back[8];
#pragma unroll
  for (int k = 0; k < 16; k += 2) {
    const uint32_t c0 = mx_e4m3_rne(f[k] * inv), c1 = mx_e4m3_rne(f[k + 1] * inv);
    cw[k >> 2] |= (c0 | (c1 << 8)) << ((k & 2) * 8);
    const f32x2 w = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c0 | (c1 << 8), 1.0f, false);      // the widening of the attention's reads: exact
    back[k >> 1] = pack2<OT>(w.x * sc, w.y * sc);
  }
  const int64_t row = (b * H + h) * Tmax + slot0 + s;
  *reinterpret_cast<u32x4*>((is_v ? Vc : Kc) + row * hs + d) = u32x4{cw[0], cw[1], cw[2], cw[3]};
  if ((d & 31) == 0) (is_v ? Vs : Ks)[row * (hs / MX_BLOCK) + (d >> 5)] = (uint8_t)sb;
  *reinterpret_cast<u32x4*>(src) = u32x4{back[0], back[1], back[2], back[3]};
  *reinterpret_cast<u32x4*>(src + 8) = u32x4{back[4], back[5], back[6], back[7]};
}

// what both entries check; `who` names the entry in the message
static int kf_check(const char* who, int B, int S, int H, int hs, int Tmax, int slot0) {
  ENH_REQUIRE(B >= 1 && S >= 1 && H >= 1, ENH_E_BADARG, "%s: B=%d S=%d H=%d", who, B, S, H);
  ENH_REQUIRE(hs >= 64 && hs <= KF_MAX_HS && hs % 64 == 0, ENH_E_SHAPE, "%s: head size must be a multiple of 64 up to 384, got %d", who, hs);
  ENH_REQUIRE(Tmax >= 1 && slot0 >= 0 && (int64_t)slot0 + S <= Tmax, ENH_E_SHAPE, "%s: slots [%d, %d + %d) outside the cache of %d slots", who, slot0, slot0,
              S, Tmax);
  ENH_REQUIRE((int64_t)H * hs <= (1 << 24), ENH_E_SHAPE, "%s: H hs = %lld columns", who, (long long)H * hs);
  return ENH_OK;
}

extern "C" int enh_kv_cache_fill(const void* qkv, int B, int S, int H, int hs, int Tmax, int slot0, void* k_cache, void* v_cache, int dtype, void* stream) {
  ENH_REQUIRE(qkv && k_cache && v_cache, ENH_E_BADARG, "enh_kv_cache_fill: null pointer");
  ENH_REQUIRE(dtype == ENH_DT_BF16 || dtype == ENH_DT_F16 || dtype == ENH_DT_F32, ENH_E_BADARG,
              "enh_kv_cache_fill: dtype must be ENH_DT_BF16 (0), ENH_DT_F16 (1) or ENH_DT_F32 (2), got %d", dtype);
  const int rc = kf_check("enh_kv_cache_fill", B, S, H, hs, Tmax, slot0);
  if (rc != ENH_OK) return rc;
  ENH_REQUIRE((((uintptr_t)qkv | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0, ENH_E_BADARG, "enh_kv_cache_fill: qkv and the caches must be 16-byte aligned");
  const int epv = dtype == ENH_DT_F32 ? 4 : 8;
  const int vpr = 2 * H * hs / epv;
  const int64_t total = (int64_t)B * S * vpr, blocks = (total + 255) / 256;
  ENH_REQUIRE(blocks <= 2147483647LL, ENH_E_SHAPE, "enh_kv_cache_fill: %lld rows of %d columns are too many for one launch", (long long)B * S, 2 * H * hs);
  enh_note_kernel_plain("kv_cache_fill_kernel");
  kv_cache_fill_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const u32x4*>(qkv), total, vpr, epv, S, H, hs, Tmax, slot0,
                                                                          reinterpret_cast<u32x4*>(k_cache), reinterpret_cast<u32x4*>(v_cache));
  return enh_check_launch("enh_kv_cache_fill");
}

extern "C" int enh_kv_cache_fill_kv8(void* qkv, int B, int S, int H, int hs, int Tmax, int slot0, uint8_t* k_codes, uint8_t* k_scales, uint8_t* v_codes,
                                     uint8_t* v_scales, int dtype, void* stream) {
  ENH_REQUIRE(qkv && k_codes && k_scales && v_codes && v_scales, ENH_E_BADARG, "enh_kv_cache_fill_kv8: null pointer");
  ENH_REQUIRE_DT(dtype, "enh_kv_cache_fill_kv8");
  const int rc = kf_check("enh_kv_cache_fill_kv8", B, S, H, hs, Tmax, slot0);
  if (rc != ENH_OK) return rc;
  ENH_REQUIRE((((uintptr_t)qkv | (uintptr_t)k_codes | (uintptr_t)v_codes) & 15) == 0, ENH_E_BADARG,
              "enh_kv_cache_fill_kv8: qkv and the code tensors must be 16-byte aligned");
  const int64_t total = (int64_t)B * S * (H * hs / 8), blocks = (total + 255) / 256;
  ENH_REQUIRE(blocks <= 2147483647LL, ENH_E_SHAPE, "enh_kv_cache_fill_kv8: %lld rows of %d columns are too many for one launch", (long long)B * S, 2 * H * hs);
  enh_note_kernel("kv_cache_fill_kv8_kernel", dtype);
  ENH_DT_DISPATCH(dtype, (kv_cache_fill_kv8_kernel<OT><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(reinterpret_cast<uint16_t*>(qkv), total, S, H, hs, Tmax,
                                                                                                         slot0, k_codes, k_scales, v_codes, v_scales)));
  return enh_check_launch("enh_kv_cache_fill_kv8");
}
