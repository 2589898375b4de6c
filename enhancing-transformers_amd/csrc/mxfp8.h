// mxfp8.h — the two number formats of the MXFP8 weight operand (OCP Microscaling Formats v1.0), stated once for the quantizer and the product of
// gpt_decode_w8.hip.  Plain integer arithmetic on the bits, host and device, so the rounding is what this file says on either.
//   element: OCP e4m3fn (bias 7, 3 mantissa bits, subnormals at 2^-9, largest finite 448 = 0x7e, 0x7f / 0xff NaN, no infinities; not the fnuz form)
//   scale  : E8M0, byte s = 2^(s - 127), one per 32 consecutive k of a row
#pragma once
#include <stdint.h>

#define MX_BLOCK 32

// the shared exponent X of a block whose largest magnitude has the f32 bits `amax_bits` (sign bit clear): floor(log2 amax) - 8 clamped to
// [-127, 127]; 0 for an all-zero block; -127 for an f32 denormal; 120 when the block holds an infinity (exponent field 255)
__host__ __device__ inline int mx_block_exponent(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int e = (int)(amax_bits >> 23) - 127;      // floor(log2 amax) for normals, -127 for denormals (whose floor is lower still: the clamp's value)
  const int X = e - 8;
  return X < -127 ? -127 : X;                      // e <= 128: the upper clamp never binds
}
// 2^-X for X in [-127, 120] as a normal f32
__host__ __device__ inline float mx_inv_scale(int X) { return __builtin_bit_cast(float, (uint32_t)(127 - X) << 23); }
// 2^(s - 127) of a scale byte; s == 0 is the f32 denormal 2^-127
__host__ __device__ inline float mx_scale_f32(uint32_t s) { return __builtin_bit_cast(float, s ? s << 23 : 0x00400000u); }

// f32 -> e4m3fn, round to nearest even, saturating: |y| > 448 (infinities too) gives +-448, a NaN gives 0x7f with its sign, -0.0 gives 0x80
__host__ __device__ inline uint8_t mx_e4m3_rne(float y) {
  const uint32_t u = __builtin_bit_cast(uint32_t, y);
  const uint32_t sign = (u >> 24) & 0x80u;
  uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint8_t)(sign | 0x7fu);
  if (a > 0x43e00000u) a = 0x43e00000u;            // 448
  if (a < 0x3c800000u) {                           // below 2^-6: a multiple of 2^-9, which is the spacing of f32 at 2^14 (ties to even by the add)
    const float f = __builtin_bit_cast(float, a) + 16384.0f;
    return (uint8_t)(sign | (__builtin_bit_cast(uint32_t, f) - 0x46800000u));
  }
  a += 0x7ffffu + ((a >> 20) & 1u);                // three mantissa bits stay; a carry moves into the exponent
  return (uint8_t)(sign | ((a >> 20) - (120u << 3)));
}
