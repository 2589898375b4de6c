// mxfp4.h — the element format of the MXFP4 weight operand (OCP Microscaling Formats v1.0), stated once for the quantizer and the product of
// gpt_decode_w4.hip.  The block size, the E8M0 scale and its helpers (MX_BLOCK, mx_inv_scale, mx_scale_f32) are mxfp8.h's.  Plain integer
// arithmetic on the bits, host and device, so the rounding is what this file says on either.
//   element: OCP e2m1 (sign, 2 exponent bits of bias 1, 1 mantissa bit): codes 0 .. 7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6; no NaN, no infinity
//   packing: two codes per byte, k even in the low nibble, k odd in the high nibble
//   scale  : E8M0 as in mxfp8.h; the byte 0xff is the format's NaN and marks a block whose masters held a NaN or an infinity
#pragma once
#include "mxfp8.h"

#define MX4_NAN_SCALE 0xffu

// the shared exponent X of a block whose largest magnitude has the f32 bits `amax_bits` (sign bit clear): floor(log2 amax) - 2 clamped to
// [-127, 127]; 0 for an all-zero block; -127 for an f32 denormal and for amax < 2^-125.  A finite amax gives X <= 125, so 2^-X is a normal f32.
// Non-finite masters (exponent field 255) are the caller's to catch: the block's scale byte is MX4_NAN_SCALE and its codes are all zero.
__host__ __device__ inline bool mx4_block_is_nan(uint32_t amax_bits) { return amax_bits >= 0x7f800000u; }
__host__ __device__ inline int mx4_block_exponent(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int X = (int)(amax_bits >> 23) - 127 - 2;
  return X < -127 ? -127 : X;
}

// f32 -> e2m1 in the low nibble, round to nearest even, saturating: |y| > 6 gives +-6, -0.0 gives 0x8.  y is finite.
__host__ __device__ inline uint8_t mx_e2m1_rne(float y) {
  const uint32_t u = __builtin_bit_cast(uint32_t, y);
  const uint32_t sign = (u >> 28) & 0x8u;
  uint32_t a = u & 0x7fffffffu;
  if (a > 0x40c00000u) a = 0x40c00000u;            // 6
  if (a < 0x3f800000u) {                           // below 1: a multiple of 0.5, which is the spacing of f32 at 2^22 (ties to even by the add)
    const float f = __builtin_bit_cast(float, a) + 4194304.0f;
    return (uint8_t)(sign | (__builtin_bit_cast(uint32_t, f) - 0x4a800000u));
  }
  a += 0x1fffffu + ((a >> 22) & 1u);               // one mantissa bit stays; a carry moves into the exponent
  return (uint8_t)(sign | ((a >> 22) - (126u << 1)));
}
