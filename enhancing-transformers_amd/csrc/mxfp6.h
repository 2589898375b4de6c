// mxfp6.h — the element format and the packing of the MXFP6 weight operand (OCP Microscaling Formats v1.0, FP6 E2M3), stated once for the quantizer
// and the product of gpt_decode_w6.hip.  The block size, the E8M0 scale and its helpers (MX_BLOCK, mx_inv_scale, mx_scale_f32) are mxfp8.h's; the
// shared exponent and the non-finite rule are mxfp4.h's (mx4_block_exponent, mx4_block_is_nan, MX4_NAN_SCALE): e2m3 and e2m1 have the same largest
// exponent, 2.  Plain integer arithmetic on the bits, host and device, so the rounding is what this file says on either.
//   element: OCP e2m3 (sign, 2 exponent bits of bias 1, 3 mantissa bits), code s << 5 | e << 3 | m: m / 8 for e = 0, 2^(e - 1) (1 + m / 8) for
//            e = 1 .. 3; the largest value is 7.5 (code 31); no NaN, no infinity
//   scale  : E8M0 as in mxfp8.h; the byte 0xff is the format's NaN and marks a block whose masters held a NaN or an infinity
//   packing: a row is a sequence of 128-k chunks of MX6_CHUNK_BYTES = 96 bytes; a last chunk that is only partly inside K is stored whole, the
//            codes of k >= K are 0.  Within chunk c, piece q = 0 .. 3 is a 192-bit little-endian integer: bits 0 .. 127 are the chunk's bytes
//            [16 q, 16 q + 16), bits 128 .. 191 its bytes [64 + 8 q, 64 + 8 q + 8).  Position j = 8 i + e of a piece (i = 0 .. 3, e = 0 .. 7)
//            is bits [6 j, 6 j + 6) and holds the code of k = 128 c + 32 i + 8 q + e.
#pragma once
#include "mxfp4.h"

#define MX6_CHUNK_K 128
#define MX6_CHUNK_BYTES 96

// bytes of a row of codes: whole chunks
__host__ __device__ inline int64_t mx6_row_bytes(int64_t K) { return (K + MX6_CHUNK_K - 1) / MX6_CHUNK_K * MX6_CHUNK_BYTES; }

// f32 -> e2m3 in the low six bits, round to nearest even, saturating: |y| > 7.5 gives +-7.5 (the tie 7.75 too), -0.0 gives 0x20.  y is finite.
__host__ __device__ inline uint8_t mx_e2m3_rne(float y) {
  const uint32_t u = __builtin_bit_cast(uint32_t, y);
  const uint32_t sign = (u >> 26) & 0x20u;
  uint32_t a = u & 0x7fffffffu;
  if (a > 0x40f00000u) a = 0x40f00000u;            // 7.5
  if (a < 0x3f800000u) {                           // below 1: a multiple of 1/8, which is the spacing of f32 at 2^20 (ties to even by the add)
    const float f = __builtin_bit_cast(float, a) + 1048576.0f;
    return (uint8_t)(sign | (__builtin_bit_cast(uint32_t, f) - 0x49800000u));
  }
  a += 0x7ffffu + ((a >> 20) & 1u);                // three mantissa bits stay; a carry moves into the exponent
  return (uint8_t)(sign | ((a >> 20) - (126u << 3)));
}

// the 32 codes of a piece, in position order, as its six dwords
__host__ __device__ inline void mx6_pack_piece(const uint8_t (&c)[32], uint32_t (&d)[6]) {
  for (int w = 0; w < 6; ++w) d[w] = 0;
  for (int j = 0; j < 32; ++j) {
    const int bit = 6 * j, w = bit >> 5, s = bit & 31;
    d[w] |= (uint32_t)c[j] << s;
    if (s > 26) d[w + 1] |= (uint32_t)c[j] >> (32 - s);
  }
}
