// MXFP4 (OCP FP4 E2M1) block quantisation of the W4A6 block linears' weights (gemm_mx_packed.hip).  One block = 32 consecutive values of a
// row along K.  amax = m 2^p (frexp, m in [0.5, 1)); the block exponent e = p - 3 + (m > 0.75) is the smallest integer with
// amax <= 6 2^e, clamped to [-127, 127] and stored as the E8M0 byte e + 127 (an all-zero block: byte 127, codes 0).  This is mx6.h's
// rule with 6 (the largest E2M1 value) in place of 7.5, so no code ever saturates.  Codes: E2M1 of x 2^-e (sign bit 3, 2 exponent bits
// of bias 1, 1 mantissa bit; values 0, 0.5, 1, 1.5, 2, 3, 4, 6), round to nearest even, the subnormal 0.5 included.  Integer / exact
// arithmetic as in mx6.h, so every producer writes the same bits; a negative value that rounds to zero keeps its sign bit (code 8).
//
// Packed storage (include/longlive_hip.h): a row of K codes (K % 256 == 0) is K/2 bytes, in 128-byte super-blocks of 256 k.  The
// 32-k block j = 0..7 of a super-block (k 32j .. 32j + 31, one scale block) is 16 bytes at byte 32 (j % 4) + 16 (j / 4): code i of
// the block in bits 4i .. 4i + 3 of the little-endian 128-bit word (byte i / 2, the low nibble for even i).  So the 32 bytes at 32 g
// hold blocks g and g + 4: exactly the two 16x16x128 MFMA K-steps' fragments of a lane of group g (16 bytes = 4 VGPRs each), two
// ds_read_b128 per row and stage.
#pragma once
#include <stdint.h>

#define MX4_BLOCK 32
#define MX4_SUPER 256                     // k per 128-byte super-block (two MFMA K-steps)
#define MX4_SUPER_BYTES 128

// E8M0 exponent of a block from its maximum magnitude (a finite bf16 value widened to fp32, >= 0)
__host__ __device__ __forceinline__ int mx4_scale_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int p;
  float m = frexpf(amax, &p);
  int e = p - 3 + (m > 0.75f ? 1 : 0);
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// E2M1 code (4 bits) of x 2^-e (x finite, |x| <= 6 2^e by the scale rule); ldexpf by a power of two is exact down to fp32's
// subnormals, far below E2M1's 2^-2 rounding threshold
__host__ __device__ __forceinline__ uint32_t mx4_code(float x, int e) {
  float v = ldexpf(x, -e);
  uint32_t b = __builtin_bit_cast(uint32_t, v);
  uint32_t sign = (b >> 28) & 0x8u;
  float a = fabsf(v);
  uint32_t c;
  if (a >= 1.0f) {                                          // normal range (>= 2^0): round the fp32 mantissa to 1 bit
    uint32_t ab = b & 0x7fffffffu;
    uint32_t r = (ab + 0x1fffffu + ((ab >> 22) & 1u)) >> 22;  // fp32 exponent | 1 mantissa bit, rounded (a carry bumps the exponent)
    c = r - ((127u - 1u) << 1);
    c = c > 0x7u ? 0x7u : c;                                // 6 (unreachable above it under the scale rule; kept as a guard)
  } else {                                                  // subnormal: multiples of 0.5 (2 = 1.0 is the smallest normal)
    c = (uint32_t)rintf(a * 2.0f);
  }
  return sign | c;
}

// eight codes of one row (consecutive k) packed into bits 4j .. 4j + 3 of a dword
__host__ __device__ __forceinline__ uint32_t mx4_pack8(const float (&f)[8], int e) {
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) w |= mx4_code(f[j], e) << (4 * j);
  return w;
}

// four codes packed into bits 4j .. 4j + 3 of a 16-bit value
__host__ __device__ __forceinline__ uint32_t mx4_pack4(float x0, float x1, float x2, float x3, int e) {
  return mx4_code(x0, e) | (mx4_code(x1, e) << 4) | (mx4_code(x2, e) << 8) | (mx4_code(x3, e) << 12);
}

// byte offset inside a packed row of the 4 bytes holding k = c8 .. c8 + 7 (c8 % 8 == 0): quarter c8 / 8 % 4 of 32-k block j
__host__ __device__ __forceinline__ int mx4_chunk_off(int c8) {
  int j = (c8 >> 5) & 7;
  return (c8 >> 8) * MX4_SUPER_BYTES + 32 * (j & 3) + 16 * (j >> 2) + 4 * ((c8 >> 3) & 3);
}
