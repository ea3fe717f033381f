// MXFP6 (OCP FP6 E2M3) block quantisation shared by the quantiser, the MXFP6-emitting producers and the FFN1 epilogue
// (gemm_mx_packed.hip, elementwise.hip).  One block = 32 consecutive values of a row along K.  amax = m 2^p (frexp, m in [0.5, 1)); the
// block exponent e = p - 3 + (m > 0.9375) is the smallest integer with amax <= 7.5 2^e, clamped to [-127, 127] and stored as the E8M0
// byte e + 127 (an all-zero block: byte 127, codes 0).  This is mx.h's rule with 7.5 (the largest E2M3 value) in place of 448, so no
// code ever saturates.  Codes: E2M3 of x 2^-e (sign bit 5, 2 exponent bits of bias 1, 3 mantissa bits; subnormals in steps of 0.125),
// round to nearest even.  Everything is integer / exact arithmetic, so every producer writes the same bits.
//
// Packed storage (include/longlive_hip.h): a row of K codes (K % 256 == 0) is 3K/4 bytes, in 192-byte super-blocks of 256 k.  The
// 32-k block j = 0..7 of a super-block (k 32j .. 32j + 31, one scale block) is 24 bytes at byte 48 (j % 4) + 24 (j / 4): code i of
// the block in bits 6i .. 6i + 5 of the little-endian 192-bit word.  So the 48 bytes at 48 g hold blocks g and g + 4: exactly the two
// 16x16x128 MFMA K-steps' fragments of a lane of group g (24 bytes = 6 VGPRs each), one contiguous 48-byte read per row and stage.
#pragma once
#include <stdint.h>

#define MX6_BLOCK 32
#define MX6_SUPER 256                     // k per 192-byte super-block (two MFMA K-steps)
#define MX6_SUPER_BYTES 192

// E8M0 exponent of a block from its maximum magnitude (a finite bf16 value widened to fp32, >= 0)
__host__ __device__ __forceinline__ int mx6_scale_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int p;
  float m = frexpf(amax, &p);
  int e = p - 3 + (m > 0.9375f ? 1 : 0);
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// E2M3 code (6 bits) of x 2^-e (x finite, |x| <= 7.5 2^e by the scale rule); ldexpf by a power of two is exact down to fp32's
// subnormals, far below E2M3's 2^-4 rounding threshold
__host__ __device__ __forceinline__ uint32_t mx6_code(float x, int e) {
  float v = ldexpf(x, -e);
  uint32_t b = __builtin_bit_cast(uint32_t, v);
  uint32_t sign = (b >> 26) & 0x20u;
  float a = fabsf(v);
  uint32_t c;
  if (a >= 1.0f) {                                          // normal range (>= 2^0): round the fp32 mantissa to 3 bits
    uint32_t ab = b & 0x7fffffffu;
    uint32_t r = (ab + 0x7ffffu + ((ab >> 20) & 1u)) >> 20;  // fp32 exponent | 3 mantissa bits, rounded (a carry bumps the exponent)
    c = r - ((127u - 1u) << 3);
    c = c > 0x1fu ? 0x1fu : c;                              // 7.5 (unreachable under the scale rule; kept as a guard)
  } else {                                                  // subnormal: multiples of 0.125 (8 = 1.0 is the smallest normal)
    c = (uint32_t)rintf(a * 8.0f);
  }
  return sign | c;
}

// eight codes of one row (consecutive k) packed into bits 6j .. 6j + 5 of a 48-bit value
__host__ __device__ __forceinline__ uint64_t mx6_pack8(const float (&f)[8], int e) {
  uint64_t w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) w |= (uint64_t)mx6_code(f[j], e) << (6 * j);
  return w;
}

// four codes packed into bits 6j .. 6j + 5 of a 24-bit value
__host__ __device__ __forceinline__ uint32_t mx6_pack4(float x0, float x1, float x2, float x3, int e) {
  return mx6_code(x0, e) | (mx6_code(x1, e) << 6) | (mx6_code(x2, e) << 12) | (mx6_code(x3, e) << 18);
}

// byte offset inside a packed row of the 12 bytes holding k = c16 .. c16 + 15 (c16 % 16 == 0): half c16 / 16 % 2 of 32-k block j
__host__ __device__ __forceinline__ int mx6_chunk_off(int c16) {
  int cg = c16 >> 4, j = (cg >> 1) & 7;
  return (cg >> 4) * MX6_SUPER_BYTES + 48 * (j & 3) + 24 * (j >> 2) + 12 * (cg & 1);
}

#ifdef __HIPCC__
// A 16-k half-block from two lanes of a wave: lane pairs (l, l ^ 1), the even lane holding k 0..7 (lo) of the chunk and the odd one
// k 8..15.  Every lane must call it (shuffles); the even lane of a pair with `store` writes the chunk's three dwords.
__device__ __forceinline__ void mx6_store_pair(uint64_t piece, uint8_t* __restrict__ dst, int lane, bool store) {
  uint32_t lo = (uint32_t)piece, hi = (uint32_t)(piece >> 32);
  uint32_t plo = __shfl_xor(lo, 1, 64), phi = __shfl_xor(hi, 1, 64);
  if (store && (lane & 1) == 0) {
    uint64_t q = ((uint64_t)phi << 32) | plo;               // the odd lane's 48 bits go to bits 48 .. 95
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    d[0] = lo;
    d[1] = (hi & 0xffffu) | ((uint32_t)q << 16);
    d[2] = (uint32_t)(q >> 16);
  }
}
#endif
