// MXFP8 block quantisation shared by the quantiser, the MX-emitting producers and the FFN1 epilogue (gemm_mx.hip, elementwise.hip).
// One block = 32 consecutive values of a row along K.  amax = m 2^p (frexp, m in [0.5, 1)); the block exponent
// e = p - 9 + (m > 0.875) is the smallest integer with amax <= 448 2^e, clamped to [-127, 127] and stored as the E8M0 byte e + 127
// (an all-zero block: byte 127, codes 0).  Codes: OCP e4m3fn of x 2^-e, round to nearest even, subnormals kept, saturated to +-448.
// Everything here is integer / exact arithmetic, so every producer that calls it on the same bf16 values writes the same bytes.
#pragma once
#include <stdint.h>

#define MX_BLOCK 32

// E8M0 byte of a block from its maximum magnitude (a finite bf16 value widened to fp32, >= 0)
__host__ __device__ __forceinline__ int mx_scale_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int p;
  float m = frexpf(amax, &p);
  int e = p - 9 + (m > 0.875f ? 1 : 0);
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// e4m3fn code of x 2^-e (x finite); ldexpf by a power of two is exact down to fp32's subnormals, far below e4m3's 2^-9 step
__host__ __device__ __forceinline__ uint32_t mx_code(float x, int e) {
  float v = ldexpf(x, -e);
  uint32_t b = __builtin_bit_cast(uint32_t, v);
  uint32_t sign = (b >> 24) & 0x80u;
  float a = fabsf(v);
  uint32_t c;
  if (a >= 0.015625f) {                                     // e4m3 normal range (>= 2^-6): round the fp32 mantissa to 3 bits
    uint32_t ab = b & 0x7fffffffu;
    uint32_t r = (ab + 0x7ffffu + ((ab >> 20) & 1u)) >> 20;  // fp32 exponent | 3 mantissa bits, rounded (a carry bumps the exponent)
    c = r - ((127u - 7u) << 3);
    c = c > 0x7eu ? 0x7eu : c;                              // saturate at 448 (0x7f is NaN)
  } else {                                                  // subnormal: multiples of 2^-9 (8 = 2^-6 is the smallest normal)
    c = (uint32_t)rintf(a * 512.0f);
  }
  return sign | c;
}

// four codes packed into a little-endian word (element j in byte j)
__host__ __device__ __forceinline__ uint32_t mx_code4(float x0, float x1, float x2, float x3, int e) {
  return mx_code(x0, e) | (mx_code(x1, e) << 8) | (mx_code(x2, e) << 16) | (mx_code(x3, e) << 24);
}

// ---- FP8 rowwise (ll_quantize_rows_f8 and the producers' f8 forms): one fp32 scale per row, sc = amax / 448 (1 for an all-zero row),
// code = e4m3fn(RNE(clamp(x * (1 / sc), -448, 448))), subnormals kept.  v_cvt_pk_fp8_f32 rounds to nearest even and keeps e4m3
// subnormals but does not saturate (above 448 it writes NaN), hence the clamp; its first operand lands in the low byte.
#define F8_MAX 448.0f

__device__ __forceinline__ float f8_clamp(float v) { return fminf(fmaxf(v, -F8_MAX), F8_MAX); }

// four codes of (already scaled) values packed into a little-endian word (a in byte 0)
__device__ __forceinline__ uint32_t f8_code4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(a), f8_clamp(b), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(c), f8_clamp(d), w, true);
  return (uint32_t)w;
}
