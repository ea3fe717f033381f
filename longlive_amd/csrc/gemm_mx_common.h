// Pieces shared by the block-scaled GEMM families (gemm_mx.hip: e4m3 operands; gemm_mx_packed.hip: E2M3 / E2M1 operands):
//   * one Fmt* struct per code format: the scale rule, and how the quantiser and the FFN1 epilogue pack and store codes;
//   * the FFN1 GELU epilogue with MX output and the quantiser kernel, each written once over a Fmt;
//   * the host path (checks, launch, gemm / qkv / plan / quantise entries) written once over a family descriptor.
// All families run the same 256(M) x 128(N) tile on 8 waves of 64 x 64 with swapped operands (A := W, B := X), so a lane's
// acc[a][b] holds 4 consecutive N of one row M, as gemm_common.h's epilogues expect.
#pragma once
#include <stdio.h>

#include "gemm_common.h"
#include "mx.h"
#include "mx4.h"
#include "mx6.h"

#define MXG_BM 256
#define MXG_BN 128
#define MXG_GROUP_M 4                        // m-tiles per group of the tile walk (tile_of; gemm.hip's default)

// ---------------------------------------------------------------------------------------------------------------
// Code formats.  Each Fmt* holds the scale rule, the packed global row bytes of K codes (row_bytes, in the caller's integer type)
// and two emitters.  Both store the codes and, on the block's first lane, its E8M0 byte, inside one guarded region, so a lane
// outside the matrix does no address arithmetic.  Every lane must call them (the packed formats shuffle); `lane` goes unused where a
// format needs no shuffle.
//   store8:      the quantiser's 8 codes of chunk c (c % 8 == 0) of row `row` of q [rows, row_bytes(K)]; lanes with `in` store.
//   store_block: the FFN1 epilogue's 2 x 4 codes of this lane (lane group fg of its row's four) in the 32-column block at nb of row
//                m of q [M, row_bytes(N)], g[h] being columns nb + 16 h + 4 fg ..; lanes with m < M and nb < N store.

// E8M0 byte of exponent e for the 32-k block holding column c of row `row` of a [rows, K] matrix
__device__ __forceinline__ void mx_store_scale(uint8_t* qs, int row, int K, int c, int e) {
  qs[(size_t)row * (K / 32) + c / 32] = (uint8_t)(e + 127);
}

struct FmtE4M3 {                             // one byte per code, element k at byte k
  static constexpr int KGRAN = MX_BLOCK;     // the quantiser's K granule
  template <class T>
  static __device__ __forceinline__ T row_bytes(T K) { return K; }
  static __device__ __forceinline__ int scale_exp(float amax) { return mx_scale_exp(amax); }
  static __device__ __forceinline__ void store8(const float (&f)[8], int e, uint8_t* q, uint8_t* qs, int row, int K, int c, int lane,
                                                bool in) {
    if (!in) return;
    *reinterpret_cast<uint2*>(q + (size_t)row * K + c) =
        make_uint2(mx_code4(f[0], f[1], f[2], f[3], e), mx_code4(f[4], f[5], f[6], f[7], e));
    if ((c & 31) == 0) mx_store_scale(qs, row, K, c, e);
  }
  static __device__ __forceinline__ void store_block(const float (&g)[2][4], int e, uint8_t* q, uint8_t* qs, int m, int M, int N, int nb,
                                                     int lane, int fg) {
    if (m < M && nb < N) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        *reinterpret_cast<uint32_t*>(q + (size_t)m * N + nb + h * 16 + fg * 4) = mx_code4(g[h][0], g[h][1], g[h][2], g[h][3], e);
      if (fg == 0) mx_store_scale(qs, m, N, nb, e);
    }
  }
};

struct FmtE2M3 {                             // mx6.h's packed rows
  static constexpr int KGRAN = MX6_SUPER;
  template <class T>
  static __device__ __forceinline__ T row_bytes(T K) { return K / 4 * 3; }
  static __device__ __forceinline__ int scale_exp(float amax) { return mx6_scale_exp(amax); }
  // a 16-k chunk of the packed row on a lane pair
  static __device__ __forceinline__ void store8(const float (&f)[8], int e, uint8_t* q, uint8_t* qs, int row, int K, int c, int lane,
                                                bool in) {
    mx6_store_pair(mx6_pack8(f, e), q + (size_t)row * row_bytes(K) + mx6_chunk_off(c & ~15), lane, in);
    if (in && (c & 31) == 0) mx_store_scale(qs, row, K, c, e);
  }
  // each n-subtile is one 16-k chunk (12 bytes) of the packed row, four codes (24 bits) per lane, and lane group fg < 3 stores dword
  // fg of it, joined with the next group's codes
  static __device__ __forceinline__ void store_block(const float (&g)[2][4], int e, uint8_t* q, uint8_t* qs, int m, int M, int N, int nb,
                                                     int lane, int fg) {
    const size_t rowb = row_bytes((size_t)N);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t piece = mx6_pack4(g[h][0], g[h][1], g[h][2], g[h][3], e);
      uint32_t next = (uint32_t)__shfl((int)piece, (lane + 16) & 63, 64);
      if (m < M && nb < N && fg < 3)
        *reinterpret_cast<uint32_t*>(q + (size_t)m * rowb + mx6_chunk_off(nb + h * 16) + 4 * fg) =
            (piece >> (8 * fg)) | (next << (24 - 8 * fg));
    }
    if (m < M && nb < N && fg == 0) mx_store_scale(qs, m, N, nb, e);
  }
};

struct FmtE2M1 {                             // mx4.h's packed rows
  static constexpr int KGRAN = MX4_SUPER;
  template <class T>
  static __device__ __forceinline__ T row_bytes(T K) { return K / 2; }
  static __device__ __forceinline__ int scale_exp(float amax) { return mx4_scale_exp(amax); }
  // one packed dword
  static __device__ __forceinline__ void store8(const float (&f)[8], int e, uint8_t* q, uint8_t* qs, int row, int K, int c, int lane,
                                                bool in) {
    if (in) {
      *reinterpret_cast<uint32_t*>(q + (size_t)row * row_bytes(K) + mx4_chunk_off(c)) = mx4_pack8(f, e);
      if ((c & 31) == 0) mx_store_scale(qs, row, K, c, e);
    }
  }
  // lane fg holds codes 4 fg .. 4 fg + 3 (h = 0) and 16 + 4 fg .. (h = 1) of the block, 16 bits each.  The block's 16-byte word is
  // four dwords: lane fg even stores dword fg / 2 (its h = 0 codes under lane fg + 1's), lane fg odd dword 2 + fg / 2 (lane fg - 1's
  // h = 1 codes under its own).
  static __device__ __forceinline__ void store_block(const float (&g)[2][4], int e, uint8_t* q, uint8_t* qs, int m, int M, int N, int nb,
                                                     int lane, int fg) {
    const size_t rowb = row_bytes((size_t)N);
    const uint32_t c0 = mx4_pack4(g[0][0], g[0][1], g[0][2], g[0][3], e);
    const uint32_t c1 = mx4_pack4(g[1][0], g[1][1], g[1][2], g[1][3], e);
    const uint32_t o0 = (uint32_t)__shfl_xor((int)c0, 16, 64), o1 = (uint32_t)__shfl_xor((int)c1, 16, 64);
    const uint32_t word = (fg & 1) ? (o1 | (c1 << 16)) : (c0 | (o0 << 16));
    const int dw = (fg & 1) ? 2 + (fg >> 1) : (fg >> 1);
    if (m < M && nb < N) {
      *reinterpret_cast<uint32_t*>(q + (size_t)m * rowb + mx4_chunk_off(nb) + 4 * dw) = word;
      if (fg == 0) mx_store_scale(qs, m, N, nb, e);
    }
  }
};

// FFN1 with MX output: the GELU epilogue's bf16 values, quantised in place.  A 32-column block of row m is the two n-subtiles
// 2p, 2p + 1 of the four lanes with this lane's row (lane & 15): 8 values per lane, block maximum over lanes l ^ 16, l ^ 32.  The
// entry points keep N a multiple of the format's block granule, so a block is wholly inside or outside the matrix.
template <class Fmt>
__device__ __forceinline__ void gemm_epilogue_gelu_mxout(f32x4 (&acc)[4][4], uint8_t* __restrict__ q, uint8_t* __restrict__ qs, int M,
                                                         int N, int mw, int nw, int lane, int fr, int fg,
                                                         const bf16* __restrict__ bias) {
  bf16x4 bv[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int n = nw + a * 16 + fg * 4;
    bv[a] = *reinterpret_cast<const bf16x4*>(bias + (n < N ? n : N - 4));
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int m = mw + b * 16 + fr;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float g[2][4];
      float mx = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = rbf(acc[2 * p + h][b][j] + (float)bv[2 * p + h][j]);
          g[h][j] = rbf(gelu_tanh(v));
          mx = fmaxf(mx, fabsf(g[h][j]));
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const int e = Fmt::scale_exp(mx);
      const int nb = nw + p * 32;                         // first column of the block
      Fmt::store_block(g, e, q, qs, m, M, N, nb, lane, fg);
    }
  }
}

// Quantiser: one thread per 8-element chunk, a 32-element block on 4 consecutive lanes (K % 32 == 0 keeps them in one row).
template <class Fmt>
__device__ __forceinline__ void quantize_mx_body(const bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx) {
  const int cpr = K / 8;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool in = t < (long long)rows * cpr;
  const long long tc = in ? t : 0;
  const int row = (int)(tc / cpr), c = (int)(tc - (long long)row * cpr) * 8;
  bf16x8 v = *reinterpret_cast<const bf16x8*>(x + (size_t)row * ldx + c);
  float f[8], mx = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f[j] = (float)v[j];
    mx = fmaxf(mx, fabsf(f[j]));
  }
  mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
  Fmt::store8(f, Fmt::scale_exp(mx), q, qs, row, K, c, threadIdx.x & 63, in);
}

// ---------------------------------------------------------------------------------------------------------------
// Host path.  A family descriptor F names one GEMM family:
//   F::gemm, F::qkv, F::plan  entry-point names (MX_FAMILY_NAMES), F::kernel the kernel's name in plan strings and traces;
//   F::word                   what messages call the MX output ("MX", "MXFP6", "MXFP4");
//   F::KGRAN, F::NGRAN        granule of K, and of N when the output is MX;
//   F::LDS, F::plan_stage     dynamic LDS bytes, and the plan string's note on the K stage;
//   F::select<EPI, MXOUT>()   the kernel instance.
typedef void (*mx_gemm_kernel_t)(const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, bf16*, uint8_t*, uint8_t*, int, int, int,
                                 int, int, int, EpiArgs);
typedef void (*mx_quant_kernel_t)(const bf16*, uint8_t*, uint8_t*, int, int, int);

#define MX_FAMILY_NAMES(tag)                                                                                     \
  static constexpr const char *gemm = "ll_gemm_" tag, *qkv = "ll_gemm_" tag "_qkv", *plan = "ll_gemm_plan_" tag, \
                              *kernel = "gemm_" tag "_kernel"

template <class F>
static int mx_check(const char* fn, const void* xq, const void* sx, const void* wq, const void* sw, int M, int N, int K, int ldo,
                    int epilogue, const void* bias, const void* res, const void* e, const void* mod, int nmod, int gate_idx,
                    int rows_per_batch, int frame_len) {
  LL_REQUIRE(xq && sx && wq && sw, "%s: codes and scales of both operands are required", fn);
  LL_REQUIRE(K > 0 && K % F::KGRAN == 0, "%s: K=%d must be a positive multiple of %d", fn, K, F::KGRAN);
  LL_REQUIRE(M >= 0, "%s: M=%d", fn, M);
  return check_epilogue(fn, M, N, ldo, epilogue, bias, res, e, mod, nmod, gate_idx, rows_per_batch, frame_len);
}

template <class F>
static int mx_launch(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, bf16* out, uint8_t* qo, uint8_t* so,
                     int M, int N, int K, int ldo, int epilogue, const EpiArgs& ea, hipStream_t s) {
  const int ntm = (M + MXG_BM - 1) / MXG_BM, ntn = (N + MXG_BN - 1) / MXG_BN;
  const mx_gemm_kernel_t k = qo != nullptr                      ? F::template select<LL_EPI_BIAS_GELU, true>()
                             : epilogue == LL_EPI_BIAS          ? F::template select<LL_EPI_BIAS, false>()
                             : epilogue == LL_EPI_BIAS_GELU     ? F::template select<LL_EPI_BIAS_GELU, false>()
                             : epilogue == LL_EPI_BIAS_GATE_RES ? F::template select<LL_EPI_BIAS_GATE_RES, false>()
                                                                : F::template select<LL_EPI_BIAS_RES, false>();
  if (int rc = ll_lds_attr((const void*)k, F::LDS)) return rc;
  hipLaunchKernelGGL(k, dim3(ntm * ntn), dim3(512), F::LDS, s, xq, sx, wq, sw, out, qo, so, M, N, K, ldo, ntm, ntn, ea);
  return LL_OK;
}

template <class F>
static int mx_gemm(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                   uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e,
                   const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream) {
  int rc = mx_check<F>(F::gemm, xq, sx, wq, sw, M, N, K, ldo, epilogue, bias, res, e, mod, nmod, gate_idx, rows_per_batch,
                       frame_len);
  if (rc) return rc;
  LL_REQUIRE((q_out == nullptr) == (s_out == nullptr), "%s: the %s output needs both codes and scales", F::gemm, F::word);
  LL_REQUIRE((out != nullptr) != (q_out != nullptr), "%s: exactly one of out (bf16) and q_out / s_out (%s) is required", F::gemm, F::word);
  if (q_out != nullptr) {
    LL_REQUIRE(epilogue == LL_EPI_BIAS_GELU, "%s: the %s output exists for the GELU epilogue only (epilogue %d)", F::gemm, F::word,
               epilogue);
    LL_REQUIRE(N % F::NGRAN == 0 && ldo == N, "%s: the %s output needs N=%d a multiple of %d and ldo == N", F::gemm, F::word, N, F::NGRAN);
  }
  if (M == 0) return LL_OK;
  EpiArgs ea{(const bf16*)bias, (const bf16*)res, (const bf16*)e, (const bf16*)mod, nullptr, nullptr, nmod, gate_idx,
             rows_per_batch, frame_len, frame_len > 0 && rows_per_batch > 0 ? rows_per_batch / frame_len : 0};
  if (int lrc = mx_launch<F>(xq, sx, wq, sw, (bf16*)out, q_out, s_out, M, N, K, ldo, epilogue, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch(F::gemm);
}

template <class F>
static int mx_gemm_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out, int M,
                       int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset, int write_len,
                       ll_stream stream) {
  int rc = mx_check<F>(F::qkv, xq, sx, wq, sw, M, N, K, ldo, LL_EPI_BIAS, bias, nullptr, nullptr, nullptr, 0, 0, 0, 0);
  if (rc) return rc;
  LL_REQUIRE(out != nullptr, "%s: out is required", F::qkv);
  if (int vrc = check_v_insert(F::qkv, M, N, B, L, S, write_start, roped_offset, write_len, cache_v)) return vrc;
  EpiArgs ea{(const bf16*)bias, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
  set_v_insert(ea, cache_v, N, L, S, write_start, roped_offset, write_len);
  if (int lrc = mx_launch<F>(xq, sx, wq, sw, (bf16*)out, nullptr, nullptr, M, N, K, ldo, LL_EPI_BIAS, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch(F::qkv);
}

template <class F>
static int mx_gemm_plan(int M, int N, int K, char* out, int cap) {
  LL_REQUIRE(out != nullptr && cap > 0, "%s: needs an output buffer", F::plan);
  (void)K;
  int ntm = (M + MXG_BM - 1) / MXG_BM, ntn = (N + MXG_BN - 1) / MXG_BN;
  snprintf(out, (size_t)cap, "%s tile %dx%d%s, %d workgroups, groups of %d m-tiles", F::kernel, MXG_BM, MXG_BN, F::plan_stage, ntm * ntn,
           MXG_GROUP_M);
  return LL_OK;
}

template <class Fmt>
static int mx_quantize(const char* fn, mx_quant_kernel_t k, const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx,
                       ll_stream stream) {
  LL_REQUIRE(x != nullptr && q != nullptr && qs != nullptr, "%s: x, codes and scales are required", fn);
  LL_REQUIRE(K > 0 && K % Fmt::KGRAN == 0, "%s: K=%d must be a positive multiple of %d", fn, K, Fmt::KGRAN);
  LL_REQUIRE(ldx >= K && ldx % 8 == 0, "%s: ldx=%d must be >= K and a multiple of 8", fn, ldx);
  LL_REQUIRE(rows >= 0, "%s: rows=%d", fn, rows);
  if (rows == 0) return LL_OK;
  const long long n = (long long)rows * (K / 8);
  LL_REQUIRE(n < (1LL << 31) * 256, "%s: too large", fn);
  hipLaunchKernelGGL(k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, q, qs, rows, K, ldx);
  return ll_check_launch(fn);
}
