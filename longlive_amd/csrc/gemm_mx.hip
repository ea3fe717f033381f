// MXFP8 block linears on the block-scaled MFMA of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4, both operands e4m3fn):
//   out[M,N] = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias)
// with e4m3fn codes X [M,K] / W [N,K] and one E8M0 scale byte per row and 32-element block of K (mx.h).  The rescale happens inside
// the MFMA, so the epilogues are the bf16 GEMM's (gemm_common.h), bit for bit the same arithmetic on the fp32 accumulator.
//
// Structure (gemm.hip's v2 tile with a 2-stage ring): 256(M) x 128(N) per workgroup, 8 waves of 64 x 64, LDS rows of 128 bytes
// (= 128 k = one MFMA K-step) staged by LDS-DMA with the chunk XOR swizzle of gemm_common.h; operands SWAPPED (A := W, B := X) so
// that a lane's accumulator holds 4 consecutive N of one row M, as the shared epilogues expect.
// Operand map of the 16x16x128 f8f6f4 MFMA with e4m3 operands: lane l holds row l & 15 of its operand, g = l >> 4: bytes 0-15 of its
// fragment are k = 16 g .. 16 g + 15 and bytes 16-31 are k = 64 + 16 g .. + 15 (two 16-byte chunks of the 128-byte row, g and g + 4),
// while its scale VGPR carries, in byte 0 (op_sel 0), the E8M0 byte of (row l & 15, K-block g) = k 32 g .. 32 g + 31.  A fragment of
// 32 consecutive k per lane would pair the right products under the wrong scales.  tests/test_mx_gpu.py checks the map with exact
// data, distinct power-of-two scales per (row, K-block) and an asymmetric B.
// Scales are read straight from global memory (4 bytes of a row per K-step, L2-resident), one K-step ahead of their use.
#include <stdio.h>
#include <string.h>

#include "gemm_common.h"
#include "mx.h"


#define MX_BM 256
#define MX_BN 128
#define MX_STAGE ((MX_BM + MX_BN) * ROWB)    // 48 KiB
#define MX_GROUP_M 4                         // m-tiles per group of the tile walk (tile_of; gemm.hip's default)

// FFN1 with MX output: the GELU epilogue's bf16 values, quantised in place.  A 32-column block of row m is the two n-subtiles
// 2p, 2p + 1 of the four lanes with this lane's row (lane & 15): 8 values per lane, block maximum over lanes l ^ 16, l ^ 32.
__device__ __forceinline__ void gemm_epilogue_gelu_mx(f32x4 (&acc)[4][4], uint8_t* __restrict__ q, uint8_t* __restrict__ qs, int M,
                                                      int N, int mw, int nw, int fr, int fg, const bf16* __restrict__ bias) {
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
      const int e = mx_scale_exp(mx);
      const int nb = nw + p * 32;                         // first column of the block (N % 32 == 0: wholly inside or outside)
      if (m < M && nb < N) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
          *reinterpret_cast<uint32_t*>(q + (size_t)m * N + nb + h * 16 + fg * 4) = mx_code4(g[h][0], g[h][1], g[h][2], g[h][3], e);
        if (fg == 0) qs[(size_t)m * (N / MX_BLOCK) + nb / MX_BLOCK] = (uint8_t)(e + 127);
      }
    }
  }
}

template <int EPI, bool MXOUT>
__global__ __launch_bounds__(512, 1) void gemm_mx_kernel(const uint8_t* __restrict__ X, const uint8_t* __restrict__ SX,
                                                         const uint8_t* __restrict__ Wt, const uint8_t* __restrict__ SW,
                                                         bf16* __restrict__ Y, uint8_t* __restrict__ QO, uint8_t* __restrict__ SO,
                                                         int M, int N, int K, int ldo, int ntm, int ntn, EpiArgs ea) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int lid = xcd_remap(blockIdx.x, ntm * ntn), mt_, nt_;
  tile_of(lid, ntm, ntn, MX_GROUP_M, mt_, nt_);
  const int m0 = mt_ * MX_BM, n0 = nt_ * MX_BN;
  const int nk = K / ROWB, kb = K / MX_BLOCK;
  const int fr = lane & 15, fg = lane >> 4;

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc_zero<GQ_BF16>();

  // scale bytes of this lane's rows: (row, K-block kt * 4 + fg); rows past the edge re-read the last row (never stored)
  const uint8_t* sxr[4];
  const uint8_t* swr[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    int mr = m0 + wm * 64 + t * 16 + fr, nr = n0 + wn * 64 + t * 16 + fr;
    sxr[t] = SX + (size_t)(mr < M ? mr : M - 1) * kb + fg;
    swr[t] = SW + (size_t)(nr < N ? nr : N - 1) * kb + fg;
  }
  int sx[4], sw[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) sx[t] = sxr[t][0], sw[t] = swr[t][0];

  auto stage = [&](int kt, int slot) {
    char* base = smem + slot * MX_STAGE;
    stage_rows((const char*)X, (size_t)K, m0, M, kt * ROWB, base, wave * 4, 4, lane);                 // 32 x 1 KiB over 8 waves
    stage_rows((const char*)Wt, (size_t)K, n0, N, kt * ROWB, base + MX_BM * ROWB, wave * 2, 2, lane);  // 16 x 1 KiB over 8 waves
  };
  stage(0, 0);

  const bool live = m0 + wm * 64 < M;       // wave-uniform
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();           // tile kt is in LDS for every wave; the other stage is no longer being read
    int nsx[4], nsw[4];
    if (kt + 1 < nk) {
      stage(kt + 1, (kt + 1) & 1);
#pragma unroll
      for (int t = 0; t < 4; ++t) nsx[t] = sxr[t][(kt + 1) * 4], nsw[t] = swr[t][(kt + 1) * 4];
    }
    const char* xs = smem + (kt & 1) * MX_STAGE;
    const char* ws = xs + MX_BM * ROWB;
    if (live) {
      __builtin_amdgcn_s_setprio(1);
      i32x8 wf[4], xf[4];
      const int c0 = fg, c1 = fg + 4;                  // k 16 fg .. + 15 and 64 + 16 fg .. + 15 (the instruction's operand map)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        int rw = wn * 64 + t * 16 + fr, rx = wm * 64 + t * 16 + fr;
        i32x4 w0 = *reinterpret_cast<const i32x4*>(ws + rw * ROWB + ((c0 ^ (rw & 7)) << 4));
        i32x4 w1 = *reinterpret_cast<const i32x4*>(ws + rw * ROWB + ((c1 ^ (rw & 7)) << 4));
        i32x4 x0 = *reinterpret_cast<const i32x4*>(xs + rx * ROWB + ((c0 ^ (rx & 7)) << 4));
        i32x4 x1 = *reinterpret_cast<const i32x4*>(xs + rx * ROWB + ((c1 ^ (rx & 7)) << 4));
        wf[t] = (i32x8){w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
        xf[t] = (i32x8){x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[a], xf[b], acc[a][b], 0, 0, 0, sw[a], 0, sx[b]);
      __builtin_amdgcn_s_setprio(0);
    }
    if (kt + 1 < nk) {
#pragma unroll
      for (int t = 0; t < 4; ++t) sx[t] = nsx[t], sw[t] = nsw[t];
    }
  }
  if (MXOUT) {
    gemm_epilogue_gelu_mx(acc, QO, SO, M, N, m0 + wm * 64, n0 + wn * 64, fr, fg, ea.bias);
  } else if (EPI == LL_EPI_BIAS_GELU) {     // (register form, as the bf16 GELU call takes it by default: same values either way)
    gemm_epilogue<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, fr, fg, ea);
  } else {
    __builtin_amdgcn_s_barrier();           // every wave has read its last K-step's fragments: the ring is free
    gemm_epilogue_lds<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, lane, smem + wave * (64 * EPI_ROW_BYTES(4)), ea);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Quantiser: one thread per 8-element chunk, a 32-element block on 4 consecutive lanes (K % 32 == 0 keeps them in one row).
__global__ __launch_bounds__(256) void quantize_mx_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ qs,
                                                          int rows, int K, int ldx) {
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
  const int e = mx_scale_exp(mx);
  if (!in) return;
  *reinterpret_cast<uint2*>(q + (size_t)row * K + c) = make_uint2(mx_code4(f[0], f[1], f[2], f[3], e), mx_code4(f[4], f[5], f[6], f[7], e));
  if ((c & (MX_BLOCK - 1)) == 0) qs[(size_t)row * (K / MX_BLOCK) + c / MX_BLOCK] = (uint8_t)(e + 127);
}

extern "C" int ll_quantize_mx(const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx, ll_stream stream) {
  LL_REQUIRE(x != nullptr && q != nullptr && qs != nullptr, "ll_quantize_mx: x, codes and scales are required");
  LL_REQUIRE(K > 0 && K % MX_BLOCK == 0, "ll_quantize_mx: K=%d must be a positive multiple of 32", K);
  LL_REQUIRE(ldx >= K && ldx % 8 == 0, "ll_quantize_mx: ldx=%d must be >= K and a multiple of 8", ldx);
  LL_REQUIRE(rows >= 0, "ll_quantize_mx: rows=%d", rows);
  if (rows == 0) return LL_OK;
  const long long n = (long long)rows * (K / 8);
  LL_REQUIRE(n < (1LL << 31) * 256, "ll_quantize_mx: too large");
  hipLaunchKernelGGL(quantize_mx_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, q, qs,
                     rows, K, ldx);
  return ll_check_launch("ll_quantize_mx");
}

extern "C" int ll_gemm_plan_mx(int M, int N, int K, char* out, int cap) {
  LL_REQUIRE(out != nullptr && cap > 0, "ll_gemm_plan_mx: needs an output buffer");
  (void)K;
  int ntm = (M + MX_BM - 1) / MX_BM, ntn = (N + MX_BN - 1) / MX_BN;
  snprintf(out, (size_t)cap, "gemm_mx_kernel tile %dx%d, %d workgroups, groups of %d m-tiles", MX_BM, MX_BN, ntm * ntn, MX_GROUP_M);
  return LL_OK;
}

static int mx_check(const char* fn, const void* xq, const void* sx, const void* wq, const void* sw, int M, int N, int K, int ldo,
                    int epilogue, const void* bias, const void* res, const void* e, int nmod, int gate_idx, int rows_per_batch,
                    int frame_len) {
  LL_REQUIRE(xq && sx && wq && sw, "%s: codes and scales of both operands are required", fn);
  LL_REQUIRE(K > 0 && K % 128 == 0, "%s: K=%d must be a positive multiple of 128", fn, K);
  LL_REQUIRE(M >= 0, "%s: M=%d", fn, M);
  LL_REQUIRE(N > 0 && N % 8 == 0, "%s: N=%d must be a positive multiple of 8", fn, N);
  LL_REQUIRE(ldo >= N && ldo % 8 == 0, "%s: ldo=%d must be >= N and a multiple of 8", fn, ldo);
  LL_REQUIRE(bias != nullptr, "%s: bias is required", fn);
  LL_REQUIRE(epilogue >= 0 && epilogue <= 3, "%s: unknown epilogue %d", fn, epilogue);
  if (epilogue == LL_EPI_BIAS_GATE_RES) {
    LL_REQUIRE(res && e, "%s: gate-residual epilogue needs res and e (mod may be NULL: e then holds bf16(mod + e))", fn);
    LL_REQUIRE(frame_len > 0 && rows_per_batch > 0 && rows_per_batch % frame_len == 0 && M % rows_per_batch == 0,
               "%s: rows_per_batch=%d / frame_len=%d do not tile M=%d", fn, rows_per_batch, frame_len, M);
    LL_REQUIRE(gate_idx >= 0 && gate_idx < nmod, "%s: gate_idx %d outside nmod %d", fn, gate_idx, nmod);
  }
  if (epilogue == LL_EPI_BIAS_RES) LL_REQUIRE(res != nullptr, "%s: residual epilogue needs res", fn);
  return LL_OK;
}

static int mx_launch(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, bf16* out, uint8_t* qo, uint8_t* so,
                     int M, int N, int K, int ldo, int epilogue, const EpiArgs& ea, hipStream_t s) {
  const int ntm = (M + MX_BM - 1) / MX_BM, ntn = (N + MX_BN - 1) / MX_BN;
  const dim3 grid(ntm * ntn), block(512);
  const int lds = 2 * MX_STAGE;
#define LAUNCH(E, Q)                                                                                                          \
  do {                                                                                                                        \
    if (int rc_ = ll_lds_attr((const void*)gemm_mx_kernel<E, Q>, lds)) return rc_;                                            \
    hipLaunchKernelGGL((gemm_mx_kernel<E, Q>), grid, block, lds, s, xq, sx, wq, sw, out, qo, so, M, N, K, ldo, ntm, ntn, ea); \
  } while (0)
  if (qo != nullptr) LAUNCH(LL_EPI_BIAS_GELU, true);
  else if (epilogue == LL_EPI_BIAS) LAUNCH(LL_EPI_BIAS, false);
  else if (epilogue == LL_EPI_BIAS_GELU) LAUNCH(LL_EPI_BIAS_GELU, false);
  else if (epilogue == LL_EPI_BIAS_GATE_RES) LAUNCH(LL_EPI_BIAS_GATE_RES, false);
  else LAUNCH(LL_EPI_BIAS_RES, false);
#undef LAUNCH
  return LL_OK;
}

extern "C" int ll_gemm_mx(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                          uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res,
                          const ll_bf16* e, const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len,
                          ll_stream stream) {
  int rc = mx_check("ll_gemm_mx", xq, sx, wq, sw, M, N, K, ldo, epilogue, bias, res, e, nmod, gate_idx, rows_per_batch, frame_len);
  if (rc) return rc;
  LL_REQUIRE((q_out == nullptr) == (s_out == nullptr), "ll_gemm_mx: the MX output needs both codes and scales");
  LL_REQUIRE((out != nullptr) != (q_out != nullptr), "ll_gemm_mx: exactly one of out (bf16) and q_out / s_out (MX) is required");
  if (q_out != nullptr) {
    LL_REQUIRE(epilogue == LL_EPI_BIAS_GELU, "ll_gemm_mx: the MX output exists for the GELU epilogue only (epilogue %d)", epilogue);
    LL_REQUIRE(N % MX_BLOCK == 0 && ldo == N, "ll_gemm_mx: the MX output needs N=%d a multiple of 32 and ldo == N", N);
  }
  if (M == 0) return LL_OK;
  EpiArgs ea{(const bf16*)bias, (const bf16*)res, (const bf16*)e, (const bf16*)mod, nullptr, nullptr, nmod, gate_idx,
             rows_per_batch, frame_len, frame_len > 0 && rows_per_batch > 0 ? rows_per_batch / frame_len : 0};
  if (int lrc = mx_launch(xq, sx, wq, sw, (bf16*)out, q_out, s_out, M, N, K, ldo, epilogue, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch("ll_gemm_mx");
}

extern "C" int ll_gemm_mx_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
                              ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start,
                              int roped_offset, int write_len, ll_stream stream) {
  int rc = mx_check("ll_gemm_mx_qkv", xq, sx, wq, sw, M, N, K, ldo, LL_EPI_BIAS, bias, nullptr, nullptr, 0, 0, 0, 0);
  if (rc) return rc;
  LL_REQUIRE(out != nullptr, "ll_gemm_mx_qkv: out is required");
  if (int vrc = check_v_insert("ll_gemm_mx_qkv", M, N, B, L, S, write_start, roped_offset, write_len, cache_v)) return vrc;
  EpiArgs ea{(const bf16*)bias, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
  set_v_insert(ea, cache_v, N, L, S, write_start, roped_offset, write_len);
  if (int lrc = mx_launch(xq, sx, wq, sw, (bf16*)out, nullptr, nullptr, M, N, K, ldo, LL_EPI_BIAS, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch("ll_gemm_mx_qkv");
}
