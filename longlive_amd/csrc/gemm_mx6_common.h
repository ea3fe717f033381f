// Pieces shared by the GEMMs over MXFP6 activations (gemm_mx6.hip: E2M3 weights, gemm_mx4.hip: E2M1 weights): the FFN1 GELU
// epilogue that writes MXFP6 codes + scales straight from the accumulators of a 64 x 64 wave tile (operands swapped: a lane's
// acc[a][b] holds 4 consecutive N of one row M), so FFN2's input is the same MXFP6 tensor whichever weight format FFN1 ran on, and the
// host-side argument check of the bf16-output entry points.
#pragma once
#include "gemm_common.h"
#include "mx6.h"

// FFN1 with MXFP6 output: the GELU epilogue's bf16 values, quantised in place.  A 32-column block of row m is the two n-subtiles
// 2p, 2p + 1 of the four lanes with this lane's row (lane & 15); each n-subtile is one 16-k chunk (12 bytes) of the packed row, four
// codes (24 bits) per lane, and lane group fg < 3 stores dword fg of it, joined with the next group's codes.
__device__ __forceinline__ void gemm_epilogue_gelu_mx6(f32x4 (&acc)[4][4], uint8_t* __restrict__ q, uint8_t* __restrict__ qs, int M,
                                                       int N, int mw, int nw, int lane, int fr, int fg, const bf16* __restrict__ bias) {
  bf16x4 bv[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int n = nw + a * 16 + fg * 4;
    bv[a] = *reinterpret_cast<const bf16x4*>(bias + (n < N ? n : N - 4));
  }
  const size_t rowb = (size_t)N / 4 * 3;
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
      const int e = mx6_scale_exp(mx);
      const int nb = nw + p * 32;                         // first column of the block (N % 256 == 0: wholly inside or outside)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        uint32_t piece = mx6_pack4(g[h][0], g[h][1], g[h][2], g[h][3], e);
        uint32_t next = (uint32_t)__shfl((int)piece, (lane + 16) & 63, 64);
        if (m < M && nb < N && fg < 3)
          *reinterpret_cast<uint32_t*>(q + (size_t)m * rowb + mx6_chunk_off(nb + h * 16) + 4 * fg) =
              (piece >> (8 * fg)) | (next << (24 - 8 * fg));
      }
      if (m < M && nb < N && fg == 0) qs[(size_t)m * (N / MX6_BLOCK) + nb / MX6_BLOCK] = (uint8_t)(e + 127);
    }
  }
}

static inline int mx6_check(const char* fn, const void* xq, const void* sx, const void* wq, const void* sw, int M, int N, int K, int ldo,
                            int epilogue, const void* bias, const void* res, const void* e, int nmod, int gate_idx, int rows_per_batch,
                            int frame_len) {
  LL_REQUIRE(xq && sx && wq && sw, "%s: codes and scales of both operands are required", fn);
  LL_REQUIRE(K > 0 && K % MX6_SUPER == 0, "%s: K=%d must be a positive multiple of 256", fn, K);
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
