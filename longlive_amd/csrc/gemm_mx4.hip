// W4A6 block linears on the block-scaled MFMA of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = 4, blgp = 2: A = OCP FP4 E2M1
// weights, B = OCP FP6 E2M3 activations, the FP4 rate, 4x bf16 per clock):
//   out[M,N] = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias)
// with packed E2M3 codes X [M, 3K/4] (mx6.h), packed E2M1 codes W [N, K/2] (mx4.h) and one E8M0 scale byte per row and 32-element
// block of K on both sides.  The rescale happens inside the MFMA, so the epilogues are the bf16 GEMM's (gemm_common.h), bit for bit the
// same arithmetic on the fp32 sums, and the FFN1 GELU epilogue is gemm_mx6.hip's (gemm_mx6_common.h): FFN2 reads the MXFP6 tensor
// the mxfp6 mode would.
//
// Operand map of the 16x16x128 f8f6f4 MFMA with an E2M1 operand (4 VGPRs; the builtin's 8-dword argument leaves the top four unread):
// lane l holds row l & 15, g = l >> 4; code i = 0..31 of its fragment sits in bits 4i .. 4i + 3 of the 128 bits and is k = 32 g + i,
// under the E8M0 byte of K-block g in byte 0 of its scale VGPR -- the E2M3 map of gemm_mx6.hip with 4-bit codes.
// tests/test_mx4_gpu.py pins it with exact data.
//
// Structure: gemm_mx6.hip's, with 128-byte W rows.  256(M) x 128(N) per workgroup, 8 waves of 64 x 64, operands SWAPPED (A := W,
// B := X).  One stage = 256 k = two MFMA K-steps: 192 bytes per X row (gemm_mx6.hip's rotated rows, unchanged) and 128 bytes per W
// row, 64 KiB of codes, two stages in LDS.  A lane's W fragments of both K-steps are the 32 contiguous bytes at 32 g of its row, read
// as two 16-byte units 2g, 2g + 1.  At a 128-byte stride the 16-byte slot of unit u of row r is 8 (r & 1) + u, so the 8 lanes of a
// lane group reading one unit of 8 rows would meet 4-way; LDS row r therefore holds unit u at position u ^ wsw(r), wsw(r) = bit 1 of
// r | 6 x bit 3 of r.  Conflict-free by construction: ds_read_b128's lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31} and their
// +32 twins) read rows fr in S1 = {0-3, 12-15} at one unit u0 and rows S2 = {4-11} at u0 ^ 2 (or the reverse).  Within each row
// parity, (r >> 1) & 7 runs over {0,1,6,7} in S1 and {2,3,4,5} in S2, and wsw maps them to {0,1,6,7} and {0,1,6,7} ^ 2 = {2,3,4,5}:
// the 16 lanes hit 16 distinct slots.  As in gemm_mx6.hip the swizzle is applied to the per-lane global address of the LDS-DMA (its
// LDS side is the wave's base + lane x 16).  Scales go through gemm_mx6.hip's 3-slot ring, loaded two stages ahead, with the same
// counted vmcnt(2) across the raw s_barrier.
#include <stdio.h>
#include <string.h>

#include "gemm_common.h"
#include "gemm_mx6_common.h"
#include "mx4.h"
#include "mx6.h"

#define M4_BM 256
#define M4_BN 128
#define M4_ROWX 192                                  // LDS X row: 256 k of E2M3 codes
#define M4_ROWW 128                                  // LDS W row: 256 k of E2M1 codes
#define M4_TILE (M4_BM * M4_ROWX + M4_BN * M4_ROWW)  // 64 KiB
#define M4_SC ((M4_BM + M4_BN) * 8)                  // 3 KiB of scale bytes per stage
#define M4_LDS (2 * M4_TILE + 3 * M4_SC)             // 137 KiB
#define M4_GROUP_M 4

// LDS position of 16-byte unit u of W row r is u ^ m4_wsw(r) (its own inverse)
__device__ __forceinline__ int m4_wsw(int r) { return ((r >> 1) & 1) | ((r >> 3) & 1) * 6; }

template <int EPI, bool MXOUT>
__global__ __launch_bounds__(512, 1) void gemm_mx4w6_kernel(const uint8_t* __restrict__ X, const uint8_t* __restrict__ SX,
                                                            const uint8_t* __restrict__ Wt, const uint8_t* __restrict__ SW,
                                                            bf16* __restrict__ Y, uint8_t* __restrict__ QO, uint8_t* __restrict__ SO,
                                                            int M, int N, int K, int ldo, int ntm, int ntn, EpiArgs ea) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int lid = xcd_remap(blockIdx.x, ntm * ntn), mt_, nt_;
  tile_of(lid, ntm, ntn, M4_GROUP_M, mt_, nt_);
  const int m0 = mt_ * M4_BM, n0 = nt_ * M4_BN;
  const int nk = K / MX6_SUPER, kb = K / MX6_BLOCK;
  const size_t rowx = (size_t)K / 4 * 3, roww = (size_t)K / 2;
  const int fr = lane & 15, fg = lane >> 4;
  char* const scl = smem + 2 * M4_TILE;

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc_zero<GQ_BF16>();

  // codes of stage kt: 3072 X units + 1024 W units of 16 bytes, 6 + 2 LDS-DMA instructions per wave.  X: LDS unit p of row r holds
  // the row's unit (p + 6) % 12 when r & 4 (gemm_mx6.hip's rotation); W: LDS unit p of row r holds unit p ^ m4_wsw(r).  Rows past
  // the edge re-read the last row (never stored).
  auto stage_tile = [&](int kt, int slot) {
    char* base = smem + slot * M4_TILE;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool isx = i < 6;
      const uint8_t* g;
      int off;
      if (isx) {
        const int inst = wave * 6 + i, idx = inst * 64 + lane, r = idx / 12, p = idx - r * 12;
        const int u = (r & 4) ? (p < 6 ? p + 6 : p - 6) : p;
        const int gr = m0 + r < M ? m0 + r : M - 1;
        g = X + (size_t)gr * rowx + (size_t)kt * M4_ROWX + u * 16;
        off = inst * 1024;
      } else {
        const int inst = wave * 2 + (i - 6), idx = inst * 64 + lane, r = idx >> 3, u = (idx & 7) ^ m4_wsw(r);
        const int gr = n0 + r < N ? n0 + r : N - 1;
        g = Wt + (size_t)gr * roww + (size_t)kt * M4_ROWW + u * 16;
        off = M4_BM * M4_ROWX + inst * 1024;
      }
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + off), 16, 0, 0);
    }
  };
  // scale bytes of stage kt: row r's 8 bytes (K-blocks 8 kt .. 8 kt + 7) at r * 8; one X and one W instruction per wave (the W
  // scales are 4 instructions' worth: waves w and w + 4 load the same dwords to the same place)
  auto stage_sc = [&](int kt, int slot) {
    char* base = scl + slot * M4_SC;
    {
      const int j = wave * 64 + lane, r = j >> 1;
      const int gr = m0 + r < M ? m0 + r : M - 1;
      const uint8_t* g = SX + (size_t)gr * kb + kt * 8 + (j & 1) * 4;
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + wave * 256), 4, 0, 0);
    }
    {
      const int w4 = wave & 3, j = w4 * 64 + lane, r = j >> 1;
      const int gr = n0 + r < N ? n0 + r : N - 1;
      const uint8_t* g = SW + (size_t)gr * kb + kt * 8 + (j & 1) * 4;
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + M4_BM * 8 + w4 * 256), 4, 0, 0);
    }
  };
  stage_tile(0, 0);
  stage_sc(0, 0);
  if (nk > 1) stage_sc(1, 1);

  const bool live = m0 + wm * 64 < M;       // wave-uniform
  for (int kt = 0; kt < nk; ++kt) {
    // issued so far, oldest first: ... tile kt, scales kt + 1 (if any).  Tile kt and scales kt must have landed.
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();           // stage kt is in LDS for every wave; tile slot (kt + 1) & 1, scale slot (kt + 2) % 3 are free
    if (kt + 1 < nk) stage_tile(kt + 1, (kt + 1) & 1);
    if (kt + 2 < nk) stage_sc(kt + 2, (kt + 2) % 3);
    const char* xs = smem + (kt & 1) * M4_TILE;
    const char* ws = xs + M4_BM * M4_ROWX;
    const uint8_t* ss = (const uint8_t*)(scl + (kt % 3) * M4_SC);
    if (live) {
      __builtin_amdgcn_s_setprio(1);
      i32x4 wf[4][2], xf[4][3];
      int sw[4][2], sx[4][2];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int rw = wn * 64 + t * 16 + fr, rx = wm * 64 + t * 16 + fr;
#pragma unroll
        for (int j = 0; j < 2; ++j) wf[t][j] = *reinterpret_cast<const i32x4*>(ws + rw * M4_ROWW + ((2 * fg + j) ^ m4_wsw(rw)) * 16);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int u = 3 * fg + j;
          const int px = (rx & 4) ? (u < 6 ? u + 6 : u - 6) : u;
          xf[t][j] = *reinterpret_cast<const i32x4*>(xs + rx * M4_ROWX + px * 16);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          sw[t][s] = ss[M4_BM * 8 + rw * 8 + 4 * s + fg];
          sx[t][s] = ss[rx * 8 + 4 * s + fg];
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        i32x8 wa[4], xb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          // K-step s: W unit 2 g + s (4 dwords; the top four of the 8-dword operand are not read with E2M1), X dwords 6 s .. 6 s + 5
          const i32x4 w = wf[t][s], x0 = xf[t][0], x1 = xf[t][1], x2 = xf[t][2];
          wa[t] = (i32x8){w[0], w[1], w[2], w[3], 0, 0, 0, 0};
          xb[t] = s == 0 ? (i32x8){x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], 0, 0} : (i32x8){x1[2], x1[3], x2[0], x2[1], x2[2], x2[3], 0, 0};
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa[a], xb[b], acc[a][b], 4, 2, 0, sw[a][s], 0, sx[b][s]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }
  if (MXOUT) {
    gemm_epilogue_gelu_mx6(acc, QO, SO, M, N, m0 + wm * 64, n0 + wn * 64, lane, fr, fg, ea.bias);
  } else if (EPI == LL_EPI_BIAS_GELU) {     // (register form, as gemm_mx6_kernel's)
    gemm_epilogue<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, fr, fg, ea);
  } else {
    __builtin_amdgcn_s_barrier();           // every wave has read its last stage's fragments: the ring is free
    gemm_epilogue_lds<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, lane, smem + wave * (64 * EPI_ROW_BYTES(4)), ea);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Quantiser: one thread per 8-element chunk (one packed dword), a 32-element block on 4 consecutive lanes.
__global__ __launch_bounds__(256) void quantize_mx4_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ qs,
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
  const int e = mx4_scale_exp(mx);
  if (in) {
    *reinterpret_cast<uint32_t*>(q + (size_t)row * (K / 2) + mx4_chunk_off(c)) = mx4_pack8(f, e);
    if ((c & (MX4_BLOCK - 1)) == 0) qs[(size_t)row * (K / MX4_BLOCK) + c / MX4_BLOCK] = (uint8_t)(e + 127);
  }
}

extern "C" int ll_quantize_mx4(const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx, ll_stream stream) {
  LL_REQUIRE(x != nullptr && q != nullptr && qs != nullptr, "ll_quantize_mx4: x, codes and scales are required");
  LL_REQUIRE(K > 0 && K % MX4_SUPER == 0, "ll_quantize_mx4: K=%d must be a positive multiple of 256", K);
  LL_REQUIRE(ldx >= K && ldx % 8 == 0, "ll_quantize_mx4: ldx=%d must be >= K and a multiple of 8", ldx);
  LL_REQUIRE(rows >= 0, "ll_quantize_mx4: rows=%d", rows);
  if (rows == 0) return LL_OK;
  const long long n = (long long)rows * (K / 8);
  LL_REQUIRE(n < (1LL << 31) * 256, "ll_quantize_mx4: too large");
  hipLaunchKernelGGL(quantize_mx4_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, q, qs,
                     rows, K, ldx);
  return ll_check_launch("ll_quantize_mx4");
}

extern "C" int ll_gemm_plan_mx4w6(int M, int N, int K, char* out, int cap) {
  LL_REQUIRE(out != nullptr && cap > 0, "ll_gemm_plan_mx4w6: needs an output buffer");
  (void)K;
  int ntm = (M + M4_BM - 1) / M4_BM, ntn = (N + M4_BN - 1) / M4_BN;
  snprintf(out, (size_t)cap, "gemm_mx4w6_kernel tile %dx%d, 256 k per stage, %d workgroups, groups of %d m-tiles", M4_BM, M4_BN,
           ntm * ntn, M4_GROUP_M);
  return LL_OK;
}

static int mx4w6_launch(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, bf16* out, uint8_t* qo, uint8_t* so,
                        int M, int N, int K, int ldo, int epilogue, const EpiArgs& ea, hipStream_t s) {
  const int ntm = (M + M4_BM - 1) / M4_BM, ntn = (N + M4_BN - 1) / M4_BN;
  const dim3 grid(ntm * ntn), block(512);
#define LAUNCH(E, Q)                                                                                                             \
  do {                                                                                                                           \
    if (int rc_ = ll_lds_attr((const void*)gemm_mx4w6_kernel<E, Q>, M4_LDS)) return rc_;                                        \
    hipLaunchKernelGGL((gemm_mx4w6_kernel<E, Q>), grid, block, M4_LDS, s, xq, sx, wq, sw, out, qo, so, M, N, K, ldo, ntm, ntn, ea); \
  } while (0)
  if (qo != nullptr) LAUNCH(LL_EPI_BIAS_GELU, true);
  else if (epilogue == LL_EPI_BIAS) LAUNCH(LL_EPI_BIAS, false);
  else if (epilogue == LL_EPI_BIAS_GELU) LAUNCH(LL_EPI_BIAS_GELU, false);
  else if (epilogue == LL_EPI_BIAS_GATE_RES) LAUNCH(LL_EPI_BIAS_GATE_RES, false);
  else LAUNCH(LL_EPI_BIAS_RES, false);
#undef LAUNCH
  return LL_OK;
}

extern "C" int ll_gemm_mx4w6(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
                             ll_bf16* out, uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res,
                             const ll_bf16* e, const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len,
                             ll_stream stream) {
  int rc = mx6_check("ll_gemm_mx4w6", xq, sx, wq, sw, M, N, K, ldo, epilogue, bias, res, e, nmod, gate_idx, rows_per_batch, frame_len);
  if (rc) return rc;
  LL_REQUIRE((q_out == nullptr) == (s_out == nullptr), "ll_gemm_mx4w6: the MXFP6 output needs both codes and scales");
  LL_REQUIRE((out != nullptr) != (q_out != nullptr), "ll_gemm_mx4w6: exactly one of out (bf16) and q_out / s_out (MXFP6) is required");
  if (q_out != nullptr) {
    LL_REQUIRE(epilogue == LL_EPI_BIAS_GELU, "ll_gemm_mx4w6: the MXFP6 output exists for the GELU epilogue only (epilogue %d)", epilogue);
    LL_REQUIRE(N % MX6_SUPER == 0 && ldo == N, "ll_gemm_mx4w6: the MXFP6 output needs N=%d a multiple of 256 and ldo == N", N);
  }
  if (M == 0) return LL_OK;
  EpiArgs ea{(const bf16*)bias, (const bf16*)res, (const bf16*)e, (const bf16*)mod, nullptr, nullptr, nmod, gate_idx,
             rows_per_batch, frame_len, frame_len > 0 && rows_per_batch > 0 ? rows_per_batch / frame_len : 0};
  if (int lrc = mx4w6_launch(xq, sx, wq, sw, (bf16*)out, q_out, s_out, M, N, K, ldo, epilogue, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch("ll_gemm_mx4w6");
}

extern "C" int ll_gemm_mx4w6_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
                                 ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start,
                                 int roped_offset, int write_len, ll_stream stream) {
  int rc = mx6_check("ll_gemm_mx4w6_qkv", xq, sx, wq, sw, M, N, K, ldo, LL_EPI_BIAS, bias, nullptr, nullptr, 0, 0, 0, 0);
  if (rc) return rc;
  LL_REQUIRE(out != nullptr, "ll_gemm_mx4w6_qkv: out is required");
  if (int vrc = check_v_insert("ll_gemm_mx4w6_qkv", M, N, B, L, S, write_start, roped_offset, write_len, cache_v)) return vrc;
  EpiArgs ea{(const bf16*)bias, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
  set_v_insert(ea, cache_v, N, L, S, write_start, roped_offset, write_len);
  if (int lrc = mx4w6_launch(xq, sx, wq, sw, (bf16*)out, nullptr, nullptr, M, N, K, ldo, LL_EPI_BIAS, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch("ll_gemm_mx4w6_qkv");
}

// ---------------------------------------------------------------------------------------------------------------
// W4A4: both operands OCP FP4 E2M1 (cbsz = 4, blgp = 4), activations in the weights' format (ll_quantize_mx4 or the MXFP4
// producers).  gemm_mx4w6_kernel's structure with X in the W layout: X rows are 128 bytes per stage and staged exactly like W rows
// (unit u of LDS row r holds the row's unit u ^ m4_wsw(r), so the conflict-free argument above holds for the X reads too), and a
// lane's X fragment of K-step s is 16-byte unit 2 g + s.  One stage = 48 KiB of codes, 4 + 2 LDS-DMA instructions per wave; both
// 8-dword MFMA operands carry 4 live dwords.  Same 256 x 128 tile, two code stages, 3-slot scale ring two stages ahead and counted
// vmcnt(2) across the raw s_barrier.  The FFN1 form writes MXFP4 codes + scales (gemm_epilogue_gelu_mx4), FFN2's input.
#define M4A_ROW 128                                  // LDS row of either operand: 256 k of E2M1 codes
#define M4A_TILE ((M4_BM + M4_BN) * M4A_ROW)         // 48 KiB
#define M4A_LDS (2 * M4A_TILE + 3 * M4_SC)           // 105 KiB (the LDS epilogue's 72 KiB fits)

// FFN1 with MXFP4 output: the GELU epilogue's bf16 values, quantised in place (operands swapped: a lane's acc[a][b] holds 4
// consecutive N of one row M).  A 32-column block of row m is the two n-subtiles 2p, 2p + 1 of the four lanes fg = 0..3 with this
// lane's row; lane fg holds codes 4 fg .. 4 fg + 3 (h = 0) and 16 + 4 fg .. (h = 1) of the block, 16 bits each.  Its 16-byte word is
// four dwords: lane fg even stores dword fg / 2 (its h = 0 codes under lane fg + 1's), lane fg odd dword 2 + fg / 2 (lane fg - 1's
// h = 1 codes under its own).
__device__ __forceinline__ void gemm_epilogue_gelu_mx4(f32x4 (&acc)[4][4], uint8_t* __restrict__ q, uint8_t* __restrict__ qs, int M,
                                                       int N, int mw, int nw, int lane, int fr, int fg, const bf16* __restrict__ bias) {
  bf16x4 bv[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int n = nw + a * 16 + fg * 4;
    bv[a] = *reinterpret_cast<const bf16x4*>(bias + (n < N ? n : N - 4));
  }
  const size_t rowb = (size_t)N / 2;
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
      const int e = mx4_scale_exp(mx);
      const int nb = nw + p * 32;                         // first column of the block (N % 256 == 0: wholly inside or outside)
      const uint32_t c0 = mx4_pack4(g[0][0], g[0][1], g[0][2], g[0][3], e);
      const uint32_t c1 = mx4_pack4(g[1][0], g[1][1], g[1][2], g[1][3], e);
      const uint32_t o0 = (uint32_t)__shfl_xor((int)c0, 16, 64), o1 = (uint32_t)__shfl_xor((int)c1, 16, 64);
      const uint32_t word = (fg & 1) ? (o1 | (c1 << 16)) : (c0 | (o0 << 16));
      const int dw = (fg & 1) ? 2 + (fg >> 1) : (fg >> 1);
      if (m < M && nb < N) {
        *reinterpret_cast<uint32_t*>(q + (size_t)m * rowb + mx4_chunk_off(nb) + 4 * dw) = word;
        if (fg == 0) qs[(size_t)m * (N / MX4_BLOCK) + nb / MX4_BLOCK] = (uint8_t)(e + 127);
      }
    }
  }
}

template <int EPI, bool MXOUT>
__global__ __launch_bounds__(512, 1) void gemm_mx4_kernel(const uint8_t* __restrict__ X, const uint8_t* __restrict__ SX,
                                                          const uint8_t* __restrict__ Wt, const uint8_t* __restrict__ SW,
                                                          bf16* __restrict__ Y, uint8_t* __restrict__ QO, uint8_t* __restrict__ SO,
                                                          int M, int N, int K, int ldo, int ntm, int ntn, EpiArgs ea) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int lid = xcd_remap(blockIdx.x, ntm * ntn), mt_, nt_;
  tile_of(lid, ntm, ntn, M4_GROUP_M, mt_, nt_);
  const int m0 = mt_ * M4_BM, n0 = nt_ * M4_BN;
  const int nk = K / MX4_SUPER, kb = K / MX4_BLOCK;
  const size_t row = (size_t)K / 2;
  const int fr = lane & 15, fg = lane >> 4;
  char* const scl = smem + 2 * M4A_TILE;

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc_zero<GQ_BF16>();

  // codes of stage kt: 2048 X units + 1024 W units of 16 bytes, 4 + 2 LDS-DMA instructions per wave; LDS unit p of row r (either
  // operand) holds the row's unit p ^ m4_wsw(r).  Rows past the edge re-read the last row (never stored).
  auto stage_tile = [&](int kt, int slot) {
    char* base = smem + slot * M4A_TILE;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const bool isx = i < 4;
      const int inst = isx ? wave * 4 + i : wave * 2 + (i - 4), idx = inst * 64 + lane, r = idx >> 3, u = (idx & 7) ^ m4_wsw(r);
      const uint8_t* g;
      int off;
      if (isx) {
        const int gr = m0 + r < M ? m0 + r : M - 1;
        g = X + (size_t)gr * row + (size_t)kt * M4A_ROW + u * 16;
        off = inst * 1024;
      } else {
        const int gr = n0 + r < N ? n0 + r : N - 1;
        g = Wt + (size_t)gr * row + (size_t)kt * M4A_ROW + u * 16;
        off = M4_BM * M4A_ROW + inst * 1024;
      }
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + off), 16, 0, 0);
    }
  };
  // scale bytes of stage kt: gemm_mx4w6_kernel's
  auto stage_sc = [&](int kt, int slot) {
    char* base = scl + slot * M4_SC;
    {
      const int j = wave * 64 + lane, r = j >> 1;
      const int gr = m0 + r < M ? m0 + r : M - 1;
      const uint8_t* g = SX + (size_t)gr * kb + kt * 8 + (j & 1) * 4;
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + wave * 256), 4, 0, 0);
    }
    {
      const int w4 = wave & 3, j = w4 * 64 + lane, r = j >> 1;
      const int gr = n0 + r < N ? n0 + r : N - 1;
      const uint8_t* g = SW + (size_t)gr * kb + kt * 8 + (j & 1) * 4;
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + M4_BM * 8 + w4 * 256), 4, 0, 0);
    }
  };
  stage_tile(0, 0);
  stage_sc(0, 0);
  if (nk > 1) stage_sc(1, 1);

  const bool live = m0 + wm * 64 < M;       // wave-uniform
  for (int kt = 0; kt < nk; ++kt) {
    // issued so far, oldest first: ... tile kt, scales kt + 1 (if any).  Tile kt and scales kt must have landed.
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();           // stage kt is in LDS for every wave; tile slot (kt + 1) & 1, scale slot (kt + 2) % 3 are free
    if (kt + 1 < nk) stage_tile(kt + 1, (kt + 1) & 1);
    if (kt + 2 < nk) stage_sc(kt + 2, (kt + 2) % 3);
    const char* xs = smem + (kt & 1) * M4A_TILE;
    const char* ws = xs + M4_BM * M4A_ROW;
    const uint8_t* ss = (const uint8_t*)(scl + (kt % 3) * M4_SC);
    if (live) {
      __builtin_amdgcn_s_setprio(1);
      i32x4 wf[4][2], xf[4][2];
      int sw[4][2], sx[4][2];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int rw = wn * 64 + t * 16 + fr, rx = wm * 64 + t * 16 + fr;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          wf[t][j] = *reinterpret_cast<const i32x4*>(ws + rw * M4A_ROW + ((2 * fg + j) ^ m4_wsw(rw)) * 16);
          xf[t][j] = *reinterpret_cast<const i32x4*>(xs + rx * M4A_ROW + ((2 * fg + j) ^ m4_wsw(rx)) * 16);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          sw[t][s] = ss[M4_BM * 8 + rw * 8 + 4 * s + fg];
          sx[t][s] = ss[rx * 8 + 4 * s + fg];
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        i32x8 wa[4], xb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          // K-step s: unit 2 g + s of either operand (4 dwords; the top four of the 8-dword operand are not read with E2M1)
          const i32x4 w = wf[t][s], x = xf[t][s];
          wa[t] = (i32x8){w[0], w[1], w[2], w[3], 0, 0, 0, 0};
          xb[t] = (i32x8){x[0], x[1], x[2], x[3], 0, 0, 0, 0};
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa[a], xb[b], acc[a][b], 4, 4, 0, sw[a][s], 0, sx[b][s]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }
  if (MXOUT) {
    gemm_epilogue_gelu_mx4(acc, QO, SO, M, N, m0 + wm * 64, n0 + wn * 64, lane, fr, fg, ea.bias);
  } else if (EPI == LL_EPI_BIAS_GELU) {     // (register form, as gemm_mx6_kernel's)
    gemm_epilogue<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, fr, fg, ea);
  } else {
    __builtin_amdgcn_s_barrier();           // every wave has read its last stage's fragments: the ring is free
    gemm_epilogue_lds<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, lane, smem + wave * (64 * EPI_ROW_BYTES(4)), ea);
  }
}

extern "C" int ll_gemm_plan_mx4(int M, int N, int K, char* out, int cap) {
  LL_REQUIRE(out != nullptr && cap > 0, "ll_gemm_plan_mx4: needs an output buffer");
  (void)K;
  int ntm = (M + M4_BM - 1) / M4_BM, ntn = (N + M4_BN - 1) / M4_BN;
  snprintf(out, (size_t)cap, "gemm_mx4_kernel tile %dx%d, 256 k per stage, %d workgroups, groups of %d m-tiles", M4_BM, M4_BN,
           ntm * ntn, M4_GROUP_M);
  return LL_OK;
}

static int mx4_launch(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, bf16* out, uint8_t* qo, uint8_t* so,
                      int M, int N, int K, int ldo, int epilogue, const EpiArgs& ea, hipStream_t s) {
  const int ntm = (M + M4_BM - 1) / M4_BM, ntn = (N + M4_BN - 1) / M4_BN;
  const dim3 grid(ntm * ntn), block(512);
#define LAUNCH(E, Q)                                                                                                            \
  do {                                                                                                                          \
    if (int rc_ = ll_lds_attr((const void*)gemm_mx4_kernel<E, Q>, M4A_LDS)) return rc_;                                        \
    hipLaunchKernelGGL((gemm_mx4_kernel<E, Q>), grid, block, M4A_LDS, s, xq, sx, wq, sw, out, qo, so, M, N, K, ldo, ntm, ntn, ea); \
  } while (0)
  if (qo != nullptr) LAUNCH(LL_EPI_BIAS_GELU, true);
  else if (epilogue == LL_EPI_BIAS) LAUNCH(LL_EPI_BIAS, false);
  else if (epilogue == LL_EPI_BIAS_GELU) LAUNCH(LL_EPI_BIAS_GELU, false);
  else if (epilogue == LL_EPI_BIAS_GATE_RES) LAUNCH(LL_EPI_BIAS_GATE_RES, false);
  else LAUNCH(LL_EPI_BIAS_RES, false);
#undef LAUNCH
  return LL_OK;
}

extern "C" int ll_gemm_mx4(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
                           ll_bf16* out, uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res,
                           const ll_bf16* e, const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len,
                           ll_stream stream) {
  int rc = mx6_check("ll_gemm_mx4", xq, sx, wq, sw, M, N, K, ldo, epilogue, bias, res, e, nmod, gate_idx, rows_per_batch, frame_len);
  if (rc) return rc;
  LL_REQUIRE((q_out == nullptr) == (s_out == nullptr), "ll_gemm_mx4: the MXFP4 output needs both codes and scales");
  LL_REQUIRE((out != nullptr) != (q_out != nullptr), "ll_gemm_mx4: exactly one of out (bf16) and q_out / s_out (MXFP4) is required");
  if (q_out != nullptr) {
    LL_REQUIRE(epilogue == LL_EPI_BIAS_GELU, "ll_gemm_mx4: the MXFP4 output exists for the GELU epilogue only (epilogue %d)", epilogue);
    LL_REQUIRE(N % MX4_SUPER == 0 && ldo == N, "ll_gemm_mx4: the MXFP4 output needs N=%d a multiple of 256 and ldo == N", N);
  }
  if (M == 0) return LL_OK;
  EpiArgs ea{(const bf16*)bias, (const bf16*)res, (const bf16*)e, (const bf16*)mod, nullptr, nullptr, nmod, gate_idx,
             rows_per_batch, frame_len, frame_len > 0 && rows_per_batch > 0 ? rows_per_batch / frame_len : 0};
  if (int lrc = mx4_launch(xq, sx, wq, sw, (bf16*)out, q_out, s_out, M, N, K, ldo, epilogue, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch("ll_gemm_mx4");
}

extern "C" int ll_gemm_mx4_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
                               ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start,
                               int roped_offset, int write_len, ll_stream stream) {
  int rc = mx6_check("ll_gemm_mx4_qkv", xq, sx, wq, sw, M, N, K, ldo, LL_EPI_BIAS, bias, nullptr, nullptr, 0, 0, 0, 0);
  if (rc) return rc;
  LL_REQUIRE(out != nullptr, "ll_gemm_mx4_qkv: out is required");
  if (int vrc = check_v_insert("ll_gemm_mx4_qkv", M, N, B, L, S, write_start, roped_offset, write_len, cache_v)) return vrc;
  EpiArgs ea{(const bf16*)bias, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
  set_v_insert(ea, cache_v, N, L, S, write_start, roped_offset, write_len);
  if (int lrc = mx4_launch(xq, sx, wq, sw, (bf16*)out, nullptr, nullptr, M, N, K, ldo, LL_EPI_BIAS, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch("ll_gemm_mx4_qkv");
}
