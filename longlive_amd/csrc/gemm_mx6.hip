// MXFP6 block linears on the block-scaled MFMA of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 2: both operands OCP
// FP6 E2M3, the FP4 rate, 4x bf16 per clock):
//   out[M,N] = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias)
// with packed E2M3 codes X [M, 3K/4] / W [N, 3K/4] (mx6.h) and one E8M0 scale byte per row and 32-element block of K.  The rescale
// happens inside the MFMA, so the epilogues are the bf16 GEMM's (gemm_common.h), bit for bit the same arithmetic on the fp32 sums.
//
// Operand map of the 16x16x128 f8f6f4 MFMA with E2M3 operands (6 VGPRs per operand; the builtin's 8-dword arguments leave the top two
// unread): lane l holds row l & 15 of its operand, g = l >> 4; code i = 0..31 of its fragment sits in bits 6i .. 6i + 5 of the 192
// bits and is k = 32 g + i: the lane's 32 consecutive k are exactly K-block g, whose E8M0 byte its scale VGPR carries in byte 0.
// This is NOT the e4m3 form's map (gemm_mx.hip: two 16-k chunks, 64 k apart, under the scale of block g), with which this kernel
// first ran: rel-L2 1.2 on exact data.  tests/test_mx6_gpu.py pins the map with exact data.
//
// Structure: 256(M) x 128(N) per workgroup, 8 waves of 64 x 64, operands SWAPPED (A := W, B := X) so a lane's accumulator holds 4
// consecutive N of one row M, as the shared epilogues expect.  One stage = 256 k = two MFMA K-steps = 192 bytes per row: 72 KiB of
// codes (256 + 128 rows), two stages in LDS.  A lane's fragments of both K-steps are 48 contiguous bytes of its row (mx6.h's layout),
// read as three 16-byte units; LDS rows with bit 2 set hold their twelve 16-byte units rotated by six, which makes the three reads
// conflict-free in every ds_read_b128 lane group (the rotation is applied to the per-lane global address of the LDS-DMA, whose LDS
// side is the wave's base + lane x 16).  Scales (8 bytes per row and stage) go through a 3-slot LDS ring, loaded two stages ahead
// by 4-byte LDS-DMA: the wait at the top of a stage is vmcnt(2), leaving the next stage's scale loads in flight across the raw
// s_barrier.
#include <stdio.h>
#include <string.h>

#include "gemm_common.h"
#include "gemm_mx6_common.h"
#include "mx6.h"

#define M6_BM 256
#define M6_BN 128
#define M6_ROWB 192                                  // LDS row: 256 k of E2M3 codes
#define M6_TILE ((M6_BM + M6_BN) * M6_ROWB)          // 72 KiB
#define M6_SC ((M6_BM + M6_BN) * 8)                  // 3 KiB of scale bytes per stage
#define M6_LDS (2 * M6_TILE + 3 * M6_SC)             // 153 KiB
#define M6_GROUP_M 4

template <int EPI, bool MXOUT>
__global__ __launch_bounds__(512, 1) void gemm_mx6_kernel(const uint8_t* __restrict__ X, const uint8_t* __restrict__ SX,
                                                          const uint8_t* __restrict__ Wt, const uint8_t* __restrict__ SW,
                                                          bf16* __restrict__ Y, uint8_t* __restrict__ QO, uint8_t* __restrict__ SO,
                                                          int M, int N, int K, int ldo, int ntm, int ntn, EpiArgs ea) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int lid = xcd_remap(blockIdx.x, ntm * ntn), mt_, nt_;
  tile_of(lid, ntm, ntn, M6_GROUP_M, mt_, nt_);
  const int m0 = mt_ * M6_BM, n0 = nt_ * M6_BN;
  const int nk = K / MX6_SUPER, kb = K / MX6_BLOCK;
  const size_t rowb = (size_t)K / 4 * 3;
  const int fr = lane & 15, fg = lane >> 4;
  char* const scl = smem + 2 * M6_TILE;

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc_zero<GQ_BF16>();

  // codes of stage kt: 3072 X units + 1536 W units of 16 bytes, 6 + 3 LDS-DMA instructions per wave.  LDS unit p of row r holds the
  // row's unit (p + 6) % 12 when r & 4 (the rotation is its own inverse); rows past the edge re-read the last row (never stored).
  auto stage_tile = [&](int kt, int slot) {
    char* base = smem + slot * M6_TILE;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const bool isx = i < 6;
      const int inst = isx ? wave * 6 + i : wave * 3 + (i - 6);
      const int idx = inst * 64 + lane, r = idx / 12, p = idx - r * 12;
      const int u = (r & 4) ? (p < 6 ? p + 6 : p - 6) : p;
      int gr = (isx ? m0 : n0) + r;
      const int lim = isx ? M : N;
      gr = gr < lim ? gr : lim - 1;
      const uint8_t* g = (isx ? X : Wt) + (size_t)gr * rowb + (size_t)kt * M6_ROWB + u * 16;
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + (isx ? 0 : M6_BM * M6_ROWB) + inst * 1024), 16, 0, 0);
    }
  };
  // scale bytes of stage kt: row r's 8 bytes (K-blocks 8 kt .. 8 kt + 7) at r * 8; one X and one W instruction per wave (the W
  // scales are 4 instructions' worth: waves w and w + 4 load the same dwords to the same place)
  auto stage_sc = [&](int kt, int slot) {
    char* base = scl + slot * M6_SC;
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
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + M6_BM * 8 + w4 * 256), 4, 0, 0);
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
    const char* xs = smem + (kt & 1) * M6_TILE;
    const char* ws = xs + M6_BM * M6_ROWB;
    const uint8_t* ss = (const uint8_t*)(scl + (kt % 3) * M6_SC);
    if (live) {
      __builtin_amdgcn_s_setprio(1);
      i32x4 wf[4][3], xf[4][3];
      int sw[4][2], sx[4][2];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int rw = wn * 64 + t * 16 + fr, rx = wm * 64 + t * 16 + fr;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int u = 3 * fg + j;
          const int pw = (rw & 4) ? (u < 6 ? u + 6 : u - 6) : u, px = (rx & 4) ? (u < 6 ? u + 6 : u - 6) : u;
          wf[t][j] = *reinterpret_cast<const i32x4*>(ws + rw * M6_ROWB + pw * 16);
          xf[t][j] = *reinterpret_cast<const i32x4*>(xs + rx * M6_ROWB + px * 16);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          sw[t][s] = ss[M6_BM * 8 + rw * 8 + 4 * s + fg];
          sx[t][s] = ss[rx * 8 + 4 * s + fg];
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        i32x8 wa[4], xb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          // K-step s: dwords 6 s .. 6 s + 5 of the lane's 12 (the top two of the 8-dword operand are not read with E2M3)
          const i32x4 w0 = wf[t][0], w1 = wf[t][1], w2 = wf[t][2], x0 = xf[t][0], x1 = xf[t][1], x2 = xf[t][2];
          wa[t] = s == 0 ? (i32x8){w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], 0, 0} : (i32x8){w1[2], w1[3], w2[0], w2[1], w2[2], w2[3], 0, 0};
          xb[t] = s == 0 ? (i32x8){x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], 0, 0} : (i32x8){x1[2], x1[3], x2[0], x2[1], x2[2], x2[3], 0, 0};
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa[a], xb[b], acc[a][b], 2, 2, 0, sw[a][s], 0, sx[b][s]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }
  if (MXOUT) {
    gemm_epilogue_gelu_mx6(acc, QO, SO, M, N, m0 + wm * 64, n0 + wn * 64, lane, fr, fg, ea.bias);
  } else if (EPI == LL_EPI_BIAS_GELU) {     // (register form, as gemm_mx_kernel's)
    gemm_epilogue<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, fr, fg, ea);
  } else {
    __builtin_amdgcn_s_barrier();           // every wave has read its last stage's fragments: the ring is free
    gemm_epilogue_lds<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, lane, smem + wave * (64 * EPI_ROW_BYTES(4)), ea);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Quantiser: one thread per 8-element chunk, a 32-element block on 4 consecutive lanes, a 16-k chunk of the packed row on a lane pair.
__global__ __launch_bounds__(256) void quantize_mx6_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ qs,
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
  const int e = mx6_scale_exp(mx);
  mx6_store_pair(mx6_pack8(f, e), q + (size_t)row * (K / 4 * 3) + mx6_chunk_off(c & ~15), threadIdx.x & 63, in);
  if (in && (c & (MX6_BLOCK - 1)) == 0) qs[(size_t)row * (K / MX6_BLOCK) + c / MX6_BLOCK] = (uint8_t)(e + 127);
}

extern "C" int ll_quantize_mx6(const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx, ll_stream stream) {
  LL_REQUIRE(x != nullptr && q != nullptr && qs != nullptr, "ll_quantize_mx6: x, codes and scales are required");
  LL_REQUIRE(K > 0 && K % MX6_SUPER == 0, "ll_quantize_mx6: K=%d must be a positive multiple of 256", K);
  LL_REQUIRE(ldx >= K && ldx % 8 == 0, "ll_quantize_mx6: ldx=%d must be >= K and a multiple of 8", ldx);
  LL_REQUIRE(rows >= 0, "ll_quantize_mx6: rows=%d", rows);
  if (rows == 0) return LL_OK;
  const long long n = (long long)rows * (K / 8);
  LL_REQUIRE(n < (1LL << 31) * 256, "ll_quantize_mx6: too large");
  hipLaunchKernelGGL(quantize_mx6_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, q, qs,
                     rows, K, ldx);
  return ll_check_launch("ll_quantize_mx6");
}

extern "C" int ll_gemm_plan_mx6(int M, int N, int K, char* out, int cap) {
  LL_REQUIRE(out != nullptr && cap > 0, "ll_gemm_plan_mx6: needs an output buffer");
  (void)K;
  int ntm = (M + M6_BM - 1) / M6_BM, ntn = (N + M6_BN - 1) / M6_BN;
  snprintf(out, (size_t)cap, "gemm_mx6_kernel tile %dx%d, 256 k per stage, %d workgroups, groups of %d m-tiles", M6_BM, M6_BN, ntm * ntn,
           M6_GROUP_M);
  return LL_OK;
}

static int mx6_launch(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, bf16* out, uint8_t* qo, uint8_t* so,
                      int M, int N, int K, int ldo, int epilogue, const EpiArgs& ea, hipStream_t s) {
  const int ntm = (M + M6_BM - 1) / M6_BM, ntn = (N + M6_BN - 1) / M6_BN;
  const dim3 grid(ntm * ntn), block(512);
#define LAUNCH(E, Q)                                                                                                           \
  do {                                                                                                                         \
    if (int rc_ = ll_lds_attr((const void*)gemm_mx6_kernel<E, Q>, M6_LDS)) return rc_;                                        \
    hipLaunchKernelGGL((gemm_mx6_kernel<E, Q>), grid, block, M6_LDS, s, xq, sx, wq, sw, out, qo, so, M, N, K, ldo, ntm, ntn, ea); \
  } while (0)
  if (qo != nullptr) LAUNCH(LL_EPI_BIAS_GELU, true);
  else if (epilogue == LL_EPI_BIAS) LAUNCH(LL_EPI_BIAS, false);
  else if (epilogue == LL_EPI_BIAS_GELU) LAUNCH(LL_EPI_BIAS_GELU, false);
  else if (epilogue == LL_EPI_BIAS_GATE_RES) LAUNCH(LL_EPI_BIAS_GATE_RES, false);
  else LAUNCH(LL_EPI_BIAS_RES, false);
#undef LAUNCH
  return LL_OK;
}

extern "C" int ll_gemm_mx6(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                           uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res,
                           const ll_bf16* e, const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len,
                           ll_stream stream) {
  int rc = mx6_check("ll_gemm_mx6", xq, sx, wq, sw, M, N, K, ldo, epilogue, bias, res, e, nmod, gate_idx, rows_per_batch, frame_len);
  if (rc) return rc;
  LL_REQUIRE((q_out == nullptr) == (s_out == nullptr), "ll_gemm_mx6: the MXFP6 output needs both codes and scales");
  LL_REQUIRE((out != nullptr) != (q_out != nullptr), "ll_gemm_mx6: exactly one of out (bf16) and q_out / s_out (MXFP6) is required");
  if (q_out != nullptr) {
    LL_REQUIRE(epilogue == LL_EPI_BIAS_GELU, "ll_gemm_mx6: the MXFP6 output exists for the GELU epilogue only (epilogue %d)", epilogue);
    LL_REQUIRE(N % MX6_SUPER == 0 && ldo == N, "ll_gemm_mx6: the MXFP6 output needs N=%d a multiple of 256 and ldo == N", N);
  }
  if (M == 0) return LL_OK;
  EpiArgs ea{(const bf16*)bias, (const bf16*)res, (const bf16*)e, (const bf16*)mod, nullptr, nullptr, nmod, gate_idx,
             rows_per_batch, frame_len, frame_len > 0 && rows_per_batch > 0 ? rows_per_batch / frame_len : 0};
  if (int lrc = mx6_launch(xq, sx, wq, sw, (bf16*)out, q_out, s_out, M, N, K, ldo, epilogue, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch("ll_gemm_mx6");
}

extern "C" int ll_gemm_mx6_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
                               ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start,
                               int roped_offset, int write_len, ll_stream stream) {
  int rc = mx6_check("ll_gemm_mx6_qkv", xq, sx, wq, sw, M, N, K, ldo, LL_EPI_BIAS, bias, nullptr, nullptr, 0, 0, 0, 0);
  if (rc) return rc;
  LL_REQUIRE(out != nullptr, "ll_gemm_mx6_qkv: out is required");
  if (int vrc = check_v_insert("ll_gemm_mx6_qkv", M, N, B, L, S, write_start, roped_offset, write_len, cache_v)) return vrc;
  EpiArgs ea{(const bf16*)bias, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
  set_v_insert(ea, cache_v, N, L, S, write_start, roped_offset, write_len);
  if (int lrc = mx6_launch(xq, sx, wq, sw, (bf16*)out, nullptr, nullptr, M, N, K, ldo, LL_EPI_BIAS, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch("ll_gemm_mx6_qkv");
}
