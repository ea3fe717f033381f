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
// The FFN1 epilogue with MX output, the quantiser and the host path are gemm_mx_common.h's, shared with the packed formats.
#include "gemm_mx_common.h"

#define MX_STAGE ((MXG_BM + MXG_BN) * ROWB)  // 48 KiB

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
  tile_of(lid, ntm, ntn, MXG_GROUP_M, mt_, nt_);
  const int m0 = mt_ * MXG_BM, n0 = nt_ * MXG_BN;
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
    stage_rows((const char*)Wt, (size_t)K, n0, N, kt * ROWB, base + MXG_BM * ROWB, wave * 2, 2, lane);  // 16 x 1 KiB over 8 waves
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
    const char* ws = xs + MXG_BM * ROWB;
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
    gemm_epilogue_gelu_mxout<FmtE4M3>(acc, QO, SO, M, N, m0 + wm * 64, n0 + wn * 64, lane, fr, fg, ea.bias);
  } else if (EPI == LL_EPI_BIAS_GELU) {     // (register form, as the bf16 GELU call takes it by default: same values either way)
    gemm_epilogue<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, fr, fg, ea);
  } else {
    __builtin_amdgcn_s_barrier();           // every wave has read its last K-step's fragments: the ring is free
    gemm_epilogue_lds<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, lane, smem + wave * (64 * EPI_ROW_BYTES(4)), ea);
  }
}

__global__ __launch_bounds__(256) void quantize_mx_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ qs,
                                                          int rows, int K, int ldx) {
  quantize_mx_body<FmtE4M3>(x, q, qs, rows, K, ldx);
}

struct FamMx {
  MX_FAMILY_NAMES("mx");
  static constexpr const char *word = "MX", *plan_stage = "";
  static constexpr int KGRAN = ROWB, NGRAN = MX_BLOCK, LDS = 2 * MX_STAGE;
  template <int EPI, bool MXOUT>
  static mx_gemm_kernel_t select() { return gemm_mx_kernel<EPI, MXOUT>; }
};

extern "C" int ll_quantize_mx(const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx, ll_stream stream) {
  return mx_quantize<FmtE4M3>("ll_quantize_mx", quantize_mx_kernel, x, q, qs, rows, K, ldx, stream);
}

extern "C" int ll_gemm_plan_mx(int M, int N, int K, char* out, int cap) { return mx_gemm_plan<FamMx>(M, N, K, out, cap); }

extern "C" int ll_gemm_mx(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                          uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res,
                          const ll_bf16* e, const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len,
                          ll_stream stream) {
  return mx_gemm<FamMx>(xq, sx, wq, sw, bias, out, q_out, s_out, M, N, K, ldo, epilogue, res, e, mod, nmod, gate_idx, rows_per_batch,
                        frame_len, stream);
}

extern "C" int ll_gemm_mx_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
                              ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start,
                              int roped_offset, int write_len, ll_stream stream) {
  return mx_gemm_qkv<FamMx>(xq, sx, wq, sw, bias, out, M, N, K, ldo, cache_v, B, L, S, write_start, roped_offset, write_len, stream);
}
