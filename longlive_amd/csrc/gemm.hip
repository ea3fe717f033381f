// GEMM  out[M,N] = epilogue(x[M,K] @ w[N,K]^T + bias)  on gfx950 MFMA, bf16 (v_mfma_f32_16x16x32_bf16),
// W8A8 int8 (v_mfma_i32_16x16x64_i8, per-row activation scale x per-output-channel weight scale) or FP8 rowwise (e4m3fn codes with
// the same two scales, v_mfma_scale_f32_16x16x128_f8f6f4 at unit block scales: gemm_common.h Ty<GQ_F8>).
//
// Both operands are K-contiguous (activations [M,K], nn.Linear weights [N,K]), which is exactly the MFMA fragment
// shape (16 consecutive bytes of k per lane), so there are no transposes anywhere.  Common structure:
//   operands SWAPPED (A := w fragment, B := x fragment) so that each lane ends up with 4 consecutive N of one row M:
//     the bf16 epilogue store is 8 bytes per lane and the per-row gate / per-column bias are cheap to fetch
//   global -> LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave instruction)
//   LDS image: rows of 128 BYTES (64 bf16 or 128 int8 of k); 16-B chunk c of row r sits at chunk position c ^ (r & 7).  The
//     DMA writes LDS linearly, so the XOR is applied to the per-lane SOURCE address and again on the ds_read_b128 side
//     (both-or-neither); every ds_read_b128 lane group then touches 16 distinct 16-B slots (conflict-free, PMC-verified)
//   workgroup id -> tile: XCD-aware (ids b, b+8, ... share an XCD/L2): each XCD gets a contiguous band of tiles, N fastest
// Two kernels, four tilings, behind one entry point (GemmPlan below decides; measured in profiles/r01_kbench_gemm_variants.txt):
//   gemm_kernel_v2: 256(M) x 128(N), 8 waves (4 x 2, 64 x 64 each), 3-stage LDS ring, counted s_waitcnt vmcnt(6) + raw s_barrier
//       -> N = 1536 GEMMs (228 workgroups ~ one per CU).  Its 64 x 64 per-wave tile needs 1/32 B of LDS reads per FLOP
//       (128 B/clk at full MFMA rate) + the DMA fill against 256 B/clk of LDS: LDS-bound around 0.8 PF.
//   gemm_kernel_v5: 256 rows x a column width that is a template parameter, 2-stage ring, one barrier per K-step:
//       256 x 256 (2 x 4 waves, 128(M) x 64(N) each, 128 accumulator registers): ~40% fewer LDS bytes per FLOP than v2
//       (4096^3: 1.00-1.05 PF vs 0.90); 256 x 192 (QKV) and 256 x 224 (FFN1) where 256 columns quantise badly on 256 CUs.
// (A first 128 x 128 / 4-wave / 2-barrier kernel, ~0.7 PF, was retired; experiments with up-front double fragment sets and
//  a DMA-issue stagger between the two waves of a SIMD measured 0...-5% and were not kept.)
#include <stdio.h>
#include <string.h>
#include <atomic>

#include "attention_common.h"
#include "gemm_asm.h"
#include "gemm_common.h"
#include "mx.h"

// Timing builds only (-DLL_GEMM_DIAG): bits 0x100 / 0x200 of the kernels' lds_epi argument switch the K-loop's staging / its compute
// off (results invalid).  In every other build ll_set_tuning refuses the bits, launch_gemm never passes them, and the two-stage
// kernel's text does not hold the tests.  v2 still tests the bits at run time: its instruction stream is the parent commit's, the
// unchanged yardstick that the two-stage kernel's change was timed against.
#ifdef LL_GEMM_DIAG
constexpr bool GEMM_DIAG = true;
#else
constexpr bool GEMM_DIAG = false;
#endif

// ---------------------------------------------------------------------------------------------------------------
// v2: 256 x 128 tile, 3-stage ring (3 x 48 KiB).  Two K-tiles stay in flight across the barrier: the only wait in the
// loop is a COUNTED s_waitcnt vmcnt(6) (the 6 DMA instructions of the newest tile may still be outstanding).
#define V2_BM 256
#define V2_STAGE ((V2_BM + BN) * ROWB)   // 48 KiB

template <int EPI, int Q>
__global__ __launch_bounds__(512, 2) void gemm_kernel_v2(const char* __restrict__ X, const char* __restrict__ Wt,
                                                         bf16* __restrict__ Y, int M, int N, int nk, size_t xrow_bytes,
                                                         size_t wrow_bytes, int ldo, int ntm, int ntn, int gm, int lds_epi, EpiArgs ea) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int lid = xcd_remap(blockIdx.x, ntm * ntn), mt_, nt_;
  tile_of(lid, ntm, ntn, gm, mt_, nt_);
  const int m0 = mt_ * V2_BM, n0 = nt_ * BN;

  typename Ty<Q>::acc acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc_zero<Q>();

  auto stage = [&](int kt, int slot) {
    char* base = smem + slot * V2_STAGE;
    stage_rows(X, xrow_bytes, m0, M, kt * ROWB, base, wave * 4, 4, lane);                  // 32 x 1 KiB over 8 waves
    stage_rows(Wt, wrow_bytes, n0, N, kt * ROWB, base + V2_BM * ROWB, wave * 2, 2, lane);  // 16 x 1 KiB over 8 waves
  };
  stage(0, 0);
  if (nk > 1) stage(1, 1);

  const int fr = lane & 15, fg = lane >> 4;
  const bool live = m0 + wm * 64 < M;       // wave-uniform
  constexpr int KS = Q == GQ_F8 ? 1 : 2;    // half steps of a 128-byte stage (lds_frag)
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");   // tile kt landed; tile kt+1 may be in flight
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // every wave's share of tile kt is in LDS; slot (kt+2)%3 is no longer being read
    const bool do_stage = kt + 2 < nk && !(lds_epi & 0x100);          // (0x100 / 0x200: timing builds, see GEMM_DIAG)
    int s2 = slot + 2;
    s2 = s2 >= 3 ? s2 - 3 : s2;
    if (do_stage) stage(kt + 2, s2);
    const char* xs = smem + slot * V2_STAGE;
    const char* ws = xs + V2_BM * ROWB;
    if (!live || (lds_epi & 0x200)) {   // rows past M (last m-tile): stage and sync only (idle matrix pipes are speed elsewhere)
      slot = slot == 2 ? 0 : slot + 1;
      continue;
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      typename Ty<Q>::frag wf[4], xf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {        // W and X alternately, MFMAs n-tile outer: v2's measured order (the two-stage kernel's differs)
        wf[t] = lds_frag<Q>(ws, wn * 64 + t * 16 + fr, ks, fg);
        xf[t] = lds_frag<Q>(xs, wm * 64 + t * 16 + fr, ks, fg);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = Ty<Q>::mma(wf[a], xf[b], acc[a][b]);
    }
    __builtin_amdgcn_s_setprio(0);
    slot = slot == 2 ? 0 : slot + 1;
  }
  if (lds_epi) {
    __builtin_amdgcn_s_barrier();      // every wave has read its last K-step's fragments: the ring is free
    gemm_epilogue_lds<EPI, Q, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, lane, smem + wave * (64 * EPI_ROW_BYTES(4)), ea);
  } else {
    gemm_epilogue<EPI, Q, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, fr, fg, ea);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// v5: 256 rows, 2-stage ring, one barrier per K-step (the MFMAs of a K-step cover the next tile's DMA latency), with the column width
// as a parameter: WM x WN waves of (MT x NT) 16 x 16 tiles, BN = WN * NT * 16.  OCC is the launch bound's waves per SIMD (2 = 256
// registers per lane, 1 = 512); LDS_EPI says whether the instance has the LDS-staged epilogue (at 128 x 64 per wave it would not fit
// the ring).
//   <2, 4, 8, 4, 2, false>: 256 x 256, the widest tile where its tile count fills the CUs
//   <2, 4, 8, 3, 1, true>:  256 x 192 (QKV, N = 4608: 456 tiles = 2 rounds of 0.75 instead of 342 = 2 rounds of 1.0)
//   <4, 2, 4, 7, 1, true>:  256 x 224 (FFN1, N = 8960: 760 tiles = 2.97 rounds of 0.875 instead of 665 = 3 rounds of 1.0)
template <int EPI, int Q, int WM, int WN, int MT, int NT, int OCC, bool LDS_EPI>
__global__ __launch_bounds__(512, OCC) void gemm_kernel_v5(const char* __restrict__ X, const char* __restrict__ Wt,
                                                           bf16* __restrict__ Y, int M, int N, int nk, size_t xrow_bytes,
                                                           size_t wrow_bytes, int ldo, int ntm, int ntn, int gm, int lds_epi, EpiArgs ea) {
  static_assert(WM * WN == 8 && WM * MT * 16 == 256, "8 waves, 256 rows");
  constexpr int BNv = WN * NT * 16, STAGE = (256 + BNv) * ROWB, NB = BNv / 8;   // NB = B pieces of 8 rows per K-step
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  int lid = xcd_remap(blockIdx.x, ntm * ntn), mt_, nt_;
  tile_of(lid, ntm, ntn, gm, mt_, nt_);
  const int m0 = mt_ * 256, n0 = nt_ * BNv;

  typename Ty<Q>::acc acc[NT][MT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[a][b] = acc_zero<Q>();

  auto stage = [&](int kt, int slot) {
    char* base = smem + slot * STAGE;
    stage_rows(X, xrow_bytes, m0, M, kt * ROWB, base, wave * 4, 4, lane);
    stage_rows(Wt, wrow_bytes, n0, N, kt * ROWB, base + 256 * ROWB, wave * (NB / 8), NB / 8, lane);
    if (NB % 8 != 0 && wave < NB % 8) stage_rows(Wt, wrow_bytes, n0, N, kt * ROWB, base + 256 * ROWB, (NB / 8) * 8 + wave, 1, lane);
  };
  stage(0, 0);

  const int fr = lane & 15, fg = lane >> 4;
  const bool live = m0 + wm * MT * 16 < M;      // wave-uniform
  constexpr int KS = Q == GQ_F8 ? 1 : 2;        // half steps of a 128-byte stage (lds_frag)
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // tile kt is in LDS for every wave; the other stage is no longer being read
    if (kt + 1 < nk && !(GEMM_DIAG && (lds_epi & 0x100))) stage(kt + 1, (kt + 1) & 1);
    const char* xs = smem + (kt & 1) * STAGE;
    const char* ws = xs + 256 * ROWB;
    if (!live || (GEMM_DIAG && (lds_epi & 0x200))) continue;   // rows past M: stage and sync only (see v2)
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      typename Ty<Q>::frag wf[NT], xf[MT];
#pragma unroll
      for (int t = 0; t < NT; ++t) wf[t] = lds_frag<Q>(ws, wn * NT * 16 + t * 16 + fr, ks, fg);
#pragma unroll
      for (int t = 0; t < MT; ++t) xf[t] = lds_frag<Q>(xs, wm * MT * 16 + t * 16 + fr, ks, fg);
#pragma unroll
      for (int b = 0; b < MT; ++b)
#pragma unroll
        for (int a = 0; a < NT; ++a) acc[a][b] = Ty<Q>::mma(wf[a], xf[b], acc[a][b]);
    }
    __builtin_amdgcn_s_setprio(0);
  }
  if (LDS_EPI && lds_epi) {
    __builtin_amdgcn_s_barrier();
    gemm_epilogue_lds<EPI, Q, NT, MT>(acc, Y, M, N, ldo, m0 + wm * MT * 16, n0 + wn * NT * 16, lane,
                                       smem + wave * (MT * 16 * EPI_ROW_BYTES(NT)), ea);
  } else {
    gemm_epilogue<EPI, Q, NT, MT>(acc, Y, M, N, ldo, m0 + wm * MT * 16, n0 + wn * NT * 16, fr, fg, ea);
  }
}

// runtime tuning switches (A/B experiments from tools/kbench; defaults are the shipped configuration)
static int g_gemm_variant = 0;
static int g_gemm_variant_wide = 0;  // like gemm_variant, but only for N >= 4096 (QKV, FFN1): A/B of the wide tilings alone
// 1: epilogue staged through LDS (whole-line residual loads / stores) in the v2 / v5 tilings, except the GELU epilogue, whose
// register form measured 1.6 % faster (FFN1 127.2 vs 129.3 us; everything else 1.5-11 % faster staged); 2: all; 0: none
static int g_gemm_lds_epi = 1;
static int g_gemm_asm = 35;        // generated kernels where they cover the call (bits 0, 1), persistent form for multi-round launches (bit 5)
static int g_gemm_group_m = 4;     // m-tiles per group in the workgroup -> tile walk (tile_of); <= 1: N fastest (round 1's order)
void ll_set_conv_halo_internal(int v);
int ll_set_jpeg_split_lanes_internal(int v);
extern "C" int ll_set_tuning(const char* key, int value) {
  if (!strcmp(key, "gemm_variant")) { g_gemm_variant = value; return LL_OK; }
  if (!strcmp(key, "gemm_group_m")) { g_gemm_group_m = value; return LL_OK; }
  if (!strcmp(key, "gemm_variant_wide")) { g_gemm_variant_wide = value; return LL_OK; }
  if (!strcmp(key, "gemm_lds_epi")) {
#ifndef LL_GEMM_DIAG      // bits 0x100 / 0x200 (K-loop staging / compute switched off: results invalid) exist for timing builds only
    if (value < 0 || value > 2) { ll_set_error("ll_set_tuning: gemm_lds_epi=%d (0, 1 or 2; diagnostic bits need -DLL_GEMM_DIAG)", value); return LL_ERR_INVALID_ARG; }
#endif
    g_gemm_lds_epi = value;
    return LL_OK;
  }
  if (!strcmp(key, "attn_variant")) { g_attn.variant = value; return LL_OK; }
  if (!strcmp(key, "attn_xcd")) { g_attn.xcd = value; return LL_OK; }
  if (!strcmp(key, "attn_pp_min_keys")) { g_attn.pp_min_keys = value; return LL_OK; }
  if (!strcmp(key, "attn_asm_min_keys")) { g_attn.asm_min_keys = value; return LL_OK; }
  if (!strcmp(key, "attn_asm")) { g_attn.asm_on = value; return LL_OK; }
  if (!strcmp(key, "conv_halo")) { ll_set_conv_halo_internal(value); return LL_OK; }
  if (!strcmp(key, "jpeg_split_lanes")) {          // lanes per wave of the JPEG subsequence kernels (jpeg_dec.hip)
    if (ll_set_jpeg_split_lanes_internal(value)) { ll_set_error("ll_set_tuning: jpeg_split_lanes=%d (1, 64, or 0 = by subsequence size)", value); return LL_ERR_INVALID_ARG; }
    return LL_OK;
  }
  if (!strcmp(key, "gemm_asm_mfma16")) {
    if (value < -1 || value > 511) { ll_set_error("ll_set_tuning: gemm_asm_mfma16=%d (a mask of 9 bits, one per kernel; -1 = the default)", value); return LL_ERR_INVALID_ARG; }
    g_gemm_asm_mfma16 = value < 0 ? g_gemm_asm_mfma16_default : value;
    return LL_OK;
  }
  if (!strcmp(key, "gemm_asm")) { g_gemm_asm = value; g_gemm_asm_persistent = (value & 32) ? 1 : 0; return LL_OK; }
  ll_set_error("ll_set_tuning: unknown key %s", key);
  return LL_ERR_INVALID_ARG;
}

// ---------------------------------------------------------------------------------------------------------------
// Small-M linear (time embedding, M = B*F <= 8 rows): one wave per output column, weights streamed once.
__global__ __launch_bounds__(256) void linear_small_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                           const bf16* __restrict__ bias, bf16* __restrict__ out, int M,
                                                           int N, int K, int act_in, int act_out) {
  int lane = threadIdx.x & 63;
  int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  float acc[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) acc[m] = 0.f;
  for (int k = lane * 8; k < K; k += 64 * 8) {
    bf16x8 wv = *reinterpret_cast<const bf16x8*>(w + (size_t)n * K + k);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      if (m < M) {
        bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + (size_t)m * K + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float xj = (float)xv[j];
          if (act_in == 1) xj = rbf(silu(xj));
          acc[m] += xj * (float)wv[j];
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    if (m < M) {
      float s = wave_sum(acc[m]);
      if (lane == 0) {
        float v = rbf(s + (float)bias[n]);
        if (act_out == 1) v = silu(v);
        out[(size_t)m * N + n] = (bf16)v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Per-row symmetric int8 quantisation: scale[r] = max|x[r,:]| / 127 (1 if the row is all zero), q = rint(x / scale).
// One wave per row, two passes over the row (the second one is served by L2).  Used for activations (per token) and,
// once at load time, for weights (rows of [N,K] = per output channel).
// F8: the FP8 rowwise form (mx.h): scale = max|x| / 448, q = e4m3fn(clamp(x / scale)), same structure and dispatch.
template <bool F8>
__device__ __forceinline__ float qrow_scale(float mx) {
  return mx > 0.f ? mx / (F8 ? F8_MAX : 127.0f) : 1.0f;
}

// 8 codes of one 16-byte chunk (element j in byte j)
template <bool F8>
__device__ __forceinline__ uint2 qrow_codes8(const bf16x8& v, float inv) {
  unsigned lo = 0, hi = 0;
  if constexpr (F8) {
    lo = f8_code4((float)v[0] * inv, (float)v[1] * inv, (float)v[2] * inv, (float)v[3] * inv);
    hi = f8_code4((float)v[4] * inv, (float)v[5] * inv, (float)v[6] * inv, (float)v[7] * inv);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int a = __float2int_rn((float)v[j] * inv), b = __float2int_rn((float)v[4 + j] * inv);
      a = a < -127 ? -127 : (a > 127 ? 127 : a);
      b = b < -127 ? -127 : (b > 127 ? 127 : b);
      lo |= (unsigned)(a & 0xFF) << (8 * j);
      hi |= (unsigned)(b & 0xFF) << (8 * j);
    }
  }
  return make_uint2(lo, hi);
}

template <bool F8>
__device__ __forceinline__ void quantize_rows_body(const bf16* __restrict__ x, int8_t* __restrict__ q, float* __restrict__ scale,
                                                   int rows, int K, int ldx) {
  int lane = threadIdx.x & 63;
  int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16* xr = x + (size_t)row * ldx;
  float mx = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + k);
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf((float)v[j]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sc = qrow_scale<F8>(mx);
  float inv = 1.0f / sc;
  if (lane == 0) scale[row] = sc;
  int8_t* qr = q + (size_t)row * K;
  for (int k = lane * 8; k < K; k += 512) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + k);
    *reinterpret_cast<uint2*>(qr + k) = qrow_codes8<F8>(v, inv);
  }
}

__global__ __launch_bounds__(256) void quantize_rows_kernel(const bf16* __restrict__ x, int8_t* __restrict__ q,
                                                            float* __restrict__ scale, int rows, int K, int ldx) {
  quantize_rows_body<false>(x, q, scale, rows, K, ldx);
}
__global__ __launch_bounds__(256) void quantize_rows_f8_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ q,
                                                               float* __restrict__ scale, int rows, int K, int ldx) {
  quantize_rows_body<true>(x, (int8_t*)q, scale, rows, K, ldx);
}

// The same arithmetic with the row RESIDENT IN REGISTERS between the two passes (K <= 512 NCH: the FFN hidden, 8960 = 17.5 x 512, is
// 18 x 16 bytes per lane): one read of the row instead of two.  Every chunk's load is issued before the first maximum is taken.
template <int NCH, bool F8>
__device__ __forceinline__ void quantize_rows_reg_body(const bf16* __restrict__ x, int8_t* __restrict__ q, float* __restrict__ scale,
                                                       int rows, int K, int ldx) {
  int lane = threadIdx.x & 63;
  int row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (row >= rows) return;
  const bf16* xr = x + (size_t)row * ldx;
  bf16x8 v[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    int k = lane * 8 + 512 * i;
    if (k < K) v[i] = *reinterpret_cast<const bf16x8*>(xr + k);
    else
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = (bf16)0.f;
  }
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf((float)v[i][j]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sc = qrow_scale<F8>(mx);
  float inv = 1.0f / sc;
  if (lane == 0) scale[row] = sc;
  int8_t* qr = q + (size_t)row * K;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    int k = lane * 8 + 512 * i;
    if (k >= K) continue;
    *reinterpret_cast<uint2*>(qr + k) = qrow_codes8<F8>(v[i], inv);
  }
}

template <int NCH>
__global__ __launch_bounds__(256) void quantize_rows_reg_kernel(const bf16* __restrict__ x, int8_t* __restrict__ q,
                                                                float* __restrict__ scale, int rows, int K, int ldx) {
  quantize_rows_reg_body<NCH, false>(x, q, scale, rows, K, ldx);
}
template <int NCH>
__global__ __launch_bounds__(256) void quantize_rows_f8_reg_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ q,
                                                                   float* __restrict__ scale, int rows, int K, int ldx) {
  quantize_rows_reg_body<NCH, true>(x, (int8_t*)q, scale, rows, K, ldx);
}

// variant 2 = 256x128 / 3-stage ring, 3 = 256x256 (128x64 per wave), 5 = 256x192, 6 = 256x224;
// 0 = auto: the shape with the smallest   rounds(on 256 CUs) x columns x per-flop cost   (v2's 64x64 wave tile costs ~15 %
// more per flop than the 128-row ones; a tile count below the CU count is one round of whatever fills most CUs).
static int pick_gemm_variant(int M, int N) {
  int variant = g_gemm_variant;
  if (N >= 4096 && g_gemm_variant_wide >= 2 && g_gemm_variant_wide <= 6) variant = g_gemm_variant_wide;
  if (variant < 2 || variant > 6 || variant == 4) {
    const int ntm_ = (M + 255) / 256;
    auto cost = [&](int bn, double eff) {
      long tiles = (long)ntm_ * ((N + bn - 1) / bn);
      double rounds = tiles <= 256 ? 1.0 + (256 - tiles) / 256.0 * 0.6 : (double)((tiles + 255) / 256);   // under-filled: idle CUs
      return rounds * bn * eff;
    };
    double c2 = cost(128, 1.15), c3 = cost(256, 1.0), c5 = cost(192, 1.03), c6 = cost(224, 1.03);
    variant = 2;
    double best = c2;
    if (M >= 2048 && N >= 1024) {
      if (c3 < best) { best = c3; variant = 3; }
      if (c5 < best) { best = c5; variant = 5; }
      if (c6 < best) { best = c6; variant = 6; }
    }
  }
  return variant;
}

// What launch_gemm runs for a shape under the current tuning: the one place that turns the variant into tile, LDS bytes, grid and
// the kernel's name (gemm_plan_text prints it; launch_gemm dispatches on it).
struct GemmPlan {
  int variant, bm, bn, lds;
  const char* name;                 // the device symbol, as traces show it
  int ntm, ntn;
};

static GemmPlan gemm_plan(int M, int N) {
  GemmPlan p{};
  p.variant = pick_gemm_variant(M, N);
  p.bm = 256;
  p.bn = p.variant == 3 ? 256 : p.variant == 5 ? 192 : p.variant == 6 ? 224 : BN;
  p.lds = p.variant == 2 ? 3 * V2_STAGE : 2 * (256 + p.bn) * ROWB;
  p.name = p.variant == 2 ? "gemm_kernel_v2" : "gemm_kernel_v5";
  p.ntm = (M + p.bm - 1) / p.bm, p.ntn = (N + p.bn - 1) / p.bn;
  return p;
}

// Which kernel instance and tile ll_gemm_bf16 / ll_gemm_w8a8 / ll_gemm_f8 launch for this shape under the current tuning (host only;
// bench.py's per-kernel table takes its kernel names from here instead of hard-coding them).
static void gemm_plan_text(int M, int N, const char* kind, char* out, int cap) {
  const GemmPlan p = gemm_plan(M, N);
  char walk[48];
  if (g_gemm_group_m > 1) snprintf(walk, sizeof walk, ", groups of %d m-tiles", g_gemm_group_m);
  else snprintf(walk, sizeof walk, ", N fastest");
  snprintf(out, (size_t)cap, "%s<%s> tile %dx%d, %d workgroups%s", p.name, kind, p.bm, p.bn, p.ntm * p.ntn, walk);
}

extern "C" int ll_gemm_plan(int M, int N, int K, int int8, char* out, int cap) {
  LL_REQUIRE(out != nullptr && cap > 0, "ll_gemm_plan: needs an output buffer");
  gemm_plan_text(M, N, int8 ? "i8" : "bf16", out, cap);
  (void)K;
  return LL_OK;
}

// ll_gemm_f8 / ll_gemm_f8_qkv: always the HIP kernels (no generated FP8 form; gemm_asm bit 4 is int8-only)
extern "C" int ll_gemm_plan_f8(int M, int N, int K, char* out, int cap) {
  LL_REQUIRE(out != nullptr && cap > 0, "ll_gemm_plan_f8: needs an output buffer");
  gemm_plan_text(M, N, "f8", out, cap);
  (void)K;
  return LL_OK;
}

// ll_gemm_plan for a call whose epilogue is known: names the generated kernel where ll_gemm_bf16 takes it under the current tuning;
// `plain` = 1 when the call has no V-cache output and no per-batch modulation vector (the block linears of the pipeline except QKV).
extern "C" int ll_gemm_plan_epi(int M, int N, int K, int int8, int epilogue, int plain, char* out, int cap);

extern "C" int ll_t5_rmsnorm(const ll_bf16* x, const ll_bf16* w, ll_bf16* out, int rows, int C, float eps, ll_stream stream);

// ===============================================================================================================
// tuning key gemm_asm (declared near ll_set_tuning): bit 0 = bf16 block linears on the generated one-wave-per-SIMD kernels (gemm_asm.hip) where a
                                // tile width fits (FFN1: 256 x 224 + GELU; N <= 2048: 256 x 128 with bias / gate-residual / residual);
                                // (bit 1 was "also in place of the split-K kernel": that kernel is gone, experiments/gemm_r02_variants.hip)
static bool gemm_asm_wanted(int epilogue) {
  return (g_gemm_asm & 1) && !((g_gemm_asm & 4) && epilogue == LL_EPI_BIAS_GELU) && !((g_gemm_asm & 8) && epilogue != LL_EPI_BIAS_GELU);
}

// the kernel instance of a tiling (GemmPlan::variant); every instance has this signature
typedef void (*gemm_kernel_t)(const char*, const char*, bf16*, int, int, int, size_t, size_t, int, int, int, int, int, EpiArgs);
template <int E, int Q>
static gemm_kernel_t gemm_instance(int variant) {
  switch (variant) {
    case 3: return gemm_kernel_v5<E, Q, 2, 4, 8, 4, 2, false>;
    case 5: return gemm_kernel_v5<E, Q, 2, 4, 8, 3, 1, true>;
    case 6: return gemm_kernel_v5<E, Q, 4, 2, 4, 7, 1, true>;
    default: return gemm_kernel_v2<E, Q>;
  }
}

template <int Q>
static int launch_gemm(const void* x, const void* w, bf16* out, int M, int N, int K, size_t xrow_bytes, size_t wrow_bytes,
                       int ldo, int epilogue, const EpiArgs& ea, hipStream_t s) {
  // gemm_asm: bit 0 = generated kernels for the shapes they cover; bit 2 / bit 3 leave the GELU (256 x 224) / the 128-wide kernels
  // out (A/B of their share in the pipeline's power budget)
  if (Q == GQ_BF16 && gemm_asm_wanted(epilogue) && wrow_bytes == (size_t)K * 2) {
    const int r = gemm_asm_launch((const bf16*)x, (const bf16*)w, out, M, N, K, (int)(xrow_bytes / 2), ldo, epilogue, ea, g_gemm_group_m, s);
    if (r) return r < 0 ? r : 0;                      // launched, or failed (error code); 0 = not covered: the HIP kernels below
  }
  if (Q == GQ_I8 && (g_gemm_asm & 16) && gemm_asm_wanted(epilogue) && xrow_bytes == (size_t)K && wrow_bytes == (size_t)K) {      // bit 4: W8A8 on the generated kernels
    const int r = gemm_asm_launch_i8((const int8_t*)x, (const int8_t*)w, out, M, N, K, ldo, epilogue, ea, g_gemm_group_m, s);
    if (r) return r < 0 ? r : 0;
  }
  const int nk = (Q == GQ_BF16 ? 2 * K : K) / ROWB;
  const GemmPlan p = gemm_plan(M, N);
  // gemm_lds_epi 1: every epilogue but GELU is staged through LDS; 2: all; the timing-experiment bits pass in timing builds only
  const int mode = g_gemm_lds_epi & 3;
  const int lds_epi = (mode == 2 || (mode == 1 && epilogue != LL_EPI_BIAS_GELU) ? 1 : 0) | (GEMM_DIAG ? g_gemm_lds_epi & 0x300 : 0);
  const gemm_kernel_t k = epilogue == LL_EPI_BIAS            ? gemm_instance<LL_EPI_BIAS, Q>(p.variant)
                          : epilogue == LL_EPI_BIAS_GELU     ? gemm_instance<LL_EPI_BIAS_GELU, Q>(p.variant)
                          : epilogue == LL_EPI_BIAS_GATE_RES ? gemm_instance<LL_EPI_BIAS_GATE_RES, Q>(p.variant)
                                                             : gemm_instance<LL_EPI_BIAS_RES, Q>(p.variant);
  (void)ll_lds_attr((const void*)k, p.lds);
  hipLaunchKernelGGL(k, dim3(p.ntm * p.ntn), dim3(512), (size_t)p.lds, s, (const char*)x, (const char*)w, out, M, N, nk, xrow_bytes,
                     wrow_bytes, ldo, p.ntm, p.ntn, g_gemm_group_m, lds_epi, ea);
  return LL_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Host path of the six GEMM entries, written once over a family description:
//   F::Q            operand kind of the kernels;
//   F::check        the family's own preconditions, in the order its entries have always reported them (then check_epilogue);
//   F::xrow, wrow   global row bytes of x [M, K] (leading dimension ldx where the family has one) and w [N, K].
struct FamBF16 {
  static constexpr int Q = GQ_BF16;
  static int check(const char* fn, const void*, const void*, const void*, const void*, const void*, int, int K, int ldx, int) {
    LL_REQUIRE(K > 0 && K % 64 == 0, "%s: K=%d must be a positive multiple of 64", fn, K);
    LL_REQUIRE(ldx >= K && ldx % 8 == 0, "%s: ldx=%d must be >= K and a multiple of 8", fn, ldx);
    return LL_OK;
  }
  static size_t xrow(int, int ldx) { return (size_t)ldx * 2; }
  static size_t wrow(int K) { return (size_t)K * 2; }
};
struct FamW8A8 {
  static constexpr int Q = GQ_I8;
  static int check(const char* fn, const void*, const void* sx, const void*, const void* sw, const void*, int, int K, int, int) {
    LL_REQUIRE(K > 0 && K % 128 == 0, "%s: K=%d must be a positive multiple of 128", fn, K);
    LL_REQUIRE(sx && sw, "%s: activation and weight scales are required", fn);
    return LL_OK;
  }
  static size_t xrow(int K, int) { return (size_t)K; }
  static size_t wrow(int K) { return (size_t)K; }
};
// FP8 rowwise: e4m3fn codes [rows, K] + one fp32 scale per row (mx.h), on the W8A8 kernels' structure (Ty<GQ_F8>)
struct FamF8 {
  static constexpr int Q = GQ_F8;
  static int check(const char* fn, const void* xq, const void* sx, const void* wq, const void* sw, const void* out, int M, int K, int,
                   int ldo) {
    LL_REQUIRE(xq && sx && wq && sw, "%s: codes and scales of both operands are required", fn);
    LL_REQUIRE(out != nullptr, "%s: out is required", fn);
    LL_REQUIRE(K > 0 && K % 128 == 0, "%s: K=%d must be a positive multiple of 128", fn, K);
    LL_REQUIRE(M >= 0, "%s: M=%d", fn, M);
    LL_REQUIRE(ldo % 8 == 0, "%s: ldo=%d must be a multiple of 8", fn, ldo);
    return LL_OK;
  }
  static size_t xrow(int K, int) { return (size_t)K; }
  static size_t wrow(int K) { return (size_t)K; }
};

template <class F>
static int gemm_call(const char* fn, const void* x, const float* sx, const void* w, const float* sw, const ll_bf16* bias, ll_bf16* out,
                     int M, int N, int K, int ldx, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e, const ll_bf16* mod,
                     int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream) {
  if (int rc = F::check(fn, x, sx, w, sw, out, M, K, ldx, ldo)) return rc;
  if (int rc = check_epilogue(fn, M, N, ldo, epilogue, bias, res, e, mod, nmod, gate_idx, rows_per_batch, frame_len)) return rc;
  if (M == 0) return LL_OK;
  EpiArgs ea{(const bf16*)bias, (const bf16*)res, (const bf16*)e, (const bf16*)mod, sx, sw, nmod, gate_idx,
             rows_per_batch, frame_len, frame_len > 0 && rows_per_batch > 0 ? rows_per_batch / frame_len : 0};
  if (int lrc = launch_gemm<F::Q>(x, w, (bf16*)out, M, N, K, F::xrow(K, ldx), F::wrow(K), ldo, epilogue, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch(fn);
}

// Fused QKV projection with the V third written into the KV cache (see EpiArgs::v_out): the family's GEMM with LL_EPI_BIAS, N = 3 C,
// plus the cache destination.  The q and k thirds land in `out` [M, ldo] as usual (they still need the full-row RMSNorm + RoPE of
// ll_qk_norm_rope_kv_store, called with cache_v = NULL afterwards); the v third of `out` is left unwritten.  M = B * L tokens.
template <class F>
static int gemm_call_qkv(const char* fn, const void* x, const float* sx, const void* w, const float* sw, const ll_bf16* bias,
                         ll_bf16* out, int M, int N, int K, int ldx, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start,
                         int roped_offset, int write_len, ll_stream stream) {
  if (int rc = F::check(fn, x, sx, w, sw, out, M, K, ldx, ldo)) return rc;
  if (int rc = check_epilogue(fn, M, N, ldo, LL_EPI_BIAS, bias, nullptr, nullptr, nullptr, 0, 0, 0, 0)) return rc;
  if (int rc = check_v_insert(fn, M, N, B, L, S, write_start, roped_offset, write_len, cache_v)) return rc;
  if (M == 0) return LL_OK;
  EpiArgs ea{(const bf16*)bias, nullptr, nullptr, nullptr, sx, sw, 0, 0, 0, 0, 0};
  set_v_insert(ea, cache_v, N, L, S, write_start, roped_offset, write_len);
  if (int lrc = launch_gemm<F::Q>(x, w, (bf16*)out, M, N, K, F::xrow(K, ldx), F::wrow(K), ldo, LL_EPI_BIAS, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch(fn);
}

extern "C" int ll_gemm_bf16(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N, int K,
                            int ldx, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e, const ll_bf16* mod,
                            int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream) {
  return gemm_call<FamBF16>("ll_gemm_bf16", x, nullptr, w, nullptr, bias, out, M, N, K, ldx, ldo, epilogue, res, e, mod, nmod, gate_idx,
                            rows_per_batch, frame_len, stream);
}

// Small-M split-K (gemm_asm.hip): how many K-ranges the call would be cut into on this device (0 = the path is not taken: the
// shape already fills half the device, N % 128, K too short, no device, or the generated kernels are switched off).
// ll_gemm_bf16 (LL_EPI_BIAS) that also leaves ssq[N / 128][M] (fp32): per row and 128-column n-tile the sum of squares of the bf16
// outputs -- the statistics of the RMSNorm that follows the projection, applied by the consumer (ll_flash_attn_qnorm).
extern "C" int ll_gemm_ssq_planes(int M, int N, int K) {
  if (!gemm_asm_wanted(LL_EPI_BIAS)) return 0;
  const GemmAsmPick p = gemm_asm_pick(GQ_BF16, M, N, K, K, LL_EPI_BIAS, true, false, false, 0, 0);      // the 128-wide bias row
  return p.k && p.k->wn == 128 && N / 128 <= 16 ? N / 128 : 0;
}
extern "C" int ll_gemm_bf16_ssq(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, float* ssq, int M, int N, int K,
                                int ldx, int ldo, ll_stream stream) {
  LL_REQUIRE(K > 0 && K % 64 == 0, "ll_gemm_bf16_ssq: K=%d must be a positive multiple of 64", K);
  LL_REQUIRE(ldx >= K && ldx % 8 == 0, "ll_gemm_bf16_ssq: ldx=%d must be >= K and a multiple of 8", ldx);
  int rc = check_epilogue("ll_gemm_bf16_ssq", M, N, ldo, LL_EPI_BIAS, bias, nullptr, nullptr, nullptr, 0, 0, 0, 0);
  if (rc) return rc;
  LL_REQUIRE(ssq != nullptr && ((size_t)ssq & 3) == 0, "ll_gemm_bf16_ssq: ssq is required");
  LL_REQUIRE(ll_gemm_ssq_planes(M, N, K) > 0 && ldx == K, "ll_gemm_bf16_ssq: %d x %d x %d is not covered by the generated kernel under the current "
             "tuning (ask ll_gemm_ssq_planes first and run ll_gemm_bf16 + ll_rmsnorm instead)", M, N, K);
  if (M == 0) return LL_OK;
  const int r = gemm_asm_ssq_launch((const bf16*)x, (const bf16*)w, (const bf16*)bias, (bf16*)out, ssq, M, N, K, ldx, ldo, g_gemm_group_m,
                                    (hipStream_t)stream);
  if (r < 0) return r;
  LL_REQUIRE(r == 1, "ll_gemm_bf16_ssq: the generated kernel refused a shape its plan accepted");
  return ll_check_launch("ll_gemm_bf16_ssq");
}

extern "C" int ll_gemm_ksplit_plan(int M, int N, int K) {
  if (!gemm_asm_wanted(LL_EPI_BIAS)) return 0;        // bit 0 off, or bit 3 ("leave the 128-wide kernels out"): gemm_asm_128_partial is one of them
  return gemm_ksplit_splits(M, N, K, device_cus());
}
extern "C" long long ll_gemm_ksplit_workspace_bytes(int M, int N, int K) {
  const int S = ll_gemm_ksplit_plan(M, N, K);
  return S ? (long long)S * M * N * 4 : 0;
}
extern "C" int ll_gemm_bf16_ksplit(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N, int K,
                                   int ldx, int ldo, int epilogue, const ll_bf16* res, void* workspace,
                                   long long workspace_bytes, ll_stream stream) {
  LL_REQUIRE(K > 0 && K % 64 == 0, "ll_gemm_bf16_ksplit: K=%d must be a positive multiple of 64", K);
  LL_REQUIRE(ldx >= K && ldx % 8 == 0, "ll_gemm_bf16_ksplit: ldx=%d must be >= K and a multiple of 8", ldx);
  LL_REQUIRE(epilogue == LL_EPI_BIAS || epilogue == LL_EPI_BIAS_RES, "ll_gemm_bf16_ksplit: epilogue %d (bias or bias + residual only)", epilogue);
  int rc = check_epilogue("ll_gemm_bf16_ksplit", M, N, ldo, epilogue, bias, res, nullptr, nullptr, 0, 0, 0, 0);
  if (rc) return rc;
  LL_REQUIRE(workspace_bytes >= 0 && (workspace != nullptr || workspace_bytes == 0), "ll_gemm_bf16_ksplit: workspace_bytes without a workspace");
  if (M == 0) return LL_OK;
  const int S = ll_gemm_ksplit_plan(M, N, K);
  if (S >= 2 && workspace != nullptr) {
    LL_REQUIRE(workspace_bytes >= (long long)S * M * N * 4 && ((size_t)workspace & 15) == 0,
               "ll_gemm_bf16_ksplit: workspace of %lld bytes, need %lld (16-byte aligned)", workspace_bytes, (long long)S * M * N * 4);
    const int r = gemm_asm_ksplit_launch((const bf16*)x, (const bf16*)w, (const bf16*)bias, (bf16*)out, M, N, K, ldx, ldo, epilogue,
                                         (const bf16*)res, (float*)workspace, S, g_gemm_group_m, (hipStream_t)stream, nullptr, 0.f, nullptr);
    if (r) return r < 0 ? r : ll_check_launch("ll_gemm_bf16_ksplit");
  }
  EpiArgs ea{(const bf16*)bias, (const bf16*)res, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
  if (int lrc = launch_gemm<GQ_BF16>(x, w, (bf16*)out, M, N, K, (size_t)ldx * 2, (size_t)K * 2, ldo, epilogue, ea, (hipStream_t)stream)) return lrc;
  return ll_check_launch("ll_gemm_bf16_ksplit");
}

// ll_gemm_bf16_ksplit with LL_EPI_BIAS_RES followed by the T5 RMSNorm of the new residual stream (wan/modules/t5.py:57-63,119-160:
// x = x + linear(...); h = norm(x)): out = x_new [M, ldo], h_out = T5LayerNorm(x_new) [M, N].  On the small-M path the K-range sum,
// bias, residual and the norm are ONE pass over the row; otherwise it is ll_gemm_bf16 + ll_t5_rmsnorm.  Same bits either way.
extern "C" int ll_gemm_bf16_ksplit_t5norm(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N, int K,
                                          int ldx, int ldo, const ll_bf16* res, const ll_bf16* norm_w, float eps, ll_bf16* h_out,
                                          void* workspace, long long workspace_bytes, ll_stream stream) {
  LL_REQUIRE(K > 0 && K % 64 == 0, "ll_gemm_bf16_ksplit_t5norm: K=%d must be a positive multiple of 64", K);
  LL_REQUIRE(ldx >= K && ldx % 8 == 0, "ll_gemm_bf16_ksplit_t5norm: ldx=%d must be >= K and a multiple of 8", ldx);
  LL_REQUIRE(norm_w != nullptr && h_out != nullptr, "ll_gemm_bf16_ksplit_t5norm: needs the norm weight and an output for the normalised rows");
  LL_REQUIRE(ldo == N, "ll_gemm_bf16_ksplit_t5norm: ldo=%d must equal N=%d (the norm runs over whole rows)", ldo, N);
  int rc = check_epilogue("ll_gemm_bf16_ksplit_t5norm", M, N, ldo, LL_EPI_BIAS_RES, bias, res, nullptr, nullptr, 0, 0, 0, 0);
  if (rc) return rc;
  LL_REQUIRE(workspace_bytes >= 0 && (workspace != nullptr || workspace_bytes == 0), "ll_gemm_bf16_ksplit_t5norm: workspace_bytes without a workspace");
  if (M == 0) return LL_OK;
  const int S = ll_gemm_ksplit_plan(M, N, K);
  if (S >= 2 && workspace != nullptr && N <= 4096) {
    LL_REQUIRE(workspace_bytes >= (long long)S * M * N * 4 && ((size_t)workspace & 15) == 0,
               "ll_gemm_bf16_ksplit_t5norm: workspace of %lld bytes, need %lld (16-byte aligned)", workspace_bytes, (long long)S * M * N * 4);
    const int r = gemm_asm_ksplit_launch((const bf16*)x, (const bf16*)w, (const bf16*)bias, (bf16*)out, M, N, K, ldx, ldo, LL_EPI_BIAS_RES,
                                         (const bf16*)res, (float*)workspace, S, g_gemm_group_m, (hipStream_t)stream, (const bf16*)norm_w, eps,
                                         (bf16*)h_out);
    if (r) return r < 0 ? r : ll_check_launch("ll_gemm_bf16_ksplit_t5norm");
  }
  rc = ll_gemm_bf16_ksplit(x, w, bias, out, M, N, K, ldx, ldo, LL_EPI_BIAS_RES, res, workspace, workspace_bytes, stream);
  if (rc) return rc;
  return ll_t5_rmsnorm(out, norm_w, h_out, M, N, eps, stream);
}

extern "C" int ll_gemm_plan_epi(int M, int N, int K, int int8, int epilogue, int plain, char* out, int cap) {
  LL_REQUIRE(out != nullptr && cap > 0, "ll_gemm_plan_epi: needs an output buffer");
  if (gemm_asm_wanted(epilogue) && (!int8 || (g_gemm_asm & 16))) {      // bit 4: W8A8 calls on the generated kernels (launch_gemm<GQ_I8>; never the FP8 calls)
    // plain: 1 = an ordinary call, 0 = per-batch modulation vector (HIP kernels), 2 = the fused QKV call with its V redirect (B = 1)
    const GemmAsmPick p = gemm_asm_pick(int8 ? GQ_I8 : GQ_BF16, M, N, K, K, epilogue, plain != 0, plain == 2, plain == 2 && (2 * (N / 3)) % 192 == 0,
                                        1, int8 ? 0 : device_cus());
    if (p.k) { gemm_asm_plan(p, out, cap); ll_plan_append_knobs(out, cap); return LL_OK; }
  }
  return ll_gemm_plan(M, N, K, int8, out, cap);
}

extern "C" int ll_gemm_w8a8(const int8_t* xq, const float* sx, const int8_t* wq, const float* sw, const ll_bf16* bias,
                            ll_bf16* out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res,
                            const ll_bf16* e, const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch,
                            int frame_len, ll_stream stream) {
  return gemm_call<FamW8A8>("ll_gemm_w8a8", xq, sx, wq, sw, bias, out, M, N, K, K, ldo, epilogue, res, e, mod, nmod, gate_idx,
                            rows_per_batch, frame_len, stream);
}

extern "C" int ll_gemm_f8(const uint8_t* xq, const float* sx, const uint8_t* wq, const float* sw, const ll_bf16* bias, ll_bf16* out,
                          int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e, const ll_bf16* mod,
                          int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream) {
  return gemm_call<FamF8>("ll_gemm_f8", xq, sx, wq, sw, bias, out, M, N, K, K, ldo, epilogue, res, e, mod, nmod, gate_idx,
                          rows_per_batch, frame_len, stream);
}

extern "C" int ll_gemm_bf16_qkv(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N, int K, int ldx,
                                int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset, int write_len,
                                ll_stream stream) {
  return gemm_call_qkv<FamBF16>("ll_gemm_bf16_qkv", x, nullptr, w, nullptr, bias, out, M, N, K, ldx, ldo, cache_v, B, L, S, write_start,
                                roped_offset, write_len, stream);
}

extern "C" int ll_gemm_w8a8_qkv(const int8_t* xq, const float* sx, const int8_t* wq, const float* sw, const ll_bf16* bias,
                                ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start,
                                int roped_offset, int write_len, ll_stream stream) {
  return gemm_call_qkv<FamW8A8>("ll_gemm_w8a8_qkv", xq, sx, wq, sw, bias, out, M, N, K, K, ldo, cache_v, B, L, S, write_start,
                                roped_offset, write_len, stream);
}

extern "C" int ll_gemm_f8_qkv(const uint8_t* xq, const float* sx, const uint8_t* wq, const float* sw, const ll_bf16* bias,
                              ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start,
                              int roped_offset, int write_len, ll_stream stream) {
  return gemm_call_qkv<FamF8>("ll_gemm_f8_qkv", xq, sx, wq, sw, bias, out, M, N, K, K, ldo, cache_v, B, L, S, write_start, roped_offset,
                              write_len, stream);
}

// Row quantisers, int8 and FP8 rowwise (the six kernels above): rows of up to 9216 elements stay in registers between the maximum and
// the rounding pass (same arithmetic, one read).  The FP8 entry also refuses null pointers and a negative row count.
template <bool F8, class TQ>
static int quantize_rows_launch(const char* fn, void (*reg4)(const bf16*, TQ*, float*, int, int, int),
                                void (*reg18)(const bf16*, TQ*, float*, int, int, int), void (*two_pass)(const bf16*, TQ*, float*, int, int, int),
                                const ll_bf16* x, TQ* q, float* scale, int rows, int K, int ldx, ll_stream stream) {
  if (F8) LL_REQUIRE(x != nullptr && q != nullptr && scale != nullptr, "%s: x, codes and scales are required", fn);
  LL_REQUIRE(K > 0 && K % 8 == 0, "%s: K=%d must be a positive multiple of 8", fn, K);
  LL_REQUIRE(ldx >= K && ldx % 8 == 0, "%s: ldx=%d must be >= K and a multiple of 8", fn, ldx);
  if (F8) LL_REQUIRE(rows >= 0, "%s: rows=%d", fn, rows);
  if (rows == 0) return LL_OK;
  hipLaunchKernelGGL(K <= 2048 ? reg4 : K <= 9216 ? reg18 : two_pass, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)x, q, scale, rows, K, ldx);
  return ll_check_launch(fn);
}

extern "C" int ll_quantize_rows(const ll_bf16* x, int8_t* q, float* scale, int rows, int K, int ldx, ll_stream stream) {
  return quantize_rows_launch<false>("ll_quantize_rows", quantize_rows_reg_kernel<4>, quantize_rows_reg_kernel<18>, quantize_rows_kernel,
                                     x, q, scale, rows, K, ldx, stream);
}

extern "C" int ll_quantize_rows_f8(const ll_bf16* x, uint8_t* q, float* scale, int rows, int K, int ldx, ll_stream stream) {
  return quantize_rows_launch<true>("ll_quantize_rows_f8", quantize_rows_f8_reg_kernel<4>, quantize_rows_f8_reg_kernel<18>,
                                    quantize_rows_f8_kernel, x, q, scale, rows, K, ldx, stream);
}

extern "C" int ll_linear_small(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N,
                               int K, int act_in, int act_out, ll_stream stream) {
  LL_REQUIRE(M >= 0 && M <= 8, "ll_linear_small: M=%d must be <= 8", M);
  LL_REQUIRE(K % 8 == 0, "ll_linear_small: K=%d must be a multiple of 8", K);
  if (M == 0 || N == 0) return LL_OK;
  hipLaunchKernelGGL(linear_small_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16*)x,
                     (const bf16*)w, (const bf16*)bias, (bf16*)out, M, N, K, act_in, act_out);
  return ll_check_launch("ll_linear_small");
}
