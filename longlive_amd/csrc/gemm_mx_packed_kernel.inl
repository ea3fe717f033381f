// The packed-format GEMM kernel (gemm_mx_packed.hip), written once and compiled under each entry symbol: the includer defines
// MXP_KERNEL (the __global__ symbol), MXP_XOP and MXP_WOP (the operand traits of X and W).  The symbols name what runs in kernel
// traces, profiles/ records and plan strings.
template <int EPI, bool MXOUT>
__global__ __launch_bounds__(512, 1) void MXP_KERNEL(const uint8_t* __restrict__ X, const uint8_t* __restrict__ SX,
                                                     const uint8_t* __restrict__ Wt, const uint8_t* __restrict__ SW,
                                                     bf16* __restrict__ Y, uint8_t* __restrict__ QO, uint8_t* __restrict__ SO, int M,
                                                     int N, int K, int ldo, int ntm, int ntn, EpiArgs ea) {
  typedef MXP_XOP XOp;
  typedef MXP_WOP WOp;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = MxpLds<XOp, WOp>::TILE;
  constexpr bool ALT = WOp::NREAD == XOp::NREAD;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int lid = xcd_remap(blockIdx.x, ntm * ntn), mt_, nt_;
  tile_of(lid, ntm, ntn, MXG_GROUP_M, mt_, nt_);
  const int m0 = mt_ * MXG_BM, n0 = nt_ * MXG_BN;
  const int nk = K / 256, kb = K / 32;
  const size_t rowx = XOp::Fmt::row_bytes((size_t)K), roww = WOp::Fmt::row_bytes((size_t)K);
  const int fr = lane & 15, fg = lane >> 4;
  char* const scl = smem + 2 * TILE;

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc_zero<GQ_BF16>();

  // codes of stage kt: rows x units 16-byte units per operand, one LDS-DMA instruction per 64, NIX + NIW per wave
  constexpr int NIX = MXG_BM * XOp::UNITS / 512, NIW = MXG_BN * WOp::UNITS / 512;
  static_assert(MXG_BM * XOp::UNITS % 512 == 0 && MXG_BN * WOp::UNITS % 512 == 0, "a whole number of LDS-DMA instructions per wave");
  auto stage_tile = [&](int kt, int slot) {
    char* base = smem + slot * TILE;
#pragma unroll
    for (int i = 0; i < NIX + NIW; ++i) {
      const bool isx = i < NIX;
      const uint8_t* g;
      int off;
      if (isx) {
        const int inst = wave * NIX + i;
        g = mxp_unit_src<XOp>(X, rowx, m0, M, kt, inst, lane);
        off = inst * 1024;
      } else {
        const int inst = wave * NIW + (i - NIX);
        g = mxp_unit_src<WOp>(Wt, roww, n0, N, kt, inst, lane);
        off = MXG_BM * XOp::ROW + inst * 1024;
      }
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + off), 16, 0, 0);
    }
  };
  // scale bytes of stage kt: row r's 8 bytes (K-blocks 8 kt .. 8 kt + 7) at r * 8; MXP_SC_LOADS = 2 instructions per wave, one for X
  // and one for W (the W scales are 4 instructions' worth: waves w and w + 4 load the same dwords to the same place)
  auto stage_sc = [&](int kt, int slot) {
    char* base = scl + slot * MXP_SC;
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
      __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(base + MXG_BM * 8 + w4 * 256), 4, 0, 0);
    }
  };
  stage_tile(0, 0);
  stage_sc(0, 0);
  if (nk > 1) stage_sc(1, 1);

  const bool live = m0 + wm * 64 < M;       // wave-uniform
  for (int kt = 0; kt < nk; ++kt) {
    // issued so far, oldest first: ... tile kt, scales kt + 1 (if any).  Tile kt and scales kt must have landed.
    static_assert(MXP_SC_LOADS == 2, "the counted wait below leaves exactly one stage_sc in flight");
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();           // stage kt is in LDS for every wave; tile slot (kt + 1) & 1, scale slot (kt + 2) % 3 are free
    if (kt + 1 < nk) stage_tile(kt + 1, (kt + 1) & 1);
    if (kt + 2 < nk) stage_sc(kt + 2, (kt + 2) % 3);
    const char* xs = smem + (kt & 1) * TILE;
    const char* ws = xs + MXG_BM * XOp::ROW;
    const uint8_t* ss = (const uint8_t*)(scl + (kt % 3) * MXP_SC);
    if (live) {
      __builtin_amdgcn_s_setprio(1);
      i32x4 wf[4][WOp::NREAD], xf[4][XOp::NREAD];
      int sw[4][2], sx[4][2];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int rw = wn * 64 + t * 16 + fr, rx = wm * 64 + t * 16 + fr;
        // one format on both sides: the W and X reads of a unit alternate; otherwise all of W's, then all of X's
        if (ALT) {
#pragma unroll
          for (int j = 0; j < WOp::NREAD; ++j) {
            wf[t][j] = *reinterpret_cast<const i32x4*>(ws + rw * WOp::ROW + WOp::pos(WOp::unit(fg, j), rw) * 16);
            xf[t][j] = *reinterpret_cast<const i32x4*>(xs + rx * XOp::ROW + XOp::pos(XOp::unit(fg, j), rx) * 16);
          }
        } else {
#pragma unroll
          for (int j = 0; j < WOp::NREAD; ++j)
            wf[t][j] = *reinterpret_cast<const i32x4*>(ws + rw * WOp::ROW + WOp::pos(WOp::unit(fg, j), rw) * 16);
#pragma unroll
          for (int j = 0; j < XOp::NREAD; ++j)
            xf[t][j] = *reinterpret_cast<const i32x4*>(xs + rx * XOp::ROW + XOp::pos(XOp::unit(fg, j), rx) * 16);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          sw[t][s] = ss[MXG_BM * 8 + rw * 8 + 4 * s + fg];
          sx[t][s] = ss[rx * 8 + 4 * s + fg];
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        i32x8 wa[4], xb[4];
        // W's reads go to frag by pointer, X's by reference: the values are the same either way, but only in this form do all
        // three kernels compile to the K-loops of the kernels they replace
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          wa[t] = WOp::template frag<const i32x4*>(wf[t], s);
          xb[t] = XOp::template frag<const i32x4(&)[XOp::NREAD]>(xf[t], s);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa[a], xb[b], acc[a][b], WOp::CODE, XOp::CODE, 0, sw[a][s], 0,
                                                                         sx[b][s]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }
  if (MXOUT) {
    gemm_epilogue_gelu_mxout<typename XOp::Fmt>(acc, QO, SO, M, N, m0 + wm * 64, n0 + wn * 64, lane, fr, fg, ea.bias);
  } else if (EPI == LL_EPI_BIAS_GELU) {     // (register form, as gemm_mx_kernel's)
    gemm_epilogue<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, fr, fg, ea);
  } else {
    __builtin_amdgcn_s_barrier();           // every wave has read its last stage's fragments: the ring is free
    gemm_epilogue_lds<EPI, GQ_BF16, 4, 4>(acc, Y, M, N, ldo, m0 + wm * 64, n0 + wn * 64, lane, smem + wave * (64 * EPI_ROW_BYTES(4)), ea);
  }
}
#undef MXP_KERNEL
#undef MXP_XOP
#undef MXP_WOP
