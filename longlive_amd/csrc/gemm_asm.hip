// Hand-scheduled bf16 GEMMs for the block linears on gfx950: 4 waves per 256 x WN output tile, one wave per SIMD, accumulators in
// AGPRs, generated body (gen/gemm_asm_gen.py -> build/gemm_asm_<WN>_<EPI>[_<form>].inc; structure, pipeline and CPU checks are
// described there).  This file computes each workgroup's tile and scalar arguments, pins them to the registers the text expects and
// launches.  Replaces gemm_kernel_v5 / v2 for the shapes ll_gemm_bf16 routes here (tuning key gemm_asm); rounding points as gemm_common.h.
#include "gemm_asm.h"

// the kernels, then their table: gemm_asm_kernels.def is the one list of both
#define GA_EACH "gemm_asm_each.inl"
#include "gemm_asm_kernels.def"
static const GemmAsmKernel g_ga_kernels[] = {
#define GA_TABLE
#include "gemm_asm_kernels.def"
#undef GA_TABLE
};
enum { GA_EPI_PARTIAL = 4, GA_EPI_SSQ = 5 };      // the generator's epilogue numbers past LL_EPI_*

int g_gemm_asm_persistent = 1;
// the shipped mask (profiles/gemm_mfma16_ab.md; ll_set_tuning value -1 restores it): every bf16 kernel.  The family moves as one: the
// suite holds its members to each other bit for bit (classic against persistent, the fused QKV projection on the 192-wide kernel
// against the unfused one on the 128-wide, the row-sum kernel against the bias kernel), which needs one order of the fp32 sum.
extern const int g_gemm_asm_mfma16_default = 511;
int g_gemm_asm_mfma16 = g_gemm_asm_mfma16_default;

// The 32-shape row of (kind, width, epilogue, form), or its MFMA-16 row where the tuning mask holds the row's bit; nullptr = no such
// kernel.  (30 rows of 5 compares: nothing beside the launch it precedes.)
static const GemmAsmKernel* ga_kernel(bool i8, int wn, int epilogue, bool persistent) {
  const GemmAsmKernel* k32 = nullptr;
  for (const GemmAsmKernel& k : g_ga_kernels)
    if (k.i8 == i8 && k.wn == wn && k.epilogue == epilogue && k.persistent == persistent) {
      if (!k.m16) k32 = &k;
      else if (g_gemm_asm_mfma16 & k.mfma16_bit) return &k;
    }
  return k32;
}

// dynamic LDS of a kernel of tile width wn.  gen/gemm_asm_gen.py Cfg.lds_bytes: 3 W slots of WN rows x 128 B + 2 X units of 8 KiB per wave
static int ga_lds(int wn) { return 3 * wn * 128 + 4 * 2 * 8192; }

// tile width of the generated kernel that covers this call, 0 = none
static int ga_width(bool i8, int M, int N, int K, int ldx, int epilogue, bool plain, bool has_v, bool v_ok, int frame_len) {
  const int kstep = i8 ? 128 : 64;      // elements of a K-step; the pipeline needs four.  Row offsets of a 256-row tile are 32-bit BYTE counts
  if (!plain || M <= 0 || K % kstep != 0 || K < 4 * kstep) return 0;
  if (i8 ? (long long)256 * K >= 0x7fffffffLL      // (W8A8 rows are dense: ldx = K)
         : (ldx % 8) != 0 || (long long)256 * ldx * 2 >= 0x7fffffffLL || (long long)256 * K * 2 >= 0x7fffffffLL) return 0;
  if (epilogue == LL_EPI_BIAS_GATE_RES && frame_len <= 0) return 0;
  if (has_v) return (v_ok && epilogue == LL_EPI_BIAS && N % 192 == 0) ? 192 : 0;
  if (epilogue == LL_EPI_BIAS_GELU) return N % 224 == 0 ? 224 : 0;
  if (epilogue == LL_EPI_BIAS && N > 2048 && N % 192 == 0) return 192;
  if (i8) return N % 128 == 0 && N <= 2048 ? 128 : 0;      // W8A8: no 256-wide kernel, the 128-wide ones for any epilogue left
  if (epilogue == LL_EPI_BIAS && M <= 1024 && N >= 16384 && N % 256 == 0) return 256;      // umT5's gated FFN (512 x 20480 x 4096): 160 tiles of 256 x 256 in ONE round,
                                                                                             // half the L2 bytes per FLOP of the 128-wide kernel (which is L2-bound at ~29 B/clk/CU)
  if (N % 128 == 0 && (N <= 2048 || M <= 1024) &&      // wide outputs of few rows (umT5's gated FFN, 512 x 20480): the HIP choice there is 256 x 128 as well
      (epilogue == LL_EPI_BIAS || epilogue == LL_EPI_BIAS_GATE_RES || epilogue == LL_EPI_BIAS_RES)) return 128;
  return 0;
}

GemmAsmPick gemm_asm_pick(int kind, int M, int N, int K, int ldx, int epilogue, bool plain, bool has_v, bool v_ok, int frame_len, int cus) {
  const bool i8 = kind == GQ_I8;
  GemmAsmPick p{};
  const int wn = ga_width(i8, M, N, K, ldx, epilogue, plain, has_v, v_ok, frame_len);
  if (!wn) return p;
  // the width fixes the epilogue of the 192 / 224 / 256 kernels; the 128-wide ones are bias, gate-res, or (everything else) res
  const int epi = wn == 224 ? LL_EPI_BIAS_GELU : wn != 128 || epilogue == LL_EPI_BIAS ? LL_EPI_BIAS
                  : epilogue == LL_EPI_BIAS_GATE_RES ? LL_EPI_BIAS_GATE_RES : LL_EPI_BIAS_RES;
  p.ntm = (M + 255) / 256, p.ntn = N / wn, p.lds = ga_lds(wn);
  // persistent form (tuning key gemm_asm bit 5, bf16 only): a launch with more tiles than CUs runs ONE workgroup per CU that walks its
  // tiles and stages the next tile's first pieces under the current epilogue (FFN1: 760 tiles, QKV: 456, the recache forward's
  // N = 1536 linears: 888) -- one pipeline fill per launch instead of one per round
  const int pcus = cus & ~7;
  if (!i8 && g_gemm_asm_persistent && pcus >= 8 && p.ntm * p.ntn > pcus) p.k = ga_kernel(i8, wn, epi, true);
  p.grid = p.k ? pcus : p.ntm * p.ntn;
  if (!p.k) p.k = ga_kernel(i8, wn, epi, false);
  return p;
}

const char* gemm_asm_plan(const GemmAsmPick& p, char* out, int cap) {
  const int wn = p.k->wn, tiles = p.ntm * p.ntn;
  if (p.k->persistent)
    snprintf(out, (size_t)cap, "%s<bf16> tile 256x%d (4 waves x 64 rows, one wave per SIMD, generated schedule), %d persistent workgroups "
             "walk %d tiles, next tile staged under the epilogue", p.k->name, wn, p.grid, tiles);
  else
    snprintf(out, (size_t)cap, "%s<%s> tile 256x%d (4 waves x 64 rows, one wave per SIMD, generated schedule), %d workgroups", p.k->name,
             p.k->i8 ? "i8" : "bf16", wn, tiles);
  return out;
}

// The kernels' 22 common arguments in the wrappers' order (gemm_asm_kernel.inl), then the tail that only some rows read: sx, sw
// (W8A8) or ssq (the row-sum kernel)
struct GemmAsmArgs {
  const void *x, *w;
  const bf16* bias;
  bf16* out;
  const bf16 *res, *gate;
  int M, N, K, ldx, ldo, frame_len, gate_stride, ntm, ntn, gm;
  bf16* v_out;
  int v_col0, v_C, v_shift, v_lo, v_hi;
  const float *sx, *sw;
  float* ssq;
};

// the one launch of a table row: 1 = launched, < 0 = an LL_ERR_* code
static int ga_launch(const GemmAsmKernel& k, int grid, hipStream_t s, GemmAsmArgs& a, const char* what) {
  const int lds = ga_lds(k.wn);
  if (int rc = ll_lds_attr(k.fn, lds)) return rc;
  void* args[] = {&a.x, &a.w, &a.bias, &a.out, &a.res, &a.gate, &a.M, &a.N, &a.K, &a.ldx, &a.ldo, &a.frame_len, &a.gate_stride, &a.ntm, &a.ntn,
                  &a.gm, &a.v_out, &a.v_col0, &a.v_C, &a.v_shift, &a.v_lo, &a.v_hi, k.i8 ? (void*)&a.sx : (void*)&a.ssq, &a.sw};
  if (hipLaunchKernel(k.fn, dim3(grid), dim3(256), args, (size_t)lds, s) != hipSuccess) return ll_check_launch(what);
  return 1;
}

// ll_gemm_bf16 / ll_gemm_bf16_qkv (kind GQ_BF16) and ll_gemm_w8a8 / ll_gemm_w8a8_qkv (GQ_I8: int8 operands with row strides K, fp32
// scales sx [M] / sw [N]; the same tile widths, epilogues and V-cache redirect.  Integer sums are exact and the epilogue applies
// gemm_common.h's operations in its order, so the results are bit-identical to the HIP W8A8 kernels)
static int ga_gemm(int kind, const void* x, const void* w, bf16* out, int M, int N, int K, int ldx, int ldo, int epilogue, const EpiArgs& ea,
                   int gm, hipStream_t s) {
  const bool has_v = ea.v_out != nullptr, i8 = kind == GQ_I8;
  const GemmAsmPick p = gemm_asm_pick(kind, M, N, K, ldx, epilogue, ea.mod == nullptr && (i8 || ea.sx == nullptr), has_v,
                                      has_v && ea.v_L == M && ea.v_col0 % 192 == 0 && ea.v_C > 0, ea.frame_len, i8 ? 0 : device_cus());
  if (!p.k) return 0;
  GemmAsmArgs a{x, w, ea.bias, out, ea.res, epilogue == LL_EPI_BIAS_GATE_RES ? ea.e + (size_t)ea.gate_idx * N : nullptr, M, N, K, ldx, ldo,
                ea.frame_len, ea.nmod * N * 2, p.ntm, p.ntn, gm, ea.v_out, ea.v_col0, ea.v_C, ea.v_write_start - ea.v_roped_offset,
                ea.v_roped_offset, ea.v_roped_offset + ea.v_write_len, ea.sx, ea.sw, nullptr};
  return ga_launch(*p.k, p.grid, s, a, "gemm_asm");
}
int gemm_asm_launch(const bf16* x, const bf16* w, bf16* out, int M, int N, int K, int ldx, int ldo, int epilogue, const EpiArgs& ea,
                    int gm, hipStream_t s) {
  return ga_gemm(GQ_BF16, x, w, out, M, N, K, ldx, ldo, epilogue, ea, gm, s);
}
int gemm_asm_launch_i8(const int8_t* x, const int8_t* w, bf16* out, int M, int N, int K, int ldo, int epilogue, const EpiArgs& ea,
                       int gm, hipStream_t s) {
  if (ea.sx == nullptr || ea.sw == nullptr) return 0;
  return ga_gemm(GQ_I8, x, w, out, M, N, K, K, ldo, epilogue, ea, gm, s);
}

// The bias kernel that also leaves per-row sums of squares of its outputs: ssq[N / 128][M] fp32 (plane = n-tile).  1 = launched,
// 0 = not covered, < 0 = error.
int gemm_asm_ssq_launch(const bf16* x, const bf16* w, const bf16* bias, bf16* out, float* ssq, int M, int N, int K, int ldx, int ldo, int gm,
                        hipStream_t s) {
  const GemmAsmPick p = gemm_asm_pick(GQ_BF16, M, N, K, ldx, LL_EPI_BIAS, true, false, false, 0, 0);      // (cus = 0: no persistent row-sum kernel)
  if (!p.k || p.k->wn != 128) return 0;
  const GemmAsmKernel* k = ga_kernel(false, 128, GA_EPI_SSQ, false);
  GemmAsmArgs a{x, w, bias, out, nullptr, nullptr, M, N, K, ldx, ldo, 0, 0, p.ntm, p.ntn, gm, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, ssq};
  return ga_launch(*k, p.grid, s, a, k->name);
}

// ---------------------------------------------------------------------------------------------------------------
// Small-M split-K (umT5's linears at 512 tokens, wan/modules/t5.py:65-117; the text K/V projections): a grid of
// ceil(M / 256) x (N / 128) tiles fills a quarter of the device, so K is cut into `splits` ranges -- each workgroup of
// gemm_asm_128_partial writes its tile's fp32 accumulators to workspace[split][M][N], and one elementwise pass sums the ranges in
// a fixed order and applies the epilogue (bias, or bias + residual) with gemm_common.h's rounding points.
template <int EPI>
__global__ __launch_bounds__(256) void gemm_ksplit_reduce_kernel(const float* __restrict__ part, int splits, int M, int N,
                                                                 const bf16* __restrict__ bias, const bf16* __restrict__ res,
                                                                 bf16* __restrict__ out, int ldo) {
  const int n8 = N / 8;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)M * n8) return;
  const int m = (int)(idx / n8), n = (int)(idx - (long long)m * n8) * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int s = 0; s < splits; ++s) {                  // fixed order: bit-identical run to run
    const float4* p = reinterpret_cast<const float4*>(part + ((size_t)s * M + m) * N + n);
    float4 a = p[0], b = p[1];
    acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w; acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
  }
  bf16x8 bv = *reinterpret_cast<const bf16x8*>(bias + n), o;
  bf16x8 rv;
  if (EPI == LL_EPI_BIAS_RES) rv = *reinterpret_cast<const bf16x8*>(res + (size_t)m * ldo + n);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bf16 v = (bf16)(acc[j] + (float)bv[j]);
    o[j] = EPI == LL_EPI_BIAS_RES ? (bf16)((float)rv[j] + (float)v) : v;
  }
  *reinterpret_cast<bf16x8*>(out + (size_t)m * ldo + n) = o;
}

// The same pass for the residual stream of umT5 (t5.py:119-160: x = x + linear(...); h = T5LayerNorm(x)): one workgroup per row sums
// the K-ranges, adds bias and residual (x_new, written to `out`) and applies the T5 RMSNorm to that row at once (h_out) -- the
// arithmetic, its order and its rounding points are gemm_ksplit_reduce_kernel's followed by t5_rmsnorm_kernel's (t5.hip: thread t
// owns columns 8 t + 2048 i, t5_block_sum), so the pair of outputs is bit-identical to the two launches it replaces.
// N <= 4096 (two column groups per thread).
__global__ __launch_bounds__(256) void gemm_ksplit_reduce_norm_kernel(const float* __restrict__ part, int splits, int M, int N,
                                                                      const bf16* __restrict__ bias, const bf16* __restrict__ res,
                                                                      bf16* __restrict__ out, int ldo, const bf16* __restrict__ nw,
                                                                      float eps, bf16* __restrict__ h_out) {
  __shared__ float sh[4];
  const int m = blockIdx.x;
  bf16x8 xn[2];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = threadIdx.x * 8 + 2048 * i;
    if (n < N) {
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      for (int s = 0; s < splits; ++s) {
        const float4* p = reinterpret_cast<const float4*>(part + ((size_t)s * M + m) * N + n);
        float4 a = p[0], b = p[1];
        acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w; acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
      }
      bf16x8 bv = *reinterpret_cast<const bf16x8*>(bias + n), rv = *reinterpret_cast<const bf16x8*>(res + (size_t)m * ldo + n), o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bf16 v = (bf16)(acc[j] + (float)bv[j]);
        o[j] = (bf16)((float)rv[j] + (float)v);
        ss += (float)o[j] * (float)o[j];
      }
      xn[i] = o;
      *reinterpret_cast<bf16x8*>(out + (size_t)m * ldo + n) = o;
    }
  }
  ss = t5_block_sum(ss, sh);
  const float r = rsqrtf(ss / (float)N + eps);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = threadIdx.x * 8 + 2048 * i;
    if (n < N) {
      bf16x8 g = *reinterpret_cast<const bf16x8*>(nw + n), o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)g[j] * rbf((float)xn[i][j] * r));
      *reinterpret_cast<bf16x8*>(h_out + (size_t)m * N + n) = o;
    }
  }
}

// K-ranges the small-M path cuts this call into on a device of `cus` compute units; 0 = not taken.  The NUMBER of ranges depends
// on N and K only (the order of the fp32 sum must not change with the batch: M = 512 and M = 1024 give the same bits per row);
// M only decides whether the path is taken at all (the plain kernels would fill less than half of the device).
int gemm_ksplit_splits(int M, int N, int K, int cus) {
  if (M <= 0 || N <= 0 || N % 128 != 0 || K % 64 != 0 || K < 1024 || cus <= 0) return 0;
  const long long tiles = (long long)((M + 255) / 256) * (N / 128);
  if (tiles * 2 > cus) return 0;                        // the plain kernels already fill half the device
  const int nk = K / 64;
  int S = (int)((long long)cus * 64 / N);               // fills the device at 512 rows (tiles = N / 64 there)
  if (S > 4) S = 4;
  if (S > nk / 8) S = nk / 8;                           // at least 8 K-steps per range: the pipeline fill is ~3
  while (S >= 2 && (S - 1) * ((nk + S - 1) / S) >= nk) --S;      // every range non-empty
  if (S < 2 || tiles * S > 2 * cus) return 0;
  return S;
}
// 1 = launched (two launches), 0 = not covered, < 0 = an LL_ERR_* code
int gemm_asm_ksplit_launch(const bf16* x, const bf16* w, const bf16* bias, bf16* out, int M, int N, int K, int ldx, int ldo,
                           int epilogue, const bf16* res, float* workspace, int splits, int gm, hipStream_t s, const bf16* norm_w,
                           float eps, bf16* h_out) {
  if (splits < 2 || (epilogue != LL_EPI_BIAS && epilogue != LL_EPI_BIAS_RES) || (ldx % 8) != 0) return 0;      // (ldo % 8 == 0: check_epilogue)
  if ((long long)256 * ldx * 2 >= 0x7fffffffLL || (long long)256 * K * 2 >= 0x7fffffffLL) return 0;
  const GemmAsmKernel* k = ga_kernel(false, 128, GA_EPI_PARTIAL, false);
  const int ntm = (M + 255) / 256, ntn = N / 128, per = (K / 64 + splits - 1) / splits;
  // the partial kernel reuses three slots (GA_PARTIAL in gemm_asm_kernel.inl): Y is the fp32 workspace [splits][M][N], ldo = N counts
  // FLOATS, and v_col0 carries the number of K-steps per split
  GemmAsmArgs a{x, w, nullptr, (bf16*)workspace, nullptr, nullptr, M, N, K, ldx, /*ldo*/ N, 0, 0, ntm, ntn, gm, nullptr, /*v_col0*/ per, 0, 0, 0, 0,
                nullptr, nullptr, nullptr};
  if (int rc = ga_launch(*k, ntm * ntn * splits, s, a, k->name); rc != 1) return rc;
  const long long threads = (long long)M * (N / 8);
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  if (norm_w != nullptr)       // (the caller checked: bias + residual, N <= 4096)
    hipLaunchKernelGGL(gemm_ksplit_reduce_norm_kernel, dim3(M), block, 0, s, (const float*)workspace, splits, M, N, bias, res,
                       out, ldo, norm_w, eps, h_out);
  else if (epilogue == LL_EPI_BIAS_RES)
    hipLaunchKernelGGL((gemm_ksplit_reduce_kernel<LL_EPI_BIAS_RES>), grid, block, 0, s, (const float*)workspace, splits, M, N, bias, res, out, ldo);
  else
    hipLaunchKernelGGL((gemm_ksplit_reduce_kernel<LL_EPI_BIAS>), grid, block, 0, s, (const float*)workspace, splits, M, N, bias, res, out, ldo);
  return 1;
}
