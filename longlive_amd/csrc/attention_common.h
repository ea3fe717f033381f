// Host interface shared by the attention files (attention.hip, attention_asm.hip, attention_mx.hip): the tuning keys, key ranges and
// their checks, the output formats, and the generated kernels' table and launcher.  The attention counterpart of gemm_asm.h.
#pragma once
#include "common.h"

#ifndef LL_ATTN_VARIANT_DEFAULT
#define LL_ATTN_VARIANT_DEFAULT 2
#endif
#define LL_LOG2E 1.4426950408889634f      // the kernels take exp2: c = scale * log2 e

// the tuning keys attn_* (gemm.hip: ll_set_tuning writes the fields; attention.hip holds the object)
struct AttnTuning {
  int variant;            // attn_variant         0: simple kernel, 1: software-pipelined, 2: + ping-pong wave groups / the generated kernel for long key ranges
  int pp_min_keys;        // attn_pp_min_keys     key ranges at least this long run the ping-pong loop (cross-attention's 512 keys: one-barrier loop)
  int xcd;                // attn_xcd             XCD-aware workgroup placement (flash_attn_pipe_kernel and the generated kernels)
  int asm_on;             // attn_asm             (0 = flash_attn_pipe_kernel<8, 1>) long contiguous key ranges run flash_attn_asm_kernel
  int asm_min_keys;       // attn_asm_min_keys    the generated kernel from 512 keys on (cross-attention: 22.7 vs 26.8 us, profiles/r03_cross_attn_asm.txt)
};
extern AttnTuning g_attn;

// Up to two key ranges [s, s + n).  attn_merge is the one place where an adjacent second range becomes part of the first (contiguous:
// one range) and an empty one is zeroed.
struct AttnKeys {
  int s0, n0, s1, n1;
};
inline AttnKeys attn_merge(int s0, int n0, int s1, int n1) {
  if (n1 > 0 && s1 == s0 + n0) { n0 += n1; n1 = 0; }
  if (n1 <= 0) { s1 = 0; n1 = 0; }
  return {s0, n0, s1, n1};
}
// the second range in any position but not overlapping the first; why = what the entry point's message adds
inline int attn_check_ranges(const char* fn, int s0, int n0, int s1, int n1, const char* why) {
  LL_REQUIRE(n1 <= 0 || s1 >= s0 + n0 || s1 + n1 <= s0, "%s: key ranges [%d, +%d) and [%d, +%d) overlap%s", fn, s0, n0, s1, n1, why);
  return LL_OK;
}
#define LL_ATTN_TWICE " (their shared keys would be counted twice)"

// output formats of the kernels that emit codes + E8M0 scales (enum ll_qfmt): bits per code, 0 = no such format
inline int qfmt_bits(int fmt) { return fmt == LL_QFMT_MX ? 8 : fmt == LL_QFMT_MX6 ? 6 : fmt == LL_QFMT_MX4 ? 4 : 0; }
inline const char* qfmt_name(int fmt) { return fmt == LL_QFMT_MX ? "mx" : fmt == LL_QFMT_MX6 ? "mx6" : "mx4"; }

// one row of the generated kernels' table (attention_asm_kernels.def)
struct AttnAsmKernel {
  const void* fn;
  const char* name;       // the device symbol, as plans and traces show it
  bool qnorm;             // the q RMSNorm prologue (tail arguments ssq .. eps)
  int qout_bits;          // 0 = bf16 rows, 8 / 6 / 4 = codes + scales of that width (tail arguments sc, ldsc)
};
const AttnAsmKernel* fa_kernel(bool qnorm, int qout_bits);
// The kernels' common arguments in the wrapper's order (attention_asm_kernel.inl; fa_launch fills Lq and nqt), then the tail only some
// rows read: sc, ldsc (quantised output: out = the code rows, ldo in bytes) or ssq .. eps (q-norm)
struct AttnAsmArgs {
  const bf16 *q, *k, *v;
  void* out;
  int Lq, ldq, ldo, ldk;
  long long k_batch_stride;
  int kstart, nkeys;
  float c;
  int nqt, xcd;
  uint8_t* sc;
  int ldsc;
  const float* ssq;
  int nplanes;
  long long plane_stride;
  const bf16* nw;
  float inv_c, eps;
};
enum { FA_ROWS = 256, FA_LDS = 128 * 1024 };      // query rows and dynamic LDS of a workgroup
// the one launch of a table row: ceil(Lq / 256) * H workgroups per batch element; LL_OK or an LL_ERR_* code
int fa_launch(const AttnAsmKernel& row, AttnAsmArgs& a, int B, int Lq, int H, hipStream_t stream, const char* what);
