// Hand-scheduled self-attention for long contiguous key ranges on gfx950: 4 waves x 64 query rows, one wave per SIMD, the whole
// 512-register file owned by the kernel text.  The body is GENERATED (gen/attn_asm_gen.py -> build/attn_asm_body.inc: structure,
// register map, pipeline and the checks it passes on the CPU are described there); this file only computes the workgroup's scalar
// arguments, pins them to the registers the text expects and launches.  Replaces attention() + the sink/window gather
// (wan/modules/attention.py:43-197, causal_model.py:331-360) for the launches ll_flash_attn routes here (tuning key attn_asm).
#include "common.h"

#define ASM_KT 64

#define LL_ASM_NAME flash_attn_asm_kernel
#define LL_ASM_INC "build/attn_asm_body.inc"
#include "attention_asm_kernel.inl"
#undef LL_ASM_NAME
#undef LL_ASM_INC
#define LL_ASM_NAME flash_attn_asm_qn_kernel
#define LL_ASM_INC "build/attn_asm_body_qn.inc"
#define LL_ASM_QNORM 1
#include "attention_asm_kernel.inl"
#undef LL_ASM_QNORM
#undef LL_ASM_NAME
#undef LL_ASM_INC
// Quantised-output forms: the epilogue writes the codes + E8M0 scales of the bf16 rows the plain form would write, in the format the
// output projection reads (gen/attn_asm_gen.py gen_epilogue_q; mx.h / mx6.h / mx4.h); prologue and loop are the plain form's text
#define LL_ASM_NAME flash_attn_asm_mx_kernel
#define LL_ASM_INC "build/attn_asm_body_mx.inc"
#define LL_ASM_QOUT 8
#include "attention_asm_kernel.inl"
#undef LL_ASM_QOUT
#undef LL_ASM_NAME
#undef LL_ASM_INC
#define LL_ASM_NAME flash_attn_asm_mx6_kernel
#define LL_ASM_INC "build/attn_asm_body_mx6.inc"
#define LL_ASM_QOUT 6
#include "attention_asm_kernel.inl"
#undef LL_ASM_QOUT
#undef LL_ASM_NAME
#undef LL_ASM_INC
#define LL_ASM_NAME flash_attn_asm_mx4_kernel
#define LL_ASM_INC "build/attn_asm_body_mx4.inc"
#define LL_ASM_QOUT 4
#include "attention_asm_kernel.inl"
#undef LL_ASM_QOUT
#undef LL_ASM_NAME
#undef LL_ASM_INC
// QNORM form: q = the raw q projection [B, Lq, H * 128] with per-(plane, row) sums of squares ssq[nplanes][B * Lq]; the kernel
// applies WanRMSNorm (weight nw, eps) to its 256 rows x one head in the prologue (wan/modules/model.py:78-86,172)
int flash_attn_asm_qn_launch(const bf16* q, const float* ssq, int nplanes, const bf16* nw, float eps, const bf16* k, const bf16* v,
                             bf16* out, int B, int Lq, int H, int ldq, int ldo, int ldk, long long k_batch_stride, int kstart, int nkeys,
                             float c, int xcd, hipStream_t stream) {
  if (int rc = ll_lds_attr((const void*)flash_attn_asm_qn_kernel, 128 * 1024)) return rc;
  const int nqt = (Lq + 255) / 256;
  hipLaunchKernelGGL(flash_attn_asm_qn_kernel, dim3(nqt * H, 1, B), dim3(256), 128 * 1024, stream, q, k, v, out, Lq, ldq, ldo, ldk,
                     k_batch_stride, kstart, nkeys, c, nqt, xcd, ssq, nplanes, (long long)B * Lq, nw, 1.0f / (float)(H * 128), eps);
  return ll_check_launch("ll_flash_attn_qnorm(asm)");
}

int flash_attn_asm_launch(const bf16* q, const bf16* k, const bf16* v, bf16* out, int B, int Lq, int H, int ldq, int ldo, int ldk,
                          long long k_batch_stride, int kstart, int nkeys, float c, int xcd, int form, hipStream_t stream) {
  if (int rc = ll_lds_attr((const void*)flash_attn_asm_kernel, 128 * 1024)) return rc;
  const int nqt = (Lq + 255) / 256;
  (void)form;
  hipLaunchKernelGGL(flash_attn_asm_kernel, dim3(nqt * H, 1, B), dim3(256), 128 * 1024, stream, q, k, v, out, Lq, ldq, ldo, ldk,
                       k_batch_stride, kstart, nkeys, c, nqt, xcd);
  return ll_check_launch("ll_flash_attn(asm)");
}

// fmt: LL_QFMT_MX / MX6 / MX4 (the caller has checked it).  codes [B * Lq][ldc bytes], scales [B * Lq][lds bytes].
int flash_attn_asm_q_launch(int fmt, const bf16* q, const bf16* k, const bf16* v, uint8_t* codes, int ldc, uint8_t* scales, int lds, int B,
                            int Lq, int H, int ldq, int ldk, long long k_batch_stride, int kstart, int nkeys, float c, int xcd,
                            hipStream_t stream) {
  const int nqt = (Lq + 255) / 256;
#define LL_Q_LAUNCH(KERNEL)                                                                                                          \
  {                                                                                                                                  \
    if (int rc = ll_lds_attr((const void*)KERNEL, 128 * 1024)) return rc;                                                            \
    hipLaunchKernelGGL(KERNEL, dim3(nqt * H, 1, B), dim3(256), 128 * 1024, stream, q, k, v, codes, Lq, ldq, ldc, ldk, k_batch_stride, \
                       kstart, nkeys, c, nqt, xcd, scales, lds);                                                                     \
  }
  if (fmt == LL_QFMT_MX) LL_Q_LAUNCH(flash_attn_asm_mx_kernel)
  else if (fmt == LL_QFMT_MX6) LL_Q_LAUNCH(flash_attn_asm_mx6_kernel)
  else LL_Q_LAUNCH(flash_attn_asm_mx4_kernel)
#undef LL_Q_LAUNCH
  return ll_check_launch("ll_flash_attn_q(asm)");
}
