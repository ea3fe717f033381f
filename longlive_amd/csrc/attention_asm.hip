// Hand-scheduled self-attention for long contiguous key ranges on gfx950: 4 waves x 64 query rows, one wave per SIMD, the whole
// 512-register file owned by the kernel text.  The body is GENERATED (gen/attn_asm_gen.py -> build/attn_asm_body.inc: structure,
// register map, pipeline and the checks it passes on the CPU are described there); this file only computes the workgroup's scalar
// arguments, pins them to the registers the text expects and launches.  Replaces attention() + the sink/window gather
// (wan/modules/attention.py:43-197, causal_model.py:331-360) for the launches ll_flash_attn routes here (tuning key attn_asm).
#include "attention_common.h"

#define ASM_KT 64

// the kernels, then their table: attention_asm_kernels.def is the one list of both
#define FA_EACH "attention_asm_each.inl"
#include "attention_asm_kernels.def"
static const AttnAsmKernel g_fa_kernels[] = {
#define FA_TABLE
#include "attention_asm_kernels.def"
#undef FA_TABLE
};

const AttnAsmKernel* fa_kernel(bool qnorm, int qout_bits) {
  for (const AttnAsmKernel& k : g_fa_kernels)
    if (k.qnorm == qnorm && k.qout_bits == qout_bits) return &k;
  return nullptr;
}

int fa_launch(const AttnAsmKernel& row, AttnAsmArgs& a, int B, int Lq, int H, hipStream_t stream, const char* what) {
  if (int rc = ll_lds_attr(row.fn, FA_LDS)) return rc;
  a.Lq = Lq, a.nqt = (Lq + FA_ROWS - 1) / FA_ROWS;
  void* args[] = {&a.q, &a.k, &a.v, &a.out, &a.Lq, &a.ldq, &a.ldo, &a.ldk, &a.k_batch_stride, &a.kstart, &a.nkeys, &a.c, &a.nqt, &a.xcd,
                  row.qnorm ? (void*)&a.ssq : (void*)&a.sc, row.qnorm ? (void*)&a.nplanes : (void*)&a.ldsc, &a.plane_stride, &a.nw, &a.inv_c,
                  &a.eps};      // (a kernel reads as many as it has: 14, + 2 quantised output, + 6 q-norm)
  (void)hipLaunchKernel(row.fn, dim3(a.nqt * H, 1, B), dim3(256), args, FA_LDS, stream);
  return ll_check_launch(what);
}
