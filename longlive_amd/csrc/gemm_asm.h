// Host interface of the generated GEMMs (gemm_asm.hip) towards gemm.hip: kernel table row, selection, launches, plan text.
#pragma once
#include "gemm_common.h"

extern int g_gemm_asm_persistent;              // tuning key gemm_asm bit 5 (set by gemm.hip's ll_set_tuning)
extern const int g_gemm_asm_mfma16_default;
extern int g_gemm_asm_mfma16;                  // tuning key gemm_asm_mfma16: OR of the GemmAsmKernel::mfma16_bit whose kernels run their 16x16x32 form

// one row of the kernel table (gemm_asm_kernels.def)
struct GemmAsmKernel {
  const void* fn;
  const char* name;                 // the device symbol, as plans and traces show it
  int wn, epilogue;                 // tile width; the generator's epilogue number (LL_EPI_* for 0..3, 4 = fp32 partial, 5 = bias + row sums)
  bool persistent, i8, m16;
  int mfma16_bit;
};

// What a call runs on the generated kernels: k == nullptr = not covered (the caller takes the HIP kernels)
struct GemmAsmPick {
  const GemmAsmKernel* k;
  int ntm, ntn, grid, lds;          // tiles of 256 x k->wn, workgroups (k->persistent: one per CU, each walks its tiles), dynamic LDS bytes
};
// Pure host function, no HIP call.  kind = GQ_BF16 | GQ_I8; plain = no per-batch modulation vector (bf16: and no int8 scales); v_ok =
// no V-cache output, or one the 192-wide kernel can redirect per tile (one batch element, the V third starting on a tile
// boundary); cus = compute units of the device (0 = none known: classic forms only)
GemmAsmPick gemm_asm_pick(int kind, int M, int N, int K, int ldx, int epilogue, bool plain, bool has_v, bool v_ok, int frame_len, int cus);
// "<symbol><kind> tile ..., N workgroups": the kernel of a pick (p.k != nullptr), as ll_gemm_plan_epi prints it
const char* gemm_asm_plan(const GemmAsmPick& p, char* out, int cap);

// 1 = launched; 0 = shape / epilogue not covered here (the caller takes the HIP kernels); < 0 = an LL_ERR_* code (attribute / launch failed)
int gemm_asm_launch(const bf16* x, const bf16* w, bf16* out, int M, int N, int K, int ldx, int ldo, int epilogue, const EpiArgs& ea,
                    int gm, hipStream_t s);
int gemm_asm_launch_i8(const int8_t* x, const int8_t* w, bf16* out, int M, int N, int K, int ldo, int epilogue, const EpiArgs& ea,
                       int gm, hipStream_t s);
int gemm_asm_ssq_launch(const bf16* x, const bf16* w, const bf16* bias, bf16* out, float* ssq, int M, int N, int K, int ldx, int ldo, int gm,
                        hipStream_t s);
int gemm_ksplit_splits(int M, int N, int K, int cus);
int gemm_asm_ksplit_launch(const bf16* x, const bf16* w, const bf16* bias, bf16* out, int M, int N, int K, int ldx, int ldo,
                           int epilogue, const bf16* res, float* workspace, int splits, int gm, hipStream_t s, const bf16* norm_w,
                           float eps, bf16* h_out);
