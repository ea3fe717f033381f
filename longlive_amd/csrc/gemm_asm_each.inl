// included by gemm_asm_kernels.def once per entry, with GA_K = (symbol, wrapper, WN, epilogue, kind, flag, MFMA, bit) defined.
// Without GA_TABLE: defines the kernel, i.e. hands the entry to its wrapper as the GA_* parameters the wrapper reads (a directive
// cannot come out of a macro, hence one inclusion per entry).  With GA_TABLE: the entry's row of g_ga_kernels.
#ifndef GA_APPLY
#define GA_APPLY(m, entry) m entry
#define GA_STR(x) #x
#define GA_WRAP_C 0
#define GA_WRAP_P 1
#define GA_KIND_BF16 0
#define GA_KIND_I8 1
#define GA_FLAG_NONE 0
#define GA_FLAG_SSQ 1
#define GA_FLAG_PARTIAL 2
// the generator's form argument (wrapper, kind, MFMA shape), as the text's file name carries it
#define GA_FORM_C_BF16_32
#define GA_FORM_C_I8_32 _i8
#define GA_FORM_P_BF16_32 _p
#define GA_FORM_C_BF16_16 _m16
#define GA_FORM_P_BF16_16 _pm16
#define GA_COL_SYM(sym, wrap, wn, epi, kind, flag, mfma, bit) sym
#define GA_COL_WRAP(sym, wrap, wn, epi, kind, flag, mfma, bit) GA_WRAP_##wrap
#define GA_COL_WN(sym, wrap, wn, epi, kind, flag, mfma, bit) wn
#define GA_COL_KIND(sym, wrap, wn, epi, kind, flag, mfma, bit) GA_KIND_##kind
#define GA_COL_FLAG(sym, wrap, wn, epi, kind, flag, mfma, bit) GA_FLAG_##flag
#define GA_COL_INC(sym, wrap, wn, epi, kind, flag, mfma, bit) GA_INC_PATH(gemm_asm_##wn##_##epi, GA_FORM_##wrap##_##kind##_##mfma)
#define GA_INC_PATH(base, form) GA_INC_PATH2(base, form)
#define GA_INC_PATH2(base, form) GA_STR(build/base##form.inc)
#define GA_COL_ROW(sym, wrap, wn, epi, kind, flag, mfma, bit) \
  {(const void*)sym, #sym, wn, epi, GA_WRAP_##wrap != 0, GA_KIND_##kind != 0, mfma == 16, bit},
#endif

#ifdef GA_TABLE
GA_APPLY(GA_COL_ROW, GA_K)
#else
#define GA_NAME GA_APPLY(GA_COL_SYM, GA_K)
#define GA_WN GA_APPLY(GA_COL_WN, GA_K)
#define GA_INC GA_APPLY(GA_COL_INC, GA_K)
#if GA_APPLY(GA_COL_KIND, GA_K) == GA_KIND_I8
#define GA_I8 1
#endif
#if GA_APPLY(GA_COL_FLAG, GA_K) == GA_FLAG_SSQ
#define GA_SSQ 1
#elif GA_APPLY(GA_COL_FLAG, GA_K) == GA_FLAG_PARTIAL
#define GA_PARTIAL 1
#endif
#if GA_APPLY(GA_COL_WRAP, GA_K) == GA_WRAP_P
#include "gemm_asm_kernel_p.inl"
#else
#include "gemm_asm_kernel.inl"
#endif
#undef GA_NAME
#undef GA_WN
#undef GA_INC
#undef GA_I8
#undef GA_SSQ
#undef GA_PARTIAL
#endif
#undef GA_K
