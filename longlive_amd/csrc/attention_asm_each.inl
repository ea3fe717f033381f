// included by attention_asm_kernels.def once per entry, with FA_K = (symbol, form, QNORM, QOUT) defined.  Without FA_TABLE: defines
// the kernel, i.e. hands the entry to the wrapper attention_asm_kernel.inl as the LL_ASM_* parameters it reads (a directive cannot come
// out of a macro, hence one inclusion per entry).  With FA_TABLE: the entry's row of g_fa_kernels.
#ifndef FA_APPLY
#define FA_APPLY(m, entry) m entry
#define FA_STR(x) #x
// the text's file name suffix per form
#define FA_FORM_plain
#define FA_FORM_qn _qn
#define FA_FORM_mx _mx
#define FA_FORM_mx6 _mx6
#define FA_FORM_mx4 _mx4
#define FA_COL_SYM(sym, form, qnorm, qout) sym
#define FA_COL_QNORM(sym, form, qnorm, qout) qnorm
#define FA_COL_QOUT(sym, form, qnorm, qout) qout
#define FA_COL_INC(sym, form, qnorm, qout) FA_INC_PATH(FA_FORM_##form)
#define FA_INC_PATH(suffix) FA_INC_PATH2(suffix)
#define FA_INC_PATH2(suffix) FA_STR(build/attn_asm_body##suffix.inc)
#define FA_COL_ROW(sym, form, qnorm, qout) {(const void*)sym, #sym, qnorm != 0, qout},
#endif

#ifdef FA_TABLE
FA_APPLY(FA_COL_ROW, FA_K)
#else
#define LL_ASM_NAME FA_APPLY(FA_COL_SYM, FA_K)
#define LL_ASM_INC FA_APPLY(FA_COL_INC, FA_K)
#if FA_APPLY(FA_COL_QNORM, FA_K)
#define LL_ASM_QNORM 1
#endif
#if FA_APPLY(FA_COL_QOUT, FA_K)
#define LL_ASM_QOUT FA_APPLY(FA_COL_QOUT, FA_K)
#endif
#include "attention_asm_kernel.inl"
#undef LL_ASM_NAME
#undef LL_ASM_INC
#undef LL_ASM_QNORM
#undef LL_ASM_QOUT
#endif
#undef FA_K
