// Block linears on packed MX operands, on the block-scaled MFMA of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4 at the FP4 rate, 4x
// bf16 per clock):
//   out[M,N] = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias)
// with packed codes X [M, .] / W [N, .] and one E8M0 scale byte per row and 32-element block of K on both sides.  Three families, one
// kernel body over a pair of operand traits:
//   gemm_mx6_kernel    X E2M3 (mx6.h), W E2M3     cbsz = blgp = 2
//   gemm_mx4w6_kernel  X E2M3,         W E2M1     cbsz = 4, blgp = 2
//   gemm_mx4_kernel    X E2M1 (mx4.h), W E2M1     cbsz = blgp = 4
// The rescale happens inside the MFMA, so the epilogues are the bf16 GEMM's (gemm_common.h), bit for bit the same arithmetic on the
// fp32 sums.  FFN1's MX output is FFN2's activation, so it is written in X's format (gemm_mx_common.h).
//
// Operand map of the 16x16x128 f8f6f4 MFMA with a packed operand of b-bit codes (b = 6: 6 VGPRs, b = 4: 4 VGPRs; the builtin's
// 8-dword argument leaves the rest unread): lane l holds row l & 15 of its operand, g = l >> 4; code i = 0..31 of its fragment sits in
// bits b i .. b i + b - 1 and is k = 32 g + i: the lane's 32 consecutive k are exactly K-block g, whose E8M0 byte its scale VGPR
// carries in byte 0.  This is NOT the e4m3 form's map (gemm_mx.hip: two 16-k chunks, 64 k apart, under the scale of block g), with
// which the E2M3 kernel first ran: rel-L2 1.2 on exact data.  tests/test_mx6_gpu.py, test_mx4_gpu.py and test_mx4a4_gpu.py pin the
// map with exact data.
//
// Structure: 256(M) x 128(N) per workgroup, 8 waves of 64 x 64, operands SWAPPED (A := W, B := X) so a lane's accumulator holds 4
// consecutive N of one row M, as the shared epilogues expect.  One stage = 256 k = two MFMA K-steps = one super-block of a packed
// row (mx6.h, mx4.h), two stages of codes in LDS.  A lane's fragments of both K-steps are contiguous bytes of its row, read as 16-byte
// units; where a unit sits in its LDS row is the trait's `pos`, an involution applied to the per-lane global address of the LDS-DMA
// (whose LDS side is the wave's base + lane x 16) and again by the reader.  Scales (8 bytes per row and stage) go through a 3-slot LDS
// ring, loaded two stages ahead by 4-byte LDS-DMA: the wait at the top of a stage leaves the next stage's scale loads in flight
// across the raw s_barrier.
#include "gemm_mx_common.h"

// ---------------------------------------------------------------------------------------------------------------
// Operand traits: what one side (X or W) of the kernel body needs to know about its code format.
//   ROW, UNITS    LDS row bytes of a 256-k stage, and its 16-byte units;
//   pos(u, r)     LDS position of unit u of row r, its own inverse in u;
//   NREAD, unit   16-byte reads of a lane per stage, and the unit index of read j for lane group fg;
//   frag(f, s)    the MFMA operand of K-step s from those reads (f: the lane's NREAD reads, as an array or a pointer to it);
//   CODE          the MFMA's format code (cbsz / blgp);
//   Fmt           the format's packing (gemm_mx_common.h): global row bytes, MX output.

// E2M3: 192-byte rows.  A lane's fragments of both K-steps are the 48 contiguous bytes at 48 g of its row, three 16-byte units.  LDS
// rows with bit 2 set hold their twelve units rotated by six, which makes the three reads conflict-free in every ds_read_b128 lane
// group.
struct OpE2M3 {
  typedef FmtE2M3 Fmt;
  static constexpr int ROW = 192, UNITS = 12, NREAD = 3, CODE = 2;
  static __device__ __forceinline__ int row_of(int idx) { return idx / UNITS; }             // row and unit of the idx-th unit of a tile
  static __device__ __forceinline__ int unit_of(int idx, int r) { return idx - r * UNITS; }
  static __device__ __forceinline__ int pos(int u, int r) { return (r & 4) ? (u < 6 ? u + 6 : u - 6) : u; }
  static __device__ __forceinline__ int unit(int fg, int j) { return 3 * fg + j; }
  // K-step s: dwords 6 s .. 6 s + 5 of the lane's 12 (the top two of the 8-dword operand are not read)
  template <class F>
  static __device__ __forceinline__ i32x8 frag(F f, int s) {
    return s == 0 ? (i32x8){f[0][0], f[0][1], f[0][2], f[0][3], f[1][0], f[1][1], 0, 0}
                  : (i32x8){f[1][2], f[1][3], f[2][0], f[2][1], f[2][2], f[2][3], 0, 0};
  }
};

// E2M1: 128-byte rows.  A lane's fragments of both K-steps are the 32 contiguous bytes at 32 g of its row, units 2g and 2g + 1.  At a
// 128-byte stride the 16-byte slot of unit u of row r is 8 (r & 1) + u, so the 8 lanes of a lane group reading one unit of 8 rows
// would meet 4-way; LDS row r therefore holds unit u at position u ^ wsw(r), wsw(r) = bit 1 of r | 6 x bit 3 of r.  Conflict-free by
// construction: ds_read_b128's lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31} and their +32 twins) read rows fr in
// S1 = {0-3, 12-15} at one unit u0 and rows S2 = {4-11} at u0 ^ 2 (or the reverse).  Within each row parity, (r >> 1) & 7 runs over
// {0,1,6,7} in S1 and {2,3,4,5} in S2, and wsw maps them to {0,1,6,7} and {0,1,6,7} ^ 2 = {2,3,4,5}: the 16 lanes hit 16 distinct
// slots.
struct OpE2M1 {
  typedef FmtE2M1 Fmt;
  static constexpr int ROW = 128, UNITS = 8, NREAD = 2, CODE = 4;
  static __device__ __forceinline__ int wsw(int r) { return ((r >> 1) & 1) | ((r >> 3) & 1) * 6; }
  static __device__ __forceinline__ int row_of(int idx) { return idx >> 3; }
  static __device__ __forceinline__ int unit_of(int idx, int r) { return idx & 7; }
  static __device__ __forceinline__ int pos(int u, int r) { return u ^ wsw(r); }
  static __device__ __forceinline__ int unit(int fg, int j) { return 2 * fg + j; }
  // K-step s: unit 2 g + s (4 dwords; the top four of the 8-dword operand are not read)
  template <class F>
  static __device__ __forceinline__ i32x8 frag(F f, int s) {
    return (i32x8){f[s][0], f[s][1], f[s][2], f[s][3], 0, 0, 0, 0};
  }
};

#define MXP_SC ((MXG_BM + MXG_BN) * 8)       // 3 KiB of scale bytes per stage
#define MXP_SC_LOADS 2                       // LDS-DMA instructions a wave issues in one stage_sc: the K-loop's vmcnt across the barrier

template <class XOp, class WOp>
struct MxpLds {                              // mx6: 72 KiB of codes per stage, 153 KiB; mx4w6: 64, 137; mx4: 48, 105
  static constexpr int TILE = MXG_BM * XOp::ROW + MXG_BN * WOp::ROW;
  static constexpr int BYTES = 2 * TILE + 3 * MXP_SC;
};

// global source of LDS-DMA instruction `inst` of one operand's stage kt: the 64 lanes fetch 64 consecutive 16-byte units of the
// operand's LDS rows, unit p of LDS row r holding the row's unit pos(p, r).  Rows past the edge re-read the last row (never stored).
template <class Op>
__device__ __forceinline__ const uint8_t* mxp_unit_src(const uint8_t* src, size_t rowb, int r0, int lim, int kt, int inst, int lane) {
  const int idx = inst * 64 + lane, r = Op::row_of(idx), u = Op::pos(Op::unit_of(idx, r), r);
  const int gr = r0 + r < lim ? r0 + r : lim - 1;
  return src + (size_t)gr * rowb + (size_t)kt * Op::ROW + u * 16;
}

// One kernel text under three entry symbols.  The text is included, not called: as a force-inlined body template under thin
// __global__ wrappers the same source compiled to other instruction streams than the kernels it replaced (the wrapper's inlining
// reorders a handful of IR operations and the scheduler follows; gemm_mx4_kernel then measured about 1 % slower per launch), while
// the included form reproduces them.
#define MXP_KERNEL gemm_mx6_kernel
#define MXP_XOP OpE2M3
#define MXP_WOP OpE2M3
#include "gemm_mx_packed_kernel.inl"
#define MXP_KERNEL gemm_mx4w6_kernel
#define MXP_XOP OpE2M3
#define MXP_WOP OpE2M1
#include "gemm_mx_packed_kernel.inl"
#define MXP_KERNEL gemm_mx4_kernel
#define MXP_XOP OpE2M1
#define MXP_WOP OpE2M1
#include "gemm_mx_packed_kernel.inl"

__global__ __launch_bounds__(256) void quantize_mx6_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ qs,
                                                           int rows, int K, int ldx) {
  quantize_mx_body<FmtE2M3>(x, q, qs, rows, K, ldx);
}
__global__ __launch_bounds__(256) void quantize_mx4_kernel(const bf16* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ qs,
                                                           int rows, int K, int ldx) {
  quantize_mx_body<FmtE2M1>(x, q, qs, rows, K, ldx);
}

// ---------------------------------------------------------------------------------------------------------------
// Host side: gemm_mx_common.h's path over three family descriptors.
#define MXP_FAMILY(Fam, tag, kern, out_word, XOp, WOp)                                \
  struct Fam {                                                                        \
    MX_FAMILY_NAMES(tag);                                                             \
    static constexpr const char *word = out_word, *plan_stage = ", 256 k per stage";  \
    static constexpr int KGRAN = 256, NGRAN = 256, LDS = MxpLds<XOp, WOp>::BYTES;     \
    template <int EPI, bool MXOUT>                                                    \
    static mx_gemm_kernel_t select() { return kern<EPI, MXOUT>; }                     \
  }
MXP_FAMILY(FamMx6, "mx6", gemm_mx6_kernel, "MXFP6", OpE2M3, OpE2M3);
MXP_FAMILY(FamMx4w6, "mx4w6", gemm_mx4w6_kernel, "MXFP6", OpE2M3, OpE2M1);
MXP_FAMILY(FamMx4, "mx4", gemm_mx4_kernel, "MXFP4", OpE2M1, OpE2M1);

extern "C" int ll_quantize_mx6(const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx, ll_stream stream) {
  return mx_quantize<FmtE2M3>("ll_quantize_mx6", quantize_mx6_kernel, x, q, qs, rows, K, ldx, stream);
}
extern "C" int ll_quantize_mx4(const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx, ll_stream stream) {
  return mx_quantize<FmtE2M1>("ll_quantize_mx4", quantize_mx4_kernel, x, q, qs, rows, K, ldx, stream);
}

extern "C" int ll_gemm_plan_mx6(int M, int N, int K, char* out, int cap) { return mx_gemm_plan<FamMx6>(M, N, K, out, cap); }
extern "C" int ll_gemm_mx6(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
               uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e,
               const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream) {
  return mx_gemm<FamMx6>(xq, sx, wq, sw, bias, out, q_out, s_out, M, N, K, ldo, epilogue, res, e, mod, nmod, gate_idx, rows_per_batch,
                 frame_len, stream);
}
extern "C" int ll_gemm_mx6_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
               ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset,
               int write_len, ll_stream stream) {
  return mx_gemm_qkv<FamMx6>(xq, sx, wq, sw, bias, out, M, N, K, ldo, cache_v, B, L, S, write_start, roped_offset, write_len, stream);
}

extern "C" int ll_gemm_plan_mx4w6(int M, int N, int K, char* out, int cap) { return mx_gemm_plan<FamMx4w6>(M, N, K, out, cap); }
extern "C" int ll_gemm_mx4w6(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
               uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e,
               const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream) {
  return mx_gemm<FamMx4w6>(xq, sx, wq, sw, bias, out, q_out, s_out, M, N, K, ldo, epilogue, res, e, mod, nmod, gate_idx, rows_per_batch,
                 frame_len, stream);
}
extern "C" int ll_gemm_mx4w6_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
               ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset,
               int write_len, ll_stream stream) {
  return mx_gemm_qkv<FamMx4w6>(xq, sx, wq, sw, bias, out, M, N, K, ldo, cache_v, B, L, S, write_start, roped_offset, write_len, stream);
}

extern "C" int ll_gemm_plan_mx4(int M, int N, int K, char* out, int cap) { return mx_gemm_plan<FamMx4>(M, N, K, out, cap); }
extern "C" int ll_gemm_mx4(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
               uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e,
               const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream) {
  return mx_gemm<FamMx4>(xq, sx, wq, sw, bias, out, q_out, s_out, M, N, K, ldo, epilogue, res, e, mod, nmod, gate_idx, rows_per_batch,
                 frame_len, stream);
}
extern "C" int ll_gemm_mx4_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias,
               ll_bf16* out, int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset,
               int write_len, ll_stream stream) {
  return mx_gemm_qkv<FamMx4>(xq, sx, wq, sw, bias, out, M, N, K, ldo, cache_v, B, L, S, write_start, roped_offset, write_len, stream);
}
