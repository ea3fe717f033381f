// MXFP8 self-attention over a block-scaled shadow of the KV cache (set_attn_quant("mxfp8")).
//
// The bf16 cache stays the master.  kv_shadow_mx_kernel derives from it, per layer:
//   K^ codes [B, S32, H, 128] e4m3fn + scales [B, S32, H, 4]: every slot's K row quantised along channels (ll_quantize_mx of the row);
//   V^ codes [B, H, S32/32, 128, 32] + scales [B, H, S32/32, 128]: for every (head, channel d, 32-slot block j anchored at slot 32 j)
//       the MX rule (mx.h) over V[32 j .. 32 j + 31, head, d]; slots >= S read as 0.  The 32 codes of a (j, d) row are stored in
//       FRAGMENT ORDER: position 16 hh + jj holds slot 32 j + (jj & 3) + 8 (jj >> 2) + 4 hh, the key order in which a score tile's
//       accumulator registers arrive, so the kernel's A fragments are plain 16-byte LDS reads.
// S32 = S rounded up to a multiple of 32.
//
// flash_attn_mx_kernel (flash_attn_kernel's structure, attention.hip): 4 waves x 32 queries of one head per workgroup, key tiles of
// 64 slots staged global -> registers -> LDS (double buffered, one barrier per tile), both products on
// v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands:
//   S^T = K^ Q^^T   (A := K^ tile, B := Q^^T in registers): a lane owns one query, row reductions stay in-lane (+ one lane ^ 32 step);
//   P^  = e4m3fn(RNE(exp2(c s - M)))  with the lazy max of the generated bf16 kernel: M (= c m_ref) moves only when a tile's c * max
//         exceeds it by more than THR = 8, so P <= 2^8 < 448 and P^ goes in with the unit scale (byte 127);
//   O^T += V^^T P^^T  (A := V^ tile with one scale byte per (d, 32-slot block), B := P^ straight from the score accumulators);
//   l   = sum of the ROUNDED P^ (v_cvt_pk_f32_fp8 back), so O / l is an exact convex combination of V^ rows.
// Operand map of the 32x32x64 form with 8-bit operands (measured with exact data: tests/test_mx_attn_gpu.py): lane l holds row
// l & 31 of its operand, h = l >> 5; bytes 0-15 of its fragment are k = 16 h .. 16 h + 15 and bytes 16-31 are k = 32 + 16 h .. + 15;
// its scale register carries (byte 0) the E8M0 byte of (row l & 31, K-block h) = k 32 h .. 32 h + 31.  A score tile's lane (q, h)
// holds keys (i & 3) + 8 (i >> 2) + 4 h of its 32 (i = 0..15): the 16 registers of key block kb = 0 are bytes 0-15 of the P^
// fragment (hardware K-block 0 = slots base .. base + 31), those of kb = 1 bytes 16-31 (K-block 1), and V^'s fragment order matches.
// Key tiles start at each segment's start rounded down to 32 (so a tile holds exactly two V^ blocks); slots outside the segment are
// masked to -inf.  Adjacent segments are merged first (as ll_flash_attn does).
#include <stdio.h>

#include "attention_common.h"
#include "mx.h"
#include "mx4.h"
#include "mx6.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4v;

#define MXA_KT 64                                  // keys per tile
#define MXA_NW 4                                   // waves per workgroup (32 queries each)
#define MXA_THR 8.0f                               // lazy-max threshold, log2 units (gen/attn_asm_gen.py THR)
#define MXA_KB (MXA_KT * 128)                      // K^ codes of a tile: 8 KiB
#define MXA_VB (2 * 128 * 32)                      // V^ codes of a tile (two blocks): 8 KiB
#define MXA_STAGE (MXA_KB + MXA_VB + 256 + 256)    // + K^ scales (64 keys x 4) + V^ scales (2 blocks x 128 d)

// ---------------------------------------------------------------------------------------------------------------
// Shadow refresh: one workgroup of 128 threads per (32-slot block j0 + blockIdx.x, batch x head): K^ rows (slot i = tid / 4, channel
// block tid % 4) and V^ columns (d = tid), one item each.
__global__ __launch_bounds__(128) void kv_shadow_mx_kernel(const bf16* __restrict__ K, const bf16* __restrict__ V, uint8_t* __restrict__ kq,
                                                           uint8_t* __restrict__ ks, uint8_t* __restrict__ vq, uint8_t* __restrict__ vs,
                                                           int S, int S32, int H, int j0) {
  const int j = j0 + blockIdx.x, b = blockIdx.y / H, hh = blockIdx.y - b * H, tid = threadIdx.x;
  const int C = H * 128, NB = S32 / 32;
  const size_t cb = (size_t)b * S * C + hh * 128;
  {
    const int i = tid >> 2, q = tid & 3;
    const int slot = 32 * j + i;
    float f[32], mx = 0.f;
    if (slot < S) {
      const bf16* src = K + cb + (size_t)slot * C + q * 32;
#pragma unroll
      for (int c8 = 0; c8 < 4; ++c8) {
        bf16x8 v = *reinterpret_cast<const bf16x8*>(src + 8 * c8);
#pragma unroll
        for (int t = 0; t < 8; ++t) f[8 * c8 + t] = (float)v[t];
      }
    } else {
#pragma unroll
      for (int t = 0; t < 32; ++t) f[t] = 0.f;
    }
#pragma unroll
    for (int t = 0; t < 32; ++t) mx = fmaxf(mx, fabsf(f[t]));
    const int e = mx_scale_exp(mx);
    uint32_t w[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) w[t] = mx_code4(f[4 * t], f[4 * t + 1], f[4 * t + 2], f[4 * t + 3], e);
    uint4* dst = reinterpret_cast<uint4*>(kq + ((size_t)b * S32 + slot) * C + hh * 128 + q * 32);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    ks[((size_t)b * S32 + slot) * (H * 4) + hh * 4 + q] = (uint8_t)(e + 127);
  }
  {
    const int d = tid;
    float f[32], mx = 0.f;
#pragma unroll
    for (int p = 0; p < 32; ++p) {
      const int jj = p & 15, slot = 32 * j + (jj & 3) + 8 * (jj >> 2) + 4 * (p >> 4);
      f[p] = slot < S ? (float)V[cb + (size_t)slot * C + d] : 0.f;
      mx = fmaxf(mx, fabsf(f[p]));
    }
    const int e = mx_scale_exp(mx);
    uint32_t w[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) w[t] = mx_code4(f[4 * t], f[4 * t + 1], f[4 * t + 2], f[4 * t + 3], e);
    const size_t row = (((size_t)b * H + hh) * NB + j) * 128 + d;
    uint4* dst = reinterpret_cast<uint4*>(vq + row * 32);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    vs[row] = (uint8_t)(e + 127);
  }
}

// ---------------------------------------------------------------------------------------------------------------
struct MxSegs {
  int a0, e0, a1, e1, nt0, nt;     // key ranges [a, e) and tile counts (tiles of segment g start at a_g & ~31)
};

__device__ __forceinline__ void mx_tile(const MxSegs& sg, int t, int& base, int& lo, int& hi) {
  if (t < sg.nt0) {
    base = (sg.a0 & ~31) + t * MXA_KT; lo = sg.a0; hi = sg.e0;
  } else {
    base = (sg.a1 & ~31) + (t - sg.nt0) * MXA_KT; lo = sg.a1; hi = sg.e1;
  }
}

__device__ __forceinline__ uint32_t cvt_fp8x4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}

__device__ __forceinline__ float fp8x4_sum(uint32_t w) {
  f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  return (lo[0] + lo[1]) + (hi[0] + hi[1]);
}

// Staging: 256 threads; K^ codes 2 x 16 B, V^ codes 2 x 16 B per thread; scales on threads 0..127 (4 B each).  Rows past the
// shadow re-read its last row / block (their keys are masked).
#define MXA_LOAD_TILE(BASE)                                                                                          \
  {                                                                                                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                               \
      const int cid_ = tid + 256 * i_;                                                                               \
      int slot_ = (BASE) + (cid_ >> 3);                                                                              \
      slot_ = slot_ < S32 ? slot_ : S32 - 1;                                                                         \
      kr[i_] = *reinterpret_cast<const uint4*>(kqh + (size_t)slot_ * C + (cid_ & 7) * 16);                          \
      int jb_ = ((BASE) >> 5) + (cid_ >> 8);                                                                         \
      jb_ = jb_ < NB ? jb_ : NB - 1;                                                                                 \
      vr[i_] = *reinterpret_cast<const uint4*>(vqh + (size_t)jb_ * 4096 + (cid_ & 255) * 16);                       \
    }                                                                                                                \
    if (tid < 64) {                                                                                                  \
      int slot_ = (BASE) + tid;                                                                                      \
      slot_ = slot_ < S32 ? slot_ : S32 - 1;                                                                         \
      sr = *reinterpret_cast<const uint32_t*>(ksh + (size_t)slot_ * (H * 4));                                       \
    } else if (tid < 128) {                                                                                          \
      int jb_ = ((BASE) >> 5) + ((tid - 64) >> 5);                                                                   \
      jb_ = jb_ < NB ? jb_ : NB - 1;                                                                                 \
      sr = *reinterpret_cast<const uint32_t*>(vsh + (size_t)jb_ * 128 + ((tid - 64) & 31) * 4);                     \
    }                                                                                                                \
  }
// LDS image: K^ rows of 128 B with 16-B chunk c of key r at position c ^ ((r >> 1) & 7); V^ as in memory (block, d, 32 B);
// then K^ scales [64 keys][4], V^ scales [2 blocks][128 d].
#define MXA_STORE_TILE(ST)                                                                                           \
  {                                                                                                                  \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                               \
      const int cid_ = tid + 256 * i_;                                                                               \
      const int key_ = cid_ >> 3, ch_ = cid_ & 7;                                                                    \
      *reinterpret_cast<uint4*>((ST) + key_ * 128 + ((ch_ ^ ((key_ >> 1) & 7)) << 4)) = kr[i_];                     \
      *reinterpret_cast<uint4*>((ST) + MXA_KB + cid_ * 16) = vr[i_];                                                 \
    }                                                                                                                \
    if (tid < 128) *reinterpret_cast<uint32_t*>((ST) + MXA_KB + MXA_VB + tid * 4) = sr;                             \
  }

// OUTF: 0 = bf16 rows O [.., ldo elements]; LL_QFMT_MX / MX6 / MX4 = the quantiser's codes of those rows, O as bytes with ldo BYTES per
// row, and their E8M0 scale bytes sc [.., ldsc bytes] (ll_flash_attn_mx_q)
template <int OUTF>
__global__ __launch_bounds__(MXA_NW * 64, 2) void flash_attn_mx_kernel(const bf16* __restrict__ Q, const uint8_t* __restrict__ kq,
                                                                       const uint8_t* __restrict__ ks, const uint8_t* __restrict__ vq,
                                                                       const uint8_t* __restrict__ vs, bf16* __restrict__ O, int Lq,
                                                                       int ldq, int ldo, int H, int S32, MxSegs sg, float c,
                                                                       uint8_t* __restrict__ sc, int ldsc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][K^ | V^ | K^ scales | V^ scales]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int q0 = blockIdx.x * (MXA_NW * 32) + wave * 32;
  const int C = H * 128, NB = S32 / 32;

  const uint8_t* kqh = kq + (size_t)b * S32 * C + head * 128;
  const uint8_t* ksh = ks + (size_t)b * S32 * (H * 4) + head * 4;
  const uint8_t* vqh = vq + ((size_t)b * H + head) * NB * 4096;
  const uint8_t* vsh = vs + ((size_t)b * H + head) * NB * 128;

  // Q^ prologue: lane (r, h) quantises its query's whole row (4 blocks of 32 channels, the MX rule) and keeps the fragments of the
  // two k-steps: bytes 0-15 = channels 64 ks + 16 h .., bytes 16-31 = 64 ks + 32 + 16 h ..; scale = block 2 ks + h.
  i32x8 qf[2];
  int qsc[2];
  {
    int qr = q0 + r;
    qr = qr < Lq ? qr : Lq - 1;
    const bf16* qp = Q + ((size_t)b * Lq + qr) * ldq + head * 128;
    float x[128];
#pragma unroll
    for (int c8 = 0; c8 < 16; ++c8) {
      bf16x8 v = *reinterpret_cast<const bf16x8*>(qp + 8 * c8);
#pragma unroll
      for (int t = 0; t < 8; ++t) x[8 * c8 + t] = (float)v[t];
    }
    int e[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      float mx = 0.f;
#pragma unroll
      for (int t = 0; t < 32; ++t) mx = fmaxf(mx, fabsf(x[32 * blk + t]));
      e[blk] = mx_scale_exp(mx);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int blk = 2 * kk + half;
        const int c0 = 64 * kk + 32 * half;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          // (h is lane-dependent: select the values, not the array index, so x stays in registers)
          float v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = h ? x[c0 + 16 + 4 * t + u] : x[c0 + 4 * t + u];
          qf[kk][4 * half + t] = (int)mx_code4(v[0], v[1], v[2], v[3], e[blk]);
        }
      }
      qsc[kk] = e[2 * kk] + h * (e[2 * kk + 1] - e[2 * kk]) + 127;   // (arithmetic select: a ?: became a scratch-indexed load)
    }
  }

  f32x16 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.f;
  float M = -INFINITY, l_run = 0.f;            // M = c * m_ref of this lane's query

  uint4 kr[2], vr[2];
  uint32_t sr = 0;
  int base, lo, hi;
  mx_tile(sg, 0, base, lo, hi);
  MXA_LOAD_TILE(base);
  MXA_STORE_TILE(smem);
  __syncthreads();

  for (int t = 0; t < sg.nt; ++t) {
    const char* st = smem + (t & 1) * MXA_STAGE;
    const int cbase = base, clo = lo, chi = hi;
    {
      const int tn = t + 1 < sg.nt ? t + 1 : t;       // clamped: the last iteration re-fetches its own tile
      mx_tile(sg, tn, base, lo, hi);
      MXA_LOAD_TILE(base);
    }

    // ---- S^T = K^ Q^^T: 2 key blocks x 2 k-steps of 64 channels ------------------------------------------------------
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int key = 32 * kb + r;
      const uint32_t ksw = *reinterpret_cast<const uint32_t*>(st + MXA_KB + MXA_VB + key * 4);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int c0 = 4 * kk + h, c1 = 4 * kk + 2 + h;
        const int sw = (key >> 1) & 7;
        i32x4v a0 = *reinterpret_cast<const i32x4v*>(st + key * 128 + ((c0 ^ sw) << 4));
        i32x4v a1 = *reinterpret_cast<const i32x4v*>(st + key * 128 + ((c1 ^ sw) << 4));
        i32x8 af = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        const int ksc = (int)((ksw >> (8 * (2 * kk + h))) & 0xffu);
        s[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, qf[kk], s[kb], 0, 0, 0, ksc, 0, qsc[kk]);
      }
    }
    // lane holds, for query r: s[kb][i] = score of slot cbase + 32 kb + (i & 3) + 8 (i >> 2) + 4 h
    if (cbase < clo || cbase + MXA_KT > chi) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int slot = cbase + 32 * kb + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (slot < clo || slot >= chi) s[kb][i] = -INFINITY;
        }
    }

    // ---- lazy-max softmax (base 2, scale folded) ------------------------------------------------------------------
    float mx = s[0][0];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, s[kb][i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float tm = mx * c;
    const float Mn = tm - M > MXA_THR ? tm : M;
    const float alpha = __builtin_amdgcn_exp2f(M - Mn);      // 1 exactly when M stays; 0 on the first tile
    uint32_t pw[2][4];
    float rs = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * g + 0], c, -Mn));
        float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * g + 1], c, -Mn));
        float p2 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * g + 2], c, -Mn));
        float p3 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * g + 3], c, -Mn));
        pw[kb][g] = cvt_fp8x4(p0, p1, p2, p3);
        rs += fp8x4_sum(pw[kb][g]);
      }
    rs += __shfl_xor(rs, 32, 64);
    l_run = l_run * alpha + rs;
    if (__any(Mn != M)) {
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[d][i] *= alpha;
    }
    M = Mn;
    const i32x8 pf = {(int)pw[0][0], (int)pw[0][1], (int)pw[0][2], (int)pw[0][3],
                      (int)pw[1][0], (int)pw[1][1], (int)pw[1][2], (int)pw[1][3]};

    // ---- O^T += V^^T P^^T: 4 d-blocks, one k-step of 64 keys each ---------------------------------------------------
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const int d = 32 * db + r;
      i32x4v a0 = *reinterpret_cast<const i32x4v*>(st + MXA_KB + d * 32 + 16 * h);
      i32x4v a1 = *reinterpret_cast<const i32x4v*>(st + MXA_KB + 4096 + d * 32 + 16 * h);
      i32x8 af = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      const int vsc = (int)*reinterpret_cast<const uint8_t*>(st + MXA_KB + MXA_VB + 256 + h * 128 + d);
      o[db] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, pf, o[db], 0, 0, 0, vsc, 0, 127);
    }

    MXA_STORE_TILE(smem + ((t + 1) & 1) * MXA_STAGE);   // other stage: last read one barrier ago
    __syncthreads();
  }

  // ---- epilogue: O^T[d][q] / l -> out[q][head * 128 + d]; lane holds d = 32 db + 8 g4 + 4 h + (0..3) -------------------------
  const int qr = q0 + r;
  if constexpr (OUTF == 0) {
    if (qr < Lq) {
      const float inv = 1.0f / l_run;
      bf16* op = O + ((size_t)b * Lq + qr) * ldo + head * 128 + 4 * h;
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          bf16x4 w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = (bf16)(o[db][4 * g4 + j] * inv);
          *reinterpret_cast<bf16x4*>(op + 32 * db + 8 * g4) = w;
        }
    }
  } else {
    // The same bf16 values, quantised per 32-channel block db: the lane (r, 1 - h) holds the block's other 16 values (one lane ^ 32
    // step for the maximum); the pieces of g4 = 0, 1 and of g4 = 2, 3 are exchanged so that lane h stores channels 16 h .. 16 h + 15 of
    // the block in one piece.  Every lane takes part in the exchanges; only rows < Lq store.
    const bool live = qr < Lq;
    const float inv = 1.0f / l_run;
    const size_t row = (size_t)b * Lq + (live ? qr : 0);
    uint8_t* cp = reinterpret_cast<uint8_t*>(O) + row * ldo +
                  (OUTF == LL_QFMT_MX ? head * 128 + 16 * h
                                      : OUTF == LL_QFMT_MX6 ? (head >> 1) * MX6_SUPER_BYTES + 24 * (head & 1) + 12 * h
                                                            : (head >> 1) * MX4_SUPER_BYTES + 16 * (head & 1) + 8 * h);
    uint32_t scw = 0;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      float x[16], mx = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        x[i] = (float)(bf16)(o[db][i] * inv);
        mx = fmaxf(mx, fabsf(x[i]));
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const int e = OUTF == LL_QFMT_MX ? mx_scale_exp(mx) : OUTF == LL_QFMT_MX6 ? mx6_scale_exp(mx) : mx4_scale_exp(mx);
      scw |= (uint32_t)(e + 127) << (8 * db);
      uint32_t w[4];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        w[g4] = OUTF == LL_QFMT_MX    ? mx_code4(x[4 * g4], x[4 * g4 + 1], x[4 * g4 + 2], x[4 * g4 + 3], e)
                : OUTF == LL_QFMT_MX6 ? mx6_pack4(x[4 * g4], x[4 * g4 + 1], x[4 * g4 + 2], x[4 * g4 + 3], e)
                                      : mx4_pack4(x[4 * g4], x[4 * g4 + 1], x[4 * g4 + 2], x[4 * g4 + 3], e);
      if constexpr (OUTF == LL_QFMT_MX4) {             // 16-bit pieces
        const uint32_t lo2 = w[0] | (w[1] << 16), hi2 = w[2] | (w[3] << 16);
        const uint32_t got = __shfl_xor(h ? lo2 : hi2, 32, 64), mine = h ? hi2 : lo2;
        const uint32_t a = h ? got : mine, bq = h ? mine : got;      // the h = 0 / h = 1 lane's pieces of this half's two g4
        if (live) *reinterpret_cast<uint2*>(cp + 32 * db) = make_uint2((a & 0xffffu) | (bq << 16), (a >> 16) | (bq & 0xffff0000u));
      } else {
        const uint32_t g0 = __shfl_xor(h ? w[0] : w[2], 32, 64), g1 = __shfl_xor(h ? w[1] : w[3], 32, 64);
        const uint32_t pa = h ? g0 : w[0], pb = h ? w[2] : g0, pc = h ? g1 : w[1], pd = h ? w[3] : g1;
        if constexpr (OUTF == LL_QFMT_MX) {
          if (live) *reinterpret_cast<uint4*>(cp + 32 * db) = make_uint4(pa, pb, pc, pd);
        } else if (live) {                             // four 24-bit pieces -> three dwords
          uint32_t* d = reinterpret_cast<uint32_t*>(cp + 48 * db);
          d[0] = pa | (pb << 24);
          d[1] = (pb >> 8) | (pc << 16);
          d[2] = (pc >> 16) | (pd << 8);
        }
      }
    }
    if (live && h == 0) *reinterpret_cast<uint32_t*>(sc + row * ldsc + head * 4) = scw;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Host side
static MxSegs mx_segs(int s0, int n0, int s1, int n1) {
  const AttnKeys k = attn_merge(s0, n0, s1, n1);      // adjacent: one range (as ll_flash_attn)
  MxSegs sg;
  sg.a0 = k.s0; sg.e0 = k.s0 + k.n0; sg.a1 = k.s1; sg.e1 = k.s1 + k.n1;
  sg.nt0 = (sg.e0 - (sg.a0 & ~31) + MXA_KT - 1) / MXA_KT;
  sg.nt = sg.nt0 + (k.n1 > 0 ? (sg.e1 - (sg.a1 & ~31) + MXA_KT - 1) / MXA_KT : 0);
  return sg;
}

static int mx_attn_check_segs(const char* fn, int S, int S32, int s0, int n0, int s1, int n1) {
  LL_REQUIRE(S > 0 && S32 == (S + 31) / 32 * 32, "%s: S32=%d must be the cache length S=%d rounded up to a multiple of 32", fn, S32, S);
  LL_REQUIRE(n0 > 0 && s0 >= 0 && s0 + n0 <= S, "%s: first key range [%d, +%d) must be non-empty and inside the cache of %d slots", fn,
             s0, n0, S);
  LL_REQUIRE(n1 >= 0 && (n1 == 0 || (s1 >= 0 && s1 + n1 <= S)), "%s: second key range [%d, +%d) outside the cache of %d slots", fn, s1,
             n1, S);
  return attn_check_ranges(fn, s0, n0, s1, n1, LL_ATTN_TWICE);
}

extern "C" int ll_kv_shadow_mx(const ll_bf16* k, const ll_bf16* v, uint8_t* kq, uint8_t* ks, uint8_t* vq, uint8_t* vs, int B, int S,
                               int S32, int H, int head_dim, int lo, int hi, ll_stream stream) {
  LL_REQUIRE(k != nullptr && v != nullptr, "ll_kv_shadow_mx: the bf16 cache k and v are required");
  LL_REQUIRE(kq != nullptr && ks != nullptr && vq != nullptr && vs != nullptr, "ll_kv_shadow_mx: shadow codes and scales of K and V are required");
  LL_REQUIRE(head_dim == 128, "ll_kv_shadow_mx: head_dim=%d (the shadow is specialised for 128)", head_dim);
  LL_REQUIRE(B >= 0 && H > 0, "ll_kv_shadow_mx: B=%d H=%d", B, H);
  LL_REQUIRE(S > 0 && S32 == (S + 31) / 32 * 32, "ll_kv_shadow_mx: S32=%d must be the cache length S=%d rounded up to a multiple of 32",
             S32, S);
  LL_REQUIRE(lo >= 0 && lo <= hi && hi <= S, "ll_kv_shadow_mx: slot range [%d, %d) outside the cache of %d slots", lo, hi, S);
  if (B == 0 || lo == hi) return LL_OK;
  const int j0 = lo / 32, j1 = (hi + 31) / 32;         // whole 32-slot blocks
  LL_REQUIRE((long long)B * H < 65536, "ll_kv_shadow_mx: B * H = %d too large", B * H);
  hipLaunchKernelGGL(kv_shadow_mx_kernel, dim3(j1 - j0, B * H), dim3(128), 0, (hipStream_t)stream, (const bf16*)k, (const bf16*)v, kq, ks, vq,
                     vs, S, S32, H, j0);
  return ll_check_launch("ll_kv_shadow_mx");
}

extern "C" int ll_flash_attn_mx_plan(int Lq, int H, int B, int seg0_start, int seg0_len, int seg1_start, int seg1_len, char* out, int cap) {
  LL_REQUIRE(out != nullptr && cap > 0, "ll_flash_attn_mx_plan: needs an output buffer");
  const MxSegs sg = mx_segs(seg0_start, seg0_len, seg1_start, seg1_len);
  snprintf(out, (size_t)cap, "flash_attn_mx_kernel (%d waves x 32 rows, v_mfma_scale_f32_32x32x64_f8f6f4), %d workgroups of %d query rows, "
           "%d key tiles of %d in %d range%s", MXA_NW, ((Lq + MXA_NW * 32 - 1) / (MXA_NW * 32)) * H * B, MXA_NW * 32, sg.nt, MXA_KT,
           sg.nt > sg.nt0 ? 2 : 1, sg.nt > sg.nt0 ? "s" : "");
  return LL_OK;
}

// The kernel instance per output form: index 0 = bf16 rows, LL_QFMT_MX / MX6 / MX4 = the codes + E8M0 scales of those rows
static const void* flash_attn_mx_instance(int fmt) {
  static const void* const t[] = {(const void*)flash_attn_mx_kernel<0>, (const void*)flash_attn_mx_kernel<LL_QFMT_MX>,
                                  (const void*)flash_attn_mx_kernel<LL_QFMT_MX6>, (const void*)flash_attn_mx_kernel<LL_QFMT_MX4>};
  return t[fmt];
}

// The one body of ll_flash_attn_mx (qout = false, fmt = 0: out = bf16 rows of stride ldo elements, no scales) and ll_flash_attn_mx_q
// (out = the code rows of stride ldo BYTES, scales of stride lds): the checks in the entries' order and words, one launch.
static int mx_attn_call(const char* fn, bool qout, int fmt, const ll_bf16* q, const uint8_t* kq, const uint8_t* ks, const uint8_t* vq,
                        const uint8_t* vs, void* out, uint8_t* scales, int B, int Lq, int H, int head_dim, int ldq, int ldo, int lds, int S,
                        int S32, int s0, int n0, int s1, int n1, float scale, ll_stream stream) {
  const int bits = qfmt_bits(fmt);
  if (qout) {
    LL_REQUIRE(bits != 0, "%s: fmt=%d is none of LL_QFMT_MX / MX6 / MX4", fn, fmt);
    LL_REQUIRE(q != nullptr && out != nullptr && scales != nullptr, "%s: q, codes and scales are required", fn);
  } else {
    LL_REQUIRE(q != nullptr && out != nullptr, "%s: q and out are required", fn);
  }
  LL_REQUIRE(kq != nullptr && ks != nullptr && vq != nullptr && vs != nullptr, "%s: shadow codes and scales of K and V are required", fn);
  LL_REQUIRE(head_dim == 128, "%s: head_dim=%d (the kernel is specialised for 128)", fn, head_dim);
  LL_REQUIRE(B >= 0 && Lq >= 0 && H > 0, "%s: B=%d Lq=%d H=%d", fn, B, Lq, H);
  if (qout) {
    LL_REQUIRE(fmt == LL_QFMT_MX || (H & 1) == 0, "%s: the packed formats pair heads in 256-k super-blocks: H=%d must be even", fn, H);
    LL_REQUIRE(ldq % 8 == 0 && ldq >= H * 128, "%s: row stride ldq=%d (>= H*128, a multiple of 8)", fn, ldq);
    LL_REQUIRE(ldo % 16 == 0 && ldo >= H * 16 * bits && lds % 4 == 0 && lds >= H * 4, "%s: code row stride %d bytes (>= %d, a "
               "multiple of 16) or scale row stride %d bytes (>= %d, a multiple of 4)", fn, ldo, H * 16 * bits, lds, H * 4);
  } else {
    LL_REQUIRE(ldq % 8 == 0 && ldo % 4 == 0 && ldq >= H * 128 && ldo >= H * 128, "%s: row strides ldq=%d ldo=%d (>= H*128, "
               "multiples of 8 / 4)", fn, ldq, ldo);
  }
  if (int rc = mx_attn_check_segs(fn, S, S32, s0, n0, s1, n1)) return rc;
  LL_REQUIRE(scale > 0.f && scale <= 3.0e38f, "%s: scale=%g must be positive and finite%s", fn, (double)scale,
             qout ? "" : " (the tile maximum is taken before the multiplication by scale * log2 e)");
  if (B == 0 || Lq == 0) return LL_OK;
  MxSegs sg = mx_segs(s0, n0, s1, n1);
  float c = scale * LL_LOG2E;
  const void* k = flash_attn_mx_instance(fmt);
  if (int rc = ll_lds_attr(k, 2 * MXA_STAGE)) return rc;
  void* args[] = {&q, &kq, &ks, &vq, &vs, &out, &Lq, &ldq, &ldo, &H, &S32, &sg, &c, &scales, &lds};
  (void)hipLaunchKernel(k, dim3((Lq + MXA_NW * 32 - 1) / (MXA_NW * 32), H, B), dim3(MXA_NW * 64), args, 2 * MXA_STAGE, (hipStream_t)stream);
  return ll_check_launch(fn);
}

extern "C" int ll_flash_attn_mx(const ll_bf16* q, const uint8_t* kq, const uint8_t* ks, const uint8_t* vq, const uint8_t* vs, ll_bf16* out,
                                int B, int Lq, int H, int head_dim, int ldq, int ldo, int S, int S32, int seg0_start, int seg0_len,
                                int seg1_start, int seg1_len, float scale, ll_stream stream) {
  return mx_attn_call("ll_flash_attn_mx", false, 0, q, kq, ks, vq, vs, out, nullptr, B, Lq, H, head_dim, ldq, ldo, 0, S, S32, seg0_start,
                      seg0_len, seg1_start, seg1_len, scale, stream);
}

// ll_flash_attn_mx with the codes + E8M0 scales of its bf16 rows as output (include/longlive_hip.h: ll_flash_attn_q's contract)
extern "C" int ll_flash_attn_mx_q(int fmt, const ll_bf16* q, const uint8_t* kq, const uint8_t* ks, const uint8_t* vq, const uint8_t* vs,
                                  uint8_t* codes, uint8_t* scales, int B, int Lq, int H, int head_dim, int ldq, int ldc, int lds, int S,
                                  int S32, int seg0_start, int seg0_len, int seg1_start, int seg1_len, float scale, ll_stream stream) {
  return mx_attn_call("ll_flash_attn_mx_q", true, fmt, q, kq, ks, vq, vs, codes, scales, B, Lq, H, head_dim, ldq, ldc, lds, S, S32,
                      seg0_start, seg0_len, seg1_start, seg1_len, scale, stream);
}
