// Planar YUV frames in and out ("Planar YUV and Y4M").  The arithmetic is csrc/yuv.h's, integer and exact;
// the kernels here only move bytes around it.  All three are memory bound and need no LDS.
//
// to_yuv420_kernel<SRC>: a lane owns a strip of 2 rows x 4 pixels of one frame, i.e. 8 luma samples and 2 + 2 chroma samples.  SRC
// says where the strip's RGB bytes come from: SrcU8 reads uint8 frames (12 bytes per row as three dwords where the row's address is
// dword aligned, as bytes otherwise and on a row's last, partial run), SrcCl reads the decoder head's channels-last bf16 (one 16-byte
// pixel at a time where ldc and the base allow, three scalars otherwise) and makes cl_to_frames_u8_kernel's bytes of it in
// registers.  A missing last row or column is replicated.  Y leaves as one dword per row where the address allows and as bytes
// otherwise, Cb and Cr as two bytes each; nothing outside the frame's H W + 2 Hc Wc bytes is written.  The strip was 2 x 8 at first
// (Y as two dwords, chroma as one): measured on 12 frames of 480 x 832, the bf16 form took 3.98 us per frame against 2.31 for 2 x 4
// -- eight 16-byte loads per lane instead of sixteen, and twice the lanes to hide them (profiles/yuv_frames.md).
//
// yuv_to_frames_u8_kernel<LAYOUT>: a lane owns a run of 8 output pixels of one row.  It reads its 8 luma bytes and, from the near
// and the far chroma row of that luma row, the 6 (subsampled) or 8 (4:4:4) chroma columns the run can touch, each column index
// clamped to the plane, blends the two rows once, and then walks its pixels in registers.  24 output bytes leave as six dwords.
#include "common.h"
#include "yuv.h"

namespace {

constexpr int YUV_RUN = 8;      // pixels of a lane's run
constexpr int FWD_RUN = 4;      // pixels per row of a lane's 2-row strip in to_yuv420_kernel

__device__ __forceinline__ bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// n <= 4 * WORDS bytes of w to o: dwords when the run is whole and o is dword aligned
template <int WORDS>
__device__ __forceinline__ void store_run(uint8_t* o, const uint32_t (&w)[WORDS], int n) {
  if (n == 4 * WORDS && aligned4(o)) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
    for (int k = 0; k < WORDS; ++k) o4[k] = w[k];
  } else {
#pragma unroll
    for (int b = 0; b < 4 * WORDS; ++b)
      if (b < n) o[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
  }
}

// RGB bytes of row r, columns x0 .. x0 + FWD_RUN - 1 of frame t; a column past the row's last (n are inside) repeats the last
struct SrcU8 {
  const uint8_t* p;
  long long st;
  __device__ __forceinline__ void row(int t, int r, int x0, int n, int H, int W, int (&px)[FWD_RUN][3]) const {
    const uint8_t* s = p + t * st + ((long long)r * W + x0) * 3;
    if (n == FWD_RUN && aligned4(s)) {
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
      uint32_t w[3 * FWD_RUN / 4];
#pragma unroll
      for (int k = 0; k < 3 * FWD_RUN / 4; ++k) w[k] = s4[k];
#pragma unroll
      for (int b = 0; b < 3 * FWD_RUN; ++b) px[b / 3][b % 3] = (int)((w[b >> 2] >> (8 * (b & 3))) & 255u);
    } else {
#pragma unroll
      for (int j = 0; j < FWD_RUN; ++j) {
        const int jj = j < n ? j : n - 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) px[j][c] = s[3 * jj + c];
      }
    }
  }
};

// cl_to_frames_u8_kernel's byte, the same fp32 expression in the same order (-ffp-contract=off keeps the multiply and the add apart)
__device__ __forceinline__ int cl_byte(float v) {
  v = fminf(fmaxf(v, -1.0f), 1.0f);
  v = fminf(fmaxf(v * 0.5f + 0.5f, 0.0f), 1.0f);
  return (int)(uint32_t)(int)(255.0f * v);
}

struct SrcCl {
  const bf16* x;
  int ldc;
  __device__ __forceinline__ void row(int t, int r, int x0, int n, int H, int W, int (&px)[FWD_RUN][3]) const {
    const bf16* s = x + (((long long)t * H + r) * W + x0) * ldc;
    const bool wide = (ldc & 7) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
#pragma unroll
    for (int j = 0; j < FWD_RUN; ++j) {
      const bf16* q = s + (long long)(j < n ? j : n - 1) * ldc;
      if (wide) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(q);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[j][c] = cl_byte((float)v[c]);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) px[j][c] = cl_byte((float)q[c]);
      }
    }
  }
};

template <typename SRC>
__global__ __launch_bounds__(256) void to_yuv420_kernel(SRC src, uint8_t* __restrict__ out, long long ost, int H, int W, int Hc, int Wc,
                                                        int runs, long long strips, long long total, int full) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;      // strip
  if (i >= total) return;
  const int t = (int)(i / strips);
  const long long rem = i - t * strips;
  const int sy = (int)(rem / runs), sx = (int)(rem - (long long)sy * runs);
  const int r0 = 2 * sy, x0 = FWD_RUN * sx;
  const bool two = r0 + 1 < H;
  const int n = W - x0 < FWD_RUN ? W - x0 : FWD_RUN;                  // pixels of this run inside the row
  int a[FWD_RUN][3], b[FWD_RUN][3];
  src.row(t, r0, x0, n, H, W, a);
  src.row(t, two ? r0 + 1 : r0, x0, n, H, W, b);
  uint32_t ya[FWD_RUN / 4] = {}, yb[FWD_RUN / 4] = {}, u[1] = {0u}, v[1] = {0u};
#pragma unroll
  for (int j = 0; j < FWD_RUN; ++j) {
    ya[j >> 2] |= (uint32_t)yuv_luma(a[j][0], a[j][1], a[j][2], full) << (8 * (j & 3));
    yb[j >> 2] |= (uint32_t)yuv_luma(b[j][0], b[j][1], b[j][2], full) << (8 * (j & 3));
  }
#pragma unroll
  for (int q = 0; q < FWD_RUN / 2; ++q) {
    int s[3], cb, cr;
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = a[2 * q][c] + a[2 * q + 1][c] + b[2 * q][c] + b[2 * q + 1][c];
    yuv_chroma(s[0], s[1], s[2], full, &cb, &cr);
    u[0] |= (uint32_t)cb << (8 * q);
    v[0] |= (uint32_t)cr << (8 * q);
  }
  uint8_t* fo = out + t * ost;
  store_run(fo + (long long)r0 * W + x0, ya, n);
  if (two) store_run(fo + (long long)(r0 + 1) * W + x0, yb, n);
  uint8_t* pu = fo + (long long)H * W + (long long)sy * Wc + (FWD_RUN / 2) * sx;
  store_run(pu, u, (n + 1) >> 1);
  store_run(pu + (long long)Hc * Wc, v, (n + 1) >> 1);
}

// NS chroma samples of one row from column c0 on, each column clamped into [0, wc - 1]
template <int NS>
__device__ __forceinline__ void chroma_slots(const uint8_t* row, int c0, int wc, int (&s)[NS]) {
  constexpr int lead = NS == 8 ? 0 : 1;                               // the subsampled forms carry one neighbour on either side
  constexpr int words = (NS - 2 * lead) / 4;
  const uint8_t* m = row + c0 + lead;
  if (c0 + NS - 1 - lead <= wc - 1 && aligned4(m)) {                  // c0 + lead >= 0 always
    const uint32_t* m4 = reinterpret_cast<const uint32_t*>(m);
#pragma unroll
    for (int k = 0; k < words; ++k) {
      const uint32_t w = m4[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) s[lead + 4 * k + e] = (int)((w >> (8 * e)) & 255u);
    }
    if (lead) {
      s[0] = row[c0 < 0 ? 0 : c0];
      s[NS - 1] = row[c0 + NS - 1 > wc - 1 ? wc - 1 : c0 + NS - 1];
    }
  } else {
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = row[yuv_clamp(c0 + k, 0, wc - 1)];
  }
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void yuv_to_frames_u8_kernel(const uint8_t* __restrict__ y, const uint8_t* __restrict__ cb,
                                                               const uint8_t* __restrict__ cr, long long sty, long long stc, int H, int W,
                                                               int runs, long long per_frame, long long total, int full,
                                                               uint8_t* __restrict__ out, long long ost) {
  constexpr int VM = yuv_vmode(LAYOUT), HM = yuv_hmode(LAYOUT);
  constexpr int NS = HM == YUV_NONE ? YUV_RUN : YUV_RUN / 2 + 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;      // run of 8 pixels of one row
  if (i >= total) return;
  const int t = (int)(i / per_frame);
  const long long rem = i - t * per_frame;
  const int oy = (int)(rem / runs), x0 = YUV_RUN * (int)(rem - (long long)oy * runs);
  const int n = W - x0 < YUV_RUN ? W - x0 : YUV_RUN;
  const uint8_t* ys = y + t * sty + (long long)oy * W + x0;
  uint32_t yw[2] = {0u, 0u};
  if (n == YUV_RUN && aligned4(ys)) {
    yw[0] = reinterpret_cast<const uint32_t*>(ys)[0];
    yw[1] = reinterpret_cast<const uint32_t*>(ys)[1];
  } else {
#pragma unroll
    for (int j = 0; j < YUV_RUN; ++j)
      if (j < n) yw[j >> 2] |= (uint32_t)ys[j] << (8 * (j & 3));
  }
  int U[NS], V[NS];                                                   // the two rows blended, in quarters
  if (LAYOUT != YUV_MONO) {
    const int hc = yuv_chroma_h(LAYOUT, H), wc = yuv_chroma_w(LAYOUT, W);
    int ny, fy, wy;
    yuv_axis(VM, oy, hc, &ny, &fy, &wy);
    const int c0 = HM == YUV_NONE ? x0 : (x0 >> 1) - 1;
    const uint8_t *pu = cb + t * stc, *pv = cr + t * stc;
    int un[NS], vn[NS];
    chroma_slots<NS>(pu + (long long)ny * wc, c0, wc, un);
    chroma_slots<NS>(pv + (long long)ny * wc, c0, wc, vn);
    if (wy != 0) {
      int uf[NS], vf[NS];
      chroma_slots<NS>(pu + (long long)fy * wc, c0, wc, uf);
      chroma_slots<NS>(pv + (long long)fy * wc, c0, wc, vf);
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        U[k] = (4 - wy) * un[k] + wy * uf[k];
        V[k] = (4 - wy) * vn[k] + wy * vf[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        U[k] = 4 * un[k];
        V[k] = 4 * vn[k];
      }
    }
  }
  uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < YUV_RUN; ++j) {                                 // x0 is even, so pixel j's parity is j's
    int U16 = 2048, V16 = 2048;
    if (LAYOUT != YUV_MONO) {
      if (HM == YUV_NONE) {
        U16 = 4 * U[j];
        V16 = 4 * V[j];
      } else {
        const int nr = 1 + (j >> 1);
        const int fr = HM == YUV_CENTRE ? ((j & 1) ? nr + 1 : nr - 1) : nr + 1;
        const int wx = HM == YUV_CENTRE ? 1 : (j & 1) ? 2 : 0;
        U16 = (4 - wx) * U[nr] + wx * U[fr];
        V16 = (4 - wx) * V[nr] + wx * V[fr];
      }
    }
    int c[3];
    yuv_rgb((int)((yw[j >> 2] >> (8 * (j & 3))) & 255u), U16, V16, full, &c[0], &c[1], &c[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int b = 3 * j + k;
      w[b >> 2] |= (uint32_t)c[k] << (8 * (b & 3));
    }
  }
  store_run(out + t * ost + ((long long)oy * W + x0) * 3, w, 3 * n);
}

struct Yuv420Plan {
  int Hc, Wc, runs;
  long long strips, total, bytes;
};

int yuv420_plan(const char* fn, int T, int H, int W, long long out_stride, Yuv420Plan* p) {
  LL_REQUIRE(T >= 1 && H >= 1 && W >= 1, "%s: empty input %d x %d x %d", fn, T, H, W);
  LL_REQUIRE(H <= 65535 && W <= 65535, "%s: H=%d, W=%d: a frame holds at most 65535 rows and columns", fn, H, W);
  p->Hc = (H + 1) / 2;
  p->Wc = (W + 1) / 2;
  p->runs = (W + FWD_RUN - 1) / FWD_RUN;
  p->strips = (long long)p->Hc * p->runs;
  p->total = p->strips * T;
  p->bytes = (long long)H * W + 2ll * p->Hc * p->Wc;
  LL_REQUIRE(out_stride >= p->bytes, "%s: out_stride=%lld bytes must span the %lld bytes of a %d x %d I420 frame", fn, out_stride, p->bytes,
             H, W);
  LL_REQUIRE((p->total + 255) / 256 <= 0x7fffffffll, "%s: %d x %d x %d is more than one launch covers", fn, T, H, W);
  return LL_OK;
}

}  // namespace

extern "C" int ll_frames_u8_to_yuv420(const uint8_t* frames, long long stride_t, int T, int H, int W, int full_range, uint8_t* out,
                                      long long out_stride, ll_stream stream) {
  LL_REQUIRE(frames != nullptr && out != nullptr, "ll_frames_u8_to_yuv420: null operand");
  Yuv420Plan p;
  if (int rc = yuv420_plan("ll_frames_u8_to_yuv420", T, H, W, out_stride, &p)) return rc;
  LL_REQUIRE(stride_t >= 3ll * H * W, "ll_frames_u8_to_yuv420: stride_t=%lld bytes must span a %d x %d x 3 frame", stride_t, H, W);
  hipLaunchKernelGGL((to_yuv420_kernel<SrcU8>), dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     SrcU8{frames, stride_t}, out, out_stride, H, W, p.Hc, p.Wc, p.runs, p.strips, p.total, full_range != 0);
  return ll_check_launch("ll_frames_u8_to_yuv420");
}

extern "C" int ll_cl_to_yuv420(const ll_bf16* x, int T, int H, int W, int ldc, int full_range, uint8_t* out, long long out_stride,
                               ll_stream stream) {
  LL_REQUIRE(x != nullptr && out != nullptr, "ll_cl_to_yuv420: null operand");
  LL_REQUIRE(ldc >= 3, "ll_cl_to_yuv420: ldc=%d, needs >= 3 channels per pixel", ldc);
  Yuv420Plan p;
  if (int rc = yuv420_plan("ll_cl_to_yuv420", T, H, W, out_stride, &p)) return rc;
  hipLaunchKernelGGL((to_yuv420_kernel<SrcCl>), dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     SrcCl{(const bf16*)x, ldc}, out, out_stride, H, W, p.Hc, p.Wc, p.runs, p.strips, p.total, full_range != 0);
  return ll_check_launch("ll_cl_to_yuv420");
}

extern "C" int ll_yuv_to_frames_u8(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, long long stride_y, long long stride_c, int T,
                                   int H, int W, int layout, int full_range, uint8_t* out, long long out_stride_t, ll_stream stream) {
  const char* fn = "ll_yuv_to_frames_u8";
  LL_REQUIRE(layout >= 0 && layout < YUV_LAYOUTS, "%s: layout=%d is not 0..5 (420jpeg, 420mpeg2, 420paldv, 422, 444, mono)", fn, layout);
  LL_REQUIRE(y != nullptr && out != nullptr && (layout == YUV_MONO || (cb != nullptr && cr != nullptr)), "%s: null operand", fn);
  LL_REQUIRE(T >= 1 && H >= 1 && W >= 1, "%s: empty input %d x %d x %d", fn, T, H, W);
  LL_REQUIRE(H <= 65535 && W <= 65535, "%s: H=%d, W=%d: a frame holds at most 65535 rows and columns", fn, H, W);
  LL_REQUIRE(stride_y >= (long long)H * W, "%s: stride_y=%lld bytes must span a %d x %d plane", fn, stride_y, H, W);
  const long long cbytes = (long long)yuv_chroma_h(layout, H) * yuv_chroma_w(layout, W);
  LL_REQUIRE(stride_c >= cbytes, "%s: stride_c=%lld bytes must span a %d x %d chroma plane", fn, stride_c, yuv_chroma_h(layout, H),
             yuv_chroma_w(layout, W));
  LL_REQUIRE(out_stride_t >= 3ll * H * W, "%s: out_stride_t=%lld bytes must span a %d x %d x 3 frame", fn, out_stride_t, H, W);
  const int runs = (W + YUV_RUN - 1) / YUV_RUN;
  const long long per_frame = (long long)H * runs, total = per_frame * T;
  LL_REQUIRE((total + 255) / 256 <= 0x7fffffffll, "%s: %d x %d x %d is more than one launch covers", fn, T, H, W);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define YUV_LAUNCH(L)                                                                                                                   \
  case L:                                                                                                                               \
    hipLaunchKernelGGL((yuv_to_frames_u8_kernel<L>), grid, block, 0, (hipStream_t)stream, y, cb, cr, stride_y, stride_c, H, W, runs,    \
                       per_frame, total, full_range != 0, out, out_stride_t);                                                           \
    break;
  switch (layout) {
    YUV_LAUNCH(YUV_420JPEG)
    YUV_LAUNCH(YUV_420MPEG2)
    YUV_LAUNCH(YUV_420PALDV)
    YUV_LAUNCH(YUV_422)
    YUV_LAUNCH(YUV_444)
    YUV_LAUNCH(YUV_MONO)
  }
#undef YUV_LAUNCH
  return ll_check_launch(fn);
}
