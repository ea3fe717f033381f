// Clip intake: a baseline JPEG decoder (ITU T.81, SOF0, 8 bits; grey, 4:4:4, 4:2:2 and 4:2:0; any Huffman and quantisation tables;
// with or without restart markers) and an antialiased resize for uint8 frames, every stage on the GPU and stream-ordered.  The mirror
// image of csrc/jpeg.hip.  The host (longlive_amd/jpeg_files.py) walks the markers and finds the restart segments; no kernel searches
// for a marker.
//
// Launches of ll_jpeg_decode_u8 (each output is written whole, so neither coef nor scratch has to start as zero):
//   (a) jpeg_huff_decode_kernel  one lane per restart segment (the whole scan without DRI), one segment per wave: jpeg_dec.h's
//                                 jpeg_decode_segment over the frame's tables, staged into LDS (BITS + HUFFVAL, walked length by
//                                 length against a 16-bit look-ahead); a block is built in a 128-byte LDS slot and leaves as eight
//                                 16-byte stores -> coef int16 [T, rows, cols, bpm, 64] in zigzag order, status[segment]
//   (b) jpeg_idct_kernel         one wave per block: dequantise, C^T . F . C with the encoder's cosine matrix in fp32, two passes,
//                                 + 128, clamp to [0, 255] unrounded -> fp32 component planes [T, rows * 8 v, cols * 8 h]
//   (c) jpeg_rgb_kernel          one lane per pixel: chroma by the triangle filter 0.75 near + 0.25 far where its factor is 2 (vertical
//                                 first, edges replicated at the component's own extent), YCbCr -> RGB, floor(v + 0.5) clamped -> uint8
// ll_resize_u8 is one launch: resize_u8_kernel, one lane per output pixel, taps from the host's tables, vertical then horizontal in fp32.
#include "common.h"
#include "jpeg_dec.h"

namespace {

__device__ const uint8_t DEC_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// C[k][n] = a_k cos((2n + 1) k pi / 16), a_0 = sqrt(1/8), a_k = 1/2: the encoder's matrix (csrc/jpeg.hip), used here as its transpose
#define C1 0.49039264020161522f
#define C2 0.46193976625564337f
#define C3 0.41573480615127262f
#define C4 0.35355339059327379f
#define C5 0.27778511650980109f
#define C6 0.19134171618254489f
#define C7 0.09754516100806412f
__device__ const float DEC_C[8][8] = {{C4, C4, C4, C4, C4, C4, C4, C4},     {C1, C3, C5, C7, -C7, -C5, -C3, -C1},
                                      {C2, C6, -C6, -C2, -C2, -C6, C6, C2}, {C3, -C7, -C1, -C5, C5, C1, C7, -C3},
                                      {C4, -C4, -C4, C4, C4, -C4, -C4, C4}, {C5, -C1, C7, C3, -C3, -C7, C1, -C5},
                                      {C6, -C2, C2, -C6, -C6, C2, -C2, C6}, {C7, -C5, C3, -C1, C1, -C3, C5, -C7}};
#undef C1
#undef C2
#undef C3
#undef C4
#undef C5
#undef C6
#undef C7

// what a (H, W, components, luma sampling) decides; planes are MCU-padded, component c at plane_off[c] + t * plane_h[c] * plane_w[c]
struct DecPlan {
  int T, H, W, ncomp, hs, vs, rows, cols, bpm;
  int plane_h[3], plane_w[3], ext_h[3], ext_w[3];
  long long per, nblk, plane_off[3], coef_bytes, scratch;
};

// (a) one lane per segment, and one segment per wave: the lanes of a wave run in lock step, and 64 segments side by side are 64 bit
// streams at 64 different points of the decoder, so every step would run every branch and wait for whichever lane's byte loads were
// due.  A frame of 30 intervals is 30 waves; the device holds thousands.  Launched as nseg workgroups of one lane.
__global__ __launch_bounds__(64) void jpeg_huff_decode_kernel(const uint8_t* __restrict__ data, long long nbytes,
                                                              const int32_t* __restrict__ segs,
                                                              const uint8_t* __restrict__ huff, const uint8_t* __restrict__ sel, int T,
                                                              long long per, int bpm, int16_t* __restrict__ coef,
                                                              int32_t* __restrict__ status) {
  __shared__ uint32_t slice[JD_SLICE / 4];
  __shared__ __attribute__((aligned(16))) int16_t stage[64];
  const int seg = blockIdx.x;
  const int32_t* row = segs + (long long)seg * JD_SEG_FIELDS;
  if (!jd_row_ok(row, nbytes, T, per)) {
    status[seg] = JD_BAD_SEGMENT;
    return;
  }
  const int t = row[2];
  jd_stage_tables(reinterpret_cast<const uint32_t*>(huff + (long long)t * JD_HUFF_FRAME), slice);
  const uint32_t s4 = *reinterpret_cast<const uint32_t*>(sel + 4ll * t);
  status[seg] = jpeg_decode_segment(data + row[0], row[1], reinterpret_cast<const uint8_t*>(slice), s4, row[4], bpm, stage,
                                    coef + ((long long)t * per + row[3]) * bpm * 64);
}

// (b) one wave per block, four per workgroup; lane = zigzag position on the way in, = (y, x) of the sample on the way out
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt,
                                                        float* __restrict__ planes, DecPlan p) {
  __shared__ float sa[4][64], sb[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long blk = (long long)blockIdx.x * 4 + wave;
  const bool live = blk < p.nblk;
  int c = 0, y0 = 0, x0 = 0;
  long long t = 0;
  if (live) {
    const long long fb = p.per * p.bpm;
    t = blk / fb;
    const long long rem = blk - t * fb, mcu = rem / p.bpm;
    const int b = (int)(rem - mcu * p.bpm), r = (int)(mcu / p.cols), m = (int)(mcu - (long long)r * p.cols);
    const int ny = p.bpm == 1 ? 1 : p.bpm - 2;
    if (b < ny) {
      y0 = (r * p.vs + b / p.hs) * 8, x0 = (m * p.hs + b % p.hs) * 8;
    } else {
      c = b - ny + 1, y0 = r * 8, x0 = m * 8;
    }
    const int nat = DEC_ZIGZAG[lane];
    sa[wave][nat] = (float)coef[blk * 64 + lane] * (float)qt[(t * 3 + c) * 64 + nat];
  }
  __syncthreads();
  const int i = lane >> 3, j = lane & 7;
  if (live) {                                       // rows of F: tmp[u][x] = sum_v F[u][v] C[v][x]
    float a = 0.f;
#pragma unroll
    for (int v = 0; v < 8; ++v) a += sa[wave][i * 8 + v] * DEC_C[v][j];
    sb[wave][lane] = a;
  }
  __syncthreads();
  if (live) {                                       // columns: out[y][x] = sum_u C[u][y] tmp[u][x]
    float a = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) a += DEC_C[u][i] * sb[wave][u * 8 + j];
    a = fminf(fmaxf(a + 128.0f, 0.0f), 255.0f);
    planes[p.plane_off[c] + (t * p.plane_h[c] + y0 + i) * p.plane_w[c] + x0 + j] = a;
  }
}

// chroma sample (cy, cx) of the pixel (y, x): triangle filter where the factor is 2, vertical first; far = the other neighbour of the
// pixel's position, both clamped to the component's own extent
__device__ __forceinline__ float dec_chroma(const float* __restrict__ pl, int pw, int eh, int ew, int y, int x, int hs, int vs) {
  int rn = y, rf = y, cn = x, cf = x;
  if (vs == 2) {
    rn = y >> 1, rf = rn + ((y & 1) ? 1 : -1);
    rf = rf < 0 ? 0 : (rf > eh - 1 ? eh - 1 : rf);
  }
  if (hs == 2) {
    cn = x >> 1, cf = cn + ((x & 1) ? 1 : -1);
    cf = cf < 0 ? 0 : (cf > ew - 1 ? ew - 1 : cf);
  }
  float vn = pl[(long long)rn * pw + cn], vf = pl[(long long)rn * pw + cf];
  if (vs == 2) {
    vn = 0.75f * vn + 0.25f * pl[(long long)rf * pw + cn];
    vf = 0.75f * vf + 0.25f * pl[(long long)rf * pw + cf];
  }
  return hs == 2 ? 0.75f * vn + 0.25f * vf : vn;
}

__device__ __forceinline__ uint8_t dec_byte(float v) { return (uint8_t)fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f); }

// (c) one lane per pixel
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const float* __restrict__ planes, uint8_t* __restrict__ out, long long stride_t,
                                                       DecPlan p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, hw = (long long)p.H * p.W;
  if (idx >= hw * p.T) return;
  const long long t = idx / hw, rem = idx - t * hw;
  const int y = (int)(rem / p.W), x = (int)(rem - (long long)y * p.W);
  const float Y = planes[p.plane_off[0] + (t * p.plane_h[0] + y) * p.plane_w[0] + x];
  uint8_t* o = out + t * stride_t + rem * 3;
  if (p.ncomp == 1) {
    const uint8_t g = dec_byte(Y);
    o[0] = g, o[1] = g, o[2] = g;
    return;
  }
  const float cb = dec_chroma(planes + p.plane_off[1] + t * p.plane_h[1] * p.plane_w[1], p.plane_w[1], p.ext_h[1], p.ext_w[1], y, x, p.hs,
                              p.vs) - 128.0f;
  const float cr = dec_chroma(planes + p.plane_off[2] + t * p.plane_h[2] * p.plane_w[2], p.plane_w[2], p.ext_h[2], p.ext_w[2], y, x, p.hs,
                              p.vs) - 128.0f;
  o[0] = dec_byte(Y + 1.402f * cr);
  o[1] = dec_byte((Y - 0.344136286f * cb) - 0.714136286f * cr);
  o[2] = dec_byte(Y + 1.772f * cb);
}

// (d) one lane per output pixel; the tables are clamped into the crop window, so no table content can move a read outside it
__global__ __launch_bounds__(256) void resize_u8_kernel(const uint8_t* __restrict__ src, long long src_stride_t, int pitch, int Hc, int Wc,
                                                        uint8_t* __restrict__ dst, long long dst_stride_t, int Hd, int Wd, int T,
                                                        const int32_t* __restrict__ ys, const int32_t* __restrict__ yn,
                                                        const float* __restrict__ yw, int ky, const int32_t* __restrict__ xs,
                                                        const int32_t* __restrict__ xn, const float* __restrict__ xw, int kx) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, hw = (long long)Hd * Wd;
  if (idx >= hw * T) return;
  const long long t = idx / hw, rem = idx - t * hw;
  const int oy = (int)(rem / Wd), ox = (int)(rem - (long long)oy * Wd);
  int y0 = ys[oy], ny = yn[oy], x0 = xs[ox], nx = xn[ox];
  y0 = y0 < 0 ? 0 : (y0 > Hc - 1 ? Hc - 1 : y0);
  x0 = x0 < 0 ? 0 : (x0 > Wc - 1 ? Wc - 1 : x0);
  ny = ny > ky ? ky : ny, ny = ny > Hc - y0 ? Hc - y0 : ny;
  nx = nx > kx ? kx : nx, nx = nx > Wc - x0 ? Wc - x0 : nx;
  const float* wy = yw + (long long)oy * ky;
  const float* wx = xw + (long long)ox * kx;
  const uint8_t* f = src + t * src_stride_t;
  float r = 0.f, g = 0.f, b = 0.f;
  for (int j = 0; j < nx; ++j) {
    const uint8_t* col = f + (long long)y0 * pitch + (x0 + j) * 3ll;
    float vr = 0.f, vg = 0.f, vb = 0.f;
    for (int i = 0; i < ny; ++i) {
      const uint8_t* q = col + (long long)i * pitch;
      const float w = wy[i];
      vr += w * (float)q[0], vg += w * (float)q[1], vb += w * (float)q[2];
    }
    const float w = wx[j];
    r += w * vr, g += w * vg, b += w * vb;
  }
  uint8_t* o = dst + t * dst_stride_t + rem * 3;
  o[0] = dec_byte(r), o[1] = dec_byte(g), o[2] = dec_byte(b);
}

inline long long dec_up(long long v, long long a) { return (v + a - 1) / a * a; }

int dec_plan(const char* fn, int T, int H, int W, int ncomp, int hs, int vs, DecPlan* p) {
  LL_REQUIRE(T >= 1 && H >= 1 && W >= 1, "%s: empty input %d x %d x %d", fn, T, H, W);
  LL_REQUIRE(H <= 65535 && W <= 65535, "%s: H=%d, W=%d: a JPEG frame holds at most 65535 rows and columns", fn, H, W);
  LL_REQUIRE(ncomp == 1 || ncomp == 3, "%s: components=%d: 1 (grey) or 3 (YCbCr)", fn, ncomp);
  if (ncomp == 1) {
    LL_REQUIRE(hs == 1 && vs == 1, "%s: sampling %d x %d: a grey frame is 1 x 1", fn, hs, vs);
  } else {
    LL_REQUIRE((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2),
               "%s: luma sampling %d x %d is not 1 x 1 (4:4:4), 2 x 1 (4:2:2) or 2 x 2 (4:2:0)", fn, hs, vs);
  }
  p->T = T, p->H = H, p->W = W, p->ncomp = ncomp, p->hs = hs, p->vs = vs;
  p->rows = (H + 8 * vs - 1) / (8 * vs), p->cols = (W + 8 * hs - 1) / (8 * hs);
  p->bpm = ncomp == 1 ? 1 : hs * vs + 2;
  p->per = (long long)p->rows * p->cols;
  p->nblk = p->per * p->bpm * T;
  LL_REQUIRE(p->nblk <= 0x7fffffffll / 4, "%s: %d x %d x %d is more than one call covers (2^29 blocks)", fn, T, H, W);
  long long o = 0;
  for (int c = 0; c < 3; ++c) {
    const int ch = c == 0 ? vs : 1, cw = c == 0 ? hs : 1;
    p->plane_h[c] = p->rows * 8 * ch, p->plane_w[c] = p->cols * 8 * cw;
    p->ext_h[c] = (H * ch + vs - 1) / vs, p->ext_w[c] = (W * cw + hs - 1) / hs;
    p->plane_off[c] = o;
    if (c < ncomp) o += (long long)T * p->plane_h[c] * p->plane_w[c];
  }
  p->coef_bytes = p->nblk * 128;
  p->scratch = dec_up(o * 4, 256);
  return LL_OK;
}

int dec_check_entropy(const char* fn, const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff,
                      const uint8_t* sel, int16_t* coef, int32_t* status) {
  LL_REQUIRE(data != nullptr && segs != nullptr && huff != nullptr && sel != nullptr && coef != nullptr && status != nullptr,
             "%s: null operand", fn);
  LL_REQUIRE(nbytes >= 0 && nbytes <= 0x7fffffffll, "%s: nbytes=%lld must be 0 .. 2^31 - 1 (segment offsets are int32)", fn, nbytes);
  LL_REQUIRE(nseg >= 1, "%s: nseg=%d: at least one segment", fn, nseg);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(segs) & 3) == 0 && (reinterpret_cast<uintptr_t>(huff) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(sel) & 3) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
             "%s: segs, huff, sel and status must be 4-byte aligned", fn);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(coef) & 15) == 0, "%s: coef must be 16-byte aligned (blocks leave as 16-byte stores)", fn);
  return LL_OK;
}

int dec_check_pixels(const char* fn, const DecPlan& p, const int16_t* coef, const uint16_t* qt, uint8_t* out, long long stride_t,
                     void* scratch, long long scratch_bytes) {
  LL_REQUIRE(coef != nullptr && qt != nullptr && out != nullptr && scratch != nullptr, "%s: null operand", fn);
  LL_REQUIRE(stride_t >= 3ll * p.H * p.W, "%s: stride_t=%lld bytes must span a %d x %d x 3 frame", fn, stride_t, p.H, p.W);
  LL_REQUIRE(scratch_bytes >= p.scratch, "%s: scratch_bytes=%lld, %d x %d x %d needs %lld (ll_jpeg_decode_sizes)", fn, scratch_bytes, p.T,
             p.H, p.W, p.scratch);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "%s: scratch must be 16-byte aligned", fn);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(coef) & 1) == 0 && (reinterpret_cast<uintptr_t>(qt) & 1) == 0,
             "%s: coef and qt must be 2-byte aligned", fn);
  return LL_OK;
}

void dec_launch_entropy(const DecPlan& p, const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff,
                        const uint8_t* sel, int16_t* coef, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_huff_decode_kernel, dim3((unsigned)nseg), dim3(1), 0, s, data, nbytes, segs, huff, sel, p.T,
                     p.per, p.bpm, coef, status);
}

void dec_launch_pixels(const DecPlan& p, const int16_t* coef, const uint16_t* qt, uint8_t* out, long long stride_t, void* scratch,
                       hipStream_t s) {
  float* planes = static_cast<float*>(scratch);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((p.nblk + 3) / 4)), dim3(256), 0, s, coef, qt, planes, p);
  const long long px = (long long)p.T * p.H * p.W;
  hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, (const float*)planes, out, stride_t, p);
}

}  // namespace

extern "C" int ll_jpeg_decode_sizes(int T, int H, int W, int ncomp, int hs, int vs, long long* coef_bytes, long long* scratch_bytes) {
  LL_REQUIRE(coef_bytes != nullptr && scratch_bytes != nullptr, "ll_jpeg_decode_sizes: null operand");
  DecPlan p;
  if (int rc = dec_plan("ll_jpeg_decode_sizes", T, H, W, ncomp, hs, vs, &p)) return rc;
  *coef_bytes = p.coef_bytes;
  *scratch_bytes = p.scratch;
  return LL_OK;
}

extern "C" int ll_jpeg_decode_coefficients(const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff,
                                           const uint8_t* sel, int T, int H, int W, int ncomp, int hs, int vs, int16_t* coef,
                                           int32_t* status, ll_stream stream) {
  const char* fn = "ll_jpeg_decode_coefficients";
  if (int rc = dec_check_entropy(fn, data, nbytes, segs, nseg, huff, sel, coef, status)) return rc;
  DecPlan p;
  if (int rc = dec_plan(fn, T, H, W, ncomp, hs, vs, &p)) return rc;
  dec_launch_entropy(p, data, nbytes, segs, nseg, huff, sel, coef, status, (hipStream_t)stream);
  return ll_check_launch(fn);
}

extern "C" int ll_jpeg_decode_pixels(const int16_t* coef, const uint16_t* qt, int T, int H, int W, int ncomp, int hs, int vs, uint8_t* out,
                                     long long stride_t, void* scratch, long long scratch_bytes, ll_stream stream) {
  const char* fn = "ll_jpeg_decode_pixels";
  DecPlan p;
  if (int rc = dec_plan(fn, T, H, W, ncomp, hs, vs, &p)) return rc;
  if (int rc = dec_check_pixels(fn, p, coef, qt, out, stride_t, scratch, scratch_bytes)) return rc;
  dec_launch_pixels(p, coef, qt, out, stride_t, scratch, (hipStream_t)stream);
  return ll_check_launch(fn);
}

extern "C" int ll_jpeg_decode_u8(const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff,
                                 const uint8_t* sel, const uint16_t* qt, int T, int H, int W, int ncomp, int hs, int vs, int16_t* coef,
                                 int32_t* status, uint8_t* out, long long stride_t, void* scratch, long long scratch_bytes,
                                 ll_stream stream) {
  const char* fn = "ll_jpeg_decode_u8";
  if (int rc = dec_check_entropy(fn, data, nbytes, segs, nseg, huff, sel, coef, status)) return rc;
  DecPlan p;
  if (int rc = dec_plan(fn, T, H, W, ncomp, hs, vs, &p)) return rc;
  if (int rc = dec_check_pixels(fn, p, coef, qt, out, stride_t, scratch, scratch_bytes)) return rc;
  dec_launch_entropy(p, data, nbytes, segs, nseg, huff, sel, coef, status, (hipStream_t)stream);
  dec_launch_pixels(p, coef, qt, out, stride_t, scratch, (hipStream_t)stream);
  return ll_check_launch(fn);
}

extern "C" int ll_resize_u8(const uint8_t* src, long long src_stride_t, int Hs, int Ws, int y0, int x0, int Hc, int Wc, uint8_t* dst,
                            long long dst_stride_t, int Hd, int Wd, int T, const int32_t* ystart, const int32_t* ycount,
                            const float* yweight, int ky, const int32_t* xstart, const int32_t* xcount, const float* xweight, int kx,
                            ll_stream stream) {
  LL_REQUIRE(src != nullptr && dst != nullptr && ystart != nullptr && ycount != nullptr && yweight != nullptr && xstart != nullptr &&
                 xcount != nullptr && xweight != nullptr, "ll_resize_u8: null operand");
  LL_REQUIRE(T >= 1 && Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1, "ll_resize_u8: empty input %d x %d x %d -> %d x %d", T, Hs, Ws, Hd, Wd);
  LL_REQUIRE(Hs <= 65535 && Ws <= 65535 && Hd <= 65535 && Wd <= 65535, "ll_resize_u8: %d x %d -> %d x %d: at most 65535 rows and columns",
             Hs, Ws, Hd, Wd);
  LL_REQUIRE(y0 >= 0 && x0 >= 0 && Hc >= 1 && Wc >= 1 && y0 + Hc <= Hs && x0 + Wc <= Ws,
             "ll_resize_u8: crop window %d x %d at (%d, %d) leaves the %d x %d frame", Hc, Wc, y0, x0, Hs, Ws);
  LL_REQUIRE(src_stride_t >= 3ll * Hs * Ws, "ll_resize_u8: src_stride_t=%lld bytes must span a %d x %d x 3 frame", src_stride_t, Hs, Ws);
  LL_REQUIRE(dst_stride_t >= 3ll * Hd * Wd, "ll_resize_u8: dst_stride_t=%lld bytes must span a %d x %d x 3 frame", dst_stride_t, Hd, Wd);
  LL_REQUIRE(ky >= 1 && kx >= 1 && ky <= Hc + 1 && kx <= Wc + 1, "ll_resize_u8: ky=%d, kx=%d taps for a %d x %d window", ky, kx, Hc, Wc);
  LL_REQUIRE((long long)T * Hd * Wd <= 0x7fffffffll * 64, "ll_resize_u8: %d x %d x %d is more than one call covers", T, Hd, Wd);
  const long long px = (long long)T * Hd * Wd;
  hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     src + ((long long)y0 * Ws + x0) * 3, src_stride_t, Ws * 3, Hc, Wc, dst, dst_stride_t, Hd, Wd, T, ystart, ycount, yweight,
                     ky, xstart, xcount, xweight, kx);
  return ll_check_launch("ll_resize_u8");
}
