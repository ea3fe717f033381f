// Planar YUV: the per-pixel integer arithmetic of csrc/yuv.hip as plain C++ that compiles for the GPU and for the CPU (the tests build
// it with the host compiler under sanitizers).  BT.601 (Kr = 0.299, Kg = 0.587, Kb = 0.114) in 2^16 fixed point, limited range
// (sy = 219/255, sc = 224/255, yoff = 16) or full range (sy = sc = 1, yoff = 0); rnd(x) = floor(x + 1/2) on the exact value, every
// shift arithmetic (floor).  DESIGN.md section 5c, "Planar YUV and Y4M", derives the constants; tests/yuv_ref.py restates them.
//
// RGB -> I420, chroma at the centre of its 2 x 2 pixels (S_c = the sum of channel c over them, 0 .. 1020):
//   Y  = yoff + ((aR R + aG G + aB B + 2^15) >> 16)        aR = rnd(Kr sy 2^16), aB = rnd(Kb sy 2^16), aG = rnd(sy 2^16) - aR - aB
//   Cb = 128 + ((bR S_R + bG S_G + bB S_B + 2^17) >> 18)   bR = -rnd(Kr / (2 (1 - Kb)) sc 2^16), bG likewise with Kg, bB = -(bR + bG)
//   Cr = 128 + ((cR S_R + cG S_G + cB S_B + 2^17) >> 18)   cG = -rnd(Kg / (2 (1 - Kr)) sc 2^16), cB likewise with Kb, cR = -(cG + cB)
//   clamped to [16, 235] / [16, 240] (limited) or [0, 255] (full).  Each chroma row sums to zero: grey gives exactly 128.
// YUV -> RGB: chroma is brought to luma resolution in units of 1/16 (U16, V16: per axis a near and a far sample with weights in
// quarters, yuv_axis), then with y = 16 cy (Y - yoff), u = U16 - 2048, v = V16 - 2048:
//   R = clamp((y + crv v + 2^19) >> 20),  G = clamp((y - cgu u - cgv v + 2^19) >> 20),  B = clamp((y + cbu u + 2^19) >> 20)
//   cy = rnd(2^16 / sy), crv = rnd(2 (1 - Kr) / sc 2^16), cbu = rnd(2 (1 - Kb) / sc 2^16), cgu = rnd(Kb 2 (1 - Kb) / Kg / sc 2^16),
//   cgv = rnd(Kr 2 (1 - Kr) / Kg / sc 2^16).  The largest accumulator is about 5.6e8: everything fits int32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YUV_HD __host__ __device__
#else
#define YUV_HD
#endif

// plane layouts of ll_yuv_to_frames_u8 (the Y4M C tags 420jpeg / 420, 420mpeg2, 420paldv, 422, 444, mono)
enum { YUV_420JPEG = 0, YUV_420MPEG2 = 1, YUV_420PALDV = 2, YUV_422 = 3, YUV_444 = 4, YUV_MONO = 5, YUV_LAYOUTS = 6 };
// how one axis of a layout sites its chroma
enum { YUV_CENTRE = 0, YUV_COSITED = 1, YUV_NONE = 2 };

YUV_HD constexpr int yuv_vmode(int layout) { return layout <= YUV_420MPEG2 ? YUV_CENTRE : layout == YUV_420PALDV ? YUV_COSITED : YUV_NONE; }
YUV_HD constexpr int yuv_hmode(int layout) { return layout == YUV_420JPEG ? YUV_CENTRE : layout <= YUV_422 ? YUV_COSITED : YUV_NONE; }
// chroma plane size of an H x W frame (0 for mono)
YUV_HD constexpr int yuv_chroma_h(int layout, int H) { return layout == YUV_MONO ? 0 : yuv_vmode(layout) == YUV_NONE ? H : (H + 1) / 2; }
YUV_HD constexpr int yuv_chroma_w(int layout, int W) { return layout == YUV_MONO ? 0 : yuv_hmode(layout) == YUV_NONE ? W : (W + 1) / 2; }

YUV_HD inline int yuv_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

YUV_HD inline int yuv_luma(int R, int G, int B, int full) {
  const int aR = full ? 19595 : 16829, aG = full ? 38470 : 33039, aB = full ? 7471 : 6416;
  const int y = (full ? 0 : 16) + ((aR * R + aG * G + aB * B + (1 << 15)) >> 16);
  return yuv_clamp(y, full ? 0 : 16, full ? 255 : 235);
}

// SR, SG, SB: the channel sums of the 2 x 2 pixels
YUV_HD inline void yuv_chroma(int SR, int SG, int SB, int full, int* cb, int* cr) {
  const int bR = full ? -11058 : -9714, bG = full ? -21710 : -19071, bB = -(bR + bG);
  const int cG = full ? -27439 : -24103, cB = full ? -5329 : -4681, cR = -(cG + cB);
  const int lo = full ? 0 : 16, hi = full ? 255 : 240;
  *cb = yuv_clamp(128 + ((bR * SR + bG * SG + bB * SB + (1 << 17)) >> 18), lo, hi);
  *cr = yuv_clamp(128 + ((cR * SR + cG * SG + cB * SB + (1 << 17)) >> 18), lo, hi);
}

// One axis of the upsampling: luma position o on an axis with n chroma samples takes sample *near with weight 4 - *wfar and sample
// *far with weight *wfar (quarters).  The far index is clamped to the plane.
YUV_HD inline void yuv_axis(int mode, int o, int n, int* near, int* far, int* wfar) {
  if (mode == YUV_NONE) {
    *near = *far = o;
    *wfar = 0;
    return;
  }
  const int c = o >> 1;
  const int f = mode == YUV_CENTRE ? ((o & 1) ? c + 1 : c - 1) : c + 1;
  *near = c;
  *far = yuv_clamp(f, 0, n - 1);
  *wfar = mode == YUV_CENTRE ? 1 : (o & 1) ? 2 : 0;
}

// U16, V16 in 1/16 (2048 = no colour)
YUV_HD inline void yuv_rgb(int Y, int U16, int V16, int full, int* R, int* G, int* B) {
  const int cy = full ? 65536 : 76309, crv = full ? 91881 : 104597, cbu = full ? 116130 : 132201;
  const int cgu = full ? 22553 : 25675, cgv = full ? 46802 : 53279;
  const int y = 16 * cy * (Y - (full ? 0 : 16)), u = U16 - 2048, v = V16 - 2048;
  // clamp((x >> 20), 0, 255) written as clamp(x, 0, 2^28 - 1) >> 20: the same value for every x.  The first form is what hipcc
  // turns into v_ashr_pk_u8_i32 on gfx950 and then reads as if the upper half of its result were zero, which it is not on the
  // hardware (the bytes packed next to it came out OR-ed with leftovers); this form compiles to v_med3_i32 and a shift.
  const int top = (256 << 20) - 1;
  *R = yuv_clamp(y + crv * v + (1 << 19), 0, top) >> 20;
  *G = yuv_clamp(y - cgu * u - cgv * v + (1 << 19), 0, top) >> 20;
  *B = yuv_clamp(y + cbu * u + (1 << 19), 0, top) >> 20;
}

// One chroma plane (hc x wc, rows contiguous) at luma position (oy, ox), in 1/16
YUV_HD inline int yuv_upsample16(const uint8_t* plane, int hc, int wc, int layout, int oy, int ox) {
  int ny, fy, wy, nx, fx, wx;
  yuv_axis(yuv_vmode(layout), oy, hc, &ny, &fy, &wy);
  yuv_axis(yuv_hmode(layout), ox, wc, &nx, &fx, &wx);
  const uint8_t *rn = plane + (long long)ny * wc, *rf = plane + (long long)fy * wc;
  return (4 - wy) * ((4 - wx) * rn[nx] + wx * rn[fx]) + wy * ((4 - wx) * rf[nx] + wx * rf[fx]);
}

// The whole inverse for one pixel of an H x W frame (cb, cr unused for mono): what every lane of yuv_to_frames_u8_kernel computes
YUV_HD inline void yuv_pixel_rgb(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, int H, int W, int layout, int full, int oy, int ox,
                                 uint8_t* rgb) {
  int U16 = 2048, V16 = 2048, R, G, B;
  if (layout != YUV_MONO) {
    const int hc = yuv_chroma_h(layout, H), wc = yuv_chroma_w(layout, W);
    U16 = yuv_upsample16(cb, hc, wc, layout, oy, ox);
    V16 = yuv_upsample16(cr, hc, wc, layout, oy, ox);
  }
  yuv_rgb(y[(long long)oy * W + ox], U16, V16, full, &R, &G, &B);
  rgb[0] = (uint8_t)R;
  rgb[1] = (uint8_t)G;
  rgb[2] = (uint8_t)B;
}
