// csrc/yuv.h on the CPU, as a stand-alone program for the host sanitizers (tests/test_yuv_host.py builds it with
// -fsanitize=address,undefined and compares every printed line with tests/yuv_ref.py).  No input; everything is seeded.
//   luma <full> <sum>            all 2^24 RGB values: sum over idx = R << 16 | G << 8 | B of Y * (1 + idx % 65521), mod 2^64
//   quad <full> <k> <cb> <cr>    2 x 2 pixel quads: the all-equal and extreme ones, then seeded ones
//   up <layout> <full> <H> <W> <sum>   the inverse over exactly-sized heap planes: sum over byte index i of rgb[i] * (1 + i % 251)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "yuv.h"

static uint32_t lcg_state;
static int lcg_byte() {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return (int)(lcg_state >> 24);
}

int main() {
  for (int full = 0; full < 2; ++full) {
    uint64_t sum = 0;
    for (uint32_t idx = 0; idx < (1u << 24); ++idx)
      sum += (uint64_t)yuv_luma((int)(idx >> 16), (int)((idx >> 8) & 255), (int)(idx & 255), full) * (1 + idx % 65521);
    std::printf("luma %d %llu\n", full, (unsigned long long)sum);
  }
  // quads: 4 pixels x RGB
  std::vector<std::vector<int>> quads;
  for (int v : {0, 1, 127, 128, 254, 255}) quads.push_back(std::vector<int>(12, v));
  for (int c = 0; c < 3; ++c)
    for (int hi = 0; hi < 2; ++hi) {      // one channel at an extreme, the others at the opposite one
      std::vector<int> q(12);
      for (int p = 0; p < 4; ++p)
        for (int k = 0; k < 3; ++k) q[3 * p + k] = (k == c) == (hi == 1) ? 255 : 0;
      quads.push_back(q);
    }
  lcg_state = 12345u;
  for (int n = 0; n < 64; ++n) {
    std::vector<int> q(12);
    for (int& b : q) b = lcg_byte();
    quads.push_back(q);
  }
  for (int full = 0; full < 2; ++full)
    for (size_t k = 0; k < quads.size(); ++k) {
      int s[3] = {0, 0, 0}, cb, cr;
      for (int p = 0; p < 4; ++p)
        for (int c = 0; c < 3; ++c) s[c] += quads[k][3 * p + c];
      yuv_chroma(s[0], s[1], s[2], full, &cb, &cr);
      std::printf("quad %d %zu %d %d\n", full, k, cb, cr);
    }
  // the six layouts over planes that are exactly as large as the layout says: a read outside one is the sanitizer's to report
  const int sizes[5][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 5}, {8, 9}};
  lcg_state = 777u;
  for (int layout = 0; layout < YUV_LAYOUTS; ++layout)
    for (int full = 0; full < 2; ++full)
      for (const auto& hw : sizes) {
        const int H = hw[0], W = hw[1], hc = yuv_chroma_h(layout, H), wc = yuv_chroma_w(layout, W);
        uint8_t* y = new uint8_t[(size_t)H * W];
        uint8_t* cb = layout == YUV_MONO ? nullptr : new uint8_t[(size_t)hc * wc];
        uint8_t* cr = layout == YUV_MONO ? nullptr : new uint8_t[(size_t)hc * wc];
        for (int i = 0; i < H * W; ++i) y[i] = (uint8_t)lcg_byte();
        for (int i = 0; i < hc * wc; ++i) cb[i] = (uint8_t)lcg_byte();
        for (int i = 0; i < hc * wc; ++i) cr[i] = (uint8_t)lcg_byte();
        uint8_t* rgb = new uint8_t[(size_t)H * W * 3];
        for (int oy = 0; oy < H; ++oy)
          for (int ox = 0; ox < W; ++ox) yuv_pixel_rgb(y, cb, cr, H, W, layout, full, oy, ox, rgb + ((size_t)oy * W + ox) * 3);
        uint64_t sum = 0;
        for (int i = 0; i < H * W * 3; ++i) sum += (uint64_t)rgb[i] * (1 + i % 251);
        std::printf("up %d %d %d %d %llu\n", layout, full, H, W, (unsigned long long)sum);
        delete[] y;
        delete[] cb;
        delete[] cr;
        delete[] rgb;
      }
  return 0;
}
