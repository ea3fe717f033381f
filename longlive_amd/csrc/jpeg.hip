// Frames out: a baseline JPEG encoder (ITU T.81, JFIF) for uint8 RGB frames [T, H, W, 3], every stage on the GPU and stream-ordered.
//
// Format, fixed: SOF0, 8 bits, Y 2x2 + Cb, Cr 1x1 (4:2:0; MCU = 16 x 16 pixels, blocks Y00 Y01 Y10 Y11 Cb Cr), the Annex K Huffman
// and quantisation tables (the latter scaled by the IJG rule), a restart interval of one MCU row, edge replication into the padding.
// Arithmetic, fixed and fp32: Y = 0.299 R + 0.587 G + 0.114 B - 128, Cb = -0.168735892 R - 0.331264108 G + 0.5 B,
// Cr = 0.5 R - 0.418687589 G - 0.081312411 B (each evaluated around G, so grey pixels are exact), chroma = mean of its 2 x 2 pixels,
// orthonormal 8 x 8 DCT-II as two passes of the 8 x 8 cosine matrix with the two k = 0 scalings applied at the end (DC = sum / 8,
// exact for whole numbers), coefficient = rint(dct / q) as int16 in zigzag order.  tests/jpeg_ref.py restates all of it in fp64.
//
// Launches of ll_jpeg_encode_u8 (nothing is accumulated in place, so no scratch has to start as zero):
//   (a) jpeg_coef_kernel      one wave per MCU: colour, DCT, quantise -> coef [T, rows, cols, 6, 64] int16
//   (b) jpeg_block_bits_kernel one lane per 8 x 8 block: its code bits, MSB first, into a private 208-byte slot + the bit count
//                              (64 coefficients x at most 16 + 10 bits; DC takes 9 + 11, ZRL 11 per 16 zeros, EOB 4)
//   (c) jpeg_interval_kernel  one workgroup per restart interval: scan of the bit counts, the interval's bytes GATHERED from the
//                              slots (a search of the scanned offsets per 8 bytes), padded with 1-bits, 0xFF bytes counted and
//                              scanned, written with FF 00 stuffing into the interval's staging slot, RSTm appended, length noted
//   (d) jpeg_assemble_kernel  one workgroup per interval: sum of the lengths before it, copy behind the header; the first writes the
//                              header (a function of W, H, quality), the last EOI and sizes[t]
#include "common.h"

namespace {

constexpr int JPEG_HEADER = 613;       // SOI 2 + APP0 18 + DQT 134 + SOF0 19 + DHT 420 + DRI 6 + SOS 14
constexpr int JPEG_SLOT_WORDS = 52;    // 208 bytes: the most bits a block can take
constexpr int JPEG_BLOCK_BYTES = 416;  // 208 bytes doubled by stuffing

// ITU T.81 Annex K, tables K.1 / K.2 (natural order)
__device__ const uint8_t Q_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

__device__ const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K, tables K.3 - K.6: BITS (codes per length 1..16) and HUFFVAL; table 0 / 1 = DC luminance / chrominance, 2 / 3 = AC
__device__ const uint8_t HUFF_BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                             {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                             {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                             {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
__device__ const uint8_t HUFF_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
     0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
     0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
     0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
     0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
     0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
     0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
     0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
     0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
     0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
     0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
     0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// the fixed bytes of the header; the H, W and restart-interval fields (zero here) and the quantisation tables are patched in
__device__ const uint8_t HDR_APP0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
__device__ const uint8_t HDR_SOF0[19] = {0xFF, 0xC0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
__device__ const uint8_t HDR_SOS[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};

// C[k][n] = a_k cos((2n + 1) k pi / 16), a_0 = sqrt(1/8), a_k = 1/2: Cj = cos(j pi / 16) / 2
#define C1 0.49039264020161522f
#define C2 0.46193976625564337f
#define C3 0.41573480615127262f
#define C4 0.35355339059327379f
#define C5 0.27778511650980109f
#define C6 0.19134171618254489f
#define C7 0.09754516100806412f
__device__ const float DCT_C[8][8] = {{C4, C4, C4, C4, C4, C4, C4, C4},     {C1, C3, C5, C7, -C7, -C5, -C3, -C1},
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

// IJG scaling of a base table entry (natural index n of table tb) for quality 1..100
__device__ __forceinline__ int jpeg_q(int tb, int n, int quality) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = ((int)Q_BASE[tb][n] * s + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}

__device__ uint8_t jpeg_header_byte(int i, int H, int W, int cols, int quality) {
  if (i < 20) return HDR_APP0[i];
  if (i < 154) {                                    // DQT: FF DB 00 84, then (id, 64 entries in zigzag order) twice
    int j = i - 20;
    if (j < 4) return j == 0 ? 0xFF : (j == 1 ? 0xDB : (j == 2 ? 0 : 132));
    j -= 4;
    const int tb = j / 65, r = j % 65;
    return r == 0 ? (uint8_t)tb : (uint8_t)jpeg_q(tb, ZIGZAG[r - 1], quality);
  }
  if (i < 173) {
    const int j = i - 154;
    if (j == 5) return (uint8_t)(H >> 8);
    if (j == 6) return (uint8_t)(H & 255);
    if (j == 7) return (uint8_t)(W >> 8);
    if (j == 8) return (uint8_t)(W & 255);
    return HDR_SOF0[j];
  }
  if (i < 593) {                                    // DHT: FF C4 01 A2, then DC lum (00), AC lum (10), DC chr (01), AC chr (11)
    int j = i - 173;
    if (j < 4) return j == 0 ? 0xFF : (j == 1 ? 0xC4 : (j == 2 ? 0x01 : 0xA2));
    j -= 4;
    const int chr = j >= 208 ? 1 : 0;
    j -= 208 * chr;
    const int ac = j >= 29 ? 1 : 0;
    j -= 29 * ac;
    if (j == 0) return (uint8_t)((ac << 4) | chr);
    if (j < 17) return HUFF_BITS[2 * ac + chr][j - 1];
    return ac ? HUFF_AC_VALS[chr][j - 17] : (uint8_t)(j - 17);
  }
  if (i < 599) {                                    // DRI: one MCU row
    const int j = i - 593;
    return j == 0 ? 0xFF : (j == 1 ? 0xDD : (j == 2 ? 0 : (j == 3 ? 4 : (j == 4 ? (uint8_t)(cols >> 8) : (uint8_t)(cols & 255)))));
  }
  return HDR_SOS[i - 599];
}

// (a) one wave per MCU, four per workgroup.  Lane l owns the 2 x 2 pixels at (2 (l / 8), 2 (l % 8)) of the MCU: four Y samples and one
// Cb / Cr mean.  Rows and columns past the frame read its last row / column.
__global__ __launch_bounds__(256) void jpeg_coef_kernel(const uint8_t* __restrict__ px, long long st, int H, int W, int rows, int cols,
                                                        int quality, int16_t* __restrict__ coef, long long mcus) {
  __shared__ float sm[4][6 * 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long mcu = (long long)blockIdx.x * 4 + wave;
  const bool live = mcu < mcus;
  float* s = sm[wave];
  if (live) {
    const long long per = (long long)rows * cols, t = mcu / per, rem = mcu - t * per;
    const int r = (int)(rem / cols), m = (int)(rem - (long long)r * cols);
    const int qy = lane >> 3, qx = lane & 7;
    const uint8_t* f = px + t * st;
    float cb = 0.f, cr = 0.f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int yy = 2 * qy + dy, xx = 2 * qx + dx;
        int y = r * 16 + yy, x = m * 16 + xx;
        y = y < H ? y : H - 1;
        x = x < W ? x : W - 1;
        const uint8_t* p = f + ((long long)y * W + x) * 3;
        const float R = (float)p[0], G = (float)p[1], B = (float)p[2];
        // the three weights of each row sum to 1, 0 and 0: written around G, a grey pixel gives exactly G - 128, 0 and 0
        const float rg = R - G, bg = B - G;
        s[((yy >> 3) * 2 + (xx >> 3)) * 64 + (yy & 7) * 8 + (xx & 7)] = (G + (0.299f * rg + 0.114f * bg)) - 128.0f;
        cb += 0.5f * bg - 0.168735892f * rg;
        cr += 0.5f * rg - 0.081312411f * bg;
      }
    s[4 * 64 + qy * 8 + qx] = 0.25f * cb;
    s[5 * 64 + qy * 8 + qx] = 0.25f * cr;
  }
  __syncthreads();
  if (live && lane < 48) {                          // rows: 6 blocks x 8, each in place
    float* row = s + (lane >> 3) * 64 + (lane & 7) * 8;
    float x[8], o[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = row[n];
    o[0] = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));      // k = 0 without its sqrt(1/8): see the last step
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      float a = 0.f;
#pragma unroll
      for (int n = 0; n < 8; ++n) a += DCT_C[k][n] * x[n];
      o[k] = a;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = o[k];
  }
  __syncthreads();
  if (live && lane < 48) {                          // columns
    float* col = s + (lane >> 3) * 64 + (lane & 7);
    float x[8], o[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = col[n * 8];
    o[0] = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));      // k = 0 without its sqrt(1/8): see the last step
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      float a = 0.f;
#pragma unroll
      for (int n = 0; n < 8; ++n) a += DCT_C[k][n] * x[n];
      o[k] = a;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) col[k * 8] = o[k];
  }
  __syncthreads();
  if (live) {                                       // lane = zigzag position: 128-byte rows of int16 leave the wave whole
    const int nat = ZIGZAG[lane];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      // the k = 0 rows of both passes are plain sums, so the DC term is sum / 8: exact for the whole-number samples of grey
      // pixels, and a flat block's quotient lands on a tie (white at q = 16: 63.5) exactly where fp64 puts it, not beside it
      const float k0 = 0.35355339059327379f;
      const float scale = nat == 0 ? 0.125f : ((nat & 7) == 0 || (nat >> 3) == 0 ? k0 : 1.0f);
      float c = __builtin_rintf(s[b * 64 + nat] * scale / (float)jpeg_q(b < 4 ? 0 : 1, nat, quality));
      // what 8-bit input can reach is [-1024, 1016] for DC and under 1000 for AC; the clamp is what keeps (b)'s 26-bit bound unconditional
      const float lo = lane == 0 ? -1024.f : -1023.f;
      c = fminf(fmaxf(c, lo), 1023.f);
      coef[(mcu * 6 + b) * 64 + lane] = (int16_t)c;
    }
  }
}

__device__ __forceinline__ int jpeg_category(int v) {
  const int a = v < 0 ? -v : v;
  return a == 0 ? 0 : 32 - __builtin_clz((unsigned)a);
}

// (b) one lane per block.  tab = (length << 16) | code, built per workgroup from BITS / HUFFVAL (canonical codes, Annex C).
__global__ __launch_bounds__(256) void jpeg_block_bits_kernel(const int16_t* __restrict__ coef, long long nblk, int bpi,
                                                              uint32_t* __restrict__ bits, int* __restrict__ nbits) {
  __shared__ uint32_t dc_tab[2][12];
  __shared__ uint32_t ac_tab[2][256];
  const int tid = threadIdx.x;
  ac_tab[0][tid] = 0u;
  ac_tab[1][tid] = 0u;
  __syncthreads();
  for (int tb = 0; tb < 4; ++tb) {
    const int count = tb < 2 ? 12 : 162;
    if (tid < count) {
      int code = 0, k = 0, len = 0;
      for (int l = 1; l <= 16; ++l) {
        const int n = HUFF_BITS[tb][l - 1];
        if (tid < k + n) {
          code += tid - k;
          len = l;
          break;
        }
        code = (code + n) << 1;
        k += n;
      }
      const uint32_t e = ((uint32_t)len << 16) | (uint32_t)code;
      if (tb < 2) dc_tab[tb][tid] = e;
      else ac_tab[tb - 2][HUFF_AC_VALS[tb - 2][tid]] = e;
    }
  }
  __syncthreads();
  const long long blk = (long long)blockIdx.x * 256 + tid;
  if (blk >= nblk) return;
  const int bi = (int)(blk % bpi), c = bi % 6, m = bi / 6;
  const int chr = c >= 4 ? 1 : 0;
  long long pb = -1;                                // the previous block of this component inside the interval
  if (c == 0) { if (m > 0) pb = blk - 3; }
  else if (c < 4) pb = blk - 1;
  else if (m > 0) pb = blk - 6;
  const int pred = pb >= 0 ? (int)coef[pb * 64] : 0;

  uint32_t* dst = bits + blk * JPEG_SLOT_WORDS;
  uint64_t acc = 0;
  int nacc = 0, words = 0, total = 0;
  auto put = [&](uint32_t code, int len) {          // len <= 26, nacc < 32 on entry
    acc = (acc << len) | code;
    nacc += len;
    total += len;
    if (nacc >= 32) {
      dst[words++] = (uint32_t)(acc >> (nacc - 32));
      nacc -= 32;
    }
  };
  auto put_value = [&](uint32_t e, int v, int cat) {
    const uint32_t amp = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
    put(((e & 0xffffu) << cat) | amp, (int)(e >> 16) + cat);
  };

  const int4* src = reinterpret_cast<const int4*>(coef + blk * 64);
  int run = 0;
  for (int g = 0; g < 8; ++g) {
    const int4 q = src[g];
    const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = (int)(int16_t)((uint32_t)w[j >> 1] >> (16 * (j & 1)));
      if (g == 0 && j == 0) {
        const int d = v - pred, cat = jpeg_category(d);
        put_value(dc_tab[chr][cat], d, cat);
      } else if (v == 0) {
        ++run;
      } else {
        while (run > 15) {
          const uint32_t z = ac_tab[chr][0xF0];
          put(z & 0xffffu, (int)(z >> 16));
          run -= 16;
        }
        const int cat = jpeg_category(v);
        put_value(ac_tab[chr][(run << 4) | cat], v, cat);
        run = 0;
      }
    }
  }
  if (run > 0) {
    const uint32_t z = ac_tab[chr][0x00];
    put(z & 0xffffu, (int)(z >> 16));
  }
  if (nacc > 0) dst[words] = (uint32_t)(acc << (32 - nacc));
  nbits[blk] = total;
}

// inclusive scan over the 256 threads of a workgroup; sh[255] is the total until the next call
__device__ __forceinline__ int jpeg_scan256(int v, int* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int t = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
  return sh[tid];
}

// (c) one workgroup per restart interval (bpi blocks).  A thread produces 8 consecutive bytes of the interval per tile of 2048.
__global__ __launch_bounds__(256) void jpeg_interval_kernel(const uint32_t* __restrict__ bits, const int* __restrict__ nbits,
                                                            int* __restrict__ boff, uint8_t* __restrict__ stuffed, long long istride,
                                                            int* __restrict__ ilen, int bpi, int rows) {
  __shared__ int sh[256];
  const int tid = threadIdx.x;
  const long long iv = blockIdx.x, b0 = iv * bpi;
  const int row = (int)(iv % rows);
  const int* nb = nbits + b0;
  int* bo = boff + b0;
  int carry = 0;
  for (int base = 0; base < bpi; base += 256) {
    const int i = base + tid, v = i < bpi ? nb[i] : 0;
    const int incl = jpeg_scan256(v, sh);
    if (i < bpi) bo[i] = carry + incl - v;
    carry += sh[255];
  }
  __syncthreads();                                  // bo[] of this workgroup is read below by its other threads
  const int nbytes = (carry + 7) >> 3;              // bpi <= 24576 blocks of <= 1664 bits: under 2^26
  uint8_t* o = stuffed + iv * istride;
  int ffs = 0;
  for (int base = 0; base < nbytes; base += 2048) {
    const int j0 = base + tid * 8;
    const int n = nbytes - j0 < 8 ? (nbytes - j0 < 0 ? 0 : nbytes - j0) : 8;
    uint64_t pk = 0;
    int nff = 0;
    if (n > 0) {
      const int p = j0 * 8;
      int lo = 0, hi = bpi - 1;                     // the last block whose first bit is at or before p (every block has >= 4 bits)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (bo[mid] <= p) lo = mid;
        else hi = mid - 1;
      }
      int k = lo, local = p - bo[k], kn = nb[k];
      for (int q = 0; q < n; ++q) {
        uint32_t val = 0;
        int need = 8;
        while (need > 0 && k < bpi) {
          const int avail = kn - local, take = need < avail ? need : avail;
          const uint32_t* w = bits + (b0 + k) * JPEG_SLOT_WORDS;
          const int wi = local >> 5, sh0 = local & 31;
          const uint64_t two = ((uint64_t)w[wi] << 32) | (uint64_t)(wi + 1 < JPEG_SLOT_WORDS ? w[wi + 1] : 0u);
          val = (val << take) | ((uint32_t)(two >> (64 - sh0 - take)) & ((1u << take) - 1u));
          need -= take;
          local += take;
          if (local == kn) {
            ++k;
            local = 0;
            kn = k < bpi ? nb[k] : 0;
          }
        }
        if (need > 0) val = (val << need) | ((1u << need) - 1u);      // the interval's last byte: padded with 1-bits
        pk |= (uint64_t)val << (8 * q);
        nff += val == 0xFFu;
      }
    }
    const int incl = jpeg_scan256(nff, sh);
    long long pos = (long long)j0 + ffs + incl - nff;
    for (int q = 0; q < n; ++q) {
      const uint8_t b = (uint8_t)(pk >> (8 * q));
      o[pos++] = b;
      if (b == 0xFF) o[pos++] = 0;
    }
    ffs += sh[255];
  }
  if (tid == 0) {
    int L = nbytes + ffs;                           // <= 2 * 208 * bpi; istride holds two more
    if (row < rows - 1) {
      o[L] = 0xFF;
      o[L + 1] = (uint8_t)(0xD0 + (row & 7));
      L += 2;
    }
    ilen[iv] = L;
  }
}

// (d) one workgroup per interval: where it lands is the sum of the lengths before it in its frame
__global__ __launch_bounds__(256) void jpeg_assemble_kernel(const uint8_t* __restrict__ stuffed, long long istride,
                                                            const int* __restrict__ ilen, uint8_t* __restrict__ out, long long out_stride,
                                                            int* __restrict__ sizes, int rows, int cols, int H, int W, int quality) {
  __shared__ long long sh[256];
  const int tid = threadIdx.x;
  const long long iv = blockIdx.x, t = iv / rows;
  const int row = (int)(iv - t * rows);
  long long part = 0;
  for (int r = tid; r < row; r += 256) part += ilen[t * rows + r];
  sh[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  const long long off = sh[0];
  const int L = ilen[iv];
  uint8_t* frame = out + t * out_stride;
  uint8_t* dst = frame + JPEG_HEADER + off;
  const uint8_t* src = stuffed + iv * istride;
  for (int i = tid; i < L; i += 256) dst[i] = src[i];
  if (row == 0)
    for (int i = tid; i < JPEG_HEADER; i += 256) frame[i] = jpeg_header_byte(i, H, W, cols, quality);
  if (row == rows - 1 && tid == 0) {
    dst[L] = 0xFF;
    dst[L + 1] = 0xD9;
    sizes[t] = (int)(JPEG_HEADER + off + L + 2);
  }
}

struct JpegPlan {
  int rows, cols, bpi;
  long long mcus, nblk, intervals, istride, out_stride;
  long long o_coef, o_bits, o_nbits, o_boff, o_stuffed, o_ilen, scratch;
};

inline long long up(long long v, long long a) { return (v + a - 1) / a * a; }

int jpeg_plan(const char* fn, int T, int H, int W, JpegPlan* p) {
  LL_REQUIRE(T >= 1 && H >= 1 && W >= 1, "%s: empty input %d x %d x %d", fn, T, H, W);
  LL_REQUIRE(H <= 65535 && W <= 65535, "%s: H=%d, W=%d: a JPEG frame holds at most 65535 rows and columns", fn, H, W);
  p->rows = (H + 15) / 16, p->cols = (W + 15) / 16, p->bpi = 6 * p->cols;
  const long long per = (long long)p->rows * p->cols;
  p->mcus = per * T, p->nblk = 6 * p->mcus, p->intervals = (long long)T * p->rows;
  p->istride = up((long long)p->bpi * JPEG_BLOCK_BYTES + 2, 16);
  p->out_stride = up(JPEG_HEADER + per * 6 * JPEG_BLOCK_BYTES + 2 * (long long)(p->rows - 1) + 2, 16);
  LL_REQUIRE(p->out_stride <= 0x7fffffffll && p->nblk <= 0x7fffffffll,
             "%s: %d x %d x %d is more than one call covers (a frame's worst case must stay under 2 GiB, the call under 2^31 blocks)", fn, T, H, W);
  long long o = 0;
  p->o_coef = o, o += up(p->nblk * 128, 256);
  p->o_bits = o, o += up(p->nblk * JPEG_SLOT_WORDS * 4, 256);
  p->o_nbits = o, o += up(p->nblk * 4, 256);
  p->o_boff = o, o += up(p->nblk * 4, 256);
  p->o_stuffed = o, o += up(p->intervals * p->istride, 256);
  p->o_ilen = o, o += up(p->intervals * 4, 256);
  p->scratch = o;
  return LL_OK;
}

void jpeg_launch_coef(const uint8_t* frames, long long stride_t, int H, int W, int quality, int16_t* coef, const JpegPlan& p, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_coef_kernel, dim3((unsigned)((p.mcus + 3) / 4)), dim3(256), 0, s, frames, stride_t, H, W, p.rows, p.cols, quality,
                     coef, p.mcus);
}

}  // namespace

extern "C" int ll_jpeg_sizes(int T, int H, int W, long long* out_stride, long long* scratch_bytes) {
  LL_REQUIRE(out_stride != nullptr && scratch_bytes != nullptr, "ll_jpeg_sizes: null operand");
  JpegPlan p;
  if (int rc = jpeg_plan("ll_jpeg_sizes", T, H, W, &p)) return rc;
  *out_stride = p.out_stride;
  *scratch_bytes = p.scratch;
  return LL_OK;
}

extern "C" int ll_jpeg_coefficients_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, int quality, int16_t* coef,
                                       ll_stream stream) {
  LL_REQUIRE(frames != nullptr && coef != nullptr, "ll_jpeg_coefficients_u8: null operand");
  LL_REQUIRE(quality >= 1 && quality <= 100, "ll_jpeg_coefficients_u8: quality=%d must be 1..100", quality);
  JpegPlan p;
  if (int rc = jpeg_plan("ll_jpeg_coefficients_u8", T, H, W, &p)) return rc;
  LL_REQUIRE(stride_t >= 3ll * H * W, "ll_jpeg_coefficients_u8: stride_t=%lld bytes must span a %d x %d x 3 frame", stride_t, H, W);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(coef) & 1) == 0, "ll_jpeg_coefficients_u8: coef must be 2-byte aligned");
  jpeg_launch_coef(frames, stride_t, H, W, quality, coef, p, (hipStream_t)stream);
  return ll_check_launch("ll_jpeg_coefficients_u8");
}

extern "C" int ll_jpeg_encode_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, int quality, uint8_t* out,
                                 long long out_stride, int32_t* sizes, void* scratch, long long scratch_bytes, ll_stream stream) {
  LL_REQUIRE(frames != nullptr && out != nullptr && sizes != nullptr && scratch != nullptr, "ll_jpeg_encode_u8: null operand");
  LL_REQUIRE(quality >= 1 && quality <= 100, "ll_jpeg_encode_u8: quality=%d must be 1..100", quality);
  JpegPlan p;
  if (int rc = jpeg_plan("ll_jpeg_encode_u8", T, H, W, &p)) return rc;
  LL_REQUIRE(stride_t >= 3ll * H * W, "ll_jpeg_encode_u8: stride_t=%lld bytes must span a %d x %d x 3 frame", stride_t, H, W);
  LL_REQUIRE(out_stride >= p.out_stride, "ll_jpeg_encode_u8: out_stride=%lld is under the worst case %lld of a %d x %d frame (ll_jpeg_sizes)",
             out_stride, p.out_stride, H, W);
  LL_REQUIRE(scratch_bytes >= p.scratch, "ll_jpeg_encode_u8: scratch_bytes=%lld, %d x %d x %d needs %lld (ll_jpeg_sizes)", scratch_bytes, T,
             H, W, p.scratch);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "ll_jpeg_encode_u8: scratch must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* base = static_cast<uint8_t*>(scratch);
  int16_t* coef = reinterpret_cast<int16_t*>(base + p.o_coef);
  uint32_t* bits = reinterpret_cast<uint32_t*>(base + p.o_bits);
  int* nbits = reinterpret_cast<int*>(base + p.o_nbits);
  int* boff = reinterpret_cast<int*>(base + p.o_boff);
  uint8_t* stuffed = base + p.o_stuffed;
  int* ilen = reinterpret_cast<int*>(base + p.o_ilen);
  jpeg_launch_coef(frames, stride_t, H, W, quality, coef, p, s);
  hipLaunchKernelGGL(jpeg_block_bits_kernel, dim3((unsigned)((p.nblk + 255) / 256)), dim3(256), 0, s, (const int16_t*)coef, p.nblk, p.bpi,
                     bits, nbits);
  hipLaunchKernelGGL(jpeg_interval_kernel, dim3((unsigned)p.intervals), dim3(256), 0, s, (const uint32_t*)bits, (const int*)nbits, boff,
                     stuffed, p.istride, ilen, p.bpi, p.rows);
  hipLaunchKernelGGL(jpeg_assemble_kernel, dim3((unsigned)p.intervals), dim3(256), 0, s, (const uint8_t*)stuffed, p.istride,
                     (const int*)ilen, out, out_stride, sizes, p.rows, p.cols, H, W, quality);
  return ll_check_launch("ll_jpeg_encode_u8");
}
