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
// ll_jpeg_decode_u8_split replaces (a) by the split route: the subsequences of a segment (split table of the host) are scanned side
// by side from a guessed state, rescanned from their predecessor's exit until no exit changes, then emitted; the serial routine takes
// whatever segment is not cut, not settled or flagged, so coef and status are (a)'s bit for bit.  Its kernels and the argument why a
// round without change settles a segment stand further down, before jpeg_split_scan_kernel.
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

// ---- the split route through the entropy stage: subsequences of a segment decode side by side (jpeg_dec.h) -------------------------
// The work buffer: per subsequence the exit states of the last two rounds (ping-pong: lane i reads its predecessor's exit of the
// round before while the predecessor writes this round's), the entry its last scan started from, its block count and the exclusive
// scan of the counts; per segment the last round in which an exit changed, a flag (0, -1 unsettled, -2 flagged), the first and last
// row of its run in the split table and the number of such runs.
struct SplitWork {
  JdState* exit[2];
  JdState* entry;
  int32_t *count, *base, *chg, *flag, *first, *last, *runs;
};

inline long long split_up4(long long n) { return (n + 3) / 4 * 4; }
inline long long split_work_bytes(int nseg, int nsub) { return 32 * split_up4(nsub) + 20 * split_up4(nseg); }

SplitWork split_work(void* work, int nseg, int nsub) {
  char* b = static_cast<char*>(work);
  const long long ns = split_up4(nsub), ng = split_up4(nseg);
  SplitWork w;
  w.exit[0] = reinterpret_cast<JdState*>(b), w.exit[1] = reinterpret_cast<JdState*>(b + 8 * ns);
  w.entry = reinterpret_cast<JdState*>(b + 16 * ns);
  w.count = reinterpret_cast<int32_t*>(b + 24 * ns), w.base = reinterpret_cast<int32_t*>(b + 28 * ns);
  int32_t* g = reinterpret_cast<int32_t*>(b + 32 * ns);
  w.chg = g, w.flag = g + ng, w.first = g + 2 * ng, w.last = g + 3 * ng, w.runs = g + 4 * ng;
  return w;
}

__global__ __launch_bounds__(256) void jpeg_split_setup_kernel(SplitWork w, int nseg) {
  const int seg = blockIdx.x * 256 + threadIdx.x;
  if (seg >= nseg) return;
  w.chg[seg] = 0, w.flag[seg] = 0, w.first[seg] = -1, w.last[seg] = -1, w.runs[seg] = 0;
}

// the frame's tables into the slice, by n lanes: jd_stage_tables word for word
__device__ __forceinline__ void split_stage_tables(const uint32_t* __restrict__ packed, uint32_t* slice, int tid, int n) {
  for (int wd = tid; wd < JD_SLICE / 4; wd += n) {
    int src;
    if (wd < 16) src = (wd >> 2) * (JD_HUFF_TABLE / 4) + (wd & 3);
    else if (wd < 24) src = ((wd - 16) >> 2) * (JD_HUFF_TABLE / 4) + 4 + ((wd - 16) & 3);
    else src = (2 + ((wd - 24) >> 6)) * (JD_HUFF_TABLE / 4) + 4 + ((wd - 24) & 63);
    slice[wd] = packed[src];
  }
}

// The tables of the lanes that have work: the lowest frame among them is staged into LDS, a lane of another frame (a workgroup that
// straddles two frames) reads the packed tables in global memory.
template <int LPW>
__device__ __forceinline__ JdTabs split_tables(bool need, int t, const uint8_t* __restrict__ huff, uint32_t* slice, int* t0) {
  if (threadIdx.x == 0) *t0 = 0x7fffffff;
  __syncthreads();
  if (need) atomicMin(t0, t);
  __syncthreads();
  const int ts = *t0;
  if (ts != 0x7fffffff) split_stage_tables(reinterpret_cast<const uint32_t*>(huff + (long long)ts * JD_HUFF_FRAME), slice, threadIdx.x, LPW);
  __syncthreads();
  return need && t != ts ? jd_tabs_packed(huff + (long long)t * JD_HUFF_FRAME) : jd_tabs_slice(reinterpret_cast<const uint8_t*>(slice));
}

// Pass 0 (round 0) and the rounds 1..R, one launch each, one lane per subsequence, LPW lanes per wave (and workgroup).
//   round 0: the lane checks its row of the split table -- inside its segment's bytes, at least JD_SUB_MIN_BYTES long, following its
//            predecessor without a gap, the first of a run at offset 0 and the last at the segment's end, runs in rising segment order --
//            and a bad row flags its segment for the serial routine.  Then it scans from the guess (its first byte, block 0, DC); for the
//            first subsequence of a segment that guess is the true state.
//   round r: subsequence i rescans from the exit that i - 1 held after round r - 1; where that is the entry of its last scan it only
//            carries its exit over.  A changed exit writes r into the segment's `chg`.
// Why a round without change settles a segment: an exit is a pure function of (bytes, entry), and subsequence 0's entry is true.  So
// after round r the exits of subsequences 0..r are true (induction: exit i of round r comes from the true exit i - 1 of round r - 1).
// If no exit of the segment changed in round r, every subsequence was given in round r the same entry as in round r - 1, namely its
// predecessor's exit of round r - 1 = of round r - 2; by induction over i from the true first entry, every entry and every exit is
// then the true one, and they stay so in every later round.  chg therefore ends as the last round with a change, and the segment
// settled in round chg + 1 when that is at most R.
template <int LPW>
__global__ __launch_bounds__(64) void jpeg_split_scan_kernel(const uint8_t* __restrict__ data, long long nbytes,
                                                             const int32_t* __restrict__ segs, int nseg, const int32_t* __restrict__ subs,
                                                             int nsub, const uint8_t* __restrict__ huff, const uint8_t* __restrict__ sel,
                                                             int T, long long per, int bpm, SplitWork w, int round) {
  __shared__ uint32_t slice[JD_SLICE / 4];
  __shared__ int t0;
  const int i = blockIdx.x * LPW + threadIdx.x;
  bool need = false;
  int seg = -1, t = 0, off = 0, len = 0;
  const int32_t* row = nullptr;
  JdState in{0, 0};
  const int rd = (round + 1) & 1, wr = round & 1;
  if (i < nsub) seg = subs[3ll * i];
  if (i < nsub && seg >= 0 && seg < nseg) {
    row = segs + (long long)seg * JD_SEG_FIELDS;
    const bool head = i == 0 || subs[3ll * (i - 1)] != seg;
    if (!jd_row_ok(row, nbytes, T, per)) {
      if (round == 0) w.flag[seg] = -2;
    } else {
      t = row[2], off = subs[3ll * i + 1], len = subs[3ll * i + 2];
      const long long seglen = row[1];
      const bool inside = off >= 0 && len >= JD_SUB_MIN_BYTES && (long long)off + len <= seglen;
      if (round == 0) {
        bool ok = inside;
        if (head) {
          ok = ok && off == 0 && (i == 0 || (subs[3ll * (i - 1)] >= 0 && subs[3ll * (i - 1)] < seg));
          w.first[seg] = i;
          atomicAdd(&w.runs[seg], 1);
        } else {
          ok = ok && (long long)subs[3ll * (i - 1) + 1] + subs[3ll * (i - 1) + 2] == off;
        }
        if (i + 1 >= nsub || subs[3ll * (i + 1)] != seg) {
          ok = ok && (long long)off + len == seglen;
          w.last[seg] = i;
        }
        if (!ok) w.flag[seg] = -2;
        in = JdState{off, 0};
        need = inside;
      } else if (inside && w.flag[seg] == 0) {
        if (!head) in = w.exit[rd][i - 1];
        if (head || jd_state_eq(in, w.entry[i])) w.exit[wr][i] = w.exit[rd][i];
        else need = true;
      }
    }
  }
  const JdTabs tb = split_tables<LPW>(need, t, huff, slice, &t0);
  if (!need) return;
  int32_t begun = 0;
  const JdState out = jd_sub_scan(data + row[0], row[1], tb, *reinterpret_cast<const uint32_t*>(sel + 4ll * t), bpm, off + len, in, &begun);
  if (round > 0 && !jd_state_eq(out, w.exit[rd][i])) w.chg[seg] = round;
  w.entry[i] = in, w.exit[wr][i] = out, w.count[i] = begun;
}

// Block scan: one workgroup per segment.  unsettled after R rounds -> flag -1; rows in more than one run, a dirty final scan or a
// total that is not mcus * bpm -> flag -2; else base[i] = the blocks that begin before subsequence i.
__global__ __launch_bounds__(256) void jpeg_split_blocks_kernel(const int32_t* __restrict__ segs, int nseg, int bpm, int rounds,
                                                                SplitWork w) {
  __shared__ long long sums[256];
  __shared__ int dirt;
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int runs = w.runs[seg];
  if (runs == 0 || w.flag[seg] != 0) return;
  const int f = w.first[seg], l = w.last[seg];
  if (runs != 1 || f < 0 || l < f) {
    if (tid == 0) w.flag[seg] = -2;
    return;
  }
  if (w.chg[seg] >= rounds) {
    if (tid == 0) w.flag[seg] = -1;
    return;
  }
  if (tid == 0) dirt = 0;
  const int n = l - f + 1, chunk = (n + 255) / 256;
  const int lo = f + (int)min((long long)tid * chunk, (long long)n), hi = f + (int)min((long long)(tid + 1) * chunk, (long long)n);
  long long s = 0;
  int d = 0;
  for (int j = lo; j < hi; ++j) {
    const int32_t c = w.count[j];
    s += c & (JD_SUB_DIRTY - 1);
    d |= c & JD_SUB_DIRTY;
  }
  sums[tid] = s;
  __syncthreads();
  if (d) dirt = 1;
  for (int st = 1; st < 256; st <<= 1) {
    const long long v = tid >= st ? sums[tid - st] : 0;
    __syncthreads();
    sums[tid] += v;
    __syncthreads();
  }
  long long run = sums[tid] - s;
  for (int j = lo; j < hi; ++j) {
    w.base[j] = (int32_t)min(run, 0x7fffffffll);
    run += w.count[j] & (JD_SUB_DIRTY - 1);
  }
  const int32_t* row = segs + (long long)seg * JD_SEG_FIELDS;
  if (tid == 0 && (dirt || sums[255] != (long long)row[4] * bpm)) w.flag[seg] = -2;
}

// Emit: one lane per subsequence of a settled, unflagged segment, from the entry its last scan started from.
template <int LPW>
__global__ __launch_bounds__(64) void jpeg_split_emit_kernel(const uint8_t* __restrict__ data, long long nbytes,
                                                             const int32_t* __restrict__ segs, int nseg, const int32_t* __restrict__ subs,
                                                             int nsub, const uint8_t* __restrict__ huff, const uint8_t* __restrict__ sel,
                                                             int T, long long per, int bpm, int16_t* __restrict__ coef, SplitWork w) {
  __shared__ uint32_t slice[JD_SLICE / 4];
  __shared__ __attribute__((aligned(16))) int16_t stage[LPW][64];
  __shared__ int t0;
  const int i = blockIdx.x * LPW + threadIdx.x;
  bool need = false;
  int seg = -1, t = 0, count = 0;
  const int32_t* row = nullptr;
  if (i < nsub) seg = subs[3ll * i];
  if (i < nsub && seg >= 0 && seg < nseg && w.runs[seg] == 1 && w.flag[seg] == 0) {
    row = segs + (long long)seg * JD_SEG_FIELDS;
    t = row[2];
    count = w.count[i] & (JD_SUB_DIRTY - 1);
    need = count > 0;
  }
  const JdTabs tb = split_tables<LPW>(need, t, huff, slice, &t0);
  if (!need) return;
  const int rc = jd_sub_emit(data + row[0], row[1], tb, *reinterpret_cast<const uint32_t*>(sel + 4ll * t), bpm, w.entry[i], count, w.base[i],
                             (long long)row[4] * bpm, stage[threadIdx.x], coef + ((long long)t * per + row[3]) * bpm * 64);
  if (rc) w.flag[seg] = -2;
}

// DC: one workgroup per settled, unflagged segment: the running sum of the DC differences per component in scan order (exact, in 64
// bits; a value outside int16 flags the segment, as jpeg_decode_segment's JD_DC_RANGE does).  A lane owns a run of whole MCUs.
__global__ __launch_bounds__(256) void jpeg_split_dc_kernel(const int32_t* __restrict__ segs, int nseg, long long per, int bpm,
                                                            int16_t* __restrict__ coef, SplitWork w) {
  __shared__ long long sums[3][256];
  const int seg = blockIdx.x, tid = threadIdx.x;
  if (w.runs[seg] != 1 || w.flag[seg] != 0) return;
  const int32_t* row = segs + (long long)seg * JD_SEG_FIELDS;
  const int mcus = row[4], ny = bpm == 1 ? 1 : bpm - 2;
  int16_t* blocks = coef + ((long long)row[2] * per + row[3]) * bpm * 64;
  const int chunk = (mcus + 255) / 256;
  const int lo = (int)min((long long)tid * chunk, (long long)mcus), hi = (int)min((long long)(tid + 1) * chunk, (long long)mcus);
  long long p[3] = {0, 0, 0};
  for (int m = lo; m < hi; ++m)
    for (int b = 0; b < bpm; ++b) p[b < ny ? 0 : b - ny + 1] += blocks[((long long)m * bpm + b) * 64];
  for (int c = 0; c < 3; ++c) sums[c][tid] = p[c];
  __syncthreads();
  for (int st = 1; st < 256; st <<= 1) {
    long long v[3] = {0, 0, 0};
    if (tid >= st)
      for (int c = 0; c < 3; ++c) v[c] = sums[c][tid - st];
    __syncthreads();
    for (int c = 0; c < 3; ++c) sums[c][tid] += v[c];
    __syncthreads();
  }
  bool bad = false;
  for (int c = 0; c < 3; ++c) p[c] = sums[c][tid] - p[c];
  for (int m = lo; m < hi; ++m)
    for (int b = 0; b < bpm; ++b) {
      const int c = b < ny ? 0 : b - ny + 1;
      int16_t* dc = blocks + ((long long)m * bpm + b) * 64;
      p[c] += *dc;
      bad = bad || p[c] < -32768 || p[c] > 32767;
      *dc = (int16_t)p[c];
    }
  if (bad) w.flag[seg] = -2;
}

// Fallback: jpeg_huff_decode_kernel's body over the segments the split table leaves out (info 0), the unsettled (-1) and the flagged
// (-2); it rewrites every block of those and their status, so the result is the serial route's for malformed data too.  A settled,
// unflagged segment gets status 0 and the round it settled in.
__global__ __launch_bounds__(64) void jpeg_split_fallback_kernel(const uint8_t* __restrict__ data, long long nbytes,
                                                                 const int32_t* __restrict__ segs, const uint8_t* __restrict__ huff,
                                                                 const uint8_t* __restrict__ sel, int T, long long per, int bpm,
                                                                 int16_t* __restrict__ coef, int32_t* __restrict__ status,
                                                                 int32_t* __restrict__ info, SplitWork w) {
  __shared__ uint32_t slice[JD_SLICE / 4];
  __shared__ __attribute__((aligned(16))) int16_t stage[64];
  const int seg = blockIdx.x;
  const int runs = w.runs[seg], flag = w.flag[seg];
  if (runs != 0 && flag == 0) {
    info[seg] = w.chg[seg] + 1;
    status[seg] = JD_OK;
    return;
  }
  info[seg] = runs == 0 && flag == 0 ? 0 : (flag == -1 ? -1 : -2);
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

// lanes per wave of the subsequence kernels (tuning key jpeg_split_lanes: 1, 64, or 0 = the shipped rule).  Measured on 81 frames of
// 480 x 832 (profiles/clip_intake.md): 64 lanes win where subsequences are short and many (128 bytes: 96 against 144 us per frame, 256:
// 124 against 132), one lane per wave where they are long (512: 133 against 179, 1024: 166 against 333), because 64 diverging bit
// streams in lock step cost more the longer each runs.  Shipped: 64 up to a mean of 384 bytes per subsequence, 1 above.
int g_split_lanes = 0;

int dec_check_split(const char* fn, const int32_t* subs, int nsub, int rounds, const int32_t* info, const void* work, long long work_bytes,
                    int nseg) {
  LL_REQUIRE(subs != nullptr && info != nullptr && work != nullptr, "%s: null operand", fn);
  LL_REQUIRE(nsub >= 1, "%s: nsub=%d: at least one subsequence (the serial entry point takes a clip without any)", fn, nsub);
  LL_REQUIRE(rounds >= 1 && rounds <= 64, "%s: rounds=%d must be 1..64", fn, rounds);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(subs) & 3) == 0 && (reinterpret_cast<uintptr_t>(info) & 3) == 0,
             "%s: subs and info must be 4-byte aligned", fn);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(work) & 15) == 0, "%s: work must be 16-byte aligned", fn);
  LL_REQUIRE(work_bytes >= split_work_bytes(nseg, nsub), "%s: work_bytes=%lld, %d segments in %d subsequences need %lld "
             "(ll_jpeg_decode_split_sizes)", fn, work_bytes, nseg, nsub, split_work_bytes(nseg, nsub));
  return LL_OK;
}

template <int LPW>
void dec_launch_split_lanes(const DecPlan& p, const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const int32_t* subs,
                            int nsub, int rounds, const uint8_t* huff, const uint8_t* sel, int16_t* coef, const SplitWork& w,
                            hipStream_t s) {
  const dim3 grid((unsigned)((nsub + LPW - 1) / LPW)), block(LPW);
  for (int r = 0; r <= rounds; ++r)
    hipLaunchKernelGGL(jpeg_split_scan_kernel<LPW>, grid, block, 0, s, data, nbytes, segs, nseg, subs, nsub, huff, sel, p.T, p.per, p.bpm, w, r);
  hipLaunchKernelGGL(jpeg_split_blocks_kernel, dim3((unsigned)nseg), dim3(256), 0, s, segs, nseg, p.bpm, rounds, w);
  hipLaunchKernelGGL(jpeg_split_emit_kernel<LPW>, grid, block, 0, s, data, nbytes, segs, nseg, subs, nsub, huff, sel, p.T, p.per, p.bpm, coef,
                     w);
}

// setup, pass 0, `rounds` rounds, block scan, emit, DC, fallback: rounds + 6 launches, stream-ordered, nothing allocated or awaited
void dec_launch_entropy_split(const DecPlan& p, const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const int32_t* subs,
                              int nsub, int rounds, const uint8_t* huff, const uint8_t* sel, int16_t* coef, int32_t* status, int32_t* info,
                              void* work, hipStream_t s) {
  const SplitWork w = split_work(work, nseg, nsub);
  hipLaunchKernelGGL(jpeg_split_setup_kernel, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, s, w, nseg);
  const int lanes = g_split_lanes ? g_split_lanes : (nbytes / nsub <= 384 ? 64 : 1);
  if (lanes == 1) dec_launch_split_lanes<1>(p, data, nbytes, segs, nseg, subs, nsub, rounds, huff, sel, coef, w, s);
  else dec_launch_split_lanes<64>(p, data, nbytes, segs, nseg, subs, nsub, rounds, huff, sel, coef, w, s);
  hipLaunchKernelGGL(jpeg_split_dc_kernel, dim3((unsigned)nseg), dim3(256), 0, s, segs, nseg, p.per, p.bpm, coef, w);
  hipLaunchKernelGGL(jpeg_split_fallback_kernel, dim3((unsigned)nseg), dim3(1), 0, s, data, nbytes, segs, huff, sel, p.T, p.per, p.bpm, coef,
                     status, info, w);
}

}  // namespace

int ll_set_jpeg_split_lanes_internal(int v) {
  if (v != 0 && v != 1 && v != 64) return -1;
  g_split_lanes = v;
  return 0;
}

extern "C" int ll_jpeg_decode_split_sizes(int nseg, int nsub, long long* work_bytes) {
  LL_REQUIRE(work_bytes != nullptr, "ll_jpeg_decode_split_sizes: null operand");
  LL_REQUIRE(nseg >= 1 && nsub >= 1, "ll_jpeg_decode_split_sizes: nseg=%d, nsub=%d: at least one of each", nseg, nsub);
  *work_bytes = split_work_bytes(nseg, nsub);
  return LL_OK;
}

extern "C" int ll_jpeg_decode_coefficients_split(const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff,
                                                 const uint8_t* sel, int T, int H, int W, int ncomp, int hs, int vs, int16_t* coef,
                                                 int32_t* status, const int32_t* subs, int nsub, int rounds, int32_t* info, void* work,
                                                 long long work_bytes, ll_stream stream) {
  const char* fn = "ll_jpeg_decode_coefficients_split";
  if (int rc = dec_check_entropy(fn, data, nbytes, segs, nseg, huff, sel, coef, status)) return rc;
  if (int rc = dec_check_split(fn, subs, nsub, rounds, info, work, work_bytes, nseg)) return rc;
  DecPlan p;
  if (int rc = dec_plan(fn, T, H, W, ncomp, hs, vs, &p)) return rc;
  dec_launch_entropy_split(p, data, nbytes, segs, nseg, subs, nsub, rounds, huff, sel, coef, status, info, work, (hipStream_t)stream);
  return ll_check_launch(fn);
}

extern "C" int ll_jpeg_decode_u8_split(const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff,
                                       const uint8_t* sel, const uint16_t* qt, int T, int H, int W, int ncomp, int hs, int vs, int16_t* coef,
                                       int32_t* status, uint8_t* out, long long stride_t, void* scratch, long long scratch_bytes,
                                       const int32_t* subs, int nsub, int rounds, int32_t* info, void* work, long long work_bytes,
                                       ll_stream stream) {
  const char* fn = "ll_jpeg_decode_u8_split";
  if (int rc = dec_check_entropy(fn, data, nbytes, segs, nseg, huff, sel, coef, status)) return rc;
  if (int rc = dec_check_split(fn, subs, nsub, rounds, info, work, work_bytes, nseg)) return rc;
  DecPlan p;
  if (int rc = dec_plan(fn, T, H, W, ncomp, hs, vs, &p)) return rc;
  if (int rc = dec_check_pixels(fn, p, coef, qt, out, stride_t, scratch, scratch_bytes)) return rc;
  dec_launch_entropy_split(p, data, nbytes, segs, nseg, subs, nsub, rounds, huff, sel, coef, status, info, work, (hipStream_t)stream);
  dec_launch_pixels(p, coef, qt, out, stride_t, scratch, (hipStream_t)stream);
  return ll_check_launch(fn);
}

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
