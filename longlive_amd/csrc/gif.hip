// Animated previews: a GIF encoder for uint8 RGB frames [T, H, W, 3] -- palette quantiser and LZW coder -- every stage on the GPU and
// stream-ordered.  csrc/gif.h's head comment defines every decision (histogram bins, median cut, nearest-entry table, ordered dither,
// LZW in chunks of GIF_CHUNK pixels each coded from a cleared dictionary); tests/gif_ref.py restates all of it.
//
// Launches of ll_gif_encode_u8 (the histogram is the one buffer accumulated in place; a memset on the stream clears it first):
//   (a) gif_hist_kernel    a thread per run of 8 pixels: equal neighbouring bins are summed in registers, then 64-bit integer atomics
//   (b) gif_cut_kernel     one workgroup per palette: the occupied bins compacted, then up to 255 splits, each two passes over them
//                          (counts per coordinate of the three axes; the move into the new box) -> palette, used entries.  A palette
//                          of fewer than 256 occupied bins is then made again over the bins' 6-bit cells (csrc/gif.h, "few colours"):
//                          gif_fine_hist_kernel, the same kernel over the cells, gif_fine_table_kernel; the others leave at once
//   (c) gif_table_kernel   a thread per bin: the nearest used entry of its centre
//   (d) gif_index_kernel   a thread per pixel -> [T, H, W] indices
//   (e) gif_lzw_kernel     one wave per chunk: the chunk and the dictionary in LDS, lane 0 runs csrc/gif.h's serial coder (each code
//                          depends on the one before it), all lanes clear, load and store -> the chunk's bits in a slot + their count
//   (f) gif_scan_kernel    one workgroup per frame: where each chunk's bits begin, the stream's bytes, sizes[t]
//       gif_pack_kernel    one workgroup per chunk: the stream's bytes whose first bit the chunk holds, shifted into place and laid into
//                          sub-blocks; the first writes the file's head, the last its terminator and trailer
// ll_gif_quantize_u8 is (a) - (d), ll_gif_lzw_u8 is (e) and (f) over T index rows without the file's framing.
#include "common.h"
#include "gif.h"
#include "../../include/longlive_gif.h"

namespace {

typedef unsigned long long u64;

constexpr int GIF_RUN = 8;                           // pixels per thread of the histogram kernel
constexpr int GIF_HIST = 4 * GIF_BINS;               // 64-bit words per histogram: counts, then the sums of r, g, b

// (a)
__global__ __launch_bounds__(256) void gif_hist_kernel(const uint8_t* __restrict__ px, long long st, long long n, long long runs_per_frame,
                                                       long long runs, int per_frame, u64* __restrict__ hist) {
  const long long step = (long long)gridDim.x * 256;
  for (long long run = (long long)blockIdx.x * 256 + threadIdx.x; run < runs; run += step) {
    const long long t = run / runs_per_frame, p0 = (run - t * runs_per_frame) * GIF_RUN, p1 = p0 + GIF_RUN < n ? p0 + GIF_RUN : n;
    const uint8_t* f = px + t * st + 3 * p0;
    u64* h = hist + (per_frame ? t : 0) * GIF_HIST;
    int cur = -1;
    unsigned c = 0, sr = 0, sg = 0, sb = 0;
    for (long long p = p0; p < p1; ++p, f += 3) {
      const int r = f[0], g = f[1], b = f[2], bin = gif_bin(r, g, b);
      if (bin != cur) {
        if (cur >= 0) atomicAdd(&h[cur], (u64)c), atomicAdd(&h[GIF_BINS + cur], (u64)sr), atomicAdd(&h[2 * GIF_BINS + cur], (u64)sg), atomicAdd(&h[3 * GIF_BINS + cur], (u64)sb);
        cur = bin, c = sr = sg = sb = 0;
      }
      ++c, sr += r, sg += g, sb += b;
    }
    if (cur >= 0) atomicAdd(&h[cur], (u64)c), atomicAdd(&h[GIF_BINS + cur], (u64)sr), atomicAdd(&h[2 * GIF_BINS + cur], (u64)sg), atomicAdd(&h[3 * GIF_BINS + cur], (u64)sb);
  }
}

struct CutShared {
  u64 held[GIF_COLORS], sum[GIF_COLORS][3], marg[3][64], best[256];
  int items[GIF_COLORS], best_at[256], scan[256];
  int axis, cut;
  uint8_t box[GIF_BINS];                             // the box of item i of the compacted list
};

// (a') the few-colour palettes' second histogram: a thread per pixel, into the eight cells of the pixel's bin's slot
__global__ __launch_bounds__(256) void gif_fine_hist_kernel(const uint8_t* __restrict__ px, long long st, long long n, long long total,
                                                            int per_frame, const uint16_t* __restrict__ occ, const int* __restrict__ mode,
                                                            u64* __restrict__ fhist) {
  const long long step = (long long)gridDim.x * 256;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += step) {
    const long long t = p / n, q = p - t * n, pi = per_frame ? t : 0;
    if (mode[2 * pi] == 0) continue;
    const uint8_t* f = px + t * st + 3 * q;
    const int r = f[0], g = f[1], b = f[2];
    const int cell = 8 * gif_slot(occ + pi * GIF_BINS, mode[2 * pi + 1], gif_bin(r, g, b)) + gif_sub(r, g, b);
    u64* h = fhist + pi * 4 * GIF_FINE_CELLS;
    atomicAdd(&h[cell], (u64)1), atomicAdd(&h[GIF_FINE_CELLS + cell], (u64)r), atomicAdd(&h[2 * GIF_FINE_CELLS + cell], (u64)g),
        atomicAdd(&h[3 * GIF_FINE_CELLS + cell], (u64)b);
  }
}

// (b) one workgroup per palette: the parallel form of csrc/gif.h's gif_median_cut.  FINE = false: the items are the occupied bins of
// the histogram; the list, its length and whether it is short of 256 (mode[2 p], mode[2 p + 1]) are left for the few-colour stage.
// FINE = true: a palette whose mode is set is made again over the occupied cells of its second histogram; the others are left.
// occ and bins are the same list when FINE is false (bins is then not read), so neither is __restrict__.
template <bool FINE>
__global__ __launch_bounds__(256) void gif_cut_kernel(const u64* __restrict__ hist, uint16_t* occ, const uint16_t* bins,
                                                      int* __restrict__ mode, uint8_t* __restrict__ pal, int* __restrict__ used) {
  __shared__ CutShared S;
  constexpr int NSRC = FINE ? GIF_FINE_CELLS : GIF_BINS, PER = NSRC / 256;
  const int tid = threadIdx.x;
  if (FINE && mode[2 * blockIdx.x] == 0) return;     // the same word for every thread
  const u64* cnt = hist + (long long)blockIdx.x * 4 * NSRC;
  uint16_t* list = occ + (long long)blockIdx.x * NSRC;
  const uint16_t* slots = bins + (long long)blockIdx.x * GIF_BINS;
  auto coord = [&](int src, int axis) { return FINE ? gif_cell_coord(slots[src >> 3], src & 7, axis) : gif_coord(src, axis); };

  int mine = 0;
  u64 part = 0;
  for (int i = tid * PER; i < (tid + 1) * PER; ++i) mine += cnt[i] != 0, part += cnt[i];
  S.scan[tid] = mine;
  S.held[tid] = 0, S.items[tid] = 0, S.sum[tid][0] = S.sum[tid][1] = S.sum[tid][2] = 0;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int a = tid >= o ? S.scan[tid - o] : 0;
    __syncthreads();
    S.scan[tid] += a;
    __syncthreads();
  }
  const int n_occ = S.scan[255];
  {
    int at = S.scan[tid] - mine;
    for (int i = tid * PER; i < (tid + 1) * PER; ++i)
      if (cnt[i] != 0) list[at] = (uint16_t)i, S.box[at++] = 0;
  }
  atomicAdd(&S.held[0], part);
  if (tid == 0) {
    S.items[0] = n_occ;
    if (!FINE) mode[2 * blockIdx.x] = n_occ < GIF_COLORS, mode[2 * blockIdx.x + 1] = n_occ;
  }
  __syncthreads();

  int boxes = 1;
  for (int split = 1; split < GIF_COLORS; ++split) {
    S.best[tid] = (tid < boxes && S.items[tid] > 1) ? S.held[tid] : 0;     // a box of two items holds two pixels or more: 0 is "none"
    S.best_at[tid] = tid;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) {
        const u64 v = S.best[tid + o];
        const int at = S.best_at[tid + o];
        if (v > S.best[tid] || (v == S.best[tid] && at < S.best_at[tid])) S.best[tid] = v, S.best_at[tid] = at;
      }
      __syncthreads();
    }
    if (S.best[0] == 0) break;                       // the same word for every thread: the loop is left together
    const int pick = S.best_at[0];
    if (tid < 192) S.marg[tid >> 6][tid & 63] = 0;
    __syncthreads();
    for (int i = tid; i < n_occ; i += 256)
      if (S.box[i] == pick) {
        const int src = list[i];
        const u64 c = cnt[src];
        atomicAdd(&S.marg[0][coord(src, 0)], c), atomicAdd(&S.marg[1][coord(src, 1)], c), atomicAdd(&S.marg[2][coord(src, 2)], c);
      }
    __syncthreads();
    if (tid == 0) {
      int lo;
      S.axis = gif_pick_axis(gif_extent(S.marg[0], 64, &lo), gif_extent(S.marg[1], 64, &lo), gif_extent(S.marg[2], 64, &lo));
      S.cut = gif_cut(S.marg[S.axis], 64, S.held[pick]);
      S.held[boxes] = 0, S.items[boxes] = 0;
    }
    __syncthreads();
    const int axis = S.axis, cut = S.cut;
    for (int i = tid; i < n_occ; i += 256)
      if (S.box[i] == pick) {
        const int src = list[i];
        if (coord(src, axis) > cut) S.box[i] = (uint8_t)boxes, atomicAdd(&S.held[boxes], cnt[src]), atomicAdd(&S.items[boxes], 1);
      }
    __syncthreads();
    if (tid == 0) S.held[pick] -= S.held[boxes], S.items[pick] -= S.items[boxes];
    ++boxes;
    __syncthreads();
  }

  for (int i = tid; i < n_occ; i += 256) {
    const int src = list[i], b = S.box[i];
    atomicAdd(&S.sum[b][0], cnt[NSRC + src]), atomicAdd(&S.sum[b][1], cnt[2 * NSRC + src]), atomicAdd(&S.sum[b][2], cnt[3 * NSRC + src]);
  }
  __syncthreads();
  uint8_t* p = pal + (long long)blockIdx.x * 3 * GIF_COLORS;
  for (int k = 0; k < 3; ++k) p[3 * tid + k] = tid < boxes ? (uint8_t)gif_mean(S.sum[tid][k], S.held[tid]) : (uint8_t)0;
  if (tid == 0) used[blockIdx.x] = boxes;
}

// (c) grid (GIF_BINS / 256, palettes)
__global__ __launch_bounds__(256) void gif_table_kernel(const uint8_t* __restrict__ pal, const int* __restrict__ used, uint8_t* __restrict__ table) {
  __shared__ uint8_t P[3 * GIF_COLORS];
  const int tid = threadIdx.x, bin = blockIdx.x * 256 + tid;
  const uint8_t* p = pal + (long long)blockIdx.y * 3 * GIF_COLORS;
  for (int i = tid; i < 3 * GIF_COLORS; i += 256) P[i] = p[i];
  __syncthreads();
  table[(long long)blockIdx.y * GIF_BINS + bin] = (uint8_t)gif_bin_nearest(P, used[blockIdx.y], bin);
}

// (c') grid (GIF_FINE_KEYS / 256, palettes): the few-colour palettes' table, by 6-bit key
__global__ __launch_bounds__(256) void gif_fine_table_kernel(const uint8_t* __restrict__ pal, const int* __restrict__ used,
                                                             const int* __restrict__ mode, uint8_t* __restrict__ ftable) {
  __shared__ uint8_t P[3 * GIF_COLORS];
  if (mode[2 * blockIdx.y] == 0) return;             // the same word for every thread
  const int tid = threadIdx.x, key = blockIdx.x * 256 + tid;
  const uint8_t* p = pal + (long long)blockIdx.y * 3 * GIF_COLORS;
  for (int i = tid; i < 3 * GIF_COLORS; i += 256) P[i] = p[i];
  __syncthreads();
  ftable[(long long)blockIdx.y * GIF_FINE_KEYS + key] = (uint8_t)gif_key6_nearest(P, used[blockIdx.y], key);
}

// (d)
__global__ __launch_bounds__(256) void gif_index_kernel(const uint8_t* __restrict__ px, long long st, long long n, int W, long long total,
                                                        int per_frame, int dither, const uint8_t* __restrict__ table,
                                                        const uint8_t* __restrict__ ftable, const int* __restrict__ mode,
                                                        uint8_t* __restrict__ idx) {
  const long long step = (long long)gridDim.x * 256;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += step) {
    const long long t = p / n, q = p - t * n, pi = per_frame ? t : 0;
    const int y = (int)(q / W), x = (int)(q - (long long)y * W), d = gif_dither(dither, y, x);
    const uint8_t* f = px + t * st + 3 * q;
    idx[p] = mode[2 * pi] ? ftable[pi * GIF_FINE_KEYS + gif_pixel_key6(f[0], f[1], f[2], d)]
                          : table[pi * GIF_BINS + gif_pixel_bin(f[0], f[1], f[2], d)];
  }
}

struct LzwShared {
  uint32_t table[GIF_TABLE];
  uint32_t out[GIF_CHUNK_WORDS];
  uint8_t idx[GIF_CHUNK];
  int bits;
};

// (e) one wave per chunk.  src: rows of n indices, `stride` apart.
__global__ __launch_bounds__(64) void gif_lzw_kernel(const uint8_t* __restrict__ src, long long stride, long long n, int nchunks,
                                                     uint32_t* __restrict__ slots, int* __restrict__ blen) {
  __shared__ LzwShared S;
  const int tid = threadIdx.x;
  const long long blk = blockIdx.x, row = blk / nchunks;
  const int c = (int)(blk - row * nchunks);
  const long long at = (long long)c * GIF_CHUNK;
  const int clen = (int)(n - at < GIF_CHUNK ? n - at : GIF_CHUNK);
  const uint8_t* g = src + row * stride + at;
  for (int i = tid; i < clen; i += 64) S.idx[i] = g[i];
  for (int i = tid; i < GIF_TABLE; i += 64) S.table[i] = 0xFFFFFFFFu;
  __syncthreads();
  if (tid == 0) S.bits = gif_lzw_chunk(S.idx, clen, c == 0, c == nchunks - 1, S.table, S.out);
  __syncthreads();
  const int words = (S.bits + 31) >> 5;
  uint32_t* slot = slots + blk * GIF_CHUNK_WORDS;
  for (int i = tid; i < words; i += 64) slot[i] = S.out[i];
  if (tid == 0) blen[blk] = S.bits;
}

// (f) one workgroup per row: the bit offset of every chunk, the stream's bytes, sizes[row]
__global__ __launch_bounds__(256) void gif_scan_kernel(const int* __restrict__ blen, int nchunks, int file, long long* __restrict__ boff,
                                                       long long* __restrict__ bytes, int* __restrict__ sizes) {
  __shared__ int sh[256];
  const int tid = threadIdx.x;
  const long long row = blockIdx.x;
  long long carry = 0;
  for (int base = 0; base < nchunks; base += 256) {
    const int c = base + tid, v = c < nchunks ? blen[row * nchunks + c] : 0;
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int a = tid >= o ? sh[tid - o] : 0;
      __syncthreads();
      sh[tid] += a;
      __syncthreads();
    }
    if (c < nchunks) boff[row * nchunks + c] = carry + sh[tid] - v;
    carry += sh[255];
    __syncthreads();
  }
  if (tid == 0) {
    const long long total = (carry + 7) >> 3;
    bytes[row] = total;
    sizes[row] = (int)(file ? gif_file_bytes(total) : total);
  }
}

__global__ __launch_bounds__(256) void gif_pack_kernel(const uint32_t* __restrict__ slots, const int* __restrict__ blen,
                                                       const long long* __restrict__ boff, const long long* __restrict__ bytes, int nchunks,
                                                       int file, int H, int W, const uint8_t* __restrict__ pal, int per_frame,
                                                       uint8_t* __restrict__ out, long long out_stride) {
  const int tid = threadIdx.x;
  const long long blk = blockIdx.x, row = blk / nchunks;
  const int c = (int)(blk - row * nchunks);
  const uint32_t* w = slots + blk * GIF_CHUNK_WORDS;
  const int bits = blen[blk], nbits = c + 1 < nchunks ? blen[blk + 1] : 0;
  const long long off = boff[blk], total = bytes[row];
  const long long j0 = (off + 7) >> 3, j1 = (off + bits + 7) >> 3;
  uint8_t* dst = out + row * out_stride;
  if (!file) {
    for (long long j = j0 + tid; j < j1; j += 256) dst[j] = (uint8_t)gif_stream_byte(j, w, bits, off, w + GIF_CHUNK_WORDS, nbits);
    return;
  }
  uint8_t* data = dst + GIF_HEAD;
  for (long long j = j0 + tid; j < j1; j += 256) {
    data[gif_block_pos(j)] = (uint8_t)gif_stream_byte(j, w, bits, off, w + GIF_CHUNK_WORDS, nbits);
    if (j % 255 == 0) data[j / 255 * 256] = (uint8_t)gif_block_len(j / 255, total);
  }
  if (c == 0) {
    const uint8_t* p = pal + (per_frame ? row : 0) * 3 * GIF_COLORS;
    for (int i = tid; i < GIF_HEAD; i += 256) dst[i] = gif_head_byte(i, W, H, p);
  }
  if (c == nchunks - 1 && tid == 0) {
    uint8_t* e = data + total + (total + 254) / 255;
    e[0] = 0x00, e[1] = 0x3B;
  }
}

inline long long up(long long v, long long a) { return (v + a - 1) / a * a; }

struct LzwPlan {
  int nchunks;
  long long blocks, o_slots, o_blen, o_boff, o_bytes, scratch;
};

// T rows of n indices; `base` is where the coder's share of the scratch begins
int lzw_plan(const char* fn, int T, long long n, long long base, bool file, long long* out_stride, LzwPlan* p) {
  LL_REQUIRE(T >= 1 && n >= 1, "%s: empty input: %d rows of %lld indices", fn, T, n);
  LL_REQUIRE(n <= 0x100000000ll, "%s: n=%lld: a row holds 2^32 indices at most", fn, n);
  const long long nchunks = (n + GIF_CHUNK - 1) / GIF_CHUNK;
  *out_stride = file ? gif_file_capacity(n) : gif_lzw_capacity(n);
  p->blocks = nchunks * T;
  LL_REQUIRE(*out_stride <= 0x7fffffffll && p->blocks <= 0x7fffffffll,
             "%s: %d rows of %lld indices are more than one call covers (a row's worst case must stay under 2 GiB, the call under 2^31 chunks)",
             fn, T, n);
  p->nchunks = (int)nchunks;
  long long o = base;
  p->o_slots = o, o += up(p->blocks * GIF_CHUNK_WORDS * 4, 256);
  p->o_blen = o, o += up(p->blocks * 4, 256);
  p->o_boff = o, o += up(p->blocks * 8, 256);
  p->o_bytes = o, o += up((long long)T * 8, 256);
  p->scratch = o;
  return LL_OK;
}

struct GifPlan {
  long long n, palettes, o_hist, o_fhist, o_occ, o_focc, o_mode, o_pal, o_used, o_table, o_ftable, o_idx, out_stride, scratch;
  LzwPlan z;
};

int gif_plan(const char* fn, int T, int H, int W, int palette, GifPlan* p) {
  LL_REQUIRE(T >= 1 && H >= 1 && W >= 1, "%s: empty input %d x %d x %d", fn, T, H, W);
  LL_REQUIRE(H <= 65535 && W <= 65535, "%s: %d x %d: a GIF image is 65535 x 65535 at most", fn, H, W);
  LL_REQUIRE(palette == GIF_PALETTE_CLIP || palette == GIF_PALETTE_FRAME, "%s: palette=%d is neither 0 (clip) nor 1 (frame)", fn, palette);
  p->n = (long long)H * W, p->palettes = palette == GIF_PALETTE_FRAME ? T : 1;
  LL_REQUIRE(p->palettes <= 65535, "%s: palette frame takes 65535 frames a call at most, not %d (the table kernels walk the palettes on a grid axis)",
             fn, T);
  long long o = 0;
  p->o_hist = o, o += p->palettes * GIF_HIST * 8;
  p->o_fhist = o, o += p->palettes * 4 * GIF_FINE_CELLS * 8;             // behind o_hist: one memset clears both
  p->o_occ = o, o += p->palettes * GIF_BINS * 2;
  p->o_focc = o, o += p->palettes * GIF_FINE_CELLS * 2;
  p->o_table = o, o += p->palettes * GIF_BINS;
  p->o_ftable = o, o += p->palettes * GIF_FINE_KEYS;
  p->o_mode = o, o += up(p->palettes * 8, 256);
  p->o_pal = o, o += up(p->palettes * 3 * GIF_COLORS, 256);
  p->o_used = o, o += up(p->palettes * 4, 256);
  p->o_idx = o, o += up((long long)T * p->n, 256);
  if (int rc = lzw_plan(fn, T, p->n, o, true, &p->out_stride, &p->z)) return rc;        // 2^31 chunks bound T H W under 2^43: the sums fit
  p->scratch = p->z.scratch;
  return LL_OK;
}

int gif_check_dither(const char* fn, int dither) {
  LL_REQUIRE(dither == GIF_DITHER_NONE || dither == GIF_DITHER_BAYER, "%s: dither=%d is neither 0 (none) nor 1 (bayer)", fn, dither);
  return LL_OK;
}

unsigned grid_for(long long items) {
  const long long blocks = (items + 255) / 256;
  return (unsigned)(blocks < 65536 ? blocks : 65536);
}

// (a) - (d): indices [T, n], palettes and used counts where the caller wants them
void quantize_launch(const uint8_t* frames, long long stride_t, int T, int W, int palette, int dither, const GifPlan& p, uint8_t* base,
                     uint8_t* idx, uint8_t* pal, int* used, hipStream_t s) {
  u64* hist = reinterpret_cast<u64*>(base + p.o_hist);
  u64* fhist = reinterpret_cast<u64*>(base + p.o_fhist);
  uint16_t* occ = reinterpret_cast<uint16_t*>(base + p.o_occ);
  uint16_t* focc = reinterpret_cast<uint16_t*>(base + p.o_focc);
  int* mode = reinterpret_cast<int*>(base + p.o_mode);
  uint8_t* table = base + p.o_table;
  uint8_t* ftable = base + p.o_ftable;
  const int per_frame = palette == GIF_PALETTE_FRAME;
  const long long runs_per_frame = (p.n + GIF_RUN - 1) / GIF_RUN, runs = runs_per_frame * T, total = p.n * T;
  const unsigned P = (unsigned)p.palettes;
  (void)hipMemsetAsync(hist, 0, (size_t)(p.o_occ - p.o_hist), s);                        // a failure is what ll_check_launch reports
  hipLaunchKernelGGL(gif_hist_kernel, dim3(grid_for(runs)), dim3(256), 0, s, frames, stride_t, p.n, runs_per_frame, runs, per_frame, hist);
  hipLaunchKernelGGL(gif_cut_kernel<false>, dim3(P), dim3(256), 0, s, (const u64*)hist, occ, (const uint16_t*)occ, mode, pal, used);
  hipLaunchKernelGGL(gif_fine_hist_kernel, dim3(grid_for(total)), dim3(256), 0, s, frames, stride_t, p.n, total, per_frame,
                     (const uint16_t*)occ, (const int*)mode, fhist);
  hipLaunchKernelGGL(gif_cut_kernel<true>, dim3(P), dim3(256), 0, s, (const u64*)fhist, focc, (const uint16_t*)occ, mode, pal, used);
  hipLaunchKernelGGL(gif_table_kernel, dim3(GIF_BINS / 256, P), dim3(256), 0, s, (const uint8_t*)pal, (const int*)used, table);
  hipLaunchKernelGGL(gif_fine_table_kernel, dim3(GIF_FINE_KEYS / 256, P), dim3(256), 0, s, (const uint8_t*)pal, (const int*)used,
                     (const int*)mode, ftable);
  hipLaunchKernelGGL(gif_index_kernel, dim3(grid_for(total)), dim3(256), 0, s, frames, stride_t, p.n, W, total, per_frame, dither,
                     (const uint8_t*)table, (const uint8_t*)ftable, (const int*)mode, idx);
}

void lzw_launch(const uint8_t* src, long long stride, long long n, int T, const LzwPlan& z, bool file, int H, int W, const uint8_t* pal,
                int per_frame, uint8_t* out, long long out_stride, int32_t* sizes, uint8_t* base, hipStream_t s) {
  uint32_t* slots = reinterpret_cast<uint32_t*>(base + z.o_slots);
  int* blen = reinterpret_cast<int*>(base + z.o_blen);
  long long* boff = reinterpret_cast<long long*>(base + z.o_boff);
  long long* bytes = reinterpret_cast<long long*>(base + z.o_bytes);
  hipLaunchKernelGGL(gif_lzw_kernel, dim3((unsigned)z.blocks), dim3(64), 0, s, src, stride, n, z.nchunks, slots, blen);
  hipLaunchKernelGGL(gif_scan_kernel, dim3((unsigned)T), dim3(256), 0, s, (const int*)blen, z.nchunks, file ? 1 : 0, boff, bytes, sizes);
  hipLaunchKernelGGL(gif_pack_kernel, dim3((unsigned)z.blocks), dim3(256), 0, s, (const uint32_t*)slots, (const int*)blen,
                     (const long long*)boff, (const long long*)bytes, z.nchunks, file ? 1 : 0, H, W, pal, per_frame, out, out_stride);
}

}  // namespace

extern "C" int ll_gif_sizes(int T, int H, int W, int palette, long long* out_stride, long long* scratch_bytes) {
  LL_REQUIRE(out_stride != nullptr && scratch_bytes != nullptr, "ll_gif_sizes: null operand");
  GifPlan p;
  if (int rc = gif_plan("ll_gif_sizes", T, H, W, palette, &p)) return rc;
  *out_stride = p.out_stride;
  *scratch_bytes = p.scratch;
  return LL_OK;
}

extern "C" int ll_gif_encode_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, int palette, int dither, uint8_t* out,
                                long long out_stride, int32_t* sizes, void* scratch, long long scratch_bytes, ll_stream stream) {
  LL_REQUIRE(frames != nullptr && out != nullptr && sizes != nullptr && scratch != nullptr, "ll_gif_encode_u8: null operand");
  GifPlan p;
  if (int rc = gif_plan("ll_gif_encode_u8", T, H, W, palette, &p)) return rc;
  if (int rc = gif_check_dither("ll_gif_encode_u8", dither)) return rc;
  LL_REQUIRE(stride_t >= 3ll * H * W, "ll_gif_encode_u8: stride_t=%lld bytes must span a %d x %d x 3 frame", stride_t, H, W);
  LL_REQUIRE(out_stride >= p.out_stride, "ll_gif_encode_u8: out_stride=%lld is under the worst case %lld of a %d x %d frame (ll_gif_sizes)",
             out_stride, p.out_stride, H, W);
  LL_REQUIRE(scratch_bytes >= p.scratch, "ll_gif_encode_u8: scratch_bytes=%lld, %d x %d x %d needs %lld (ll_gif_sizes)", scratch_bytes, T, H,
             W, p.scratch);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "ll_gif_encode_u8: scratch must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* base = static_cast<uint8_t*>(scratch);
  uint8_t* idx = base + p.o_idx;
  uint8_t* pal = base + p.o_pal;
  quantize_launch(frames, stride_t, T, W, palette, dither, p, base, idx, pal, reinterpret_cast<int*>(base + p.o_used), s);
  lzw_launch(idx, p.n, p.n, T, p.z, true, H, W, pal, palette == GIF_PALETTE_FRAME, out, out_stride, sizes, base, s);
  return ll_check_launch("ll_gif_encode_u8");
}

extern "C" int ll_gif_quantize_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, int palette, int dither, uint8_t* indices,
                                  uint8_t* palettes, int32_t* used, void* scratch, long long scratch_bytes, ll_stream stream) {
  LL_REQUIRE(frames != nullptr && indices != nullptr && palettes != nullptr && used != nullptr && scratch != nullptr,
             "ll_gif_quantize_u8: null operand");
  GifPlan p;
  if (int rc = gif_plan("ll_gif_quantize_u8", T, H, W, palette, &p)) return rc;
  if (int rc = gif_check_dither("ll_gif_quantize_u8", dither)) return rc;
  LL_REQUIRE(stride_t >= 3ll * H * W, "ll_gif_quantize_u8: stride_t=%lld bytes must span a %d x %d x 3 frame", stride_t, H, W);
  LL_REQUIRE(scratch_bytes >= p.scratch, "ll_gif_quantize_u8: scratch_bytes=%lld, %d x %d x %d needs %lld (ll_gif_sizes)", scratch_bytes, T,
             H, W, p.scratch);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "ll_gif_quantize_u8: scratch must be 16-byte aligned");
  quantize_launch(frames, stride_t, T, W, palette, dither, p, static_cast<uint8_t*>(scratch), indices, palettes, used, (hipStream_t)stream);
  return ll_check_launch("ll_gif_quantize_u8");
}

extern "C" int ll_gif_lzw_sizes(int T, long long n, long long* out_stride, long long* scratch_bytes) {
  LL_REQUIRE(out_stride != nullptr && scratch_bytes != nullptr, "ll_gif_lzw_sizes: null operand");
  LzwPlan z;
  if (int rc = lzw_plan("ll_gif_lzw_sizes", T, n, 0, false, out_stride, &z)) return rc;
  *scratch_bytes = z.scratch;
  return LL_OK;
}

extern "C" int ll_gif_lzw_u8(const uint8_t* rows, long long stride, int T, long long n, uint8_t* out, long long out_stride, int32_t* sizes,
                             void* scratch, long long scratch_bytes, ll_stream stream) {
  LL_REQUIRE(rows != nullptr && out != nullptr && sizes != nullptr && scratch != nullptr, "ll_gif_lzw_u8: null operand");
  LzwPlan z;
  long long need = 0;
  if (int rc = lzw_plan("ll_gif_lzw_u8", T, n, 0, false, &need, &z)) return rc;
  LL_REQUIRE(stride >= n, "ll_gif_lzw_u8: stride=%lld bytes must span a row of %lld", stride, n);
  LL_REQUIRE(out_stride >= need, "ll_gif_lzw_u8: out_stride=%lld is under the worst case %lld of a row of %lld indices (ll_gif_lzw_sizes)",
             out_stride, need, n);
  LL_REQUIRE(scratch_bytes >= z.scratch, "ll_gif_lzw_u8: scratch_bytes=%lld, %d rows of %lld indices need %lld (ll_gif_lzw_sizes)",
             scratch_bytes, T, n, z.scratch);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "ll_gif_lzw_u8: scratch must be 16-byte aligned");
  lzw_launch(rows, stride, n, T, z, false, 0, 0, nullptr, 0, out, out_stride, sizes, static_cast<uint8_t*>(scratch), (hipStream_t)stream);
  return ll_check_launch("ll_gif_lzw_u8");
}
