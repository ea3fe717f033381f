// Lossless frames out: a PNG encoder for uint8 RGB frames [T, H, W, 3] and the zlib compressor inside it, every stage on the GPU and
// stream-ordered.  csrc/png.h's head comment defines the deterministic DEFLATE (chunks of PNG_CHUNK bytes, one dynamic-Huffman block of
// literals and distance-1 matches per chunk, stored when that is shorter); tests/png_ref.py restates all of it.
//
// File, fixed: signature, IHDR (8 bits, colour type 2, no interlace), one IDAT per deflate chunk (the first begins with the zlib header
// 78 01), one IDAT of 4 bytes with the Adler-32, IEND.  Filter per row: of None, Sub, Up, Average, Paeth (bpp = 3, row 0 against a
// zero row) the type with the smallest sum of min(b, 256 - b) over the filtered bytes, the lower type on a tie.
//
// Launches of ll_png_encode_u8 (nothing is accumulated in place, so no scratch has to start as zero):
//   (a) png_filter_kernel   one wave per row: the five costs in one pass, the chosen form in a second -> [T, H, 1 + 3W]
//   (b) zlib_chunk_kernel   one workgroup per chunk, the chunk in LDS: repeat spans by two scans, histogram, code lengths and block
//                           header (one thread, csrc/png.h's routines), bits ORed into LDS at scanned offsets or the stored form, the
//                           IDAT framing and its CRC-32 from per-slice shares, the chunk's Adler-32 sums -> a staging slot + its length
//   (c) zlib_assemble_kernel one workgroup per chunk: sum of the lengths before it, copy behind the header; the first writes signature
//                           and IHDR, the last joins the Adler-32 sums and writes the tail and sizes[t]
// ll_zlib_compress_u8 is (b) and (c) over T byte rows, without the PNG framing.
#include "common.h"
#include "png.h"

namespace {

constexpr int PNG_SLICE = PNG_CHUNK / 256;          // positions per thread of the chunk kernel
constexpr int PNG_SLOT = PNG_CHUNK + 32;             // staging bytes per chunk: 10 of framing, 5 + PNG_CHUNK of block, 4 of CRC
constexpr int PNG_HEAD = 33;                         // signature 8 + IHDR 25
constexpr int PNG_TAIL = 28;                         // the Adler-32's IDAT 16 + IEND 12

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int png_filtered(int kind, int x, int a, int b, int c) {
  const int pred = kind == 0 ? 0 : kind == 1 ? a : kind == 2 ? b : kind == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
  return (x - pred) & 255;
}

// (a) one wave per row, four per workgroup
__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t* __restrict__ px, long long st, int H, int W,
                                                         uint8_t* __restrict__ out, long long rows) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long long t = row / H;
  const int r = (int)(row - t * H), n = 3 * W;
  const uint8_t* cur = px + t * st + (long long)r * n;
  const uint8_t* up = cur - n;
  const bool has_up = r > 0;
  int cost[5] = {0, 0, 0, 0, 0};
  for (int i = lane; i < n; i += 64) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = has_up ? up[i] : 0, c = (has_up && i >= 3) ? up[i - 3] : 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int v = png_filtered(k, x, a, b, c);
      cost[k] += v < 256 - v ? v : 256 - v;
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k)
    for (int o = 32; o > 0; o >>= 1) cost[k] += __shfl_xor(cost[k], o, 64);
  int kind = 0;
#pragma unroll
  for (int k = 1; k < 5; ++k)
    if (cost[k] < cost[kind]) kind = k;
  uint8_t* o = out + row * (n + 1);
  if (lane == 0) o[0] = (uint8_t)kind;
  for (int i = lane; i < n; i += 64) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = has_up ? up[i] : 0, c = (has_up && i >= 3) ? up[i - 3] : 0;
    o[1 + i] = (uint8_t)png_filtered(kind, x, a, b, c);
  }
}

__device__ __forceinline__ void png_put_shared(uint32_t* w, int pos, uint32_t v, int n) {      // png_put from many threads
  const int word = pos >> 5, sh = pos & 31;
  const uint64_t x = (uint64_t)v << sh;
  atomicOr(&w[word], (uint32_t)x);
  if (sh + n > 32) atomicOr(&w[word + 1], (uint32_t)(x >> 32));
}

// The tokens of positions [i0, i1) of a chunk in order.  d[-1] is the byte before the chunk when `first_can_repeat`; `before` is the
// last position under i0 that is no repeat (-1: none), `after` the first one from i1 on (the chunk's length: none).
template <class Lit, class Match>
__device__ __forceinline__ void png_walk(const uint8_t* d, int i0, int i1, bool first_can_repeat, int before, int after, Lit lit, Match match) {
  auto repeat = [&](int i) { return (i > 0 || first_can_repeat) && d[i] == d[i - 1]; };
  int i = i0;
  while (i < i1) {
    if (!repeat(i)) {
      lit((int)d[i]);
      before = i++;
      continue;
    }
    int j = i + 1;
    while (j < i1 && repeat(j)) ++j;
    const int s = before + 1, L = (j < i1 ? j : after) - s;
    for (; i < j; ++i) {
      int len = 0;
      const int t = png_span_token(i - s, L, &len);
      if (t == 1) lit((int)d[i]);
      else if (t == 2) match(len);
    }
  }
}

struct ChunkShared {
  uint32_t out[PNG_SLOT / 4];
  uint32_t hist[PNG_LITLEN + 2];
  uint32_t weight[2 * PNG_LITLEN];
  uint32_t crc_tab[256];
  int scan_a[256], scan_b[256];
  int16_t order[PNG_LITLEN + 2];
  int16_t parent[2 * PNG_LITLEN];
  uint16_t code[PNG_LITLEN + 2];
  uint8_t len[PNG_LITLEN + 2];
  uint8_t in[PNG_CHUNK + 16];                        // the chunk from in[4]; in[3] is the byte before it
  PngHeader header;
  int stored, token_bit, bytes;
  uint32_t crc, adler_a, adler_b;
};

// (b) one workgroup per chunk.  src: rows of n bytes, `stride` apart.  With `png` the slot holds an IDAT chunk (length, type, data,
// CRC-32), else the data alone; the data of a row's first chunk begins with 78 01.
__global__ __launch_bounds__(256) void zlib_chunk_kernel(const uint8_t* __restrict__ src, long long stride, long long n, int nchunks, int png,
                                                         uint8_t* __restrict__ slots, int* __restrict__ slen, uint32_t* __restrict__ adler) {
  __shared__ ChunkShared S;
  const int tid = threadIdx.x;
  const long long blk = blockIdx.x, row = blk / nchunks;
  const int c = (int)(blk - row * nchunks);
  const long long at = (long long)c * PNG_CHUNK;
  const int clen = (int)(n - at < PNG_CHUNK ? n - at : PNG_CHUNK);
  const bool final = c == nchunks - 1, has_prev = c > 0;
  const uint8_t* g = src + row * stride + at;
  uint8_t* d = S.in + 4;

  for (int i = tid; i < clen; i += 256) d[i] = g[i];
  if (tid == 0) d[-1] = has_prev ? g[-1] : (uint8_t)0;
  for (int i = tid; i < PNG_SLOT / 4; i += 256) S.out[i] = 0u;
  for (int i = tid; i < PNG_LITLEN + 2; i += 256) S.hist[i] = i == 256 ? 1u : 0u, S.len[i] = 0;
  S.crc_tab[tid] = png_crc_entry((uint32_t)tid);
  if (tid == 0) S.crc = 0u, S.adler_a = 0u, S.adler_b = 0u;
  __syncthreads();

  // the slice's neighbours that are no repeats: an exclusive running maximum from the left, a running minimum from the right
  const int i0 = tid * PNG_SLICE < clen ? tid * PNG_SLICE : clen, i1 = i0 + PNG_SLICE < clen ? i0 + PNG_SLICE : clen;
  {
    int last = -1, first = clen;
    for (int i = i0; i < i1; ++i)
      if (!((i > 0 || has_prev) && d[i] == d[i - 1])) {
        last = i;
        if (first == clen) first = i;
      }
    S.scan_a[tid] = last, S.scan_b[tid] = first;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int a = tid >= o ? S.scan_a[tid - o] : -1, b = tid + o < 256 ? S.scan_b[tid + o] : clen;
      __syncthreads();
      S.scan_a[tid] = a > S.scan_a[tid] ? a : S.scan_a[tid];
      S.scan_b[tid] = b < S.scan_b[tid] ? b : S.scan_b[tid];
      __syncthreads();
    }
  }
  const int before = tid > 0 ? S.scan_a[tid - 1] : -1, after = tid < 255 ? S.scan_b[tid + 1] : clen;

  png_walk(
      d, i0, i1, has_prev, before, after, [&](int b) { atomicAdd(&S.hist[b], 1u); },
      [&](int len) {
        int eb, ev;
        atomicAdd(&S.hist[png_length_symbol(len, &eb, &ev)], 1u);
      });
  __syncthreads();

  for (int s = tid; s < PNG_LITLEN; s += 256) {
    const int r = png_rank(S.hist, PNG_LITLEN, s);
    if (r >= 0) S.order[r] = (int16_t)s;
  }
  __syncthreads();

  const int prefix = (png ? 8 : 0) + (c == 0 ? 2 : 0);           // bytes of the slot before the deflate data
  if (tid == 0) {
    int used = 0;
    for (int s = 0; s < PNG_LITLEN; ++s) used += S.hist[s] != 0u;
    png_code_lengths(S.hist, S.order, used, PNG_MAX_BITS, S.len, S.weight, S.parent);
    png_canonical_codes(S.len, PNG_LITLEN, S.code);
    png_header_build(S.len, &S.header);
    const long long bits = png_block_bits(S.hist, S.len, &S.header);
    const int dyn = png_dynamic_bytes(bits, final);
    S.stored = dyn > clen + 5;
    S.bytes = S.stored ? clen + 5 : dyn;
    uint8_t* o = reinterpret_cast<uint8_t*>(S.out);
    if (png) {
      const int m = S.bytes + (c == 0 ? 2 : 0);
      o[0] = 0, o[1] = 0, o[2] = (uint8_t)(m >> 8), o[3] = (uint8_t)(m & 255);
      o[4] = 'I', o[5] = 'D', o[6] = 'A', o[7] = 'T';
    }
    if (c == 0) o[prefix - 2] = 0x78, o[prefix - 1] = 0x01;
    if (S.stored) {
      uint8_t* b = o + prefix;
      b[0] = final ? 1 : 0, b[1] = (uint8_t)(clen & 255), b[2] = (uint8_t)(clen >> 8), b[3] = (uint8_t)(~clen & 255), b[4] = (uint8_t)((~clen >> 8) & 255);
    } else {
      const long long p0 = 8ll * prefix, p1 = png_header_write(&S.header, final, S.out, p0);
      S.token_bit = (int)p1;
      const long long eob = p0 + bits - S.len[256];
      png_put(S.out, eob, S.code[256], S.len[256]);
      png_block_close(S.out, eob + S.len[256], final);           // the prefix is whole bytes: the padding is the block's own
    }
  }
  __syncthreads();

  if (S.stored) {
    uint8_t* o = reinterpret_cast<uint8_t*>(S.out) + prefix + 5;
    for (int i = tid; i < clen; i += 256) o[i] = d[i];
  } else {
    int mine = 0;
    png_walk(
        d, i0, i1, has_prev, before, after, [&](int b) { mine += S.len[b]; },
        [&](int len) {
          int eb, ev;
          mine += S.len[png_length_symbol(len, &eb, &ev)] + eb + 1;
        });
    S.scan_a[tid] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int a = tid >= o ? S.scan_a[tid - o] : 0;
      __syncthreads();
      S.scan_a[tid] += a;
      __syncthreads();
    }
    int pos = S.token_bit + S.scan_a[tid] - mine;
    png_walk(
        d, i0, i1, has_prev, before, after,
        [&](int b) {
          png_put_shared(S.out, pos, S.code[b], S.len[b]);
          pos += S.len[b];
        },
        [&](int len) {
          int eb, ev;
          const int sym = png_length_symbol(len, &eb, &ev);
          const int l = S.len[sym];
          png_put_shared(S.out, pos, (uint32_t)S.code[sym] | ((uint32_t)ev << l), l + eb);      // the distance code is one 0 bit
          pos += l + eb + 1;
        });
  }
  __syncthreads();

  // the IDAT's CRC-32 over type and data, from the shares of 64-byte slices; the chunk's Adler-32 sums over its input
  const uint8_t* o = reinterpret_cast<const uint8_t*>(S.out);
  const int body = prefix + S.bytes;                             // slot bytes so far; the CRC covers [4, body)
  if (png) {
    uint32_t share = 0u;
    for (int p = 4 + tid * 64; p < body; p += 256 * 64) {
      const int q = p + 64 < body ? p + 64 : body;
      uint32_t raw = 0u;
      for (int i = p; i < q; ++i) raw = S.crc_tab[(raw ^ o[i]) & 0xFFu] ^ (raw >> 8);
      share ^= png_crc_share(raw, body - q);
    }
    atomicXor(&S.crc, share);
  }
  {
    uint32_t a = 0u, b = 0u;
    for (int i = i0; i < i1; ++i) a += d[i], b += (uint32_t)(i1 - i) * d[i];
    b = (uint32_t)((b + (uint64_t)(clen - i1) * a) % 65521u);
    atomicAdd(&S.adler_a, a);                                    // 256 x 64 x 255 and 256 x 65520 stay under 2^32
    atomicAdd(&S.adler_b, b);
  }
  __syncthreads();
  int total = body;
  if (png) {
    total += 4;
    if (tid == 0) {
      const uint32_t crc = png_crc_finish(S.crc, body - 4);
      uint8_t* ob = reinterpret_cast<uint8_t*>(S.out) + body;
      ob[0] = (uint8_t)(crc >> 24), ob[1] = (uint8_t)(crc >> 16), ob[2] = (uint8_t)(crc >> 8), ob[3] = (uint8_t)crc;
    }
  }
  if (tid == 0) {
    slen[blk] = total;
    adler[2 * blk] = S.adler_a % 65521u, adler[2 * blk + 1] = S.adler_b % 65521u;
  }
  __syncthreads();
  uint32_t* slot = reinterpret_cast<uint32_t*>(slots + blk * PNG_SLOT);
  for (int i = tid; i < (total + 3) / 4; i += 256) slot[i] = S.out[i];
}

// (c) one workgroup per chunk: where it lands is the sum of the lengths before it in its row
__global__ __launch_bounds__(256) void zlib_assemble_kernel(const uint8_t* __restrict__ slots, const int* __restrict__ slen,
                                                            const uint32_t* __restrict__ adler, long long n, int nchunks, int png, int H, int W,
                                                            uint8_t* __restrict__ out, long long out_stride, int* __restrict__ sizes) {
  __shared__ long long sh[256];
  const int tid = threadIdx.x;
  const long long blk = blockIdx.x, row = blk / nchunks;
  const int c = (int)(blk - row * nchunks);
  long long part = 0;
  for (int k = tid; k < c; k += 256) part += slen[row * nchunks + k];
  sh[tid] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  const int head = png ? PNG_HEAD : 0, L = slen[blk];
  uint8_t* file = out + row * out_stride;
  uint8_t* dst = file + head + sh[0];
  const uint8_t* s = slots + blk * PNG_SLOT;
  for (int i = tid; i < L; i += 256) dst[i] = s[i];
  if (c == 0 && png && tid == 0) {
    const uint8_t ihdr[PNG_HEAD - 4] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R',
                                       (uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8), (uint8_t)W,
                                       (uint8_t)(H >> 24), (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H, 8, 2, 0, 0, 0};
    for (int i = 0; i < PNG_HEAD - 4; ++i) file[i] = ihdr[i];
    const uint32_t crc = png_crc_bytes(ihdr + 12, 17);
    for (int i = 0; i < 4; ++i) file[PNG_HEAD - 4 + i] = (uint8_t)(crc >> (24 - 8 * i));
  }
  if (c == nchunks - 1 && tid == 0) {
    uint32_t A = 1u, B = 0u;
    for (int k = 0; k < nchunks; ++k) {
      const long long m = k == nchunks - 1 ? n - (long long)k * PNG_CHUNK : PNG_CHUNK;
      png_adler_join(&A, &B, adler[2 * (row * nchunks + k)], adler[2 * (row * nchunks + k) + 1], m);
    }
    const uint32_t sum = (B << 16) | A;
    uint8_t* e = dst + L;
    long long size = head + sh[0] + L;
    if (png) {
      uint8_t tail[PNG_TAIL] = {0, 0, 0, 4, 'I', 'D', 'A', 'T', (uint8_t)(sum >> 24), (uint8_t)(sum >> 16), (uint8_t)(sum >> 8), (uint8_t)sum,
                                0, 0, 0, 0, 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
      const uint32_t crc = png_crc_bytes(tail + 4, 8);
      for (int i = 0; i < 4; ++i) tail[12 + i] = (uint8_t)(crc >> (24 - 8 * i));
      for (int i = 0; i < PNG_TAIL; ++i) e[i] = tail[i];
      size += PNG_TAIL;
    } else {
      for (int i = 0; i < 4; ++i) e[i] = (uint8_t)(sum >> (24 - 8 * i));
      size += 4;
    }
    sizes[row] = (int)size;
  }
}

struct ZlibPlan {
  int nchunks;
  long long blocks, out_stride, o_slots, o_slen, o_adler, scratch;
};

inline long long up(long long v, long long a) { return (v + a - 1) / a * a; }

// T rows of n bytes; with `png` the rows are filtered frames and the capacity holds the file's framing
int zlib_plan(const char* fn, int T, long long n, bool png, ZlibPlan* p) {
  LL_REQUIRE(T >= 1 && n >= 1, "%s: empty input: %d rows of %lld bytes", fn, T, n);
  const long long nchunks = (n + PNG_CHUNK - 1) / PNG_CHUNK;
  p->out_stride = png ? up(PNG_HEAD + n + 17 * nchunks + 2 + PNG_TAIL, 16) : up(2 + n + 5 * nchunks + 4, 16);
  p->blocks = nchunks * T;
  LL_REQUIRE(p->out_stride <= 0x7fffffffll && p->blocks <= 0x7fffffffll,
             "%s: %d rows of %lld bytes are more than one call covers (a row's worst case must stay under 2 GiB, the call under 2^31 chunks)", fn,
             T, n);
  p->nchunks = (int)nchunks;
  long long o = 0;
  p->o_slots = o, o += up(p->blocks * PNG_SLOT, 256);
  p->o_slen = o, o += up(p->blocks * 4, 256);
  p->o_adler = o, o += up(p->blocks * 8, 256);
  p->scratch = o;
  return LL_OK;
}

struct PngPlan {
  long long n, rows, o_filtered, scratch;
  ZlibPlan z;
};

int png_plan(const char* fn, int T, int H, int W, PngPlan* p) {
  LL_REQUIRE(T >= 1 && H >= 1 && W >= 1, "%s: empty input %d x %d x %d", fn, T, H, W);
  LL_REQUIRE(W <= 0x2aaaaaaa, "%s: W=%d: a row of 3 W bytes must stay under 2^31", fn, W);
  p->n = (long long)H * (1 + 3ll * W), p->rows = (long long)T * H;
  LL_REQUIRE(p->rows <= 0x7fffffffll, "%s: %d x %d x %d is more than one call covers (under 2^31 rows)", fn, T, H, W);
  if (int rc = zlib_plan(fn, T, p->n, true, &p->z)) return rc;
  p->o_filtered = p->z.scratch;
  p->scratch = p->o_filtered + up((long long)T * p->n, 256);
  return LL_OK;
}

void png_launch_filter(const uint8_t* frames, long long stride_t, int H, int W, uint8_t* out, long long rows, hipStream_t s) {
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, frames, stride_t, H, W, out, rows);
}

void zlib_launch(const uint8_t* src, long long stride, long long n, const ZlibPlan& z, bool png, int H, int W, uint8_t* out,
                 long long out_stride, int32_t* sizes, uint8_t* base, hipStream_t s) {
  uint8_t* slots = base + z.o_slots;
  int* slen = reinterpret_cast<int*>(base + z.o_slen);
  uint32_t* adler = reinterpret_cast<uint32_t*>(base + z.o_adler);
  hipLaunchKernelGGL(zlib_chunk_kernel, dim3((unsigned)z.blocks), dim3(256), 0, s, src, stride, n, z.nchunks, png ? 1 : 0, slots, slen, adler);
  hipLaunchKernelGGL(zlib_assemble_kernel, dim3((unsigned)z.blocks), dim3(256), 0, s, (const uint8_t*)slots, (const int*)slen,
                     (const uint32_t*)adler, n, z.nchunks, png ? 1 : 0, H, W, out, out_stride, sizes);
}

}  // namespace

extern "C" int ll_png_sizes(int T, int H, int W, long long* out_stride, long long* scratch_bytes) {
  LL_REQUIRE(out_stride != nullptr && scratch_bytes != nullptr, "ll_png_sizes: null operand");
  PngPlan p;
  if (int rc = png_plan("ll_png_sizes", T, H, W, &p)) return rc;
  *out_stride = p.z.out_stride;
  *scratch_bytes = p.scratch;
  return LL_OK;
}

extern "C" int ll_png_filter_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, uint8_t* out, ll_stream stream) {
  LL_REQUIRE(frames != nullptr && out != nullptr, "ll_png_filter_u8: null operand");
  PngPlan p;
  if (int rc = png_plan("ll_png_filter_u8", T, H, W, &p)) return rc;
  LL_REQUIRE(stride_t >= 3ll * H * W, "ll_png_filter_u8: stride_t=%lld bytes must span a %d x %d x 3 frame", stride_t, H, W);
  png_launch_filter(frames, stride_t, H, W, out, p.rows, (hipStream_t)stream);
  return ll_check_launch("ll_png_filter_u8");
}

extern "C" int ll_png_encode_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, uint8_t* out, long long out_stride,
                                int32_t* sizes, void* scratch, long long scratch_bytes, ll_stream stream) {
  LL_REQUIRE(frames != nullptr && out != nullptr && sizes != nullptr && scratch != nullptr, "ll_png_encode_u8: null operand");
  PngPlan p;
  if (int rc = png_plan("ll_png_encode_u8", T, H, W, &p)) return rc;
  LL_REQUIRE(stride_t >= 3ll * H * W, "ll_png_encode_u8: stride_t=%lld bytes must span a %d x %d x 3 frame", stride_t, H, W);
  LL_REQUIRE(out_stride >= p.z.out_stride, "ll_png_encode_u8: out_stride=%lld is under the worst case %lld of a %d x %d frame (ll_png_sizes)",
             out_stride, p.z.out_stride, H, W);
  LL_REQUIRE(scratch_bytes >= p.scratch, "ll_png_encode_u8: scratch_bytes=%lld, %d x %d x %d needs %lld (ll_png_sizes)", scratch_bytes, T, H,
             W, p.scratch);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "ll_png_encode_u8: scratch must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* base = static_cast<uint8_t*>(scratch);
  uint8_t* filtered = base + p.o_filtered;
  png_launch_filter(frames, stride_t, H, W, filtered, p.rows, s);
  zlib_launch(filtered, p.n, p.n, p.z, true, H, W, out, out_stride, sizes, base, s);
  return ll_check_launch("ll_png_encode_u8");
}

extern "C" int ll_zlib_sizes(int T, long long n, long long* out_stride, long long* scratch_bytes) {
  LL_REQUIRE(out_stride != nullptr && scratch_bytes != nullptr, "ll_zlib_sizes: null operand");
  ZlibPlan z;
  if (int rc = zlib_plan("ll_zlib_sizes", T, n, false, &z)) return rc;
  *out_stride = z.out_stride;
  *scratch_bytes = z.scratch;
  return LL_OK;
}

extern "C" int ll_zlib_compress_u8(const uint8_t* src, long long stride, int T, long long n, uint8_t* out, long long out_stride,
                                   int32_t* sizes, void* scratch, long long scratch_bytes, ll_stream stream) {
  LL_REQUIRE(src != nullptr && out != nullptr && sizes != nullptr && scratch != nullptr, "ll_zlib_compress_u8: null operand");
  ZlibPlan z;
  if (int rc = zlib_plan("ll_zlib_compress_u8", T, n, false, &z)) return rc;
  LL_REQUIRE(stride >= n, "ll_zlib_compress_u8: stride=%lld bytes must span a row of %lld", stride, n);
  LL_REQUIRE(out_stride >= z.out_stride, "ll_zlib_compress_u8: out_stride=%lld is under the worst case %lld of a row of %lld bytes (ll_zlib_sizes)",
             out_stride, z.out_stride, n);
  LL_REQUIRE(scratch_bytes >= z.scratch, "ll_zlib_compress_u8: scratch_bytes=%lld, %d rows of %lld bytes need %lld (ll_zlib_sizes)",
             scratch_bytes, T, n, z.scratch);
  LL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "ll_zlib_compress_u8: scratch must be 16-byte aligned");
  zlib_launch(src, stride, n, z, false, 0, 0, out, out_stride, sizes, static_cast<uint8_t*>(scratch), (hipStream_t)stream);
  return ll_check_launch("ll_zlib_compress_u8");
}
