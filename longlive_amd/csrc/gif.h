// Animated previews: what csrc/gif.hip's kernels and a host program both compile (the tests build tests/gif_host_main.cpp from this
// file with the host compiler under sanitizers).  DESIGN.md section 5c, "Animated previews: GIF", gives the format; tests/gif_ref.py
// restates every routine here.
//
// The quantiser and the coder are deterministic and integer only:
//   histogram   GIF_BINS bins by (r >> 3, g >> 3, b >> 3): per bin the pixel count and the sums of the 8-bit r, g, b (64-bit)
//   median cut  one box over the occupied bins; until there are 256 boxes or no box holds more than one occupied bin, the box of
//               the largest pixel count among those (the lowest index on a tie) is split along the axis of largest extent of its
//               occupied bins (ties G, R, B: gif_pick_axis) at the smallest coordinate where the cumulative count reaches half, moved
//               down when the upper half would hold no occupied bin (gif_cut); the upper half becomes the next box.  Entry i is the
//               rounded mean of box i's true colours (gif_mean); entries past the boxes are 0.  When fewer than 256 bins are occupied
//               the cut runs over the bins' eight 6-bit cells each instead (below, "few colours"), so no entry stays unused for want
//               of resolution; table and lookup are then by the pixel's (r >> 2, g >> 2, b >> 2) key.
//   table       per bin centre ((c5 << 3) | 4 per channel) the used entry at the smallest squared distance, the lowest on a tie
//   indices     table[bin(clamp(p + d))], d = 0 or the 8 x 8 ordered-dither offset of the pixel's position (gif_dither)
//   LZW         the row-major indices of a frame in chunks of GIF_CHUNK pixels, each coded from a cleared dictionary (minimum code size
//               8, Clear 256, EOI 257, first free code 258): a chunk adds at most GIF_CHUNK - 1 entries, so the dictionary never fills
//               and the width never passes 12.  A chunk's bits are its codes and the Clear (the EOI behind the last chunk) that closes
//               it, written at the width after the entry the decoder adds for the chunk's last code; chunk 0 begins with a Clear at
//               9 bits.  The frame's stream is the chunks' bits joined bit by bit, packed from bit 0 of byte 0 (gif_stream_byte).
//   file        GIF89a, a logical screen descriptor without a global table, a graphic control extension, an image descriptor with a
//               local table of 256, the table, 08, the stream in sub-blocks of up to 255 bytes, 00, 3B (gif_head_byte, gif_block_pos)
#pragma once
#include <stdint.h>

typedef unsigned long long gif_u64;                 // what the 64-bit atomics take on the device, the same type on the host

#if defined(__HIPCC__)
#define GIF_HD __host__ __device__
#else
#define GIF_HD
#endif

enum {
  GIF_BINS = 32768,
  GIF_COLORS = 256,
  GIF_CHUNK = 3584,                                  // pixels per independently coded piece of a frame
  GIF_TABLE = 8192,                                  // slots of the coder's open-addressed dictionary: over twice GIF_CHUNK - 1 entries
  GIF_CLEAR = 256,
  GIF_EOI = 257,
  GIF_FIRST = 258,
  GIF_CHUNK_BITS = 9 + 12 * GIF_CHUNK + 12,          // a chunk's bits at most: the opening Clear, every pixel a 12-bit code, the close
  GIF_CHUNK_WORDS = (GIF_CHUNK_BITS + 31) / 32,
  GIF_FINE_CELLS = 2048,                             // cells of a few-colour palette: 8 per slot, under 256 slots
  GIF_FINE_KEYS = 262144,                            // (r >> 2, g >> 2, b >> 2) keys
  GIF_HEAD = 800,                                    // file bytes before the first sub-block: 6 + 7 + 8 + 10 + 768 + 1
  GIF_PALETTE_CLIP = 0,                              // `palette`: one table for the call's frames / one per frame
  GIF_PALETTE_FRAME = 1,
  GIF_DITHER_NONE = 0,                               // `dither`
  GIF_DITHER_BAYER = 1
};

// ---- pixels to bins ---------------------------------------------------------------------------------------------------------------
// Entry (y, x) of the 8 x 8 matrix of the recursion B(2n) = [[4B, 4B + 2], [4B + 3, 4B + 1]], B(1) = [0]: bit k of (y, x) picks the
// quadrant at scale 2^k, and the finest scale carries the largest weight.
GIF_HD inline int gif_bayer8(int y, int x) {
  int v = 0;
  for (int k = 0; k < 3; ++k) {
    const int a = (y >> k) & 1, b = (x >> k) & 1;
    v += (a ? (b ? 1 : 3) : (b ? 2 : 0)) << (2 * (2 - k));
  }
  return v;
}

// What is added to the three channels of pixel (y, x) before binning: -8 .. +7 under GIF_DITHER_BAYER
GIF_HD inline int gif_dither(int mode, int y, int x) { return mode == GIF_DITHER_BAYER ? (2 * gif_bayer8(y & 7, x & 7) - 63) >> 3 : 0; }

GIF_HD inline int gif_clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
GIF_HD inline int gif_bin(int r, int g, int b) { return ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3); }
GIF_HD inline int gif_pixel_bin(int r, int g, int b, int d) { return gif_bin(gif_clamp8(r + d), gif_clamp8(g + d), gif_clamp8(b + d)); }
GIF_HD inline int gif_coord(int bin, int axis) { return (bin >> (10 - 5 * axis)) & 31; }       // axis 0 = R, 1 = G, 2 = B

// Few colours: a palette whose frames occupy fewer than 256 bins would get one entry per bin and leave the rest unused.  It is made
// over CELLS instead: each occupied bin (its place in rising bin order is its slot) is cut in eight by bit 2 of r, g, b, so a cell is a
// (r >> 2, g >> 2, b >> 2) cube, at most 255 x 8 of them are occupied, and the same median cut runs over their 6-bit coordinates.
// The lookup is then by the pixel's 18-bit key, table entries by cell centres ((c6 << 2) | 2).
GIF_HD inline int gif_sub(int r, int g, int b) { return (((r >> 2) & 1) << 2) | (((g >> 2) & 1) << 1) | ((b >> 2) & 1); }
GIF_HD inline int gif_cell_coord(int bin, int sub, int axis) { return 2 * gif_coord(bin, axis) + ((sub >> (2 - axis)) & 1); }
GIF_HD inline int gif_key6(int r, int g, int b) { return ((r >> 2) << 12) | ((g >> 2) << 6) | (b >> 2); }
GIF_HD inline int gif_pixel_key6(int r, int g, int b, int d) { return gif_key6(gif_clamp8(r + d), gif_clamp8(g + d), gif_clamp8(b + d)); }
// The slot of an occupied bin: its place in the rising list of the n < 256 occupied ones (eight halvings at most)
GIF_HD inline int gif_slot(const uint16_t* bins, int n, int bin) {
  int lo = 0, hi = n - 1;
  for (int k = 0; k < 8 && lo < hi; ++k) {
    const int mid = (lo + hi) >> 1;
    if (bins[mid] < bin) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- median cut -------------------------------------------------------------------------------------------------------------------
// The extent of a box along an axis from its pixel counts per coordinate (n of them); *lo is its lowest occupied coordinate
GIF_HD inline int gif_extent(const gif_u64* marg, int n, int* lo) {
  int a = 0, b = n - 1;
  for (; a < n - 1 && marg[a] == 0; ++a) {}
  for (; b > a && marg[b] == 0; --b) {}
  *lo = a;
  return b - a;
}

GIF_HD inline int gif_pick_axis(int er, int eg, int eb) {
  int axis = 1, e = eg;
  if (er > e) axis = 0, e = er;
  if (eb > e) axis = 2;
  return axis;
}

// marg: the box's pixel counts per coordinate of the split axis (at least two of the n occupied), total their sum.  Coordinates up to
// the returned one stay; the rest become the new box.
GIF_HD inline int gif_cut(const gif_u64* marg, int n, gif_u64 total) {
  int first;
  const int last = gif_extent(marg, n, &first) + first;
  gif_u64 cum = 0;
  int c = first;
  for (; c < last; ++c) {
    cum += marg[c];
    if (cum >= total - cum) break;
  }
  if (c >= last)                                     // the upper half would be empty: the cut moves under the last occupied coordinate
    for (c = last - 1; c > first && marg[c] == 0; --c) {}
  return c;
}

GIF_HD inline int gif_mean(gif_u64 sum, gif_u64 count) { return (int)((2 * sum + count) / (2 * count)); }

// The serial form of csrc/gif.hip's median-cut kernel over a list of n occupied items (bins, coordinates under 32, or cells, under 64):
// xyz 3 n coordinates, cnt their pixels, sr / sg / sb their sums; pal: 768 bytes; box: n bytes of workspace.  Returns the used entries.
inline int gif_median_cut(int n, const uint8_t* xyz, const gif_u64* cnt, const gif_u64* sr, const gif_u64* sg, const gif_u64* sb,
                          uint8_t* pal, uint8_t* box) {
  gif_u64 held[GIF_COLORS], sum[GIF_COLORS][3];
  int items[GIF_COLORS], boxes = 1;
  held[0] = 0, items[0] = n;
  for (int i = 0; i < n; ++i) box[i] = 0, held[0] += cnt[i];
  for (int split = 1; split < GIF_COLORS; ++split) {
    int pick = -1;
    for (int i = 0; i < boxes; ++i)
      if (items[i] > 1 && (pick < 0 || held[i] > held[pick])) pick = i;
    if (pick < 0) break;
    gif_u64 marg[3][64];
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 64; ++c) marg[a][c] = 0;
    for (int i = 0; i < n; ++i)
      if (box[i] == pick)
        for (int a = 0; a < 3; ++a) marg[a][xyz[3 * i + a]] += cnt[i];
    int lo;
    const int axis = gif_pick_axis(gif_extent(marg[0], 64, &lo), gif_extent(marg[1], 64, &lo), gif_extent(marg[2], 64, &lo));
    const int c = gif_cut(marg[axis], 64, held[pick]);
    held[boxes] = 0, items[boxes] = 0;
    for (int i = 0; i < n; ++i)
      if (box[i] == pick && xyz[3 * i + axis] > c) box[i] = (uint8_t)boxes, held[boxes] += cnt[i], ++items[boxes];
    held[pick] -= held[boxes], items[pick] -= items[boxes];
    ++boxes;
  }
  for (int i = 0; i < GIF_COLORS; ++i) sum[i][0] = sum[i][1] = sum[i][2] = 0;
  for (int i = 0; i < n; ++i) sum[box[i]][0] += sr[i], sum[box[i]][1] += sg[i], sum[box[i]][2] += sb[i];
  for (int i = 0; i < GIF_COLORS; ++i)
    for (int k = 0; k < 3; ++k) pal[3 * i + k] = i < boxes ? (uint8_t)gif_mean(sum[i][k], held[i]) : (uint8_t)0;
  return boxes;
}

// ---- nearest entry ----------------------------------------------------------------------------------------------------------------
GIF_HD inline int gif_nearest(const uint8_t* pal, int used, int r, int g, int b) {
  int best = 0, bd = 0x7fffffff;
  for (int i = 0; i < used; ++i) {
    const int dr = r - pal[3 * i], dg = g - pal[3 * i + 1], db = b - pal[3 * i + 2], d = dr * dr + dg * dg + db * db;
    if (d < bd) bd = d, best = i;
  }
  return best;
}

GIF_HD inline int gif_bin_nearest(const uint8_t* pal, int used, int bin) {
  return gif_nearest(pal, used, (gif_coord(bin, 0) << 3) | 4, (gif_coord(bin, 1) << 3) | 4, (gif_coord(bin, 2) << 3) | 4);
}

GIF_HD inline int gif_key6_nearest(const uint8_t* pal, int used, int key) {
  return gif_nearest(pal, used, (((key >> 12) & 63) << 2) | 2, (((key >> 6) & 63) << 2) | 2, ((key & 63) << 2) | 2);
}

// ---- LZW --------------------------------------------------------------------------------------------------------------------------
GIF_HD inline uint32_t gif_hash(uint32_t key) { return (key * 2654435761u) >> 19; }              // 13 bits: a slot of GIF_TABLE

// One chunk: idx[0 .. n), 1 <= n <= GIF_CHUNK.  table: GIF_TABLE words, all ones on entry (an entry is key << 12 | code with the key
// prefix << 8 | byte; all ones is no entry: codes stay under 4095).  w receives (bits + 31) / 32 words, at most GIF_CHUNK_WORDS; the
// chunk's bits are returned.  Every probe ends: at most GIF_CHUNK - 1 of the GIF_TABLE slots are ever taken, and the walk is counted.
GIF_HD inline int gif_lzw_chunk(const uint8_t* idx, int n, int first, int last, uint32_t* table, uint32_t* w) {
  gif_u64 acc = 0;
  int held = 0, words = 0, bits = 0;
  auto emit = [&](uint32_t code, int width) {
    acc |= (gif_u64)code << held;
    held += width, bits += width;
    if (held >= 32) w[words++] = (uint32_t)acc, acc >>= 32, held -= 32;
  };
  int width = 9;
  uint32_t next = GIF_FIRST, prefix = idx[0];
  if (first) emit(GIF_CLEAR, 9);
  for (int i = 1; i < n; ++i) {
    const uint32_t byte = idx[i], key = (prefix << 8) | byte;
    uint32_t h = gif_hash(key), code = 0;
    bool hit = false;
    for (int probe = 0; probe < GIF_TABLE; ++probe) {
      const uint32_t e = table[h];
      if (e == 0xFFFFFFFFu) break;
      if ((e >> 12) == key) {
        code = e & 0xFFFu, hit = true;
        break;
      }
      h = (h + 1) & (GIF_TABLE - 1);
    }
    if (hit) {
      prefix = code;
      continue;
    }
    emit(prefix, width);
    table[h] = (key << 12) | next;
    if (next == (1u << width)) ++width;
    ++next;
    prefix = byte;
  }
  emit(prefix, width);
  if (next == (1u << width)) ++width;               // the decoder adds an entry for this last code too
  emit(last ? GIF_EOI : GIF_CLEAR, width);
  if (held > 0) w[words] = (uint32_t)acc;
  return bits;
}

// The 8 bits from bit `at` (0 <= at < bits) of a chunk's words; bits past the chunk's end read as 0
GIF_HD inline uint32_t gif_chunk_byte(const uint32_t* w, int bits, int at) {
  const int word = at >> 5, sh = at & 31;
  gif_u64 x = w[word];
  if (sh > 24 && (word + 1) * 32 < bits) x |= (gif_u64)w[word + 1] << 32;
  uint32_t v = (uint32_t)(x >> sh) & 0xFFu;
  if (bits - at < 8) v &= (1u << (bits - at)) - 1u;
  return v;
}

// Byte j of a stream of chunks joined bit by bit, for the chunk that holds the byte's first bit: w / bits / off are that chunk's words,
// bit count and bit offset in the stream, nw / nbits the next chunk's (nbits = 0: there is none).  Every chunk holds 18 bits or more, so
// a byte never reaches past the next chunk.
GIF_HD inline uint32_t gif_stream_byte(long long j, const uint32_t* w, int bits, long long off, const uint32_t* nw, int nbits) {
  const int at = (int)(8 * j - off);
  uint32_t v = gif_chunk_byte(w, bits, at);
  if (at + 8 > bits && nbits > 0) v |= (gif_chunk_byte(nw, nbits, 0) << (bits - at)) & 0xFFu;
  return v;
}

// ---- file -------------------------------------------------------------------------------------------------------------------------
GIF_HD inline long long gif_lzw_bytes_max(long long n) {
  const long long chunks = (n + GIF_CHUNK - 1) / GIF_CHUNK;
  return (9 + 12 * n + 12 * chunks + 7) >> 3;
}
GIF_HD inline long long gif_up16(long long v) { return (v + 15) / 16 * 16; }
GIF_HD inline long long gif_lzw_capacity(long long n) { return gif_up16(gif_lzw_bytes_max(n)); }
// Bytes of a file whose stream holds `bytes`: the head, a length byte per sub-block, the terminator, the trailer
GIF_HD inline long long gif_file_bytes(long long bytes) { return GIF_HEAD + bytes + (bytes + 254) / 255 + 2; }
GIF_HD inline long long gif_file_capacity(long long n) { return gif_up16(gif_file_bytes(gif_lzw_bytes_max(n))); }
// Where byte j of the stream lies behind the head, and the length byte of sub-block k of a stream of `bytes`
GIF_HD inline long long gif_block_pos(long long j) { return j + j / 255 + 1; }
GIF_HD inline int gif_block_len(long long k, long long bytes) { return bytes - 255 * k < 255 ? (int)(bytes - 255 * k) : 255; }

// Byte i < GIF_HEAD of the file: signature, logical screen descriptor (no global table, 8 bits of colour resolution), graphic control
// extension (disposal 1, no delay: cli's write_gif sets one, no transparency), image descriptor (local table of 256), table, 08
GIF_HD inline uint8_t gif_head_byte(int i, int W, int H, const uint8_t* pal) {
  const uint8_t w0 = (uint8_t)(W & 255), w1 = (uint8_t)(W >> 8), h0 = (uint8_t)(H & 255), h1 = (uint8_t)(H >> 8);
  const uint8_t fixed[31] = {'G', 'I', 'F', '8', '9', 'a', w0, w1, h0, h1, 0x70, 0, 0, 0x21, 0xF9, 4, 0x04, 0, 0, 0, 0,
                             0x2C, 0, 0, 0, 0, w0, w1, h0, h1, 0x87};
  return i < 31 ? fixed[i] : i < 31 + 3 * GIF_COLORS ? pal[i - 31] : (uint8_t)8;
}
