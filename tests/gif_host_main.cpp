// csrc/gif.h as a stand-alone host program (tests/test_gif_host.py builds it with -fsanitize=address,undefined and compares every
// printed line with tests/gif_ref.py).  argv[1] is a file of cases, each a line of decimal numbers:
//   B                                   -> "B d(0,0) d(0,1) .. d(7,7)" the 64 dither offsets
//   S n i0 .. i(n-1)                    a row of indices -> "S <hex of its LZW stream>"
//   Q T H W palette dither p0 ..        T frames of H x W x 3 bytes -> per palette "P used <hex of the 768 bytes>", then "I <hex of the
//                                       T H W indices>", then per frame "F <hex of its file>"
// Every buffer is a heap block of exactly the size the routines are promised, so the sanitizer sees any step past an end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gif.h"

static bool next(FILE* f, long long* v) { return fscanf(f, "%lld", v) == 1; }

static void hex(const char* tag, const uint8_t* p, long long n) {
  printf("%s", tag);
  for (long long i = 0; i < n; ++i) printf("%02x", p[i]);
  printf("\n");
}

// The stream of one row: every chunk through gif_lzw_chunk, then byte by byte through gif_stream_byte as the pack kernel walks them
static std::vector<uint8_t> stream_of(const uint8_t* idx, long long n) {
  const int chunks = (int)((n + GIF_CHUNK - 1) / GIF_CHUNK);
  std::vector<uint32_t*> words(chunks);
  std::vector<int> bits(chunks);
  std::vector<long long> off(chunks + 1, 0);
  for (int c = 0; c < chunks; ++c) {
    const long long at = (long long)c * GIF_CHUNK;
    const int clen = (int)(n - at < GIF_CHUNK ? n - at : GIF_CHUNK);
    uint8_t* in = new uint8_t[clen];
    memcpy(in, idx + at, clen);
    uint32_t* table = new uint32_t[GIF_TABLE];
    memset(table, 0xFF, sizeof(uint32_t) * GIF_TABLE);
    words[c] = new uint32_t[((c == 0 ? 9 : 0) + 12 * clen + 12 + 31) / 32];
    bits[c] = gif_lzw_chunk(in, clen, c == 0, c == chunks - 1, table, words[c]);
    off[c + 1] = off[c] + bits[c];
    delete[] in, delete[] table;
  }
  const long long total = (off[chunks] + 7) >> 3;
  if (total > gif_lzw_bytes_max(n)) exit(4);
  std::vector<uint8_t> out(total);
  for (int c = 0; c < chunks; ++c) {
    const bool more = c + 1 < chunks;
    for (long long j = (off[c] + 7) >> 3; j < (off[c] + bits[c] + 7) >> 3; ++j)
      out[j] = (uint8_t)gif_stream_byte(j, words[c], bits[c], off[c], more ? words[c + 1] : nullptr, more ? bits[c + 1] : 0);
  }
  for (int c = 0; c < chunks; ++c) delete[] words[c];
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char kind[4];
  while (fscanf(f, "%1s", kind) == 1) {
    long long n, v;
    if (kind[0] == 'B') {
      printf("B");
      for (int y = 0; y < 8; ++y)
        for (int x = 0; x < 8; ++x) printf(" %d", gif_dither(GIF_DITHER_BAYER, y + 8, x + 16));
      printf("\n");
    } else if (kind[0] == 'S') {
      if (!next(f, &n)) return 3;
      uint8_t* idx = new uint8_t[n];
      for (long long i = 0; i < n; ++i) {
        if (!next(f, &v)) return 3;
        idx[i] = (uint8_t)v;
      }
      const std::vector<uint8_t> s = stream_of(idx, n);
      hex("S ", s.data(), (long long)s.size());
      delete[] idx;
    } else if (kind[0] == 'Q') {
      long long T, H, W, palette, dither;
      if (!next(f, &T) || !next(f, &H) || !next(f, &W) || !next(f, &palette) || !next(f, &dither)) return 3;
      const long long px = H * W;
      uint8_t* frames = new uint8_t[T * px * 3];
      for (long long i = 0; i < T * px * 3; ++i) {
        if (!next(f, &v)) return 3;
        frames[i] = (uint8_t)v;
      }
      const long long P = palette == GIF_PALETTE_FRAME ? T : 1;
      uint8_t* pal = new uint8_t[P * 768];
      uint8_t* table = new uint8_t[P * GIF_BINS];
      int* entries = new int[P];
      bool* fine = new bool[P];
      for (long long p = 0; p < P; ++p) {
        gif_u64* hist = new gif_u64[4 * GIF_BINS]();
        const long long t0 = palette == GIF_PALETTE_FRAME ? p : 0, t1 = palette == GIF_PALETTE_FRAME ? p + 1 : T;
        for (long long i = t0 * px; i < t1 * px; ++i) {
          const uint8_t* q = frames + 3 * i;
          const int bin = gif_bin(q[0], q[1], q[2]);
          ++hist[bin], hist[GIF_BINS + bin] += q[0], hist[2 * GIF_BINS + bin] += q[1], hist[3 * GIF_BINS + bin] += q[2];
        }
        int occupied = 0;
        for (int bin = 0; bin < GIF_BINS; ++bin) occupied += hist[bin] != 0;
        uint16_t* bins = new uint16_t[occupied];
        for (int bin = 0, at = 0; bin < GIF_BINS; ++bin)
          if (hist[bin]) bins[at++] = (uint16_t)bin;
        fine[p] = occupied < GIF_COLORS;
        // the items: the occupied bins, or under 256 of them the occupied cells of their slots
        const int nsrc = fine[p] ? 8 * occupied : GIF_BINS;
        gif_u64* src = hist;
        if (fine[p]) {
          src = new gif_u64[4 * nsrc]();
          for (long long i = t0 * px; i < t1 * px; ++i) {
            const uint8_t* q = frames + 3 * i;
            const int cell = 8 * gif_slot(bins, occupied, gif_bin(q[0], q[1], q[2])) + gif_sub(q[0], q[1], q[2]);
            ++src[cell], src[nsrc + cell] += q[0], src[2 * nsrc + cell] += q[1], src[3 * nsrc + cell] += q[2];
          }
        }
        int n = 0;
        for (int i = 0; i < nsrc; ++i) n += src[i] != 0;
        uint8_t* xyz = new uint8_t[3 * n];
        gif_u64* item = new gif_u64[4 * n];
        for (int i = 0, at = 0; i < nsrc; ++i)
          if (src[i]) {
            for (int a = 0; a < 3; ++a) xyz[3 * at + a] = (uint8_t)(fine[p] ? gif_cell_coord(bins[i >> 3], i & 7, a) : gif_coord(i, a));
            for (int k = 0; k < 4; ++k) item[k * n + at] = src[k * nsrc + i];
            ++at;
          }
        uint8_t* box = new uint8_t[n];
        const int used = gif_median_cut(n, xyz, item, item + n, item + 2 * n, item + 3 * n, pal + p * 768, box);
        for (int bin = 0; bin < GIF_BINS; ++bin) table[p * GIF_BINS + bin] = (uint8_t)gif_bin_nearest(pal + p * 768, used, bin);
        entries[p] = used;                             // the few-colour table is looked up key by key below, not built whole
        printf("P %d ", used);
        hex("", pal + p * 768, 768);
        if (fine[p]) delete[] src;
        delete[] hist, delete[] bins, delete[] xyz, delete[] item, delete[] box;
      }
      uint8_t* idx = new uint8_t[T * px];
      for (long long t = 0; t < T; ++t)
        for (long long y = 0; y < H; ++y)
          for (long long x = 0; x < W; ++x) {
            const uint8_t* q = frames + 3 * (t * px + y * W + x);
            const long long p = palette == GIF_PALETTE_FRAME ? t : 0;
            const int d = gif_dither((int)dither, (int)y, (int)x);
            idx[t * px + y * W + x] = fine[p] ? (uint8_t)gif_key6_nearest(pal + p * 768, entries[p], gif_pixel_key6(q[0], q[1], q[2], d))
                                              : table[p * GIF_BINS + gif_pixel_bin(q[0], q[1], q[2], d)];
          }
      hex("I ", idx, T * px);
      for (long long t = 0; t < T; ++t) {
        const std::vector<uint8_t> s = stream_of(idx + t * px, px);
        const long long total = (long long)s.size(), size = gif_file_bytes(total);
        if (size > gif_file_capacity(px)) return 4;
        uint8_t* file = new uint8_t[size];
        const uint8_t* p = pal + (palette == GIF_PALETTE_FRAME ? t : 0) * 768;
        for (int i = 0; i < GIF_HEAD; ++i) file[i] = gif_head_byte(i, (int)W, (int)H, p);
        for (long long j = 0; j < total; ++j) {
          file[GIF_HEAD + gif_block_pos(j)] = s[j];
          if (j % 255 == 0) file[GIF_HEAD + j / 255 * 256] = (uint8_t)gif_block_len(j / 255, total);
        }
        file[size - 2] = 0x00, file[size - 1] = 0x3B;
        hex("F ", file, size);
        delete[] file;
      }
      delete[] frames, delete[] pal, delete[] table, delete[] entries, delete[] fine, delete[] idx;
    } else {
      return 3;
    }
  }
  fclose(f);
  return 0;
}
