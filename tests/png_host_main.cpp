// csrc/png.h as a stand-alone host program (tests/test_png_host.py builds it with -fsanitize=address,undefined and compares every
// printed line with tests/png_ref.py).  argv[1] is a file of cases, each a line of decimal numbers:
//   H maxbits n c0 .. c(n-1)            a histogram -> "H l0 l1 .." the limited code lengths, then "C .." the bit-reversed codes
//   D has_prev final n b(-1) b0 ..      a chunk (the byte before it first) -> "D <hex of the chunk's deflate bytes>"
//   K piece n b0 ..                     CRC-32 from shares of `piece` bytes and Adler-32 from joined pieces -> "K crc adler"
// Every buffer is a heap block of exactly the size the routines are promised, so the sanitizer sees any step past an end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png.h"

static bool next(FILE* f, long long* v) { return fscanf(f, "%lld", v) == 1; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char kind[4];
  while (fscanf(f, "%1s", kind) == 1) {
    long long a, b, n, v;
    if (kind[0] == 'H') {
      if (!next(f, &a) || !next(f, &n)) return 3;
      uint32_t* count = new uint32_t[n];
      for (long long i = 0; i < n; ++i) {
        if (!next(f, &v)) return 3;
        count[i] = (uint32_t)v;
      }
      int16_t* order = new int16_t[n];
      int used = 0;
      for (int i = 0; i < n; ++i) {
        const int r = png_rank(count, (int)n, i);
        if (r >= 0) order[r] = (int16_t)i, ++used;
      }
      uint8_t* len = new uint8_t[n]();
      uint32_t* weight = new uint32_t[2 * used + 1];
      int16_t* parent = new int16_t[2 * used + 1];
      png_code_lengths(count, order, used, (int)a, len, weight, parent);
      uint16_t* code = new uint16_t[n];
      png_canonical_codes(len, (int)n, code);
      printf("H");
      for (int i = 0; i < n; ++i) printf(" %d", len[i]);
      printf("\nC");
      for (int i = 0; i < n; ++i) printf(" %d", code[i]);
      printf("\n");
      delete[] count, delete[] order, delete[] len, delete[] weight, delete[] parent, delete[] code;
    } else if (kind[0] == 'D') {
      if (!next(f, &a) || !next(f, &b) || !next(f, &n)) return 3;
      uint8_t* d = new uint8_t[n + 1];
      for (long long i = 0; i <= n; ++i) {
        if (!next(f, &v)) return 3;
        d[i] = (uint8_t)v;
      }
      const size_t words = (size_t)(n + 16 + 3) / 4;
      uint32_t* w = new uint32_t[words]();
      const int bytes = png_deflate_chunk(d + 1, (int)n, (int)a, (int)b, w);
      if (bytes > n + 5) return 4;
      const uint8_t* o = reinterpret_cast<const uint8_t*>(w);
      printf("D ");
      for (int i = 0; i < bytes; ++i) printf("%02x", o[i]);
      printf("\n");
      delete[] d, delete[] w;
    } else if (kind[0] == 'K') {
      if (!next(f, &a) || !next(f, &n)) return 3;
      uint8_t* d = new uint8_t[n ? n : 1];
      for (long long i = 0; i < n; ++i) {
        if (!next(f, &v)) return 3;
        d[i] = (uint8_t)v;
      }
      uint32_t shares = 0, A = 1, B = 0;
      for (long long at = 0; at < n; at += a) {
        const long long m = n - at < a ? n - at : a;
        uint32_t raw = 0, pa = 0, pb = 0;
        for (long long i = 0; i < m; ++i) {
          raw = png_crc_entry((raw ^ d[at + i]) & 0xFFu) ^ (raw >> 8);
          pa = (pa + d[at + i]) % 65521u;
          pb = (uint32_t)((pb + (uint64_t)(m - i) * d[at + i]) % 65521u);
        }
        shares ^= png_crc_share(raw, n - at - m);
        png_adler_join(&A, &B, pa, pb, m);
      }
      const uint32_t crc = png_crc_finish(shares, n);
      if (crc != png_crc_bytes(d, n)) return 5;
      printf("K %u %u\n", crc, (B << 16) | A);
      delete[] d;
    } else {
      return 3;
    }
  }
  fclose(f);
  return 0;
}
