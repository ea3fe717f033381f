// Lossless frames: what csrc/png.hip's kernels and a host program both compile (the tests build tests/png_host_main.cpp from this file
// with the host compiler under sanitizers).  DESIGN.md section 5c, "Lossless frames: PNG", gives the format; tests/png_ref.py restates
// every routine here.
//
// The compressor is DEFLATE (RFC 1951) in a zlib wrapper (RFC 1950), deterministic and cut into chunks of PNG_CHUNK input bytes, one
// block per chunk:
//   parse    a position whose byte equals the byte before it (the previous chunk's last byte for a chunk's first position, nothing for
//            the stream's first) is a REPEAT.  A maximal span of L repeats inside a chunk is cut into matches of 258 (distance 1), then
//            one match of 3..257 or 1-2 literals (png_span_token).  Every other position is a literal.  zlib's Z_RLE parse.
//   lengths  the used symbols sorted by (count, index) (png_rank); a two-queue Huffman merge, the leaf queue first on equal weight; the
//            number of codes per depth, nodes past the limit held at it and folded back as zlib's gen_bitlen does; lengths handed
//            out along the sorted order, the longest to the rarest (png_code_lengths).  One used symbol gets length 1.
//   codes    canonical (RFC 1951 3.2.2), stored bit-reversed: the stream is packed from bit 0 up (png_canonical_codes)
//   header   HLIT = 257 or up to the last used symbol, HDIST = 1 with the one distance code 0 of length 1 whether or not the chunk
//            has a match (zlib's inflate takes that incomplete code), the lengths run-length coded greedily: a run of r zeros is
//            18 (138 at a time) while r >= 11, then 17 if r >= 3, then single zeros; a run of r equal lengths is the length once, then
//            16 (6 at a time) while the rest is >= 3, then single lengths.  The 19-symbol code is limited to 7 bits (png_header_*).
//   block    BTYPE = 10.  A block that is not the stream's last is followed by an empty stored block (3 bits, padding, 00 00 FF FF),
//            so every chunk is a whole number of bytes.  If that is longer than the stored form (5 + the chunk's bytes), the chunk is
//            a stored block (png_deflate_chunk, the serial form of csrc/png.hip's chunk kernel).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__
#else
#define PNG_HD
#endif

enum {
  PNG_CHUNK = 16384,       // input bytes per deflate block
  PNG_LITLEN = 286,        // literal / length symbols
  PNG_CLSYMS = 19,         // symbols of the code-length code
  PNG_MAX_BITS = 15,
  PNG_MAX_CL_BITS = 7,
  PNG_MAX_MATCH = 258,
  PNG_SEQ = PNG_LITLEN + 1 // the lengths the header carries at most: literal / length codes and the one distance code
};

// ---- bits: the stream is packed from the least significant bit of byte 0; words are little-endian ------------------------------
PNG_HD inline void png_put(uint32_t* w, long long pos, uint32_t v, int n) {      // n <= 32 bits of v at bit `pos` of a zeroed buffer
  const long long word = pos >> 5;
  const int sh = (int)(pos & 31);
  const uint64_t x = (uint64_t)v << sh;
  w[word] |= (uint32_t)x;
  if (sh + n > 32) w[word + 1] |= (uint32_t)(x >> 32);
}

// ---- parse ------------------------------------------------------------------------------------------------------------------------
// Position k of a span of L repeats: 0 = inside a match, 1 = a literal, 2 = a match of *len starts here.
PNG_HD inline int png_span_token(int k, int L, int* len) {
  const int k0 = k - k % PNG_MAX_MATCH, rest = L - k0, piece = rest < PNG_MAX_MATCH ? rest : PNG_MAX_MATCH;
  if (piece < 3) return 1;
  if (k != k0) return 0;
  *len = piece;
  return 2;
}

// RFC 1951 3.2.5: symbol, number of extra bits and their value for a match length 3..258
PNG_HD inline int png_length_symbol(int len, int* ebits, int* eval) {
  if (len == PNG_MAX_MATCH) {
    *ebits = 0, *eval = 0;
    return 285;
  }
  const int l = len - 3;
  int e = 0;
  while ((l >> (e + 3)) != 0) ++e;
  *ebits = e, *eval = l & ((1 << e) - 1);
  return 257 + 4 * e + (l >> e);
}

PNG_HD inline int png_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }

// ---- code lengths -----------------------------------------------------------------------------------------------------------------
// Place of symbol i among the used symbols in rising (count, index) order; -1 for an unused one.
PNG_HD inline int png_rank(const uint32_t* count, int n, int i) {
  const uint32_t c = count[i];
  if (c == 0) return -1;
  int r = 0;
  for (int j = 0; j < n; ++j) {
    const uint32_t d = count[j];
    r += (d != 0 && (d < c || (d == c && j < i))) ? 1 : 0;
  }
  return r;
}

// order[0 .. used) = the used symbols by png_rank; len[] must be zero on entry.  weight and parent hold 2 * used entries.
PNG_HD inline void png_code_lengths(const uint32_t* count, const int16_t* order, int used, int maxbits, uint8_t* len, uint32_t* weight,
                                    int16_t* parent) {
  if (used == 0) return;
  if (used == 1) {
    len[order[0]] = 1;
    return;
  }
  for (int i = 0; i < used; ++i) weight[i] = count[order[i]];
  int leaf = 0, inner = used;
  for (int next = used; next < 2 * used - 1; ++next) {
    uint32_t sum = 0;
    for (int k = 0; k < 2; ++k) {
      int pick;
      if (leaf < used && (inner >= next || weight[leaf] <= weight[inner])) pick = leaf++;
      else pick = inner++;
      sum += weight[pick];
      parent[pick] = (int16_t)next;
    }
    weight[next] = sum;
  }
  const int root = 2 * used - 2;
  weight[root] = 0;                                  // from here on weight[] holds depths
  int overflow = 0;                                  // nodes, inner ones too, that sat below the limit: each is held at it
  for (int node = root - 1; node >= 0; --node) {
    uint32_t d = weight[parent[node]] + 1;
    if (d > (uint32_t)maxbits) d = (uint32_t)maxbits, ++overflow;
    weight[node] = d;
  }
  int per[PNG_MAX_BITS + 1];
  for (int b = 0; b <= PNG_MAX_BITS; ++b) per[b] = 0;
  for (int i = 0; i < used; ++i) ++per[weight[i]];
  while (overflow > 0) {                             // zlib's gen_bitlen: a leaf one level down, an overflowing one beside it
    int bits = maxbits - 1;
    while (per[bits] == 0) --bits;
    --per[bits];
    per[bits + 1] += 2;
    --per[maxbits];
    overflow -= 2;
  }
  int at = 0;
  for (int bits = maxbits; bits >= 1; --bits)
    for (int c = 0; c < per[bits]; ++c) len[order[at++]] = (uint8_t)bits;
}

PNG_HD inline uint32_t png_reverse_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

PNG_HD inline void png_canonical_codes(const uint8_t* len, int n, uint16_t* code) {
  int per[PNG_MAX_BITS + 1], next[PNG_MAX_BITS + 2];
  for (int b = 0; b <= PNG_MAX_BITS; ++b) per[b] = 0;
  for (int i = 0; i < n; ++i) ++per[len[i]];
  per[0] = 0;
  int c = 0;
  next[0] = 0;
  for (int b = 1; b <= PNG_MAX_BITS; ++b) {
    c = (c + per[b - 1]) << 1;
    next[b] = c;
  }
  for (int i = 0; i < n; ++i) code[i] = len[i] ? (uint16_t)png_reverse_bits((uint32_t)next[len[i]]++, len[i]) : (uint16_t)0;
}

// ---- block header -----------------------------------------------------------------------------------------------------------------
struct PngHeader {
  int hlit, hclen, nsym, bits;                       // bits: HLIT .. the last coded length (without BFINAL / BTYPE)
  uint8_t seq[PNG_SEQ + 1];                          // the lengths: hlit literal / length codes, then the distance code's 1
  uint8_t sym[PNG_SEQ + 1], ext[PNG_SEQ + 1];        // the run-length coded form: symbol 0..18 and its extra value
  uint8_t cl_len[PNG_CLSYMS];
  uint16_t cl_code[PNG_CLSYMS];
};

PNG_HD inline int png_rle_lengths(const uint8_t* seq, int n, uint8_t* sym, uint8_t* ext) {
  int out = 0, i = 0;
  while (i < n) {
    const uint8_t v = seq[i];
    int run = 1;
    while (i + run < n && seq[i + run] == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int t = run < 138 ? run : 138;
        sym[out] = 18, ext[out++] = (uint8_t)(t - 11);
        run -= t;
      }
      if (run >= 3) {
        sym[out] = 17, ext[out++] = (uint8_t)(run - 3);
        run = 0;
      }
      for (; run > 0; --run) sym[out] = 0, ext[out++] = 0;
    } else {
      sym[out] = v, ext[out++] = 0;
      --run;
      while (run >= 3) {
        const int t = run < 6 ? run : 6;
        sym[out] = 16, ext[out++] = (uint8_t)(t - 3);
        run -= t;
      }
      for (; run > 0; --run) sym[out] = v, ext[out++] = 0;
    }
  }
  return out;
}

PNG_HD inline int png_cl_order(int i) {
  const uint8_t ord[PNG_CLSYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return ord[i];
}

PNG_HD inline void png_header_build(const uint8_t* len, PngHeader* h) {
  int hlit = PNG_LITLEN;
  while (hlit > 257 && len[hlit - 1] == 0) --hlit;
  h->hlit = hlit;
  for (int i = 0; i < hlit; ++i) h->seq[i] = len[i];
  h->seq[hlit] = 1;
  h->nsym = png_rle_lengths(h->seq, hlit + 1, h->sym, h->ext);
  uint32_t count[PNG_CLSYMS], weight[2 * PNG_CLSYMS];
  int16_t order[PNG_CLSYMS], parent[2 * PNG_CLSYMS];
  for (int i = 0; i < PNG_CLSYMS; ++i) count[i] = 0, h->cl_len[i] = 0;
  for (int i = 0; i < h->nsym; ++i) ++count[h->sym[i]];
  int used = 0;
  for (int i = 0; i < PNG_CLSYMS; ++i) {
    const int r = png_rank(count, PNG_CLSYMS, i);
    if (r >= 0) order[r] = (int16_t)i, ++used;
  }
  png_code_lengths(count, order, used, PNG_MAX_CL_BITS, h->cl_len, weight, parent);
  png_canonical_codes(h->cl_len, PNG_CLSYMS, h->cl_code);
  int hclen = PNG_CLSYMS;
  while (hclen > 4 && h->cl_len[png_cl_order(hclen - 1)] == 0) --hclen;
  h->hclen = hclen;
  int bits = 5 + 5 + 4 + 3 * hclen;
  for (int i = 0; i < PNG_CLSYMS; ++i) bits += (int)count[i] * (h->cl_len[i] + (i == 16 ? 2 : i == 17 ? 3 : i == 18 ? 7 : 0));
  h->bits = bits;
}

// BFINAL, BTYPE = 10 and the header at bit `pos`; returns the position after it
PNG_HD inline long long png_header_write(const PngHeader* h, int final, uint32_t* w, long long pos) {
  png_put(w, pos, (uint32_t)(final ? 1 : 0) | (2u << 1), 3), pos += 3;
  png_put(w, pos, (uint32_t)(h->hlit - 257), 5), pos += 5;
  png_put(w, pos, 0u, 5), pos += 5;
  png_put(w, pos, (uint32_t)(h->hclen - 4), 4), pos += 4;
  for (int i = 0; i < h->hclen; ++i) png_put(w, pos, h->cl_len[png_cl_order(i)], 3), pos += 3;
  for (int i = 0; i < h->nsym; ++i) {
    const int s = h->sym[i];
    png_put(w, pos, h->cl_code[s], h->cl_len[s]), pos += h->cl_len[s];
    const int e = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
    if (e) png_put(w, pos, h->ext[i], e), pos += e;
  }
  return pos;
}

// Bits of the dynamic block of a histogram (count[256] = 1 included) under `len`: BFINAL / BTYPE, header, tokens, one distance bit per
// match, the end-of-block code.
PNG_HD inline long long png_block_bits(const uint32_t* count, const uint8_t* len, const PngHeader* h) {
  long long bits = 3 + h->bits;
  for (int s = 0; s < PNG_LITLEN; ++s) bits += (long long)count[s] * (len[s] + (s > 256 ? png_extra_bits(s) + 1 : 0));
  return bits;
}

// Bytes of the chunk whose dynamic block takes `bits`: padded, and with the empty stored block behind it unless it ends the stream.
PNG_HD inline int png_dynamic_bytes(long long bits, int final) { return final ? (int)((bits + 7) >> 3) : (int)((bits + 3 + 7) >> 3) + 4; }

// The end of a dynamic chunk at bit `pos` (after the end-of-block code); returns the chunk's bytes.
PNG_HD inline int png_block_close(uint32_t* w, long long pos, int final) {
  if (final) return (int)((pos + 7) >> 3);
  pos += 3;                                          // BFINAL = 0, BTYPE = 00
  const long long at = ((pos + 7) >> 3) << 3;
  png_put(w, at, 0xFFFF0000u, 32);                   // LEN = 0, NLEN = FFFF
  return (int)(at >> 3) + 4;
}

// ---- CRC-32 (the PNG / zlib polynomial, reflected) and Adler-32 --------------------------------------------------------------------
PNG_HD inline uint32_t png_crc_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ 0xEDB88320u : i >> 1;
  return i;
}

// a(x) b(x) mod p(x), polynomials in the reflected form (x^0 = bit 31)
PNG_HD inline uint32_t png_gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m != 0; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}

PNG_HD inline uint32_t png_x8n(long long n) {       // x^(8 n) mod p(x)
  uint32_t r = 0x80000000u, p = 0x00800000u;
  for (; n; n >>= 1) {
    if (n & 1) r = png_gf_mul(p, r);
    p = png_gf_mul(p, p);
  }
  return r;
}

// The register of a piece of `after` bytes before the message's end, run from a zero register, as its share of the whole message's
// register: the shares of all pieces XOR to the register of the message run from zero.
PNG_HD inline uint32_t png_crc_share(uint32_t raw, long long after) { return png_gf_mul(png_x8n(after), raw); }
// CRC-32 of a message of n bytes from the XOR of its shares: the all-ones start register carried through n bytes, the final inversion
PNG_HD inline uint32_t png_crc_finish(uint32_t shares, long long n) { return shares ^ png_gf_mul(png_x8n(n), 0xFFFFFFFFu) ^ 0xFFFFFFFFu; }

PNG_HD inline uint32_t png_crc_bytes(const uint8_t* p, long long n) {        // serial, table-free: the few header bytes
  uint32_t c = 0xFFFFFFFFu;
  for (long long i = 0; i < n; ++i) c = png_crc_entry((c ^ p[i]) & 0xFFu) ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

// Adler-32 over pieces: a piece of n bytes d[i] is (a, b) = (sum d[i], sum (n - i) d[i]) mod 65521; A = 1, B = 0 before the first.
PNG_HD inline void png_adler_join(uint32_t* A, uint32_t* B, uint32_t a, uint32_t b, long long n) {
  *B = (uint32_t)((*B + (uint64_t)(n % 65521) * *A + b) % 65521u);
  *A = (*A + a) % 65521u;
}

// ---- one chunk, serially (the host's form of csrc/png.hip's chunk kernel) ---------------------------------------------------------
// d[0 .. n) is the chunk; d[-1] is read when has_prev.  w: zeroed words holding n + 16 bytes.  Returns the chunk's bytes.
inline int png_deflate_chunk(const uint8_t* d, int n, int has_prev, int final, uint32_t* w) {
  uint32_t count[PNG_LITLEN], weight[2 * PNG_LITLEN];
  int16_t order[PNG_LITLEN], parent[2 * PNG_LITLEN];
  uint8_t len[PNG_LITLEN];
  uint16_t code[PNG_LITLEN];
  PngHeader h;
  for (int s = 0; s < PNG_LITLEN; ++s) count[s] = 0, len[s] = 0;
  count[256] = 1;
  auto repeat = [&](int i) { return (i > 0 || has_prev) && d[i] == d[i - 1]; };
  for (int pass = 0; pass < 2; ++pass) {
    long long pos = 0;
    if (pass == 1) {
      int used = 0;
      for (int s = 0; s < PNG_LITLEN; ++s) {
        const int r = png_rank(count, PNG_LITLEN, s);
        if (r >= 0) order[r] = (int16_t)s, ++used;
      }
      png_code_lengths(count, order, used, PNG_MAX_BITS, len, weight, parent);
      png_canonical_codes(len, PNG_LITLEN, code);
      png_header_build(len, &h);
      if (png_dynamic_bytes(png_block_bits(count, len, &h), final) > n + 5) {
        uint8_t* o = reinterpret_cast<uint8_t*>(w);
        o[0] = (uint8_t)(final ? 1 : 0), o[1] = (uint8_t)(n & 255), o[2] = (uint8_t)(n >> 8), o[3] = (uint8_t)(~n & 255), o[4] = (uint8_t)((~n >> 8) & 255);
        for (int i = 0; i < n; ++i) o[5 + i] = d[i];
        return n + 5;
      }
      pos = png_header_write(&h, final, w, 0);
    }
    int i = 0;
    while (i < n) {
      if (!repeat(i)) {
        if (pass == 0) ++count[d[i]];
        else png_put(w, pos, code[d[i]], len[d[i]]), pos += len[d[i]];
        ++i;
        continue;
      }
      const int s = i;
      int e = i + 1;
      while (e < n && repeat(e)) ++e;
      for (; i < e; ++i) {
        int ml = 0;
        const int t = png_span_token(i - s, e - s, &ml);
        if (t == 1) {
          if (pass == 0) ++count[d[i]];
          else png_put(w, pos, code[d[i]], len[d[i]]), pos += len[d[i]];
        } else if (t == 2) {
          int eb, ev;
          const int sym = png_length_symbol(ml, &eb, &ev);
          if (pass == 0) ++count[sym];
          else {
            png_put(w, pos, code[sym], len[sym]), pos += len[sym];
            if (eb) png_put(w, pos, (uint32_t)ev, eb), pos += eb;
            pos += 1;                                // the distance code: one 0 bit
          }
        }
      }
    }
    if (pass == 1) {
      png_put(w, pos, code[256], len[256]), pos += len[256];
      return png_block_close(w, pos, final);
    }
  }
  return 0;
}
