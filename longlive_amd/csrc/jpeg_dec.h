// Clip intake: the entropy decoder of one restart segment of a baseline JPEG scan (ITU T.81 F.2.2), as plain C++ that compiles for
// the GPU (csrc/jpeg_dec.hip, one lane per segment) and for the CPU (tests build it with the host compiler under sanitizers).
//
// Contract of jpeg_decode_segment:
//   * bytes are read from [data, data + length) only; past the end the reader sees 1-bits, and a segment that consumes one fails
//     with JD_OVERRUN; `slice` is 4-byte aligned
//   * blocks are written to [out, out + mcus * bpm * 64) only, each one whole (zeros included, 128 aligned bytes at a time), so
//     `out` may hold anything on entry; the block being decoded lives in `stage`, 64 int16 of the caller's
//   * every loop is bounded: a symbol takes at most 16 bits, a block at most 64 symbols, a segment mcus * bpm blocks
//   * on an invalid code, a coefficient index above 63, a DC category above 11 or an AC size above 10 it stops, zero-fills the block
//     it was in and every later block of the segment, and returns a non-zero JD_* code
// Tables: canonical codes walked length by length over BITS (first code of a length, count of that length: Annex F.2.2.3 without the
// derived MAXCODE / VALPTR arrays) against a 16-bit look-ahead, so a table is BITS + HUFFVAL, nothing has to be built before the
// first symbol, and a symbol costs one read of BITS (four words), a loop in registers and one read of HUFFVAL.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JD_HD __host__ __device__
#else
#define JD_HD
#endif

enum {
  JD_OK = 0,
  JD_OVERRUN = 1,       // the segment's bytes ran out
  JD_BAD_CODE = 2,      // 16 bits without a Huffman code
  JD_DC_CATEGORY = 3,   // DC category above 11
  JD_AC_SIZE = 4,       // AC size above 10, or a run with size 0 that is neither EOB nor ZRL
  JD_COEF_INDEX = 5,    // a run that passes coefficient 63
  JD_MARKER = 6,        // FF followed by anything but 00 inside the segment
  JD_BAD_SEGMENT = 7,   // a row of the segment table that points outside the data, the frames or the frame's MCUs
  JD_DC_RANGE = 8       // a DC value outside int16
};

// The packed tables of one frame: 4 x (BITS[16], HUFFVAL[256]) = DC id 0, DC id 1, AC id 0, AC id 1.
constexpr int JD_HUFF_TABLE = 272;
constexpr int JD_HUFF_FRAME = 4 * JD_HUFF_TABLE;
// The slice the decoder reads: the four BITS lists (64 bytes), 16 values per DC table (32 bytes), 256 per AC table (512 bytes).
constexpr int JD_SLICE = 608;
constexpr int JD_SEG_FIELDS = 5;      // byte offset, byte length, frame, first MCU, MCU count

// slice <- packed tables, as 32-bit words (both are 4-byte aligned)
JD_HD inline void jd_stage_tables(const uint32_t* packed, uint32_t* slice) {
  for (int tb = 0; tb < 4; ++tb) {
    const uint32_t* src = packed + tb * (JD_HUFF_TABLE / 4);
    for (int i = 0; i < 4; ++i) slice[tb * 4 + i] = src[i];
    const int n = tb < 2 ? 4 : 64;
    uint32_t* dst = slice + (tb < 2 ? 16 + tb * 4 : 24 + (tb - 2) * 64);
    for (int i = 0; i < n; ++i) dst[i] = src[4 + i];
  }
}

JD_HD inline bool jd_row_ok(const int32_t* row, long long nbytes, int T, long long mcus_per_frame) {
  const long long off = row[0], len = row[1], first = row[3], count = row[4];
  return off >= 0 && len >= 0 && off + len <= nbytes && row[2] >= 0 && row[2] < T && first >= 0 && count >= 1 &&
         first + count <= mcus_per_frame;
}

// The bit reader looks ahead: up to 8 raw bytes are loaded at once (independent loads: one memory latency per 8 bytes, never past
// `end`), and the accumulator holds up to 64 bits.  What lies past the data enters as 1-bits and is counted in `pad`; only CONSUMING
// such a bit is an error (JD_OVERRUN, or JD_MARKER when the data ended at an FF that no 00 follows).
struct JdBits {
  const uint8_t* p;      // the next raw byte not yet in `raw`
  const uint8_t* end;
  uint64_t raw, acc;     // raw: rn bytes, the next one lowest; acc: cnt bits, the next one highest
  int rn, cnt, pad, err, enderr;
};

JD_HD inline void jd_load(JdBits& b) {
  const long long left = b.end - b.p;
  uint64_t w = 0;
  if (left >= 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w |= (uint64_t)b.p[i] << (8 * i);
    b.rn = 8;
  } else {
    for (int i = 0; i < (int)left; ++i) w |= (uint64_t)b.p[i] << (8 * i);
    b.rn = (int)left;
  }
  b.raw = w;
  b.p += b.rn;
}

// tops the accumulator up to more than 56 bits; FF 00 is one FF, any other FF ends the data
JD_HD inline void jd_fill(JdBits& b) {
  while (b.cnt <= 56) {
    uint32_t v = 0xFF;
    if (b.rn == 0 && b.p < b.end) jd_load(b);
    if (b.rn > 0) {
      v = (uint32_t)(b.raw & 0xFFu);
      b.raw >>= 8, --b.rn;
      if (v == 0xFF) {
        if (b.rn == 0 && b.p < b.end) jd_load(b);
        if (b.rn > 0 && (b.raw & 0xFFu) == 0) {
          b.raw >>= 8, --b.rn;
        } else {                                    // a marker, or an FF as the last byte: not data
          b.enderr = JD_MARKER;
          b.p = b.end, b.rn = 0;
          b.pad += 8;
        }
      }
    } else {
      b.pad += 8;
    }
    b.acc = (b.acc << 8) | v;
    b.cnt += 8;
  }
}

JD_HD inline void jd_skip(JdBits& b, int n) {
  b.cnt -= n;
  if (b.cnt < b.pad) {
    if (!b.err) b.err = b.enderr;
    b.pad = b.cnt;
  }
}

// n = 1..16
JD_HD inline int jd_bits(JdBits& b, int n) {
  if (b.cnt < n) jd_fill(b);
  const int v = (int)((b.acc >> (b.cnt - n)) & ((1u << n) - 1u));
  jd_skip(b, n);
  return v;
}

// the next symbol of a table, or -1 (16 bits consumed); bits = the table's BITS list as four words, lengths 1..4 in the first, the
// lowest byte first; `mask` keeps the index inside the slice whatever BITS holds
JD_HD inline int jd_symbol(JdBits& b, const uint32_t* bits, const uint8_t* vals, int mask) {
  if (b.cnt < 16) jd_fill(b);
  const int v = (int)((b.acc >> (b.cnt - 16)) & 0xFFFFu);
  const uint32_t w[4] = {bits[0], bits[1], bits[2], bits[3]};
  int first = 0, k = 0;
#pragma unroll
  for (int l = 0; l < 16; ++l) {
    const int n = (int)((w[l >> 2] >> (8 * (l & 3))) & 0xFFu), code = v >> (15 - l);
    if (code - first < n) {
      jd_skip(b, l + 1);
      return vals[(k + code - first) & mask];
    }
    k += n;
    first = (first + n) << 1;
  }
  jd_skip(b, 16);
  return -1;
}

// T.81 F.2.2.1 EXTEND: the s-bit amplitude v as a signed value
JD_HD inline int jd_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One block is decoded into `stage` (64 int16 the caller owns: an LDS slice on the GPU) and leaves as 128 aligned bytes: eight wide
// stores per block where scattered 2-byte stores would each be a partial line of their own.
JD_HD inline void jd_copy_block(int16_t* dst, const int16_t* src) {
  __builtin_memcpy(__builtin_assume_aligned(dst, 16), __builtin_assume_aligned(src, 16), 128);
}

JD_HD inline void jd_zero_block(int16_t* dst) { __builtin_memset(__builtin_assume_aligned(dst, 16), 0, 128); }

// sel: byte c = (AC table id << 4) | DC table id of component c.  bpm = blocks per MCU: 1 (grey) or h * v + 2, chroma last.
// slice: 4-byte aligned; stage and out: 16-byte aligned.  *done (when given) = the blocks decoded whole: mcus * bpm on success, else
// the index of the block the failure fell in, the first of the zero-filled ones.
JD_HD inline int jpeg_decode_segment(const uint8_t* data, long long length, const uint8_t* slice, uint32_t sel, int mcus, int bpm,
                                     int16_t* stage, int16_t* out, long long* done = nullptr) {
  JdBits b{data, data + (length > 0 ? length : 0), 0ull, 0ull, 0, 0, 0, 0, JD_OVERRUN};
  const uint32_t* words = reinterpret_cast<const uint32_t*>(slice);
  const long long nblk = (long long)mcus * bpm;
  const int ny = bpm == 1 ? 1 : bpm - 2;
  int p0 = 0, p1 = 0, p2 = 0, err = 0, bi = 0;
  long long blk = 0;
  for (; blk < nblk; ++blk) {
    const int c = bi < ny ? 0 : bi - ny + 1;
    bi = bi + 1 == bpm ? 0 : bi + 1;
    const uint32_t s8 = (sel >> (8 * c)) & 0xFFu;
    const int td = (int)(s8 & 1u), ta = (int)((s8 >> 4) & 1u);
    jd_zero_block(stage);
    int s = jd_symbol(b, words + 4 * td, slice + 64 + 16 * td, 15);
    if (b.err) { err = b.err; break; }
    if (s < 0) { err = JD_BAD_CODE; break; }
    if (s > 11) { err = JD_DC_CATEGORY; break; }
    int pred = c == 0 ? p0 : (c == 1 ? p1 : p2);
    if (s > 0) {
      pred += jd_extend(jd_bits(b, s), s);
      if (b.err) { err = b.err; break; }
      if (pred < -32768 || pred > 32767) { err = JD_DC_RANGE; break; }
    }
    if (c == 0) p0 = pred;
    else if (c == 1) p1 = pred;
    else p2 = pred;
    stage[0] = (int16_t)pred;
    int k = 1;
    while (k < 64) {
      const int rs = jd_symbol(b, words + 8 + 4 * ta, slice + 96 + 256 * ta, 255);
      if (b.err) { err = b.err; break; }
      if (rs < 0) { err = JD_BAD_CODE; break; }
      const int r = rs >> 4;
      s = rs & 15;
      if (s == 0) {
        if (r == 0) break;                          // EOB
        if (r != 15) { err = JD_AC_SIZE; break; }
        if (k + 16 > 64) { err = JD_COEF_INDEX; break; }
        k += 16;                                    // ZRL
        continue;
      }
      if (s > 10) { err = JD_AC_SIZE; break; }
      k += r;
      if (k > 63) { err = JD_COEF_INDEX; break; }
      const int v = jd_extend(jd_bits(b, s), s);
      if (b.err) { err = b.err; break; }
      stage[k++] = (int16_t)v;
    }
    if (err) break;
    jd_copy_block(out + blk * 64, stage);
  }
  if (done) *done = blk;
  if (err)
    for (; blk < nblk; ++blk) jd_zero_block(out + blk * 64);
  return err;
}
