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

// ---- decoding inside a segment in parallel: subsequences ------------------------------------------------------------------------------
// A segment is cut into subsequences at byte offsets (longlive_amd/jpeg_files.py: split_segments).  A baseline bit stream
// self-synchronises: a decoder started at a wrong state falls into step with the true one after a short distance, so every
// subsequence is scanned from a guess, then rescanned from its predecessor's exit until no exit changes (csrc/jpeg_dec.hip).
//
// State (JdState): a position and where the decoder stands in the MCU.
//   * off, bit: raw byte offset from the segment's start in the STUFFED data and the bit inside that byte, 0 = the highest.  The
//     position is canonical: `off` names a data byte that still holds an unread bit, or the first byte past the data, and never the
//     00 that follows an FF.  Equal stream positions therefore give equal states, and states compare with ==.
//   * bi: block index inside the MCU; k: the coefficient that comes next, 0 = the block's DC symbol.
//   * JD_STATE_END: the scan consumed a bit past the segment's data (the 1-bits the reader pads with).  It is terminal.
// An FF that no 00 follows (a marker, or the segment's last byte) ends the data there, as in jpeg_decode_segment.
//
// jd_sub_scan(entry, end) walks symbols (a Huffman code and its amplitude bits) from `entry` to the first symbol boundary at or past
// the byte offset `end`, writes no coefficient and returns the exit state; *begun = the blocks that BEGIN in the subsequence (their DC
// symbol starts before `end` and is read whole) | JD_SUB_DIRTY when it met one of the events below.
//
// Speculation policy: what the scan does where jpeg_decode_segment would stop with an error.  It is a function of (bytes, entry)
// alone, and every step consumes at least one bit or ends the scan, so a scan takes at most (bits from entry to end) + 32 steps.
//   no code in 16 bits, or a DC category above 11   the symbol's bits are put back, ONE bit is skipped, the state becomes (block 0, DC)
//   a run (or ZRL) that would pass coefficient 63   the code is consumed, its amplitude is not; the block ends there
//   run/size with size 0 that is not EOB or ZRL     taken as EOB
//   an AC size above 10                             decoded as it stands (a size is at most 15 bits)
//   a bit past the data is consumed                 the scan ends in JD_STATE_END; this is no event: the last subsequence of a valid
//                                                   segment ends so when the padding 1-bits are read as the start of a further block
// From a true state on valid data none of the first four can occur, so a subsequence whose final scan is dirty marks a segment that
// the serial routine has to decode (it alone owns the JD_* code and the zero-fill).
//
// jd_sub_emit(entry, count) follows the same path from a final entry state: it skips what is left of the block a predecessor began,
// then decodes `count` blocks (the scan's count), finishing the last one past the subsequence's end (a block is at most 208 bytes),
// and stores each whole with jd_copy_block at block `first + j`, clamped into [0, nblk) before the store.  stage[0] holds the DC
// DIFFERENCE: the running sum is a pass of its own.  Any event above, a consumed bit past the data included, ends it with a non-zero
// JD_* code; the caller then hands the segment to jpeg_decode_segment.
struct JdState {
  int32_t off, pack;     // pack = bit | bi << 3 | k << 6
};
constexpr int32_t JD_STATE_END_OFF = 0x7fffffff;
constexpr int32_t JD_SUB_DIRTY = 1 << 30;
constexpr int JD_SUB_FIELDS = 3;      // segment, byte offset inside the segment, byte length
constexpr int JD_SUB_MIN_BYTES = 7;   // a cut moved off a stuffing byte shortens the row after it by one: 8 - 1

JD_HD inline bool jd_state_eq(const JdState& a, const JdState& b) { return a.off == b.off && a.pack == b.pack; }

// Where BITS and HUFFVAL of the four tables lie: in the staged slice (jd_stage_tables) or in the packed tables of a frame.
struct JdTabs {
  const uint8_t* base;
  int bits_stride, dc_off, dc_stride, ac_off, ac_stride;
};
JD_HD inline JdTabs jd_tabs_slice(const uint8_t* slice) { return JdTabs{slice, 16, 64, 16, 96, 256}; }
JD_HD inline JdTabs jd_tabs_packed(const uint8_t* packed) {
  return JdTabs{packed, JD_HUFF_TABLE, 16, JD_HUFF_TABLE, 16 + 2 * JD_HUFF_TABLE, JD_HUFF_TABLE};
}

// The reader of the subsequence routines: JdBits' look-ahead (eight independent byte loads at a time, a 64-bit accumulator) over
// offsets, so that the position of the next unread bit can be told: every byte in the accumulator stands for one raw byte, or for
// two when it is an FF (its stuffed 00 went with it).
struct JdCur {
  const uint8_t* seg;
  int len, q;            // len: where the data ends; q: the next raw byte not yet in `raw`
  uint64_t raw, acc;
  int rn, cnt, pad;
};

JD_HD inline void jd_cur_load(JdCur& c) {
  const int left = c.len - c.q;
  const uint8_t* p = c.seg + c.q;
  uint64_t w = 0;
  if (left >= 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w |= (uint64_t)p[i] << (8 * i);
    c.rn = 8;
  } else {
    for (int i = 0; i < left; ++i) w |= (uint64_t)p[i] << (8 * i);
    c.rn = left;
  }
  c.raw = w;
  c.q += c.rn;
}

JD_HD inline void jd_cur_fill(JdCur& c) {
  while (c.cnt <= 56) {
    uint32_t v = 0xFF;
    if (c.rn == 0 && c.q < c.len) jd_cur_load(c);
    if (c.rn > 0) {
      v = (uint32_t)(c.raw & 0xFFu);
      if (v == 0xFF) {
        if (c.rn == 1 && c.q < c.len) {             // the byte after the FF is not loaded yet: load it behind the FF
          const int at = c.q - 1;
          c.q = at, c.rn = 0;
          jd_cur_load(c);
        }
        if (c.rn > 1 && ((c.raw >> 8) & 0xFFu) == 0) {
          c.raw >>= 16, c.rn -= 2;
        } else {                                    // a marker, or an FF as the last byte: the data ends before it
          c.len = c.q - c.rn, c.q = c.len, c.rn = 0;
          c.pad += 8;
        }
      } else {
        c.raw >>= 8, --c.rn;
      }
    } else {
      c.pad += 8;
    }
    c.acc = (c.acc << 8) | v;
    c.cnt += 8;
  }
}

// the canonical position of the next unread bit; only asked while no padding bit has been consumed (cnt >= pad)
JD_HD inline void jd_cur_position(const JdCur& c, int* off, int* bit) {
  int o = c.q - c.rn;
  const int nb = (c.cnt + 7) >> 3;
  for (int j = c.pad >> 3; j < nb; ++j) o -= 1 + (int)(((c.acc >> (8 * j)) & 0xFFu) == 0xFFu);
  *off = o;
  *bit = (8 - (c.cnt & 7)) & 7;
}

// the next 16 bits, not consumed
JD_HD inline int jd_cur_peek16(JdCur& c) {
  if (c.cnt < 16) jd_cur_fill(c);
  return (int)((c.acc >> (c.cnt - 16)) & 0xFFFFu);
}

// consumes n bits (0..16); false when one of them lies past the data
JD_HD inline bool jd_cur_drop(JdCur& c, int n) {
  if (c.cnt < n) jd_cur_fill(c);
  c.cnt -= n;
  return c.cnt >= c.pad;
}

// (symbol << 8) | code length of the code that heads the 16 bits v, or -1
JD_HD inline int jd_lookup(int v, const uint8_t* bits, const uint8_t* vals, int mask) {
  const uint32_t* bw = reinterpret_cast<const uint32_t*>(bits);
  const uint32_t w[4] = {bw[0], bw[1], bw[2], bw[3]};
  int first = 0, k = 0;
#pragma unroll
  for (int l = 0; l < 16; ++l) {
    const int n = (int)((w[l >> 2] >> (8 * (l & 3))) & 0xFFu), code = v >> (15 - l);
    if (code - first < n) return ((int)vals[(k + code - first) & mask] << 8) | (l + 1);
    k += n;
    first = (first + n) << 1;
  }
  return -1;
}

// The one walk that jd_sub_scan and jd_sub_emit share, so that both follow the same path by construction.
template <bool EMIT>
JD_HD inline int jd_sub_walk(const uint8_t* seg, int seglen, const JdTabs& tb, uint32_t sel, int bpm, int end, JdState in, JdState* exit,
                             int32_t* begun, int count, long long first, long long nblk, int16_t* stage, int16_t* out) {
  const int ny = bpm == 1 ? 1 : bpm - 2;
  int bi = (in.pack >> 3) & 7, k = (in.pack >> 6) & 63, nbegun = 0, dirty = 0, stored = 0;
  bool storing = k == 0;
  if (bi >= bpm) bi = 0;
  if (!EMIT) {
    *begun = 0;
    *exit = in;
    if (in.off >= end) return JD_OK;                // the predecessor's last symbol passed this subsequence whole (JD_STATE_END too)
  } else if (count <= 0) {
    return JD_OK;
  }
  if (in.off < 0 || in.off > seglen) return JD_OVERRUN;      // no state of this segment: nothing is read
  JdCur c{seg, seglen, in.off, 0ull, 0ull, 0, 0, 0};
  if (!jd_cur_drop(c, in.pack & 7)) {
    if (!EMIT) *exit = JdState{JD_STATE_END_OFF, 0};
    return JD_OVERRUN;
  }
  for (;;) {
    if (!EMIT) {                                    // a symbol boundary: at or past the end?
      const int nb = (c.cnt + 7) >> 3;
      if (c.q - c.rn - nb + (c.pad >> 3) >= end) {
        int off, bit;
        jd_cur_position(c, &off, &bit);
        if (off >= end) {
          *exit = JdState{off, bit | (bi << 3) | (k << 6)};
          break;
        }
      }
    } else if (k == 0 && storing && stored >= count) {
      break;
    }
    const int comp = bi < ny ? 0 : bi - ny + 1;
    const uint32_t s8 = (sel >> (8 * comp)) & 0xFFu;
    const int td = (int)(s8 & 1u), ta = (int)((s8 >> 4) & 1u);
    int code = 0;                                   // the JD_* event of this step, 0 = none
    bool over = false, endblk = false, resync = false;
    if (k == 0) {
      const int sl = jd_lookup(jd_cur_peek16(c), tb.base + td * tb.bits_stride, tb.base + tb.dc_off + td * tb.dc_stride, 15);
      const int s = sl >> 8;
      if (sl < 0) {
        if (c.cnt - c.pad < 16) over = true;
        else code = JD_BAD_CODE, resync = true;
      } else if (c.cnt - c.pad < (sl & 255)) {
        over = true;
      } else if (s > 11) {
        code = JD_DC_CATEGORY, resync = true;
      } else {
        jd_cur_drop(c, sl & 255);
        int diff = 0;
        if (s > 0) {
          const int v = jd_cur_peek16(c) >> (16 - s);
          if (!jd_cur_drop(c, s)) over = true;
          diff = jd_extend(v, s);
        }
        if (!over) {
          ++nbegun;
          if (EMIT && storing) {
            jd_zero_block(stage);
            stage[0] = (int16_t)diff;
          }
          k = 1;
        }
      }
    } else {
      const int sl = jd_lookup(jd_cur_peek16(c), tb.base + (2 + ta) * tb.bits_stride, tb.base + tb.ac_off + ta * tb.ac_stride, 255);
      if (sl < 0) {
        if (c.cnt - c.pad < 16) over = true;
        else code = JD_BAD_CODE, resync = true;
      } else if (!jd_cur_drop(c, sl & 255)) {
        over = true;
      } else {
        const int rs = sl >> 8, r = rs >> 4, s = rs & 15;
        if (s == 0) {
          if (r == 0) endblk = true;                // EOB
          else if (r != 15) code = JD_AC_SIZE, endblk = true;
          else if (k + 16 > 64) code = JD_COEF_INDEX, endblk = true;
          else k += 16;                             // ZRL
        } else {
          if (s > 10) code = JD_AC_SIZE;
          if (k + r > 63) {
            if (!code) code = JD_COEF_INDEX;
            endblk = true;
          } else {
            const int v = jd_cur_peek16(c) >> (16 - s);
            if (!jd_cur_drop(c, s)) over = true;
            else {
              k += r;
              if (EMIT && storing) stage[k] = (int16_t)jd_extend(v, s);
              ++k;
            }
          }
        }
        if (k >= 64) endblk = true;
      }
    }
    if (over) {
      if (!EMIT) *exit = JdState{JD_STATE_END_OFF, 0};
      if (EMIT) return JD_OVERRUN;
      break;
    }
    if (code) {
      if (EMIT) return code;
      dirty = JD_SUB_DIRTY;
    }
    if (resync) {
      jd_cur_drop(c, 1);                            // at least 16 bits of data lie ahead: this cannot pass the end
      bi = 0, k = 0;
      storing = true;
    } else if (endblk) {
      if (EMIT) {
        if (storing) {
          long long b = first + stored;
          b = b < 0 ? 0 : (b > nblk - 1 ? nblk - 1 : b);
          jd_copy_block(out + b * 64, stage);
          ++stored;
        }
        storing = true;
      }
      bi = bi + 1 == bpm ? 0 : bi + 1;
      k = 0;
    }
  }
  if (!EMIT) *begun = nbegun | dirty;
  return JD_OK;
}

JD_HD inline JdState jd_sub_scan(const uint8_t* seg, int seglen, const JdTabs& tb, uint32_t sel, int bpm, int end, JdState in,
                                 int32_t* begun) {
  JdState exit;
  jd_sub_walk<false>(seg, seglen, tb, sel, bpm, end, in, &exit, begun, 0, 0, 0, nullptr, nullptr);
  return exit;
}

// out: the segment's first block; first: the index (inside the segment) of the first block that begins in this subsequence
JD_HD inline int jd_sub_emit(const uint8_t* seg, int seglen, const JdTabs& tb, uint32_t sel, int bpm, JdState in, int count,
                             long long first, long long nblk, int16_t* stage, int16_t* out) {
  if (nblk < 1) return JD_OK;
  return jd_sub_walk<true>(seg, seglen, tb, sel, bpm, 0, in, nullptr, nullptr, count, first, nblk, stage, out);
}
