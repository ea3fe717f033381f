// Stand-alone host program over csrc/jpeg_dec.h (built by tests/test_jpeg_split_host.py with the host compiler and
// -fsanitize=address,undefined): plays the passes of the split entropy route (csrc/jpeg_dec.hip) in plain loops over one segment per
// case -- row check, pass 0, the rounds with ping-pong exits, block scan, emit, DC pass, fallback -- next to jpeg_decode_segment on
// the same bytes, and writes what both gave.
//
// Input:  u32 ncases, then per case: u32 flags (1 = write the coefficients), u32 sel, i32 mcus, i32 bpm, i32 length, i32 rounds,
//         i32 nrows, 1088 bytes of packed tables, `length` bytes of segment data, nrows x (i32 offset, i32 length).
// Output: per case: i32 same, i32 status, i32 done, i32 info, then mcus * bpm * 64 int16 of the split route when flags & 1.
//         same = 1 when coefficients (every sample of the segment), status and the `done` index of the split route equal
//         jpeg_decode_segment's.  info: r >= 1 settled in round r, -1 fell back unsettled, -2 fell back flagged.
// Data, tables, staging block, states, counts and both outputs live in heap blocks of their exact sizes, so an access outside the
// segment's bytes or blocks is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_dec.h"

static bool take(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

template <typename T>
static T* block(size_t n) {
  return static_cast<T*>(aligned_alloc(16, n * sizeof(T)));      // whole blocks of 128 bytes: a multiple of the alignment
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint32_t ncases = 0;
  if (!take(in, &ncases, 4)) return 2;
  for (uint32_t i = 0; i < ncases; ++i) {
    uint32_t flags = 0, sel = 0;
    int32_t mcus = 0, bpm = 0, length = 0, rounds = 0, nrows = 0;
    if (!take(in, &flags, 4) || !take(in, &sel, 4) || !take(in, &mcus, 4) || !take(in, &bpm, 4) || !take(in, &length, 4) ||
        !take(in, &rounds, 4) || !take(in, &nrows, 4))
      return 2;
    if (mcus < 1 || bpm < 1 || bpm > 6 || length < 0 || rounds < 1 || rounds > 64 || nrows < 1) return 2;
    uint32_t* packed = static_cast<uint32_t*>(malloc(JD_HUFF_FRAME));
    uint8_t* data = static_cast<uint8_t*>(malloc(length > 0 ? length : 1));
    uint32_t* slice = static_cast<uint32_t*>(malloc(JD_SLICE));
    int32_t* rows = static_cast<int32_t*>(malloc((size_t)nrows * 8));
    const long long nblk = (long long)mcus * bpm;
    const size_t n = (size_t)nblk * 64;
    int16_t* ref = block<int16_t>(n);
    int16_t* coef = block<int16_t>(n);
    int16_t* stage = block<int16_t>(64);
    JdState* exits[2] = {static_cast<JdState*>(malloc((size_t)nrows * 8)), static_cast<JdState*>(malloc((size_t)nrows * 8))};
    JdState* entry = static_cast<JdState*>(malloc((size_t)nrows * 8));
    int32_t* count = static_cast<int32_t*>(malloc((size_t)nrows * 4));
    int32_t* base = static_cast<int32_t*>(malloc((size_t)nrows * 4));
    if (!packed || !data || !slice || !rows || !ref || !coef || !stage || !exits[0] || !exits[1] || !entry || !count || !base) return 2;
    if (!take(in, packed, JD_HUFF_FRAME) || !take(in, data, (size_t)length) || !take(in, rows, (size_t)nrows * 8)) return 2;
    for (size_t k = 0; k < n; ++k) ref[k] = coef[k] = 0x7FFF;
    jd_stage_tables(packed, slice);
    const uint8_t* seg = length > 0 ? data : data + 1;           // length 0: an empty range at the end of the 1-byte block
    const uint8_t* sl = reinterpret_cast<const uint8_t*>(slice);
    long long ref_done = -1;
    const int32_t ref_status = jpeg_decode_segment(seg, length, sl, sel, mcus, bpm, stage, ref, &ref_done);

    // the split route; odd cases read the packed tables where they lie, even ones the staged slice
    const JdTabs tb = (i & 1) ? jd_tabs_packed(reinterpret_cast<const uint8_t*>(packed)) : jd_tabs_slice(sl);
    int32_t info = 0;
    bool flagged = false;
    for (int r = 0; r < nrows; ++r) {                             // the row check of pass 0
      const long long off = rows[2 * r], len = rows[2 * r + 1];
      bool ok = off >= 0 && len >= JD_SUB_MIN_BYTES && off + len <= length;
      ok = ok && (r == 0 ? off == 0 : (long long)rows[2 * r - 2] + rows[2 * r - 1] == off);
      if (r == nrows - 1) ok = ok && off + len == length;
      if (!ok) flagged = true;
    }
    int last_change = 0;
    if (!flagged) {
      for (int r = 0; r < nrows; ++r) {                           // pass 0
        entry[r] = JdState{rows[2 * r], 0};
        exits[0][r] = jd_sub_scan(seg, length, tb, sel, bpm, rows[2 * r] + rows[2 * r + 1], entry[r], &count[r]);
      }
      for (int round = 1; round <= rounds; ++round) {
        JdState* rd = exits[(round + 1) & 1];
        JdState* wr = exits[round & 1];
        for (int r = 0; r < nrows; ++r) {
          const JdState e = r == 0 ? entry[0] : rd[r - 1];
          if (r == 0 || jd_state_eq(e, entry[r])) {
            wr[r] = rd[r];
            continue;
          }
          int32_t begun = 0;
          const JdState x = jd_sub_scan(seg, length, tb, sel, bpm, rows[2 * r] + rows[2 * r + 1], e, &begun);
          if (!jd_state_eq(x, rd[r])) last_change = round;
          entry[r] = e, wr[r] = x, count[r] = begun;
        }
      }
      if (last_change >= rounds) {
        info = -1;
      } else {
        long long total = 0;
        int dirty = 0;
        for (int r = 0; r < nrows; ++r) {                         // block scan
          base[r] = (int32_t)(total > 0x7fffffffll ? 0x7fffffffll : total);
          total += count[r] & (JD_SUB_DIRTY - 1);
          dirty |= count[r] & JD_SUB_DIRTY;
        }
        flagged = dirty || total != nblk;
        for (int r = 0; r < nrows && !flagged; ++r)               // emit
          if (jd_sub_emit(seg, length, tb, sel, bpm, entry[r], count[r] & (JD_SUB_DIRTY - 1), base[r], nblk, stage, coef)) flagged = true;
        if (!flagged) {                                           // DC pass
          const int ny = bpm == 1 ? 1 : bpm - 2;
          long long p[3] = {0, 0, 0};
          for (long long b = 0; b < nblk; ++b) {
            const int bi = (int)(b % bpm), c = bi < ny ? 0 : bi - ny + 1;
            p[c] += coef[b * 64];
            if (p[c] < -32768 || p[c] > 32767) flagged = true;
            coef[b * 64] = (int16_t)p[c];
          }
        }
        if (!flagged) info = last_change + 1;
      }
    }
    if (flagged) info = -2;
    int32_t status = 0;
    long long done = nblk;
    if (info < 0) status = jpeg_decode_segment(seg, length, sl, sel, mcus, bpm, stage, coef, &done);      // fallback
    const int32_t same = status == ref_status && done == ref_done && memcmp(coef, ref, n * 2) == 0;
    const int32_t done32 = (int32_t)done;
    fwrite(&same, 4, 1, out);
    fwrite(&status, 4, 1, out);
    fwrite(&done32, 4, 1, out);
    fwrite(&info, 4, 1, out);
    if (flags & 1) fwrite(coef, 2, n, out);
    free(packed), free(data), free(slice), free(rows), free(ref), free(coef), free(stage), free(exits[0]), free(exits[1]), free(entry),
        free(count), free(base);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
