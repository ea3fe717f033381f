// Stand-alone host program over csrc/jpeg_dec.h (built by tests/test_clip_gpu_intake_host.py with the host compiler and
// -fsanitize=address,undefined): runs jpeg_decode_segment on every case of an input file and writes what it returned.
//
// Input:  u32 ncases, then per case: u32 flags (1 = write the coefficients), u32 sel, i32 mcus, i32 bpm, i32 length,
//         1088 bytes of packed tables, `length` bytes of segment data.
// Output: per case: i32 status, i32 whole, i32 done, then mcus * bpm * 64 int16 when flags & 1.  done = the blocks the routine
//         reports as decoded whole.  whole = 1 when done is mcus * bpm exactly on success and less on a failure, no block before
//         `done` still holds the guard value, and every sample of every block from `done` on is zero.
// Data, table slice, staging block and output live in heap blocks of their exact sizes, so any access outside them is the
// sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_dec.h"

static bool take(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint32_t ncases = 0;
  if (!take(in, &ncases, 4)) return 2;
  for (uint32_t i = 0; i < ncases; ++i) {
    uint32_t flags = 0, sel = 0;
    int32_t mcus = 0, bpm = 0, length = 0;
    if (!take(in, &flags, 4) || !take(in, &sel, 4) || !take(in, &mcus, 4) || !take(in, &bpm, 4) || !take(in, &length, 4)) return 2;
    if (mcus < 1 || bpm < 1 || bpm > 6 || length < 0) return 2;
    uint32_t* packed = static_cast<uint32_t*>(malloc(JD_HUFF_FRAME));
    uint8_t* data = static_cast<uint8_t*>(malloc(length > 0 ? length : 1));
    uint32_t* slice = static_cast<uint32_t*>(malloc(JD_SLICE));
    const size_t n = (size_t)mcus * bpm * 64;
    int16_t* coef = static_cast<int16_t*>(aligned_alloc(16, n * 2));
    int16_t* stage = static_cast<int16_t*>(aligned_alloc(16, 128));
    if (!packed || !data || !slice || !coef || !stage) return 2;
    if (!take(in, packed, JD_HUFF_FRAME) || !take(in, data, (size_t)length)) return 2;
    for (size_t k = 0; k < n; ++k) coef[k] = 0x7FFF;
    jd_stage_tables(packed, slice);
    // length 0: an empty range at the end of the 1-byte block
    long long done = -1;
    const int32_t status = jpeg_decode_segment(length > 0 ? data : data + 1, length, reinterpret_cast<const uint8_t*>(slice), sel, mcus, bpm,
                                               stage, coef, &done);
    const long long nblk = (long long)mcus * bpm;
    int32_t whole = status == 0 ? done == nblk : (done >= 0 && done < nblk);
    for (size_t k = 0; whole && k < n; ++k) {
      if ((long long)(k >> 6) < done) {
        if ((k & 63) != 0 && coef[k] == 0x7FFF) whole = 0;     // an AC position never decodes to 0x7FFF (10 bits at most)
      } else if (coef[k] != 0) {
        whole = 0;
      }
    }
    const int32_t done32 = (int32_t)done;
    fwrite(&status, 4, 1, out);
    fwrite(&whole, 4, 1, out);
    fwrite(&done32, 4, 1, out);
    if (flags & 1) fwrite(coef, 2, n, out);
    free(packed), free(data), free(slice), free(coef), free(stage);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
