/* Animated previews: the GIF entry points of liblonglive_hip.so ("Animated previews: GIF").  They are part of
 * ABI version 111 (LL_ABI_VERSION in longlive_hip.h) and follow its conventions: 0 on success, LL_ERR_* otherwise with the message in
 * ll_last_error(); every argument is checked before anything is launched; launches go to `stream` and nothing is read back; scratch
 * may hold anything on entry.  longlive_amd/gif.py binds them.
 *
 * palette: 0 = one table for all T frames of the call ("clip"), 1 = one per frame ("frame").
 * dither:  0 = none, 1 = 8 x 8 ordered ("bayer"). */
#ifndef LONGLIVE_GIF_H
#define LONGLIVE_GIF_H

#include "longlive_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  out_stride: bytes per frame of ll_gif_encode_u8's `out` (the worst case of a frame's file); scratch_bytes: what
 * ll_gif_encode_u8 and ll_gif_quantize_u8 need for T frames of H x W under `palette`. */
int ll_gif_sizes(int T, int H, int W, int palette, long long* out_stride, long long* scratch_bytes);

/* frames: uint8 RGB [T, H, W, 3], each frame contiguous, stride_t bytes apart.  out + t * out_stride receives frame t's complete
 * single-image GIF89a file (local colour table of 256, LZW in independently coded chunks of 3584 pixels), sizes[t] its length. */
int ll_gif_encode_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, int palette, int dither, uint8_t* out,
                     long long out_stride, int32_t* sizes, void* scratch, long long scratch_bytes, ll_stream stream);

/* The encoder's first stages alone: indices uint8 [T, H, W], palettes uint8 [T or 1, 256, 3] (entries past the used ones are 0),
 * used int32 [T or 1]. */
int ll_gif_quantize_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, int palette, int dither, uint8_t* indices,
                       uint8_t* palettes, int32_t* used, void* scratch, long long scratch_bytes, ll_stream stream);

/* The coder alone: T rows of n 8-bit indices, `stride` bytes apart -> out + t * out_stride receives row t's LZW stream (Clear, the
 * chunks' codes, EOI; before sub-blocking), sizes[t] its bytes. */
int ll_gif_lzw_sizes(int T, long long n, long long* out_stride, long long* scratch_bytes);
int ll_gif_lzw_u8(const uint8_t* rows, long long stride, int T, long long n, uint8_t* out, long long out_stride, int32_t* sizes,
                  void* scratch, long long scratch_bytes, ll_stream stream);

#ifdef __cplusplus
}
#endif
#endif
