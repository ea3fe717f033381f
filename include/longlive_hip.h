/*
 * longlive_hip.h -- C ABI of liblonglive_hip.so: the MI355X (gfx950) native replacement for the per-frame
 * denoising hot path of LongLive (reference: kpham-augment/LongLive).
 *
 * The reference has no FFI/plugin registry: its "operator API" on this path is the set of PyTorch module calls made
 * inside CausalWanModel._forward_inference.  Each entry point below replaces one of those call sites (file:line of
 * the reference is cited per function); the Python host layer (longlive_amd/) mirrors the reference's Python
 * interface on top of this ABI.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch allocation); bf16 tensors are `uint16_t` bit patterns;
 *   - every function is asynchronous on `stream` (a hipStream_t passed as void*), never allocates, never syncs;
 *   - every function returns 0 on success, a negative ll_status otherwise; ll_last_error() gives the message;
 *   - "rows" are tokens (latent patches); C = model width; token order inside a forward is (frame, h, w).
 */
#ifndef LONGLIVE_HIP_H
#define LONGLIVE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t ll_bf16;
typedef void* ll_stream;

enum ll_status {
  LL_OK = 0,
  LL_ERR_INVALID_ARG = -1,   /* shape / alignment precondition violated (message names it) */
  LL_ERR_LAUNCH = -2,        /* hipLaunchKernel failed */
  LL_ERR_UNSUPPORTED = -3
};

/* GEMM epilogues (ll_gemm_bf16). */
enum ll_epilogue {
  LL_EPI_BIAS = 0,           /* out = bf16(acc + bias)                                         nn.Linear */
  LL_EPI_BIAS_GELU = 1,      /* out = bf16(gelu_tanh(bf16(acc + bias)))                        ffn.0 + GELU */
  LL_EPI_BIAS_GATE_RES = 2,  /* out = res + bf16(bf16(acc+bias) * gate[frame(row)])            causal_model.py:456,467 */
  LL_EPI_BIAS_RES = 3        /* out = res + bf16(acc + bias)                                   causal_model.py:460 */
};

/* ABI version of this header.  Any change to an existing signature or the removal of an entry point bumps it; the Python binding
 * (longlive_amd/_lib.py) and any other caller must find ll_version() == LL_ABI_VERSION or refuse the library: a stale .so would
 * otherwise shift `stream` and the pointers silently.  100 = rounds 1-3; 105 = round 4's removals (workspace arguments of
 * ll_flash_attn, the split-K hand-off entry points); 106 = round 5 (ll_conv_cl_rms added); 107 = MXFP8 block linears;
 * 108 = MXFP8 self-attention (ll_kv_shadow_mx, ll_flash_attn_mx, ll_flash_attn_mx_plan);
 * 109 = FP8 rowwise block linears (ll_quantize_rows_f8, ll_gemm_f8, ll_gemm_f8_qkv, ll_ln_modulate_f8, ll_ln_modulate_tab_f8,
 * ll_layernorm_affine_f8, ll_gemm_plan_f8);
 * 110 = MXFP6 block linears (ll_quantize_mx6, ll_gemm_mx6, ll_gemm_mx6_qkv, ll_ln_modulate_mx6, ll_ln_modulate_tab_mx6,
 * ll_layernorm_affine_mx6, ll_gemm_plan_mx6);
 * 111 = MXFP4 weights over MXFP6 activations (ll_quantize_mx4, ll_gemm_mx4w6, ll_gemm_mx4w6_qkv, ll_gemm_plan_mx4w6); W4A4 block
 * linears (ll_gemm_mx4, ll_gemm_mx4_qkv, ll_ln_modulate_mx4, ll_ln_modulate_tab_mx4, ll_layernorm_affine_mx4, ll_gemm_plan_mx4) only
 * add entry points, so they keep 111; so does ll_conv_plan, and so do the VAE encoder's entry points (ll_conv_cl_down, ll_conv_cl_tdown,
 * ll_conv_down_plan, ll_pixels_to_cl, ll_vae_scale_tchw), and so do the attention entry points with quantised output
 * (ll_flash_attn_q_ok, ll_flash_attn_q, ll_flash_attn_q_plan, ll_flash_attn_mx_q), and so does the uint8 video intake
 * (ll_pixels_u8_to_cl), and so do the frames-out entry points (ll_cl_to_frames_u8, ll_jpeg_sizes, ll_jpeg_encode_u8,
 * ll_jpeg_coefficients_u8), and so do the clip-intake entry points (ll_jpeg_decode_sizes, ll_jpeg_decode_coefficients,
 * ll_jpeg_decode_pixels, ll_jpeg_decode_u8, ll_resize_u8), and so do the split entropy route's (ll_jpeg_decode_split_sizes,
 * ll_jpeg_decode_coefficients_split, ll_jpeg_decode_u8_split), and so do the planar YUV entry points (ll_frames_u8_to_yuv420,
 * ll_cl_to_yuv420, ll_yuv_to_frames_u8), and so do the lossless frames-out entry points (ll_png_sizes, ll_png_encode_u8,
 * ll_png_filter_u8, ll_zlib_sizes, ll_zlib_compress_u8): 111 covers them too.  The animated-preview (GIF) entry points are declared
 * in longlive_gif.h, not here, and are exported by the same library under ABI 111. */
#define LL_ABI_VERSION 111
int ll_version(void);
const char* ll_last_error(void);
/* Development knob for A/B timing of kernel variants (tools/kbench, tools/kenergy, LL_TUNING=key=value,... for bench.py);
 * the defaults are the shipped configuration; every key names a path some shipped call can take.  Keys:
 *   "gemm_asm"  bit 0 = the generated one-wave-per-SIMD GEMM kernels where they cover the call (gemm_asm_224_gelu: FFN1;
 *               gemm_asm_192_bias: QKV with its V-cache redirect; gemm_asm_128_*: N <= 2048 with bias / gate-residual / residual),
 *               bits 2 / 3 = leave the GELU / the 128-wide kernels out, bit 4 (16) = ll_gemm_w8a8 / ll_gemm_w8a8_qkv on the
 *               generated W8A8 kernels too (bit-identical results, measured slower end to end), bit 5 (32) = launches with more
 *               tiles than CUs run the PERSISTENT form (gemm_asmp_*: one workgroup per CU walks its tiles and stages the next
 *               tile's first pieces under the current epilogue; bit-identical results); default 35; 0 = HIP kernels only
 *   "gemm_asm_mfma16"  mask of the generated bf16 kernels that run their v_mfma_f32_16x16x32_bf16 form (gemm_asm*_m16: the same tile
 *               per wave, staging and epilogue arithmetic; only the fp32 summation order inside an MFMA differs): bit 0 = 128_bias,
 *               1 = 128_res, 2 = 128_gate_res (each classic and persistent), 3 = 128_bias_ssq, 4 / 5 = 192_bias persistent / classic,
 *               6 / 7 = 224_gelu persistent / classic, 8 = 256_bias; 0 = every kernel on v_mfma_f32_32x32x16_bf16; default 511
 *               (the whole family: its members are held to each other bit for bit, which needs one order of the fp32 sum;
 *               profiles/gemm_mfma16_ab.md); -1 restores the default
 *   "gemm_variant" / "gemm_variant_wide" (N >= 4096 only)  tile of the HIP kernels (int8, embeddings / head, gemm_asm = 0):
 *               0 = auto (cost model), 2 = 256x128 (gemm_kernel_v2, 3-stage ring), 3 = 256x256, 5 = 256x192, 6 = 256x224 (all three
 *               instances of the two-stage gemm_kernel_v5; ll_gemm_plan names the kernel and tile a shape takes)
 *   "gemm_group_m"  m-tiles per group of the GEMM tile walk (default 4; <= 1: N fastest);  "gemm_lds_epi" 0 / 1 / 2 = HIP epilogues
 *               staged through LDS: none / all but GELU (default) / all (256x256 always keeps the register epilogue: its wave tile's
 *               LDS image would not fit the ring); any other value is refused (timing-experiment bits need a -DLL_GEMM_DIAG build)
 *   "attn_asm"  1 (default) = the generated attention kernel (flash_attn_asm_kernel) for single key ranges of at least
 *               "attn_asm_min_keys" keys (default 512: self- and cross-attention), 0 = the HIP kernels
 *   "attn_variant"  HIP attention: 0 = plain kernel, 1 = software-pipelined, 2 = + ping-pong wave groups from "attn_pp_min_keys"
 *               keys on (default 2);  "attn_xcd" 0 / 1 = XCD-aware workgroup placement (default 1)
 *   "conv_halo" 0 / 1 = halo-tile convolution kernel of the VAE decoder (default 1)
 * Unknown key: LL_ERR_INVALID_ARG. */
int ll_set_tuning(const char* key, int value);
/* Host-only introspection: the kernel instance + tile + grid that ll_gemm_bf16 / ll_gemm_w8a8 / ll_flash_attn would launch
 * for a shape under the current tuning, as text in out[cap] (bench.py's per-kernel table names kernels from here). */
int ll_gemm_plan(int M, int N, int K, int int8, char* out, int cap);
/* The same for a call whose epilogue is known (LL_EPI_*): names the generated one-wave-per-SIMD kernel (gemm_asm_*, tuning key
 * "gemm_asm") where ll_gemm_bf16 / ll_gemm_w8a8 takes it, else ll_gemm_plan's text.  plain = 1: an ordinary call (no V-cache
 * output, no per-batch modulation vector); 2: the fused QKV call (ll_gemm_bf16_qkv, one batch element); 0: a call with a
 * modulation vector. */
int ll_gemm_plan_epi(int M, int N, int K, int int8, int epilogue, int plain, char* out, int cap);
int ll_flash_attn_plan(int Lq, int H, int B, int seg0_len, int seg1_len, int seg_adjacent, char* out, int cap);
/* The same for ll_conv_cl (rms = 0) / ll_conv_cl_rms (rms = 1): "conv_halo_kernel<epilogue, NCB n, UP u, RMS r> tile ..., grid" or
 * "conv_cl_kernel<epilogue, NT n, MODE m> tile ..., grid, k-steps", from the predicate and arithmetic the launch itself uses (tuning
 * key "conv_halo" included).  Shapes ll_conv_cl rejects are rejected here; rms = 1 where ll_conv_cl_rms_ok is 0 is rejected too. */
int ll_conv_plan(int T, int H, int W, int Cin, int Cout, int KT, int KH, int upsample, int with_res, int rms, char* out, int cap);

/* ---- norms / modulation ------------------------------------------------------------------------------------- */

/* out[r,:] = LN(x[r,:]) * (1 + s) + t  with s = bf16(mod[scale_idx,:] + e[b,f,scale_idx,:]), t likewise, f = frame of
 * row r.  Replaces `norm1(x).unflatten(..) * (1 + e[1]) + e[0]` (wan/modules/causal_model.py:445,463-464) and
 * CausalHead's 2-way form (:506-507).  x,out [B, L, C]; e [B, F, nmod, C]; mod [nmod, C]; L = F * frame_len. */
int ll_ln_modulate(const ll_bf16* x, ll_bf16* out, const ll_bf16* e, const ll_bf16* mod, int nmod, int shift_idx,
                   int scale_idx, int B, int L, int C, int F, float eps, ll_stream stream);

/* out[l, bf, i, :] = bf16(mods[l, i, :] + e[bf, i, :]) for all layers l of one forward: `e = modulation + e0`
 * (wan/modules/causal_model.py:440) evaluated once per (layer, frame) instead of once per token row.  A layer's slice
 * out[l] [B*F, nmod, C] may be passed as `e` with mod = NULL to ll_ln_modulate / ll_ln_modulate_q8 and to the gate-residual
 * epilogue of ll_gemm_bf16 / ll_gemm_w8a8: same values, two vector loads and six operations per element fewer. */
int ll_modulation_table(const ll_bf16* e, const ll_bf16* mods, ll_bf16* out, int num_layers, int BF, int nmod, int C,
                        ll_stream stream);

/* The fp32 form of the table for ll_ln_modulate_tab: out[l, bf, i, :] = float(bf16(mods[l, i, :] + e[bf, i, :])), and for the chunks
 * whose bit is set in one_plus_mask (the scale chunks 1 and 4 of a block's six) float(bf16(1 + that)) -- exactly the `1 + e[1]` the
 * reference forms per token row (wan/modules/causal_model.py:445,463), once per (layer, frame).  out [num_layers, BF, nmod, C] fp32. */
int ll_modulation_table_f32(const ll_bf16* e, const ll_bf16* mods, float* out, int num_layers, int BF, int nmod, int C,
                            unsigned one_plus_mask, ll_stream stream);

/* ll_ln_modulate / ll_ln_modulate_q8 from a layer's slice tab [B*F, nmod, C] of ll_modulation_table_f32 (scale_idx must be a chunk
 * of its one_plus_mask): out = bf16(bf16(bf16(LN(x)) * tab[scale_idx]) + tab[shift_idx]), the same bits with eight vector
 * instructions per element pair fewer.  Exactly one of out (bf16 [B, L, C]) and q (int8 [B, L, C] with qscale [B*L]) is non-NULL. */
int ll_ln_modulate_tab(const ll_bf16* x, ll_bf16* out, int8_t* q, float* qscale, const float* tab, int nmod, int shift_idx,
                       int scale_idx, int B, int L, int C, int F, float eps, ll_stream stream);

/* out = LayerNorm(x) * w + b  (norm3, wan/modules/causal_model.py:397-399,460; wan/modules/model.py:89-99). */
int ll_layernorm_affine(const ll_bf16* x, const ll_bf16* w, const ll_bf16* b, ll_bf16* out, int rows, int C,
                        float eps, ll_stream stream);

/* int8 mode: the same two kernels emitting per-row symmetric int8 + scale (bit-identical to ll_quantize_rows applied to
 * their bf16 output) so the following W8A8 GEMM reads its operand without an extra pass. */
int ll_ln_modulate_q8(const ll_bf16* x, int8_t* q, float* qscale, const ll_bf16* e, const ll_bf16* mod, int nmod,
                      int shift_idx, int scale_idx, int B, int L, int C, int F, float eps, ll_stream stream);
int ll_layernorm_affine_q8(const ll_bf16* x, const ll_bf16* w, const ll_bf16* b, int8_t* q, float* qscale, int rows,
                           int C, float eps, ll_stream stream);

/* out = bf16(x * rsqrt(mean(x^2) + eps)) * w over the FULL width C (WanRMSNorm, wan/modules/model.py:70-86).
 * ldx / ldo = row strides in elements (lets the caller normalise a column slice of a fused projection). */
int ll_rmsnorm(const ll_bf16* x, const ll_bf16* w, ll_bf16* out, int rows, int C, int ldx, int ldo, float eps,
               ll_stream stream);

/* Fused q/k RMSNorm + 3-axis RoPE + KV-cache insert for self-attention
 * (wan/modules/causal_model.py:122-126,206-211,264-269,302-311; causal_rope_apply :32-60).
 *   qkv      [B, L, 3C]  fused projection output (q | k | v)
 *   q_out    [B, L, C]   roped queries
 *   cache_k/v[B, S, C]   rows [write_start, write_start+write_len) receive roped k / v of tokens
 *                        [roped_offset, roped_offset+write_len)
 *   rope_f   [1024, nf, 2] (cos,sin) fp32 for the frame axis, rope_hw [frame_len, nhw, 2] for the (h,w) axes;
 *            nf + nhw = head_dim / 2.  start_frame = current_start / frame_len.
 *   cache_v may be NULL: V was already inserted by ll_gemm_bf16_qkv / ll_gemm_w8a8_qkv and the v third of qkv is not read. */
int ll_qk_norm_rope_kv_store(const ll_bf16* qkv, const ll_bf16* wq, const ll_bf16* wk, const float* rope_f,
                             const float* rope_hw, ll_bf16* q_out, ll_bf16* cache_k, ll_bf16* cache_v, int B, int L,
                             int C, int head_dim, int frame_len, int start_frame, int S, int write_start,
                             int roped_offset, int write_len, float eps, ll_stream stream);

/* cache[:, dst:dst+n] = cache[:, src:src+n] for K and V, src > dst (left shift that discards evicted tokens while
 * the sink stays put: wan/modules/causal_model.py:257-260, 874-877).  Overlap-safe (chunked by src-dst). */
int ll_kv_roll(ll_bf16* cache_k, ll_bf16* cache_v, int B, int S, int C, int dst, int src, int n, ll_stream stream);

/* ---- dense contractions (MFMA) -------------------------------------------------------------------------------- */

/* out[M,N] = epilogue(x[M,K] @ w[N,K]^T + bias[N]); bf16 in/out, fp32 accumulate.  K % 64 == 0, N % 8 == 0.
 * x [M, ldx], out [M, ldo]: row strides in elements, ldx >= K, ldo >= N, both multiples of 8 (rows start on 16 bytes: the
 * widest loads and stores are 16-byte vectors; anything else is LL_ERR_INVALID_ARG).  The same holds for every ll_gemm_* entry point.
 * Replaces nn.Linear q/k/v/o, ffn.0/ffn.2, text_embedding, patch_embedding (as GEMM), head.head
 * (wan/modules/causal_model.py:90-93,406-408,599-603; wan/modules/model.py:172-193).
 * res [M, ldo] may alias out.  For LL_EPI_BIAS_GATE_RES: gate = bf16(mod[gate_idx,:] + e[b, f, gate_idx, :]) with
 * b = row / rows_per_batch, f = (row % rows_per_batch) / frame_len; e [B, F, nmod, N], mod [nmod, N]; mod = NULL: e already
 * holds that sum (ll_modulation_table). */
int ll_gemm_bf16(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N, int K, int ldx,
                 int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e, const ll_bf16* mod, int nmod,
                 int gate_idx, int rows_per_batch, int frame_len, ll_stream stream);

/* Small-M form of ll_gemm_bf16 for the 512-token linears of the text side (umT5 self-attention / FFN projections,
 * wan/modules/t5.py:65-117,134-160; the text K/V projections of cross-attention, wan/modules/model.py:183-188): a grid of
 * ceil(M / 256) x (N / 128) tiles fills a fraction of the device, so K is cut into ll_gemm_ksplit_plan(M, N, K) ranges (0 = not
 * taken for this shape on this device), each range's fp32 tile sums go to `workspace` ([splits][M][N] floats, caller-owned, at
 * least ll_gemm_ksplit_workspace_bytes bytes, 16-byte aligned, no initialisation needed) and one pass adds them in a fixed order
 * and applies the epilogue (LL_EPI_BIAS or LL_EPI_BIAS_RES).  Results equal ll_gemm_bf16's up to the order of the fp32 sum;
 * bit-identical run to run.  workspace = NULL or plan = 0: it IS ll_gemm_bf16.  The NUMBER of ranges depends on N and K only;
 * WHETHER the path is taken depends on M and on the device's CU count (tiles * 2 <= CUs) and on tuning key "gemm_asm"
 * (bit 0 off or bit 3 set: never), so a row's fp32 sum order is stable only inside that region. */
int ll_gemm_ksplit_plan(int M, int N, int K);
long long ll_gemm_ksplit_workspace_bytes(int M, int N, int K);
int ll_gemm_bf16_ksplit(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N, int K, int ldx,
                        int ldo, int epilogue, const ll_bf16* res, void* workspace, long long workspace_bytes, ll_stream stream);
/* ll_gemm_bf16_ksplit (LL_EPI_BIAS_RES) followed by T5LayerNorm of the new residual stream (wan/modules/t5.py:57-63,119-160:
 * x = x + linear(.); h = norm(x)): out = x_new [M, N] (ldo = N), h_out = bf16(norm_w * bf16(x_new * rsqrt(mean(x_new^2) + eps))).
 * On the small-M path the K-range sum, bias, residual and norm are one pass over each row; otherwise ll_gemm_bf16 +
 * ll_t5_rmsnorm.  The two outputs carry the same bits either way. */
int ll_gemm_bf16_ksplit_t5norm(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N, int K, int ldx,
                               int ldo, const ll_bf16* res, const ll_bf16* norm_w, float eps, ll_bf16* h_out, void* workspace,
                               long long workspace_bytes, ll_stream stream);

/* W8A8 variant of ll_gemm_bf16 for BASELINE config 5 ("INT8-quantized linear layers"; the reference ships no INT8 code,
 * reports.md:24,39): out = epilogue(sx[m] * sw[n] * (xq[M,K] . wq[N,K]^T) + bias) with int8 operands, exact int32
 * accumulation on v_mfma_i32_16x16x64_i8 and the same fused epilogues.  sx [M] / sw [N] fp32; K % 128 == 0. */
int ll_gemm_w8a8(const int8_t* xq, const float* sx, const int8_t* wq, const float* sw, const ll_bf16* bias, ll_bf16* out,
                 int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e, const ll_bf16* mod,
                 int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream);

/* The fused q|k|v projection (N = 3 C, LL_EPI_BIAS) with the V third written straight into the KV cache by the GEMM epilogue:
 * token t of batch b goes to cache_v[b, write_start + (t - roped_offset), :] when 0 <= t - roped_offset < write_len, exactly the
 * insert of wan/modules/causal_model.py:264-269,302-311 (V is copied unrotated, so the bits are the projection's).  The q and k
 * thirds land in out[M, ldo]; its v third is left unwritten.  M = B * L.  Saves one write and one read of V per layer. */
int ll_gemm_bf16_qkv(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N, int K, int ldx, int ldo,
                     ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset, int write_len, ll_stream stream);
int ll_gemm_w8a8_qkv(const int8_t* xq, const float* sx, const int8_t* wq, const float* sw, const ll_bf16* bias, ll_bf16* out,
                     int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset,
                     int write_len, ll_stream stream);

/* Symmetric per-row int8 quantisation: scale[r] = max|x[r,:]| / 127 (1 for an all-zero row), q = rint(x / scale).
 * Per token for activations, per output channel for weights ([N,K] rows), x row stride ldx elements. */
int ll_quantize_rows(const ll_bf16* x, int8_t* q, float* scale, int rows, int K, int ldx, ll_stream stream);

/* MXFP8 mode of the block linears (v_mfma_scale_f32_16x16x128_f8f6f4, both operands OCP e4m3fn).  A row is quantised along K in
 * blocks of 32: amax = m 2^p (frexp), e = p - 9 + (m > 0.875) clamped to [-127, 127] (the smallest e with amax <= 448 2^e), scale
 * byte e + 127 (E8M0; an all-zero block stores 127), codes e4m3fn(RNE(x 2^-e)) with subnormals kept.  Codes [rows, K] (1 byte each),
 * scales [rows, K / 32] (uint8), row-major.
 *   ll_quantize_mx: bf16 rows (stride ldx elements) -> codes + scales, one launch; K % 32 == 0.
 *   ll_gemm_mx:     out = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias) with ll_gemm_bf16's epilogues and rounding points; K % 128 == 0.
 *                   With the GELU epilogue, q_out / s_out (instead of out) receive the MX codes + scales of the bf16 GELU output
 *                   (N % 32 == 0, ldo == N), bit-identical to ll_quantize_mx of the bf16 result.  Exactly one form is given.
 *   ll_gemm_mx_qkv: ll_gemm_bf16_qkv's fused q|k|v projection (V third into cache_v) on MX operands.
 *   ll_ln_modulate_mx / ll_ln_modulate_tab_mx / ll_layernorm_affine_mx: the producers of the same names emitting MX codes + scales
 *                   of their bf16 output (bit-identical to ll_quantize_mx of it); C % 32 == 0.
 *   ll_gemm_plan_mx: kernel instance, tile and grid of an ll_gemm_mx / ll_gemm_mx_qkv call (host only). */
int ll_quantize_mx(const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx, ll_stream stream);
int ll_gemm_mx(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
               uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e,
               const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream);
int ll_gemm_mx_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                   int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset,
                   int write_len, ll_stream stream);
int ll_ln_modulate_mx(const ll_bf16* x, uint8_t* q, uint8_t* qs, const ll_bf16* e, const ll_bf16* mod, int nmod, int shift_idx,
                      int scale_idx, int B, int L, int C, int F, float eps, ll_stream stream);
int ll_ln_modulate_tab_mx(const ll_bf16* x, uint8_t* q, uint8_t* qs, const float* tab, int nmod, int shift_idx, int scale_idx,
                          int B, int L, int C, int F, float eps, ll_stream stream);
int ll_layernorm_affine_mx(const ll_bf16* x, const ll_bf16* w, const ll_bf16* b, uint8_t* q, uint8_t* qs, int rows, int C,
                           float eps, ll_stream stream);
int ll_gemm_plan_mx(int M, int N, int K, char* out, int cap);

/* MXFP6 mode of the block linears (v_mfma_scale_f32_16x16x128_f8f6f4 with both operands OCP FP6 E2M3: the FP4 rate, twice the int8 /
 * FP8 modes').  A row is quantised along K in blocks of 32: amax = m 2^p (frexp), e = p - 3 + (m > 0.9375) clamped to [-127, 127]
 * (the smallest e with amax <= 7.5 2^e, so no code saturates), scale byte e + 127 (E8M0; an all-zero block stores 127), codes
 * E2M3(RNE(x 2^-e)) with subnormals kept (steps of 0.125, maximum 7.5).  Scales [rows, K / 32] (uint8), row-major.
 * Codes [rows, 3K / 4] bytes, K % 256 == 0, packed 6 bits per code in 192-byte super-blocks of 256 k: the 32-k block j = 0..7 of a
 * super-block (k 32 j .. 32 j + 31, one scale block) occupies the 24 bytes at 48 (j % 4) + 24 (j / 4), code i of the block in bits
 * 6 i .. 6 i + 5 of that little-endian 192-bit word.  (The 48 bytes at 48 g are then blocks g and g + 4: the two 16x16x128 K-steps'
 * operand fragments of MFMA lane group g, read as one contiguous piece.)
 *   ll_quantize_mx6: bf16 rows (stride ldx elements) -> codes + scales, one launch; K % 256 == 0.
 *   ll_gemm_mx6:     out = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias) with ll_gemm_bf16's epilogues and rounding points; K % 256 == 0.
 *                    With the GELU epilogue, q_out / s_out (instead of out) receive the MXFP6 codes + scales of the bf16 GELU output
 *                    (N % 256 == 0, ldo == N), bit-identical to ll_quantize_mx6 of the bf16 result.  Exactly one form is given.
 *   ll_gemm_mx6_qkv: ll_gemm_bf16_qkv's fused q|k|v projection (V third into cache_v) on MXFP6 operands.
 *   ll_ln_modulate_mx6 / ll_ln_modulate_tab_mx6 / ll_layernorm_affine_mx6: the producers of the same names emitting MXFP6 codes +
 *                    scales of their bf16 output (bit-identical to ll_quantize_mx6 of it); C % 256 == 0.
 *   ll_gemm_plan_mx6: kernel instance, tile and grid of an ll_gemm_mx6 / ll_gemm_mx6_qkv call (host only). */
int ll_quantize_mx6(const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx, ll_stream stream);
int ll_gemm_mx6(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e,
                const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream);
int ll_gemm_mx6_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                    int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset,
                    int write_len, ll_stream stream);
int ll_ln_modulate_mx6(const ll_bf16* x, uint8_t* q, uint8_t* qs, const ll_bf16* e, const ll_bf16* mod, int nmod, int shift_idx,
                       int scale_idx, int B, int L, int C, int F, float eps, ll_stream stream);
int ll_ln_modulate_tab_mx6(const ll_bf16* x, uint8_t* q, uint8_t* qs, const float* tab, int nmod, int shift_idx, int scale_idx,
                           int B, int L, int C, int F, float eps, ll_stream stream);
int ll_layernorm_affine_mx6(const ll_bf16* x, const ll_bf16* w, const ll_bf16* b, uint8_t* q, uint8_t* qs, int rows, int C,
                            float eps, ll_stream stream);
int ll_gemm_plan_mx6(int M, int N, int K, char* out, int cap);

/* W4A6 mode of the block linears (set_quant("mxfp4_a6"): v_mfma_scale_f32_16x16x128_f8f6f4 with OCP FP4 E2M1 weights and the MXFP6
 * E2M3 activations above, the FP4 rate).  Weights are quantised along K in blocks of 32: amax = m 2^p (frexp), e = p - 3 + (m > 0.75)
 * clamped to [-127, 127] (the smallest e with amax <= 6 2^e, so no code saturates), scale byte e + 127 (E8M0; an all-zero block
 * stores 127), codes E2M1(RNE(x 2^-e)) (sign bit 3, values 0, 0.5, 1, 1.5, 2, 3, 4, 6; a negative value rounding to zero keeps its
 * sign).  Scales [rows, K / 32] (uint8), row-major.
 * Codes [rows, K / 2] bytes, K % 256 == 0, packed 4 bits per code in 128-byte super-blocks of 256 k: the 32-k block j = 0..7 of a
 * super-block (k 32 j .. 32 j + 31, one scale block) occupies the 16 bytes at 32 (j % 4) + 16 (j / 4), code i of the block in bits
 * 4 i .. 4 i + 3 of that little-endian 128-bit word.  (The 32 bytes at 32 g are then blocks g and g + 4: the two 16x16x128 K-steps'
 * operand fragments of MFMA lane group g.)
 *   ll_quantize_mx4:    bf16 rows (stride ldx elements) -> codes + scales, one launch; K % 256 == 0.
 *   ll_gemm_mx4w6:      ll_gemm_mx6 with E2M1 weights (wq / sw from ll_quantize_mx4) and MXFP6 activations (xq / sx from
 *                       ll_quantize_mx6 or the MXFP6 producers): the same epilogues, rounding points and MXFP6 GELU output.
 *   ll_gemm_mx4w6_qkv:  ll_gemm_mx6_qkv with E2M1 weights.
 *   ll_gemm_plan_mx4w6: kernel instance, tile and grid of an ll_gemm_mx4w6 / ll_gemm_mx4w6_qkv call (host only). */
int ll_quantize_mx4(const ll_bf16* x, uint8_t* q, uint8_t* qs, int rows, int K, int ldx, ll_stream stream);
int ll_gemm_mx4w6(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                  uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e,
                  const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream);
int ll_gemm_mx4w6_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                      int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset,
                      int write_len, ll_stream stream);
int ll_gemm_plan_mx4w6(int M, int N, int K, char* out, int cap);

/* W4A4 mode of the block linears (set_quant("mxfp4_a4"): v_mfma_scale_f32_16x16x128_f8f6f4 with both operands OCP FP4 E2M1, the FP4
 * rate).  Activations use the weights' scheme and layout above (ll_quantize_mx4: codes [rows, K / 2], scales [rows, K / 32]).
 *   ll_gemm_mx4:      ll_gemm_mx4w6 with E2M1 activations (xq / sx from ll_quantize_mx4 or the MXFP4 producers): the same epilogues
 *                     and rounding points.  With the GELU epilogue, q_out / s_out (instead of out) receive the MXFP4 codes + scales of
 *                     the bf16 GELU output (N % 256 == 0, ldo == N), bit-identical to ll_quantize_mx4 of the bf16 result.  Exactly
 *                     one form is given.
 *   ll_gemm_mx4_qkv:  ll_gemm_mx6_qkv on E2M1 operands (V third into cache_v).
 *   ll_ln_modulate_mx4 / ll_ln_modulate_tab_mx4 / ll_layernorm_affine_mx4: the producers of the same names emitting MXFP4 codes +
 *                     scales of their bf16 output (bit-identical to ll_quantize_mx4 of it); C % 256 == 0.
 *   ll_gemm_plan_mx4: kernel instance, tile and grid of an ll_gemm_mx4 / ll_gemm_mx4_qkv call (host only). */
int ll_gemm_mx4(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                uint8_t* q_out, uint8_t* s_out, int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e,
                const ll_bf16* mod, int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream);
int ll_gemm_mx4_qkv(const uint8_t* xq, const uint8_t* sx, const uint8_t* wq, const uint8_t* sw, const ll_bf16* bias, ll_bf16* out,
                    int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset,
                    int write_len, ll_stream stream);
int ll_ln_modulate_mx4(const ll_bf16* x, uint8_t* q, uint8_t* qs, const ll_bf16* e, const ll_bf16* mod, int nmod, int shift_idx,
                       int scale_idx, int B, int L, int C, int F, float eps, ll_stream stream);
int ll_ln_modulate_tab_mx4(const ll_bf16* x, uint8_t* q, uint8_t* qs, const float* tab, int nmod, int shift_idx, int scale_idx,
                           int B, int L, int C, int F, float eps, ll_stream stream);
int ll_layernorm_affine_mx4(const ll_bf16* x, const ll_bf16* w, const ll_bf16* b, uint8_t* q, uint8_t* qs, int rows, int C,
                            float eps, ll_stream stream);
int ll_gemm_plan_mx4(int M, int N, int K, char* out, int cap);

/* FP8 rowwise mode of the block linears (set_quant("fp8_rowwise")): ll_gemm_w8a8's per-token / per-output-channel scheme with OCP e4m3fn
 * codes instead of int8.  Per row (a token of the activations, an output channel of a [N, K] weight): amax = max |x| over its bf16
 * values (fp32), sc = amax / 448 (1 for an all-zero row), inv = 1 / sc, code = e4m3fn(RNE(clamp(x * inv, -448, 448))) with subnormals
 * kept.  Codes [rows, K] (uint8), scales [rows] (fp32).
 *   ll_quantize_rows_f8: bf16 rows (stride ldx elements) -> codes + scales; ll_quantize_rows' kernels and dispatch.
 *   ll_gemm_f8:     out = epilogue(sx[m] * sw[n] * sum_k dec(xq[m,k]) dec(wq[n,k]) + bias), fp32 accumulation on
 *                   v_mfma_scale_f32_16x16x128_f8f6f4 at unit block scales, ll_gemm_w8a8's kernels, epilogues and rounding points;
 *                   K % 128 == 0, ldo % 8 == 0.
 *   ll_gemm_f8_qkv: ll_gemm_w8a8_qkv's fused q|k|v projection (V third into cache_v) on FP8 operands.
 *   ll_ln_modulate_f8 / ll_ln_modulate_tab_f8 / ll_layernorm_affine_f8: the producers of the same names emitting the codes + row scale of
 *                   their bf16 output (bit-identical to ll_quantize_rows_f8 of it).
 *   ll_gemm_plan_f8: kernel instance, tile and grid of an ll_gemm_f8 / ll_gemm_f8_qkv call (host only). */
int ll_quantize_rows_f8(const ll_bf16* x, uint8_t* q, float* scale, int rows, int K, int ldx, ll_stream stream);
int ll_gemm_f8(const uint8_t* xq, const float* sx, const uint8_t* wq, const float* sw, const ll_bf16* bias, ll_bf16* out,
               int M, int N, int K, int ldo, int epilogue, const ll_bf16* res, const ll_bf16* e, const ll_bf16* mod,
               int nmod, int gate_idx, int rows_per_batch, int frame_len, ll_stream stream);
int ll_gemm_f8_qkv(const uint8_t* xq, const float* sx, const uint8_t* wq, const float* sw, const ll_bf16* bias, ll_bf16* out,
                   int M, int N, int K, int ldo, ll_bf16* cache_v, int B, int L, int S, int write_start, int roped_offset,
                   int write_len, ll_stream stream);
int ll_ln_modulate_f8(const ll_bf16* x, uint8_t* q, float* qscale, const ll_bf16* e, const ll_bf16* mod, int nmod, int shift_idx,
                      int scale_idx, int B, int L, int C, int F, float eps, ll_stream stream);
int ll_ln_modulate_tab_f8(const ll_bf16* x, uint8_t* q, float* qscale, const float* tab, int nmod, int shift_idx, int scale_idx,
                          int B, int L, int C, int F, float eps, ll_stream stream);
int ll_layernorm_affine_f8(const ll_bf16* x, const ll_bf16* w, const ll_bf16* b, uint8_t* q, float* qscale, int rows, int C,
                           float eps, ll_stream stream);
int ll_gemm_plan_f8(int M, int N, int K, char* out, int cap);

/* MXFP8 self-attention (set_attn_quant("mxfp8")) over a block-scaled SHADOW of one layer's bf16 KV cache k, v [B, S, H, 128]; the bf16
 * cache stays the master, S32 = S rounded up to a multiple of 32.  MX rule as ll_quantize_mx.
 *   K^: codes kq [B, S32, H, 128] e4m3fn + scales ks [B, S32, H, 4]: each slot's K row quantised along channels (ll_quantize_mx of it).
 *   V^: codes vq [B, H, S32 / 32, 128, 32] + scales vs [B, H, S32 / 32, 128]: per (head, channel d, slots 32 j .. 32 j + 31) the MX rule
 *       over the 32 values V[32 j + i, head, d] (slots >= S read as 0); code position 16 hh + jj of a row holds slot
 *       32 j + (jj & 3) + 8 (jj >> 2) + 4 hh (the order in which the kernel's score registers arrive).
 *   ll_kv_shadow_mx: re-derives K^ rows and V^ blocks of the slots [lo, hi), widened to whole 32-slot blocks: blocks lo / 32 ..
 *       ceil(hi / 32) - 1 of all four arrays are rewritten (padding slots >= S of the last block: zero codes under scale byte 127 in
 *       K^, zeros in V^'s block), no other byte is touched, lo == hi launches nothing.  It follows every write
 *       of the cache in block_forward (the QKV epilogue's V insert and qk_norm_rope_kv_store's K insert, causal_model.py:264-269,302-311;
 *       ll_kv_roll, :257-260) and any external change of k / v (the pipelines' in-place zero_ before a recache).
 *   ll_flash_attn_mx: ll_flash_attn's self-attention (wan/modules/attention.py:43-197 over the sink/window of causal_model.py:331-360)
 *       on v_mfma_scale_f32_32x32x64_f8f6f4: q [B, Lq, H*128] (row stride ldq) quantised per row in the kernel's prologue,
 *       s = sum_b 2^(eq + ek) sum q^ k^ in fp32, P^ = e4m3fn(exp2(c s - c m_ref)) with the lazy max (m_ref moves only when a tile's max
 *       exceeds it by more than 8 / c), O = sum P^ V^ / sum P^ written as bf16 (row stride ldo).  Key tiles of 64 slots start at each
 *       range's start rounded down to 32 (adjacent ranges are merged first); slots outside the ranges are masked.  head_dim must be 128.
 *       Preconditions, each refused with LL_ERR_INVALID_ARG before anything is launched: S32 == S rounded up to 32; both ranges inside
 *       [0, S), the first non-empty, the second in any position but NOT overlapping the first (shared keys would be counted twice;
 *       ll_flash_attn refuses overlap alike); scale positive and finite (the tile maximum is taken before the multiplication by
 *       scale * log2 e); ldq % 8 == 0, ldo % 4 == 0 (a lane stores 4 bf16 at column offsets that are multiples of 4: rows on 8 bytes
 *       suffice), both >= H * 128.  Padding columns of q and out are neither read nor written.
 *       Not checkable here: EVERY 32-SLOT BLOCK A TILE STAGES MUST HAVE BEEN DERIVED OR ZEROED.  A tile is two blocks, so the last
 *       tile of a range may stage a block past its end (for [0, 9360) block 293) whose keys are masked: P^ = 0 there, but the block's
 *       V^ codes and scale bytes still enter the MFMA, and an e4m3 NaN code (0x7f / 0xff) or an E8M0 NaN byte (0xff) times 0 is NaN.
 *       Allocate the shadow zero-filled (ops.kv_shadow_mx_alloc does) or refresh it over [0, S) first.  K^ rows of masked slots and
 *       blocks no tile stages may hold anything.
 *   ll_flash_attn_mx_plan: kernel, tile and grid of an ll_flash_attn_mx call (host only). */
int ll_kv_shadow_mx(const ll_bf16* k, const ll_bf16* v, uint8_t* kq, uint8_t* ks, uint8_t* vq, uint8_t* vs, int B, int S, int S32, int H,
                    int head_dim, int lo, int hi, ll_stream stream);
int ll_flash_attn_mx(const ll_bf16* q, const uint8_t* kq, const uint8_t* ks, const uint8_t* vq, const uint8_t* vs, ll_bf16* out, int B,
                     int Lq, int H, int head_dim, int ldq, int ldo, int S, int S32, int seg0_start, int seg0_len, int seg1_start,
                     int seg1_len, float scale, ll_stream stream);
int ll_flash_attn_mx_plan(int Lq, int H, int B, int seg0_start, int seg0_len, int seg1_start, int seg1_len, char* out, int cap);

/* Small-M linear (M <= 8): out = act_out(act_in(x) @ w^T + b); act: 0 none, 1 SiLU.  time_embedding /
 * time_projection (wan/modules/causal_model.py:605-608,976-979). */
int ll_linear_small(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int M, int N, int K,
                    int act_in, int act_out, ll_stream stream);

/* Non-causal softmax(q k^T / sqrt(d)) v, head_dim 128, keys taken from up to two row ranges of the K/V buffers
 * ([seg0_start, +seg0_len) then [seg1_start, +seg1_len)): frame sink + sliding window of the KV cache, or the 512
 * text tokens for cross-attention.  Replaces attention()/flash_attention() (wan/modules/attention.py:43-197) and the
 * sink/window gather + cat (wan/modules/causal_model.py:331-360).
 *   q,out [B, Lq, H*128] with row strides ldq/ldo; k,v [B, Sk, H*128] with row stride ldk, batch stride k_batch_stride.
 *   A single key range of >= 512 keys runs the generated kernel (flash_attn_asm_kernel: 4 waves x 64 query rows, one wave per
 *   SIMD), shorter or two-piece ranges the HIP kernels. */
int ll_flash_attn(const ll_bf16* q, const ll_bf16* k, const ll_bf16* v, ll_bf16* out, int B, int Lq, int H, int ldq,
                  int ldo, int ldk, long long k_batch_stride, int seg0_start, int seg0_len, int seg1_start,
                  int seg1_len, float scale, ll_stream stream);

/* Cross-attention's q path with two launches fewer: `q = self.norm_q(self.q(x))` then attention over the text keys
 * (wan/modules/model.py:172,189; WanRMSNorm :78-86 normalises over ALL H*128 channels of a row).
 *   ll_gemm_bf16_ssq   = ll_gemm_bf16 with LL_EPI_BIAS that also writes ssq[N / 128][M] (fp32): per row and 128-column n-tile the
 *                        sum of squares of the bf16 outputs (the projection's epilogue; fixed summation order).
 *   ll_flash_attn_qnorm = ll_flash_attn over ONE key range whose Q prologue sums the planes in plane order, forms
 *                        rsq(sum / C + eps) and applies bf16(bf16(x * rinv) * norm_w) -- WanRMSNorm's rounding points -- before its
 *                        own scaling: the separate RMSNorm launch (and its 2 x 14.4 MB of traffic) disappears.
 * Both exist only as generated gfx950 kernels: ll_gemm_ssq_planes (planes written, 0 = not covered) and ll_flash_attn_qnorm_ok
 * (1 / 0) say whether a shape is covered under the current tuning; otherwise the caller runs ll_gemm_bf16 + ll_rmsnorm +
 * ll_flash_attn (the entry points return LL_ERR_INVALID_ARG rather than fall back).  q [B, Lq, H*128] contiguous rows (ldq = H*128),
 * ssq rows are b * Lq + l. */
int ll_gemm_ssq_planes(int M, int N, int K);
int ll_gemm_bf16_ssq(const ll_bf16* x, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, float* ssq, int M, int N, int K, int ldx,
                     int ldo, ll_stream stream);
int ll_flash_attn_qnorm_ok(int H, int nkeys);
int ll_flash_attn_qnorm(const ll_bf16* q, const float* ssq, const ll_bf16* norm_w, float eps, const ll_bf16* k, const ll_bf16* v,
                        ll_bf16* out, int B, int Lq, int H, int ldq, int ldo, int ldk, long long k_batch_stride, int key_start,
                        int nkeys, float scale, ll_stream stream);

/* Attention whose epilogue writes what the NEXT GEMM reads in the block-scaled modes: instead of the bf16 rows [B, Lq, H*128] the
 * codes and E8M0 scale bytes ll_quantize_mx / _mx6 / _mx4 would make of them (same layouts: codes [B*Lq][ldc bytes], H*128 codes of
 * 8 / 6 / 4 bits per row, packed formats in 256-k super-blocks; scales [B*Lq][lds bytes], one byte per 32 channels).  Contract: the
 * pair is bit-identical to ll_quantize_<fmt>(ll_flash_attn(...)) (ll_flash_attn_mx for the _mx_q form) under the same tuning -- the
 * kernel rounds O / l to bf16 as its bf16 twin does and applies the format's rule to the rounded values.  A scale block is 32 channels
 * of one row and a head is 128, so a workgroup owns whole blocks; head h owns blocks 4 (h & 1) + (0..3) of super-block h >> 1, hence
 * the packed formats need an even H.  Rows of the buffers outside [0, B*Lq) and bytes outside the H heads' are not written.
 *   ll_flash_attn_q_ok: 1 exactly when the generated gfx950 kernel takes the launch under the current tuning: the key ranges are
 *       one contiguous range after merging adjacent ones, that range is long enough for it (tuning key attn_asm_min_keys, at least
 *       two key tiles), H is even for LL_QFMT_MX6 / MX4.  Otherwise 0, and the caller runs ll_flash_attn + ll_quantize_<fmt>:
 *   ll_flash_attn_q returns LL_ERR_INVALID_ARG where ll_flash_attn_q_ok is 0 (no fall-back inside the library).  ldc: a multiple of
 *       16 bytes, at least the row's H*16*bits bytes; lds: a multiple of 4, at least 4*H; ldq and ldk (elements): multiples of 8, at
 *       least H*128; k_batch_stride in elements, the ranges may not overlap.  ll_flash_attn_q_ok assumes ldk = H*128: with wider key
 *       rows the call also needs seg_len * ldk * 2 bytes below 2^31.  A refused call launches nothing and writes nothing.
 *   ll_flash_attn_q_plan: the kernel and grid of such a launch, or that it is not covered (host only).
 *   ll_flash_attn_mx_q: ll_flash_attn_mx with the same output forms; every launch ll_flash_attn_mx takes is covered (even H for the
 *       packed formats). */
enum ll_qfmt { LL_QFMT_MX = 1, LL_QFMT_MX6 = 2, LL_QFMT_MX4 = 3 };
int ll_flash_attn_q_ok(int fmt, int H, int seg0_start, int seg0_len, int seg1_start, int seg1_len);
int ll_flash_attn_q_plan(int fmt, int Lq, int H, int B, int seg0_start, int seg0_len, int seg1_start, int seg1_len, char* out, int cap);
int ll_flash_attn_q(int fmt, const ll_bf16* q, const ll_bf16* k, const ll_bf16* v, uint8_t* codes, uint8_t* scales, int B, int Lq, int H,
                    int ldq, int ldc, int lds, int ldk, long long k_batch_stride, int seg0_start, int seg0_len, int seg1_start,
                    int seg1_len, float scale, ll_stream stream);
int ll_flash_attn_mx_q(int fmt, const ll_bf16* q, const uint8_t* kq, const uint8_t* ks, const uint8_t* vq, const uint8_t* vs,
                       uint8_t* codes, uint8_t* scales, int B, int Lq, int H, int head_dim, int ldq, int ldc, int lds, int S, int S32,
                       int seg0_start, int seg0_len, int seg1_start, int seg1_len, float scale, ll_stream stream);

/* ---- embeddings / head / scheduler ------------------------------------------------------------------------------ */

/* im2col of Conv3d k=s=(1,2,2) (wan/modules/causal_model.py:599-600,959-963): x [B,F,Cin,H,W] (the wrapper's layout,
 * utils/wan_wrapper.py:249 permute folded in) -> patches [B, F*(H/2)*(W/2), Cin*4] with column (c, p, q). */
int ll_patchify(const ll_bf16* x, ll_bf16* patches, int B, int F, int Cin, int H, int W, ll_stream stream);

/* sinusoidal_embedding_1d (wan/modules/model.py:15-25) in fp64 then cast to bf16: out [n, dim]. */
int ll_sinusoid(const float* t, ll_bf16* out, int n, int dim, ll_stream stream);

/* unpatchify ('fhwpqrc->cfphqwr', wan/modules/causal_model.py:1240-1263) + flow->x0 in fp64
 * (utils/wan_wrapper.py:175-199): head [B, F*h*w, 4*Cout] -> flow, x0 [B,F,Cout,H,W]; x0 = xt - sigma[b,f]*flow. */
int ll_unpatchify_x0(const ll_bf16* head, const ll_bf16* xt, const float* sigma, ll_bf16* flow, ll_bf16* x0, int B,
                     int F, int Cout, int H, int W, ll_stream stream);

/* FlowMatchScheduler.add_noise (utils/scheduler.py:159-176): out = bf16((1-sigma)*x0 + sigma*noise), fp32,
 * sigma[n] per leading index; x0/noise/out [N, inner]. */
int ll_add_noise(const ll_bf16* x0, const ll_bf16* noise, const float* sigma, ll_bf16* out, int N, long long inner,
                 ll_stream stream);

/* out[i] = sigmas[argmin_j |timesteps[j] - t[i]|]: the table lookup shared by flow->x0 and add_noise
 * (utils/wan_wrapper.py:195-197; utils/scheduler.py:172-174).  All fp32 device arrays; lowest index wins ties.
 * A query with no nearest entry -- t[i] NaN, or +-inf against a finite table (every distance NaN or +inf) -- gives sigmas[0], the
 * index torch.argmin returns for such a row; no query reads outside the tables. */
int ll_sigma_lookup(const float* t, const float* timesteps, const float* sigmas, float* out, int n, int n_table,
                    ll_stream stream);

/* Synthetic data for bench.py / the tests (no reference call site: the reference loads checkpoints, inference.py:72-94, and draws
 * noise with torch.randn, :193-195): out[i] (fp32, device) = the counter hash of longlive_amd/synth.py at counter lo + i under
 * stream_const -- kind 0: uniform [0, 1) with 24 bits, kind 1: Irwin-Hall normal.  Bit-identical to synth.hash_uniform /
 * hash_normal on any host (csrc/synth_hash.h is compiled for both sides; tests/test_synth_hash.py). */
int ll_synth_hash(float* out, long long lo, long long n, unsigned long long stream_const, int kind, ll_stream stream);

/* ---- VAE decoder and encoder (wan/modules/vae.py, utils/wan_wrapper.py:80-116) ------- */

/* CausalConv3d 3x3x3 / (3,1,1) / 1x1x1 and Conv2d 3x3 / 1x1 (wan/modules/vae.py:17-36; the Upsample + Conv2d pair of
 * Resample, vae.py:74-84, with upsample=1) as one implicit GEMM on channels-last activations:
 *   out[(t,ho,wo), co] = bias[co] (+ res[(t,ho,wo), co]) + sum x[t+kt-(KT-1), (ho+kh-p)>>up, (wo+kw-p)>>up, ci] * w[co, (kt,kh,kw), ci]
 * x points at the first of T new frames [T,H,W,Cin]; when KT == 3 the two frames BEFORE it in memory (x - 2*H*W*Cin
 * elements) must hold the previous two input frames of the stream -- the reference's feat_cache (vae.py:29-34) -- or
 * zeros at the start of a stream.  zero16 = 16 zero bytes on the device (source of spatial / K padding);
 * w [Cout, Kpad] bf16 with k = ((kt*KH + kh)*KH + kw)*Cin + ci, zero padded to Kpad = ceil(KT*KH*KH*Cin / 64) * 64;
 * out/res rows of ldo elements (ldo >= Cout, ldo % 4 == 0: every store is one aligned 8-byte group of 4 channels), output spatial
 * size (H<<up, W<<up).  res may alias out (a lane reads exactly the residual elements it overwrites, before it stores); x may not.
 * Reads of x stay inside the T (+ 2 history) frames; columns >= Cout of a row and rows beyond the last pixel are never written. */
int ll_conv_cl(const ll_bf16* x, const ll_bf16* zero16, const ll_bf16* w, const ll_bf16* bias, const ll_bf16* res,
               ll_bf16* out, int T, int H, int W, int Cin, int Cout, int Kpad, int KT, int KH, int upsample, int ldo,
               ll_stream stream);
/* ll_conv_cl whose epilogue also applies the RMS_norm (+ SiLU) the decoder runs on that tensor next (ResidualBlock: conv -> RMS_norm
 * -> SiLU -> conv, wan/modules/vae.py:193-220; rounding points of ll_rms_silu_cl): out_rms [pixels, Cout] = rms_silu(out), written by
 * the same launch; `out` (the un-normalised tensor, with the residual when `res`) may be NULL when nothing else reads it.  Only for
 * convolutions whose workgroup holds every channel of a pixel -- ll_conv_cl_rms_ok(...) = 1: the halo-tile kernel with Cout = 96 (the
 * 480x832 stage, 70 % of the decoder's FLOPs); otherwise run ll_conv_cl + ll_rms_silu_cl.  ldo = Cout. */
int ll_conv_cl_rms_ok(int H, int W, int Cin, int Cout, int KT, int KH, int upsample);
int ll_conv_cl_rms(const ll_bf16* x, const ll_bf16* zero16, const ll_bf16* w, const ll_bf16* bias, const ll_bf16* res, ll_bf16* out,
                   const ll_bf16* rms_gamma, ll_bf16* out_rms, int rms_silu, int T, int H, int W, int Cin, int Cout, int Kpad, int KT,
                   int KH, int upsample, int ldo, ll_stream stream);

/* RMS_norm over channels (+ SiLU) (wan/modules/vae.py:39-55,193-197) on channels-last rows with the reference's bf16
 * rounding points: n = bf16(||x||); y = bf16(bf16(bf16(x / max(n, bf16(1e-12))) * sqrt(C)) * gamma); out = silu(y) if do_silu
 * (F.normalize's clamp_min on a bf16 norm rounds its eps to bf16). */
int ll_rms_silu_cl(const ll_bf16* x, const ll_bf16* gamma, ll_bf16* out, long long pixels, int C, int do_silu,
                   ll_stream stream);

/* p[:, :N] = softmax(scale * s[:, :N]) along rows of ld elements, p[:, N:ld] = 0 (the decoder's single-head attention,
 * F.scaled_dot_product_attention at vae.py:249-254, as GEMM + softmax + GEMM). */
int ll_softmax_rows(const ll_bf16* s, ll_bf16* p, int rows, int N, int ld, float scale, ll_stream stream);

/* Latent un-scaling z / (1/std) + mean in bf16 (utils/wan_wrapper.py:99-110, wan/modules/vae.py:548-550) fused with the
 * layout change [T, C, h, w] -> channels-last [T, h, w, C]. */
int ll_vae_unscale_cl(const ll_bf16* z, const ll_bf16* mean, const ll_bf16* inv_std, ll_bf16* out, int T, int C, int h,
                      int w, ll_stream stream);

/* Decoder output: channels-last bf16 [T,H,W,ldc] (first 3 channels) -> fp32 [T,3,H,W] clamped to [-1,1]
 * (wan/modules/vae.py decode's clamp_ + utils/wan_wrapper.py:112-116). */
int ll_cl_to_tchw_clamp(const ll_bf16* x, float* out, int T, int H, int W, int ldc, ll_stream stream);

/* -- frames out ("Frames out") -- */

/* Decoder output as video frames: channels-last bf16 x [T,H,W,ldc] (first 3 channels, ldc >= 3) -> uint8 out [T,H,W,3] (rows and
 * pixels contiguous, stride_t in BYTES >= H*W*3, any alignment).  Each byte, in fp32 with no FMA contraction:
 *   trunc(255.0f * clamp(clamp((float)x, -1, 1) * 0.5f + 0.5f, 0, 1)),  NaN -> 0 (a signalling bit pattern -> 255, as below),
 * i.e. ll_cl_to_tchw_clamp, then the pipelines' `(video * 0.5 + 0.5).clamp(0, 1)` (stream_video, inference, the side decoder), then
 * the CLI's `(255.0 * video.permute(0, 1, 3, 4, 2)).to(torch.uint8)`, bit for bit, without the three fp32 passes.  Bytes of out
 * outside the T frames of H*W*3 bytes are never written. */
int ll_cl_to_frames_u8(const ll_bf16* x, uint8_t* out, long long stride_t, int T, int H, int W, int ldc, ll_stream stream);

/* Baseline JPEG (JFIF, SOF0, 8 bits, 4:2:0, Annex K Huffman tables, Annex K quantisation tables scaled by the IJG rule for quality
 * 1..100, restart interval = one row of 16 x 16 MCUs, RSTm cycling 0..7, edge replication into the padding), one complete file
 * SOI ... EOI per frame.  Replaces the uncompressed write_avi_rgb24 fallback of the CLI's write_video; arithmetic in csrc/jpeg.hip's
 * head comment, restated in tests/jpeg_ref.py.
 *
 * ll_jpeg_sizes (host only): *out_stride = the worst case of one frame = 613 header bytes + MCUs * 6 * 416 (208 bytes per block,
 * doubled by FF 00 stuffing) + 2 per restart marker + 2 for EOI, rounded up to 16; *scratch_bytes = what ll_jpeg_encode_u8 needs
 * for T frames.  H, W <= 65535; a frame whose worst case passes 2 GiB is refused. */
int ll_jpeg_sizes(int T, int H, int W, long long* out_stride, long long* scratch_bytes);
/* frames uint8 [T,H,W,3] RGB (stride_t in BYTES >= H*W*3) -> out + t * out_stride holds frame t's file, sizes[t] its length in bytes
 * (device int32 [T]); bytes of out past sizes[t] are left alone.  No allocation, no synchronisation; scratch (16-byte aligned,
 * scratch_bytes >= ll_jpeg_sizes') may hold anything: no stage accumulates in place.  Refused before any launch: null operands,
 * quality outside 1..100, T, H, W < 1, H or W > 65535, short stride_t / out_stride / scratch_bytes. */
int ll_jpeg_encode_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, int quality, uint8_t* out, long long out_stride,
                      int32_t* sizes, void* scratch, long long scratch_bytes, ll_stream stream);
/* The first stage alone: colour conversion, 8 x 8 DCT and quantisation -> coef int16 [T, ceil(H/16), ceil(W/16), 6, 64], blocks
 * Y00 Y01 Y10 Y11 Cb Cr of every MCU, each in zigzag order (what the tests pin the arithmetic with). */
int ll_jpeg_coefficients_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, int quality, int16_t* coef, ll_stream stream);

/* Lossless frames out: PNG (8 bits, colour type 2, no interlace), one complete file per frame: signature, IHDR, one IDAT per deflate
 * chunk of 16384 filtered bytes (the first begins with the zlib header 78 01), one IDAT with the Adler-32, IEND; every CRC-32 is
 * computed on the device.  Filter per row: the type of the five (bpp = 3, row 0 against a zero row) with the smallest sum of
 * min(b, 256 - b), the lower type on a tie.  DEFLATE, deterministic: literals and distance-1 matches (zlib's Z_RLE parse), one
 * dynamic-Huffman block per chunk (15-bit codes, 7-bit code-length code) followed by an empty stored block unless it is the last,
 * or a stored block when that is shorter; csrc/png.h's head comment is the definition, tests/png_ref.py its restatement.
 *
 * ll_png_sizes (host only): *out_stride = the worst case of one frame = 33 + n + 17 * ceil(n / 16384) + 2 + 28 with
 * n = H * (1 + 3 W), rounded up to 16; *scratch_bytes = what ll_png_encode_u8 needs for T frames. */
int ll_png_sizes(int T, int H, int W, long long* out_stride, long long* scratch_bytes);
/* frames uint8 [T,H,W,3] RGB (stride_t in BYTES >= H*W*3) -> out + t * out_stride holds frame t's file, sizes[t] its length in bytes
 * (device int32 [T]); bytes of out past sizes[t] are left alone.  No allocation, no synchronisation; scratch (16-byte aligned,
 * scratch_bytes >= ll_png_sizes') may hold anything.  Refused before any launch: null operands, T, H, W < 1, a frame whose worst
 * case passes 2 GiB, short stride_t / out_stride / scratch_bytes. */
int ll_png_encode_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, uint8_t* out, long long out_stride, int32_t* sizes,
                     void* scratch, long long scratch_bytes, ll_stream stream);
/* The first stage alone: out uint8 [T, H, 1 + 3 W], each row's filter type and its filtered bytes. */
int ll_png_filter_u8(const uint8_t* frames, long long stride_t, int T, int H, int W, uint8_t* out, ll_stream stream);
/* The compressor alone over T byte rows of n bytes (stride in BYTES >= n): out + t * out_stride holds row t's zlib stream (78 01,
 * the chunks, Adler-32), sizes[t] its length.  ll_zlib_sizes (host only): *out_stride = 2 + n + 5 * ceil(n / 16384) + 4 rounded up
 * to 16.  Scratch and refusals as for ll_png_encode_u8. */
int ll_zlib_sizes(int T, long long n, long long* out_stride, long long* scratch_bytes);
int ll_zlib_compress_u8(const uint8_t* src, long long stride, int T, long long n, uint8_t* out, long long out_stride, int32_t* sizes,
                        void* scratch, long long scratch_bytes, ll_stream stream);

/* Clip intake: a baseline JPEG decoder (SOF0, 8 bits; 1 component, or 3 as YCbCr with luma sampling hs x vs = 1x1, 2x1 or 2x2 and
 * chroma 1x1; any tables; any restart interval) and an antialiased resize.  The host parses the files (longlive_amd/jpeg_files.py);
 * every array below except the two size outputs is a DEVICE pointer.  Arithmetic in csrc/jpeg_dec.hip's head comment, restated in
 * tests/jpeg_dec_ref.py.  MCU grid: rows = ceil(H / (8 vs)), cols = ceil(W / (8 hs)), bpm = hs * vs + 2 blocks per MCU (1 for grey).
 *   data  uint8 [nbytes]      the frames' entropy-coded bytes, still stuffed
 *   segs  int32 [nseg, 5]     per restart segment: byte offset, byte length, frame, first MCU, MCU count
 *   huff  uint8 [T, 4, 272]   per frame (BITS[16], HUFFVAL[256]) of DC id 0, DC id 1, AC id 0, AC id 1
 *   sel   uint8 [T, 4]        per frame and component (AC id << 4) | DC id
 *   qt    uint16 [T, 3, 64]   per frame and component, natural order
 *   coef  int16 [T, rows, cols, bpm, 64]   zigzag order, blocks in scan order (for 2x2 the layout of ll_jpeg_coefficients_u8)
 *   status int32 [nseg]       0, or the JD_* code of csrc/jpeg_dec.h; a failed segment's remaining blocks are zero
 * A segment row that points outside data, the T frames or a frame's MCUs is not decoded (status 7).  Nothing checks the rows
 * against each other: rows that overlap, or that leave MCUs of a frame uncovered, leave those blocks of coef as they were.  The
 * table is the host parser's (pack_jpegs), which covers every MCU of every frame exactly once.  No allocation, no
 * synchronisation; coef, status and scratch may hold anything.  Refused before any launch: null operands, T, H, W < 1, H or W > 65535,
 * other component counts or sampling, nbytes outside 0 .. 2^31 - 1, nseg < 1, misaligned tables (4 bytes) or coef (16 bytes in the
 * entropy stage), short stride_t / scratch_bytes.
 *
 * ll_jpeg_decode_sizes (host only): *coef_bytes = the coefficient tensor, *scratch_bytes = the fp32 component planes. */
int ll_jpeg_decode_sizes(int T, int H, int W, int ncomp, int hs, int vs, long long* coef_bytes, long long* scratch_bytes);
int ll_jpeg_decode_coefficients(const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff,
                                const uint8_t* sel, int T, int H, int W, int ncomp, int hs, int vs, int16_t* coef, int32_t* status,
                                ll_stream stream);
/* coef -> out uint8 [T,H,W,3] RGB (stride_t in BYTES >= H*W*3; bytes outside the T frames are never written; grey writes Y thrice). */
int ll_jpeg_decode_pixels(const int16_t* coef, const uint16_t* qt, int T, int H, int W, int ncomp, int hs, int vs, uint8_t* out,
                          long long stride_t, void* scratch, long long scratch_bytes, ll_stream stream);
/* Both stages: three launches. */
int ll_jpeg_decode_u8(const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff, const uint8_t* sel,
                      const uint16_t* qt, int T, int H, int W, int ncomp, int hs, int vs, int16_t* coef, int32_t* status, uint8_t* out,
                      long long stride_t, void* scratch, long long scratch_bytes, ll_stream stream);
/* The split route through the entropy stage: the subsequences of a segment decode side by side (csrc/jpeg_dec.h: resumable decoder
 * and speculation policy; csrc/jpeg_dec.hip: passes).  coef and status are the serial entry points', bit for bit, for every input.
 *   subs  int32 [nsub, 3]     per subsequence: segment, byte offset inside the segment, byte length; the rows of a segment follow
 *                             one another and tile its bytes in order, segments in rising order (jpeg_files.split_segments); a
 *                             segment without rows is decoded serially
 *   rounds 1..64              resynchronisation rounds after pass 0, one launch each
 *   info  int32 [nseg]        0 = serial by table, r >= 1 = settled in round r, -1 = fell back unsettled, -2 = fell back flagged
 *                             (a bad row of subs, a block count that is not the segment's, any JD_* condition)
 *   work                      ll_jpeg_decode_split_sizes(nseg, nsub) bytes, 16-byte aligned, any content
 * Every row of subs is checked on the device before it is used.  rounds + 6 launches, no allocation, no synchronisation.  Refused
 * before any launch: what the serial entry points refuse, null operands, nsub < 1, rounds outside 1..64, misaligned or short work. */
int ll_jpeg_decode_split_sizes(int nseg, int nsub, long long* work_bytes);
int ll_jpeg_decode_coefficients_split(const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff,
                                      const uint8_t* sel, int T, int H, int W, int ncomp, int hs, int vs, int16_t* coef, int32_t* status,
                                      const int32_t* subs, int nsub, int rounds, int32_t* info, void* work, long long work_bytes,
                                      ll_stream stream);
int ll_jpeg_decode_u8_split(const uint8_t* data, long long nbytes, const int32_t* segs, int nseg, const uint8_t* huff, const uint8_t* sel,
                            const uint16_t* qt, int T, int H, int W, int ncomp, int hs, int vs, int16_t* coef, int32_t* status, uint8_t* out,
                            long long stride_t, void* scratch, long long scratch_bytes, const int32_t* subs, int nsub, int rounds,
                            int32_t* info, void* work, long long work_bytes, ll_stream stream);
/* Separable antialiased triangle-filter resize of the crop window Hc x Wc at (y0, x0) of uint8 frames [T,Hs,Ws,3] into [T,Hd,Wd,3]
 * (strides in BYTES).  Per axis the host passes, as device pointers, start int32 [out], count int32 [out] and weights fp32 [out, k]
 * (k = ky or kx, rows padded with zeros; indices relative to the window).  fp32, vertical then horizontal, no rounding in between,
 * then clamp(floor(v + 0.5), 0, 255).  The kernel clamps start and count into the window, so no table can move a read outside it. */
int ll_resize_u8(const uint8_t* src, long long src_stride_t, int Hs, int Ws, int y0, int x0, int Hc, int Wc, uint8_t* dst,
                 long long dst_stride_t, int Hd, int Wd, int T, const int32_t* ystart, const int32_t* ycount, const float* yweight, int ky,
                 const int32_t* xstart, const int32_t* xcount, const float* xweight, int kx, ll_stream stream);

/* -- planar YUV ("Planar YUV and Y4M"): BT.601 in 2^16 fixed point, limited range (full_range = 0: Y 16..235,
 * chroma 16..240) or full range (0..255); the integer arithmetic is csrc/yuv.h's, restated in tests/yuv_ref.py.  An I420 frame is
 * contiguous: the Y plane H*W, then Cb and Cr of Hc*Wc each, Hc = ceil(H/2), Wc = ceil(W/2), chroma sited at the centre of its 2 x 2
 * pixels (Y4M C420jpeg), a missing last row or column replicated; frame strides are in BYTES, any alignment.  Stream-ordered, no
 * allocation; every byte of the frames is written whole and nothing outside them.  Refused before any launch: null operands, T, H,
 * W < 1, H or W > 65535, short strides, more than one launch covers. -- */

/* frames uint8 [T,H,W,3] RGB (stride_t >= H*W*3) -> out: T I420 frames out_stride >= H*W + 2*Hc*Wc apart. */
int ll_frames_u8_to_yuv420(const uint8_t* frames, long long stride_t, int T, int H, int W, int full_range, uint8_t* out,
                           long long out_stride, ll_stream stream);
/* The decoder head's channels-last bf16 x [T,H,W,ldc] (first 3 channels, ldc >= 3) -> the same I420 frames: the bytes of
 * ll_cl_to_frames_u8 feed ll_frames_u8_to_yuv420's arithmetic in registers, bit for bit the two calls in a row. */
int ll_cl_to_yuv420(const ll_bf16* x, int T, int H, int W, int ldc, int full_range, uint8_t* out, long long out_stride, ll_stream stream);
/* Planes -> frames uint8 out [T,H,W,3] RGB (out_stride_t >= H*W*3).  layout: 0 = 4:2:0 chroma at the centre (C420jpeg, C420),
 * 1 = 4:2:0 centred vertically and co-sited horizontally (C420mpeg2), 2 = 4:2:0 co-sited on both axes (C420paldv), 3 = 4:2:2 co-sited
 * (C422), 4 = 4:4:4 (C444), 5 = luma only (Cmono: cb and cr may be NULL).  y [T] planes of H*W stride_y apart; cb, cr [T] planes of
 * the layout's chroma size (ceil(H/2) or H rows of ceil(W/2) or W) stride_c apart; the three pointers are separate, so the packed
 * payloads of a Y4M stream and loose planes both work.  Chroma is interpolated to luma resolution with weights in quarters per axis
 * (3, 1 around a centred sample; 4, 0 and 2, 2 between co-sited ones), the far sample clamped to the plane. */
int ll_yuv_to_frames_u8(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, long long stride_y, long long stride_c, int T, int H,
                        int W, int layout, int full_range, uint8_t* out, long long out_stride_t, ll_stream stream);

/* -- encoder (Encoder3d + conv1, wan/modules/vae.py:265-366, 517-543): every stride-1 convolution runs on ll_conv_cl; the two
 * strided gathers below are further gather modes of the same implicit GEMM (same LDS staging, swizzle and epilogue). -- */

/* Resample 'downsample2d' / 'downsample3d' (vae.py:87-94, 139-141): ZeroPad2d((0,1,0,1)) + Conv2d(Cin, Cout, 3, stride 2) per frame:
 *   out[t,ho,wo,co] = bias[co] + sum_{kh,kw,ci} x[t, 2ho+kh, 2wo+kw, ci] * w[co,(kh,kw),ci],  Ho = H / 2, Wo = W / 2 (H, W >= 2),
 * taps with 2ho+kh >= H or 2wo+kw >= W read zero (pad on the right and bottom only; never read when H / W is odd).  x [T,H,W,Cin],
 * w [Cout, Kpad] in ll_conv_cl's layout (KT = 1, KH = 3), out rows of ldo elements (ldo >= Cout, ldo % 4 == 0), Cin % 8 == 0,
 * Cout % 8 == 0.  Reads stay inside the T frames; columns >= Cout and rows beyond the last pixel are never written. */
int ll_conv_cl_down(const ll_bf16* x, const ll_bf16* zero16, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int T, int H, int W,
                    int Cin, int Cout, int Kpad, int ldo, ll_stream stream);
/* Resample 'downsample3d' time_conv = CausalConv3d(C, C, (3,1,1), stride (2,1,1), padding 0) over [cached last frame | chunk]
 * (vae.py:95-96, 151-158):  out[j,p,co] = bias[co] + sum_{kt,ci} x[2j+kt-1, p, ci] * w[co,kt,ci] for j < T / 2, T even.
 * x points at the first of T new frames; the ONE frame before it in memory is the stream's previous frame (feat_cache[idx][:, :, -1:]).
 * No zero padding in time; frames before x - 1 frame are never read.  w [Cout, Kpad] with KT = 3, KH = 1. */
int ll_conv_cl_tdown(const ll_bf16* x, const ll_bf16* zero16, const ll_bf16* w, const ll_bf16* bias, ll_bf16* out, int T, int H, int W,
                     int Cin, int Cout, int Kpad, int ldo, ll_stream stream);
/* Host only: kernel instance, tile, grid and k-steps of ll_conv_cl_down (kind 0) / ll_conv_cl_tdown (kind 1) as text, from the plan
 * the launcher dispatches on.  Shapes the entry points reject are rejected here. */
int ll_conv_down_plan(int kind, int T, int H, int W, int Cin, int Cout, char* out, int cap);

/* Encoder input: pixels [3,T,H,W] or [T,3,H,W] (element strides stride_c / stride_t, rows of a frame contiguous), fp32 (is_f32 = 1,
 * rounded to bf16 once: the pixel.to(bf16) of the reference's callers) or bf16 -> channels-last bf16 [T,H,W,Cpad], channels >= 3 zero;
 * Cpad in {8, 16, 32}.  encoder.conv1 (vae.py:288, 3 -> 96) then runs on ll_conv_cl with zero-padded weights. */
int ll_pixels_to_cl(const void* px, int is_f32, long long stride_c, long long stride_t, ll_bf16* out, int T, int H, int W, int Cpad,
                    ll_stream stream);

/* Encoder input from video frames: uint8 px [T,H,W,3] (rows and pixels contiguous, stride_t in BYTES >= H*W*3) -> channels-last bf16
 * [T,H,W,Cpad], channels >= 3 zero, Cpad in {8, 16, 32}, out 16-byte aligned.  Value, as a bit pattern:
 *   out = bf16_rne(fsub_rn(fdiv_rn((float)u, 127.5f), 1.0f)),
 * what `(u.float() / 127.5 - 1).to(torch.bfloat16)` gives: 0 -> -1 and 255 -> +1 exactly, no FMA contraction.  Bytes of px outside the
 * T frames of H*W*3 bytes are never read. */
int ll_pixels_u8_to_cl(const uint8_t* px, long long stride_t, ll_bf16* out, int T, int H, int W, int Cpad, ll_stream stream);

/* Latent scaling of WanVAE_.encode (vae.py:537-539) with scale = [bf16(mean), bf16(1 / bf16(std))] (utils/wan_wrapper.py:83-84), the
 * layout change and .float() (wan_wrapper.py:87): channels-last mu [T,h,w,ld] (first z_dim channels) -> fp32 [T,z_dim,h,w] =
 * float(bf16(bf16(mu - mean) * inv_std)). */
int ll_vae_scale_tchw(const ll_bf16* mu, const ll_bf16* mean, const ll_bf16* inv_std, float* out, int T, int z_dim, int h, int w, int ld,
                      ll_stream stream);

/* ---- umT5 text encoder (wan/modules/t5.py, utils/wan_wrapper.py:16-57) ----------------- */

/* T5LayerNorm.forward (wan/modules/t5.py:57-63): out = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))), fp32 statistics;
 * x, out [rows, C] contiguous, any C % 8 == 0 (4096 for umT5-xxl). */
int ll_t5_rmsnorm(const ll_bf16* x, const ll_bf16* w, ll_bf16* out, int rows, int C, float eps, ll_stream stream);

/* T5FeedForward's gated activation (t5.py:46-50,134-139): out[M,F] = bf16(h[:, F:2F] * GELU(h[:, 0:F])) with the
 * reference's python tanh-GELU evaluated op by op in bf16; h [M, 2F] = x @ [gate.0.weight; fc1.weight]^T. */
int ll_t5_gated_gelu(const ll_bf16* h, ll_bf16* out, long long M, int F, ll_stream stream);

/* token_embedding(ids) (t5.py:297): out[i, :] = table[ids[i], :]; ids int64 on the device, validated by the caller. */
int ll_gather_rows(const ll_bf16* table, const long long* ids, ll_bf16* out, int n, int C, long long vocab, ll_stream stream);

/* T5Attention.forward (t5.py:85-117), self-attention of one sequence, head_dim 64, L in {64,128,256,512} keys = queries:
 * out = bf16(softmax_fp32(bf16(bf16(q k^T) + bias), keys >= seq_len masked) v), no 1/sqrt(d) scaling.
 * q,k [L, ...] with row stride ldqk (head h at columns h*64..); vt [H*64, L] = V transposed (x Wv^T computed as
 * Wv x^T); bias_tab [H, 2L-1] with bias_tab[h, j - i + L - 1] = pos_embedding[bucket(j - i), h] (t5.py:219-263);
 * out [L, ...] row stride ldo. */
int ll_t5_attention(const ll_bf16* q, const ll_bf16* k, const ll_bf16* vt, const ll_bf16* bias_tab, ll_bf16* out, int L,
                    int H, int ldqk, int ldo, int seq_len, ll_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* LONGLIVE_HIP_H */
