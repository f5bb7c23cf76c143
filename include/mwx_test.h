/*
 * mwx_test.h — per-stage entry points of the mwx engine used by the parity
 * tests (tests/test_gpu_parity.py). They run one stage of the device hot path
 * for a single clip and copy the result back to the host as f32, so each stage
 * can be compared with the CPU oracle (oracle/) in isolation. Not used by the
 * service path.
 */
#ifndef MWX_TEST_H
#define MWX_TEST_H

#include "mwx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device log-mel of one clip. out receives [n_mels][n_len] (if out_cap is
 * large enough); returns n_len, or <0 on error. */
int mwx_test_mel(struct mwx_context* ctx, struct mwx_state* state, const float* pcm, int n,
                 float* out, long out_cap);

/* mel + conv stem + encoder + cross K/V of one clip at `seek`. enc_out:
 * [n_audio_ctx][n_audio_state] (encoder output after ln_post, as stored on the
 * device); k_out / v_out (nullable): [n_text_layer][n_audio_ctx][n_text_state]
 * cross K/V. The cross K/V stay resident in `state` for mwx_test_decode. */
int mwx_test_encode(struct mwx_context* ctx, struct mwx_state* state, const float* pcm, int n,
                    int seek, float* enc_out, float* k_out, float* v_out);

/* mwx_test_encode at an audio context of audio_ctx = K frames (1 ..
 * n_audio_ctx; else -5; mwx_full_params.audio_ctx): enc_out [K][n_audio_state],
 * k_out / v_out [n_text_layer][K][n_audio_state]. The cross K/V and the key
 * count K stay resident in `state` for mwx_test_decode* / mwx_test_dtw_align. */
int mwx_test_encode_ctx(struct mwx_context* ctx, struct mwx_state* state, const float* pcm, int n,
                        int seek, int audio_ctx, float* enc_out, float* k_out, float* v_out);

/* Teacher-forced decoder run against the cross K/V left by mwx_test_encode:
 * token i at position i, logits_out [n][n_vocab] (raw logits). */
/* The encoder of one clip window with its intermediates copied out: x_out
 * [n_audio_layer + 1][n_audio_ctx][n_audio_state] f32 = the residual stream
 * after the conv stem and after each layer; a_out[0..3] = per layer the four
 * GEMM A operands as the model's 16-bit type (raw bits), before any MX-fp8
 * quantization: attention LayerNorm out, attention out, MLP LayerNorm out
 * ([L][n_ctx][d] each) and GELU out ([L][n_ctx][4 d]). */
int mwx_test_encode_dump(struct mwx_context* ctx, struct mwx_state* state, const float* pcm,
                         int n, int seek, float* x_out, uint16_t* const* a_out);

int mwx_test_decode(struct mwx_context* ctx, struct mwx_state* state, const int* tokens, int n,
                    float* logits_out);

/* As mwx_test_decode_last, with tokens 0 .. n-2 run by the batched prompt
 * prefill (one pass of the layer stack) and only token n-1 as a decode step. */
int mwx_test_decode_last_prefill(struct mwx_context* ctx, struct mwx_state* state,
                                 const int* tokens, int n, float* logits_last);

/* Self-attention K / V cache of row 0 of a state for one decoder layer,
 * positions 0 .. n_pos-1, as f32 [n_pos][n_text_head][64] each. */
int mwx_test_self_kv(struct mwx_state* state, int layer, int n_pos, float* k_out, float* v_out);

/* The engine's load-time dequantizer (host code, no device work): n values
 * of ggml block type `type` (legacy q4_0 .. q8_0 or K q2_K .. q6_K; n a
 * multiple of the block) from src into dst as f32, before the f16 rounding
 * of the upload. Returns 0, or -1 for an unsupported type / length. */
int mwx_test_dequantize(int type, const void* src, long n, float* dst);

/* Decode work counters of a state (the first state of a batch drives it):
 * decode steps launched and prompt positions run by the batched prompt
 * prefill since the last reset. reset != 0 zeroes them after reading. */
int mwx_test_decode_counters(struct mwx_state* state, long* steps, long* prefill_positions,
                             int reset);

/* Window counters of a state (the first state of a batch drives it): clip
 * windows decoded, decode attempts run (one per window and temperature
 * tried, so attempts - windows = temperature-fallback re-runs) and decode
 * steps summed over the clips live in each (each such clip-step reads the
 * clip's cross K/V once per layer) since the last reset. reset != 0 zeroes
 * them after reading. */
int mwx_test_window_counters(struct mwx_state* state, long* windows, long* attempts,
                             long* clip_steps, int reset);

/* Run-ahead decode attempts a state redid on the host-driven token loop
 * because the device's advance and the host's replay disagreed (or
 * MWX_TEST_RA_MISMATCH=k forced it at step k). reset != 0 zeroes it. */
long mwx_test_runahead_fallbacks(struct mwx_state* state, int reset);

/* As mwx_test_decode, but only the logits of the last token are copied out
 * (logits_last [n_vocab]). */
int mwx_test_decode_last(struct mwx_context* ctx, struct mwx_state* state, const int* tokens,
                         int n, float* logits_last);

/* One MX-fp8 GEMM as the fp8 compute mode runs it: a [M][K] is rounded to
 * bf16 and quantized by the device kernel, w [N][K] by the load-time host
 * quantizer, c [M][N] = the block-scaled fp8 MFMA product (f32). K % 128 == 0.
 * Returns 0 or <0. */
int mwx_test_gemm_mx(struct mwx_context* ctx, int M, int N, int K, const float* a,
                     const float* w, float* c);

/* The encoder FFN1 GEMM with its GELU epilogue on given data: a [M][K] and
 * w [N][K] rounded to bf16 (bf16 != 0) or f16, bias [N]; out [M][N] =
 * gelu_ggml(a.w + bias) in that type, widened to f32. use_table: the f16 GELU
 * table looked up from LDS (the engine's path) or tanhf per output. N % 64 ==
 * 0, K % 64 == 0. Returns 0 or <0. */
int mwx_test_gemm_gelu(struct mwx_context* ctx, int M, int N, int K, const float* a,
                       const float* w, const float* bias, int bf16, int use_table, float* out);

/* std::discrete_distribution draws on the device (k_misc.hip sample_draws):
 * probs / logprobs [R][V], u [R][KD] (generate_canonical<double, 53> values),
 * ndraw [R] (<= KD <= 16); ids [R][KD] out. exact != 0 runs only the
 * sequential-order kernel. reps > 1 repeats the launch and returns the mean
 * microseconds per launch in *us (HIP events). Returns 0 or <0. */
int mwx_test_sample_draws(struct mwx_context* ctx, const float* probs, const float* logprobs,
                          int R, int V, const double* u, const int* ndraw, int KD, int exact,
                          int reps, int* ids, double* us);

/* MX-fp8 grouped cross-attention scores and P.V on MFMA (1, the default) or
 * the v_dot2 kernel (0); -1 restores the MWX_XATTN_MFS default. Returns the
 * previous setting. */
int mwx_test_set_xattn_mfs(int on);

/* Decode GEMMs at more than 64 rows (beam / best-of decoders of many clips):
 * the shared-A kernels (1, the default) or the per-strip grids (0); -1
 * restores the MWX_DEC_SHARED default. Returns the previous setting. */
int mwx_test_set_dec_shared(int on);

/* The encoder GEMM's 8-phase main loop (bit-identical to the default 2-stage
 * ring) on (1) / off (0) / back to the MWX_GEMM_8PH environment default (-1).
 * Returns the previous mode. */
int mwx_test_set_gemm_8ph(int on);

/* The decode LayerNorms folded into the GEMM that consumes them: those before
 * the QKV and cross-Q projections into the split-K GEMMs (gemm_splitk_ln) and
 * the one before FFN1 into the full-K GEMM with the GELU epilogue
 * (gemm_decode_ln), each bit-identical to the separate LayerNorm launch. The
 * fold applies only to single-row decode steps that are not a prompt prefill;
 * every other step launches the LayerNorms on their own whatever the mode.
 * On (1) / off (0) / back to the MWX_LN_FOLD environment default, on (-1).
 * Read when a decode step is captured. Returns the previous mode. */
int mwx_test_set_ln_fold(int on);


/* The MX-fp8 cross K/V cache's widening of e4m3 codes to f16 as the
 * cross-attention kernels run it: n8 groups of 8 codes (codes[8 n8]), each
 * group with one E8M0 exponent (e8[n8]); out[8 n8] = f16 bits. */
int mwx_test_mx_widen(struct mwx_context* ctx, const uint8_t* codes, const uint8_t* e8, int n8,
                      uint16_t* out);

/* Fault injection of the run-ahead safety net: run-ahead step `step` of every
 * later attempt is treated as a device/host disagreement (-1: none; -2: back
 * to the MWX_TEST_RA_MISMATCH environment default). Returns the previous
 * setting. */
long mwx_test_set_ra_mismatch(long step);

/* The MX-fp8 grouped cross-attention kernel on given data: q [R][H*64] f32
 * queries (rounded to f16 by the kernel), K / V as e4m3 codes [R/nq][H][n][64]
 * with E8M0 scales [R/nq][H][n][2] (one per 32-element half), rows
 * g*nq .. g*nq+nq-1 reading slot g; o [R][H*64] f32 = the kernel's 16-bit
 * output (the context's weight type). Scores / P.V on MFMA or v_dot2 per
 * mwx_test_set_xattn_mfs. Returns 0 or <0. */
int mwx_test_xattn_mx(struct mwx_context* ctx, int R, int H, int n, int nq, const float* q,
                      const uint8_t* k8, const uint8_t* ks, const uint8_t* v8, const uint8_t* vs,
                      float* o);

/* One decode attention launch on given data, for an f64 reference at chosen
 * positions (tests/test_gpu_decode_kernels.py). bf16 selects the kernels'
 * weight / output type (bf16 or f16) whatever the context's model holds.
 * fixed_len == 0: self-attention (dec_attention<T>, pcols = 3 H 64, row r
 * attends positions 0 .. pos[r], appending its own); prefill != 0: kv_append<T>
 * first, then dec_attention with write_new = 0. fixed_len > 0: cross-attention
 * over fixed_len keys (pcols = H 64), by dec_attention<T>, or with grouped != 0
 * by dec_cross_attention_grouped<T> on the f16 caches (nq 2..8, qscale 1).
 *   P [KS][R][pcols] f32 split-K slabs, bias [pcols];
 *   kcache / vcache [slots][H][cap][64] f16 bits, in and out (the caches as
 *     they are after the launch);
 *   kv_index [R] (nullable: row r uses slot r), pos [R] (self), active [R];
 *   kvmap [R][cap] and own_from [R] (self, both or neither): position
 *     j < own_from[r] of row r is read from slot kvmap[r][j] - map_row0;
 *   o [R][H 64] f32 = the 16-bit output unpacked from the pack_index layout;
 *     a row the launch did not write is NaN.
 * Every index is checked on the host first: -1 without a launch unless
 * R <= 1024, H <= 32, slots <= 64 (R <= slots without kv_index),
 * KS in 1..8, nq in 1..8, R % nq == 0, cap <= 1536, fixed_len <= cap, and for
 * every row (active or not) kv_index in [0, slots), pos < cap, own_from <= pos
 * and each used kvmap word - map_row0 in [0, slots). Returns 0, -1 (arguments),
 * -2 (device error) or -4 (group size the grouped kernel does not serve). */
int mwx_test_dec_attn(struct mwx_context* ctx, int bf16, int grouped, int prefill, int R, int H,
                      int cap, int slots, int KS, int nq, int fixed_len, const float* P,
                      const float* bias, float qscale, float kscale, float scale,
                      uint16_t* kcache, uint16_t* vcache, const int* kv_index, const int* pos,
                      const int* active, const int* kvmap, const int* own_from, int map_row0,
                      float* o);

/* One decode GEMM on given 16-bit weights: a [M][K] and w [N][K] are rounded
 * to bf16 (bf16 != 0) or f16 and packed as fragment tiles (pack_index; a
 * zero-padded to a multiple of 64 rows, w to a multiple of 16 columns, as the
 * engine's buffers are). mode 0: gemm_splitk_partials<T>, *ks_out = KS and
 * out = the slabs P [KS][M][N] (room for 8 M N floats); mode 1: gemm_decode<T>
 * with EPI_F32, out = c [M][N]; mode 2: gemm_decode<T> with EPI_RES, out =
 * (a.w + bias[n]) + res[m][n] (bias nullable; modes 0 / 1 take neither).
 * The device output starts as sentinel words between two guard bands of them.
 * Returns 0, -1 (arguments; K % 32, M <= 512, N <= 4096, K <= 8192), -2
 * (device error), -3 (the launch changed a guard band) or -4 (K not served by
 * the kernel family). */
int mwx_test_gemm_dec(struct mwx_context* ctx, int bf16, int mode, int M, int N, int K,
                      const float* a, const float* w, const float* bias, const float* res,
                      int* ks_out, float* out);

/* The rest of the decode GEMM family through the same launchers
 * (mwx_test_gemm_dec is this hook with w8 = ln = 0 and mode 0 .. 2). In
 * whatever context: the kernels take their operands directly.
 * mode 3: gemm_decode<T> with EPI_GELU and pack_out (the decode FFN1
 *   epilogue), ldc = N, N % 32 == 0, bias [N] required: T(gelu_ggml(a.w +
 *   bias[n])) at pack_index(m, n, N) of a buffer of ceil64(M) N 16-bit words,
 *   which starts as 0xFFFF words; out16 receives all of it, out the rows
 *   < M unpacked and widened to f32 [M][N].
 * w8 != 0: MX-fp8 weights instead of w: e4m3 codes wq [N][K] and E8M0 scales
 *   ws [N][K / 32] (any bytes), placed in fragment tiles by the model loader's
 *   packer (mx_pack_dec_weight). bf16 only, as the engine enables them: -4
 *   with bf16 == 0, before any launch.
 * ln != 0 (M = 1, mode 0 or 3): the A operand is the folded LayerNorm
 *   (gemm_splitk_ln<T> / gemm_decode_ln<T>) of x_in [K] + (the sum of the KS
 *   slabs P [KS][K] + pbias [K]; KS = 0 .. 8, both NULL at 0), weight ln_w and
 *   bias ln_b [K], active [1]; a is not read. x_out [K] receives the residual
 *   buffer the launch wrote (it starts as sentinel words 0x7fc5a5a5 between
 *   guard bands) and x_in is read back from the device after the launch. A
 *   launcher that returns 0 / false (K not served by the fold) gives -4.
 * ks_out (nullable): KS of mode 0, else 1. out: 8 M N floats of room in mode
 * 0, M N otherwise. Every device output starts as sentinel words between two
 * guard bands. Returns 0, -1 (a missing pointer, K % 32, N % 32 in mode 3,
 * ln with M != 1 or a mode other than 0 / 3, KS outside 0 .. 8, bias / res
 * given to a mode that takes none, M > 512, N > 4096, K > 8192), -2 (device
 * error), -3 (a guard band changed) or -4 (shape or type not served). */
struct mwx_test_gemm_dec_args {
  int bf16, mode, w8, ln;
  int M, N, K, KS;
  const float* a;       /* [M][K] (ln == 0) */
  const float* w;       /* [N][K] (w8 == 0) */
  const uint8_t* wq;    /* [N][K] (w8 != 0) */
  const uint8_t* ws;    /* [N][K / 32] */
  const float* bias;    /* [N]: mode 2 (nullable), mode 3 */
  const float* res;     /* [M][N]: mode 2 */
  float* x_in;          /* ln: [K], in; read back after the launch */
  const float* P;       /* ln: [KS][K] */
  const float* pbias;   /* ln: [K] */
  const float* ln_w;
  const float* ln_b;
  const int* active;    /* ln: [1] */
  float* x_out;         /* ln: [K], out */
  int* ks_out;
  float* out;
  uint16_t* out16;      /* mode 3: [ceil64(M) N] */
};
int mwx_test_gemm_dec_ex(struct mwx_context* ctx, const struct mwx_test_gemm_dec_args* args);

/* The load-time MX-fp8 quantizer (mx_quantize_row; host code, no device work):
 * x [rows][K] f32, K % 32 == 0, into e4m3fn codes q [rows][K] and E8M0 scales
 * s [rows][K / 32]. Per 32 values: scale 2^e, e the smallest integer with
 * amax <= 448 2^e (clamped to -127 .. 127; 0 for an all-zero block), codes
 * the round-to-nearest-even of x / 2^e. Returns 0, or -1. */
int mwx_test_mx_quantize_rows(const float* x, int rows, int K, uint8_t* q, uint8_t* s);

/* --- encoder kernels on given data (tests/test_gpu_encoder_kernels.py) ------
 * Every hook below checks every size and index on the host (-1 without a
 * launch), keeps each device output between two guard bands of sentinel words
 * (-3 if a launch changed one), and returns -2 on a device error and -4 for a
 * shape the kernel family does not serve. bf16 selects the kernels' 16-bit
 * type T (bf16 or f16) whatever the context's model holds. */

/* One enc_attention<T> launch. q, k: f16 bits [B][H][L][64]; vt: f16 bits
 * [B][H][64][Lp], Lp = (L + 7) & ~7, the pad columns [L, Lp) supplied by the
 * caller; lens (nullable) [B]: clip b attends over its first lens[b] frames
 * (the VL instantiation). o: f32 [B L][H 64] = the T output widened; a word
 * the launch did not write is NaN. The kernel reads the V^T columns [L, Lp)
 * (under lens: [lens[b], L) too) and multiplies them by an exact zero: they
 * must be finite (never NaN or Inf); Q and K rows >= lens[b] are never read.
 * -1 unless B H <= 64, 1 <= L <= 1536 and every lens[b] in 1 .. L. */
int mwx_test_enc_attn(struct mwx_context* ctx, int bf16, int B, int H, int L, const int* lens,
                      float scale, const uint16_t* q, const uint16_t* k, const uint16_t* vt,
                      float* o);

/* One encoder GEMM launch (gemm<T>, the 256 x 256 tile kernel with its staged
 * epilogues). a (a_len floats) and w [N][K] are rounded to T on the host; row m
 * of batch z of A starts at a + z a_bstride + m lda (rows may overlap, lda < K:
 * the conv stem's im2col view). epi is the EPI_* value of csrc/kernels.h:
 *   1 EPI_GELU   c16 (c_len 16-bit words, in and out) receives
 *                T(gelu_ggml(acc + bias)) (out16 != 0: f16 whatever T is) at
 *                c_off + z c_bstride + m ldc + n; use_table: the GELU table.
 *   2 EPI_RES    c32 (c_len floats, in and out; the residual is read in place
 *                as the engine calls it) = (acc + bias) + c32, bias nullable.
 *   3 EPI_CONV2  c32 = pe[m][n] + gelu_ggml(acc + bias), pe [M][ldc].
 *   0 EPI_ENC_QKV  N = 3 d, H 64 = d: q, k f16 bits [M / L][H][L][64] and v =
 *                V^T [M / L][H][64][ldv] (in and out: the columns >= L keep
 *                what the caller put there). -1 unless L % 4 == 0, M % L == 0,
 *                ldv % 4 == 0, ldv >= L (the 8-byte V^T stores).
 *   5 EPI_CROSS_KV N = layers 2 d: k, v f16 bits [layers][ncap][H][lcap][64] (in
 *                and out), clip b = m / L goes to slot[b] (injective, in
 *                [0, ncap)), K = f16(acc kscale), V = f16(acc + bias). With
 *                kv8 != 0 the cache is MX-fp8 instead: k8, v8 e4m3 codes in
 *                that shape and ks8, vs8 [layers][ncap][H][lcap][2] E8M0 scales
 *                (one per 32-element half), all in and out; k, v unused.
 * mx != 0: the MX-fp8 compute mode, mx_quantize<T> of the T-rounded a (dense:
 * lda = K, batch = 1) followed by gemm_mx<T> on w quantized by the load-time
 * host quantizer, as mwx_test_gemm_mx runs it; K % 128 == 0, epi 0, 1 (T
 * output), 2 or 5.
 * -1 unless M <= 4096, N <= 2048, K <= 5120, batch <= 8, K % 64 == 0,
 * N % 64 == 0, d % 64 == 0, lda, a_bstride, ldc, c_bstride and c_off are
 * multiples of 8 (16-byte vector accesses), the last A element read lies
 * inside a_len and the last output inside c_len. */
struct mwx_test_gemm_enc_args {
  int bf16, epi, out16, use_table, mx, kv8;
  int M, N, K, batch;
  long lda, a_bstride, a_len;
  long ldc, c_bstride, c_off, c_len;
  int L, H, d, ldv, lcap, ncap;
  float kscale;
  const float* a;
  const float* w;
  const float* bias;
  const float* pe;
  const int* slot;
  uint16_t* c16;
  float* c32;
  uint16_t* q;
  uint16_t* k;
  uint16_t* v;
  uint8_t* k8;
  uint8_t* v8;
  uint8_t* ks8;
  uint8_t* vs8;
};
int mwx_test_gemm_enc(struct mwx_context* ctx, const struct mwx_test_gemm_enc_args* args);

/* layer_norm<T> (dec == 0) or layer_norm_dec<T> (dec != 0) on x [M][N] (in
 * and out), w, b [N], active (nullable) [M], P (nullable) [KS][M][N] with
 * pbias [N]. dec with te != NULL (EmbedIn): x is first formed as
 * T(te[tok[r]]) + pe[pos[r]], te [n_tok][N] (rounded to T), pe [n_pos][N],
 * tok / pos [M] (any value: the kernel clamps them). y [M][N] f32 = the T
 * output (dec: unpacked from the pack_index layout); a row the launch did not
 * write is NaN. -4 for N > 2048 (layer_norm launches nothing there) and, dec,
 * N % 32 != 0 (pack_index tiles are 32 deep). -1 unless M <= 1024, KS 1 .. 8. */
int mwx_test_layer_norm(struct mwx_context* ctx, int bf16, int dec, int M, int N, float* x,
                        const float* w, const float* b, const int* active, const float* P, int KS,
                        const float* pbias, const float* te, const float* pe, const int* tok,
                        const int* pos, int n_tok, int n_pos, float* y);

/* The context's device-built f16 GELU table: entry i < 0x4901 = the f16 bits
 * of gelu(h) for the f16 h with bits i, entry 0x4901 + i for bits 0x8000 | i.
 * out receives mwx_test_gelu_table_size() words. */
int mwx_test_gelu_table_size(void);
int mwx_test_gelu_table(struct mwx_context* ctx, uint16_t* out);

/* vad_segments_kernel on caller-supplied probabilities: clip b has
 * mwx_vad_n_chunks(n_samples[b]) of them at probs + probs_offset[b] and its own
 * params[b]. Out: n_segments[b], compact_len[b], its segments as (start, end)
 * pairs at segments + 2 * out_offset[b] and its pieces as (src, len, dst)
 * triples at pieces + 3 * out_offset[b]; room for as many entries as the clip
 * has chunks. Returns 0 or < 0. */
int mwx_test_vad_segments(struct mwx_vad_context* vctx, const struct mwx_vad_params* params,
                          const float* probs, const int* probs_offset, const int* n_samples,
                          int n_clips, int* n_segments, int64_t* compact_len, int64_t* segments,
                          int64_t* pieces, const int* out_offset);

/* Copies a compacted clip of a trimmed batch to the host. Returns its sample
 * count, or < 0 on bad arguments, cap too small or a device error. */
int64_t mwx_test_vad_trimmed_pcm(const struct mwx_vad_trimmed* t, int clip, float* out,
                                 int64_t cap);

/* --- DTW token timestamps (mwx_context_params.dtw_token_timestamps) -------- */

/* align_qk_kernel on given data: for every row r with active[r] and
 * pos[r] >= pos0, and every pair heads[i] = (head, a), the softmax over n_keys
 * keys of scale * q.k, q = f16((sum of the KS slabs of P [KS][R][H 64] +
 * bias [H 64]) * qscale), keys of slot kv_index[r]. k: f16 bits
 * [slots][H][n_keys][64], or with mx != 0 e4m3 codes in that shape with kscale
 * [slots][H][n_keys][2] E8M0 (one per 32-element half), widened as the grouped
 * cross-attention widens them. The cross cache is f16 (or MX) for f16 and
 * bf16 models alike, so there is no bf16 variant. out
 * [slots][A][n_rows_cap][n_keys] f32, in and out: row (kv_index[r], a,
 * pos[r] - pos0) is written, every other word keeps what the caller put there.
 * Indices are checked on the host: -1 without a launch. 0, -1, -2 (device
 * error) or -4 (shape the kernel does not serve). */
int mwx_test_align_probs(struct mwx_context* ctx, int mx, int R, int H, int KS, int n_keys,
                         int slots, int n_heads, const int* heads, int A, int pos0,
                         int n_rows_cap, const float* P, const float* bias, float qscale,
                         float scale, const void* k, const uint8_t* kscale, const int* kv_index,
                         const int* pos, const int* active, float* out);

/* dtw_cost_kernel: w [B][A][n_rows_cap][n_keys] probabilities, clip b uses
 * rows 0 .. Ns[b]-1 and columns 0 .. Ts[b]-1; cost: clip b's [Ns[b]][Ts[b]]
 * matrix (rows compact) at cost + b * n_rows_cap * max(Ts). */
int mwx_test_dtw_cost(struct mwx_context* ctx, int B, int A, int n_rows_cap, int n_keys,
                      const int* Ns, const int* Ts, const float* w, float* cost);

/* dtw_path_kernel on B cost matrices in one launch: clip b's [Ns[b]][Ts[b]]
 * matrix (rows compact) at cost + b * max(Ns) * max(Ts). frames [B][max(Ns)]:
 * the path's first column in each row; path [B][max(Ns) + max(Ts)][2]: the
 * path's (row, column) pairs in order, right-aligned, path_len[b] of them.
 * Ns <= 256, Ts <= 1536. */
int mwx_test_dtw_path(struct mwx_context* ctx, int B, const int* Ns, const int* Ts,
                      const float* cost, int* frames, int* path, int* path_len);

/* A state keeps (on != 0) the results of every DTW pass of its next
 * mwx_full* calls on the host: one pass per 30-s window that emitted
 * segments. Returns the previous setting. */
int mwx_test_dtw_keep(struct mwx_state* state, int on);
int mwx_test_dtw_n_passes(struct mwx_state* state);
/* Pass `pass` of the state's last call: dims = {N, T, A, n_audio_ctx}, the
 * window's seek, probs [A][N][n_audio_ctx], cost [N][T], frames [N] (each
 * nullable; *_cap = room in elements). */
int mwx_test_dtw_last(struct mwx_state* state, int pass, int* dims, int64_t* seek, float* probs,
                      long probs_cap, float* cost, long cost_cap, int* frames, long frames_cap);

/* The DTW alignment pass (teacher-forced, positions 0 .. n-1, the alignment
 * rows from pos0 on, n_cols columns) over the cross K/V that mwx_test_encode
 * left in `state`, in a context with DTW on; the result is pass 0 of
 * mwx_test_dtw_last. Returns 0 or < 0. */
int mwx_test_dtw_align(struct mwx_context* ctx, struct mwx_state* state, const int* tokens, int n,
                       int pos0, int n_cols);

/* vad_segments_kernel, then vad_chunks_kernel on
 * caller-supplied probabilities, laid out as for mwx_test_vad_segments; clip b
 * is packed with its own cap caps[b] >= 1 in samples. Out: n_chunks[b] and its
 * chunks as (first piece, n pieces, start, len) at chunks + 4 * out_offset[b];
 * room for as many entries as the clip has 512-sample chunks. Returns 0 or < 0. */
int mwx_test_vad_chunks(struct mwx_vad_context* vctx, const struct mwx_vad_params* params,
                        const int64_t* caps, const float* probs, const int* probs_offset,
                        const int* n_samples, int n_clips, int* n_chunks, int64_t* chunks,
                        const int* out_offset);

/* vad_stream_scan_kernel (the online scan of a stream) on
 * caller-supplied probabilities that bypass the net: a stream of `vctx` with
 * `params` receives the n_probs probabilities as whole chunks in n_splits
 * calls of splits[k] >= 0 chunks each (their sum = n_probs). Out: *n_events and
 * the events as (start, end, closed_at) triples (room for n_probs of them),
 * and state[6] = the scan's registers after the last call (trig, start,
 * temp_end, prev_end, next_start, chunk count). The tail rule is not applied.
 * Returns 0 or < 0. */
int mwx_test_vad_stream_scan(struct mwx_vad_context* vctx, const struct mwx_vad_params* params,
                             const float* probs, int n_probs, const int* splits, int n_splits,
                             int* n_events, int64_t* events, int64_t* state);

/* --- logits processing on given data (tests/test_gpu_logits_kernels.py) ---- */

/* RowCtl (csrc/kernels.h) of one row, as plain ints plus the temperature. */
struct mwx_test_logits_ctl {
  int active, sample, is_initial, last_ts, penult_ts, has_ts, seek_delta, want_probs, want_nosp;
  float temperature;
};
/* LogitsConst (csrc/kernels.h). */
struct mwx_test_logits_const {
  int n_vocab, eot, beg, space_id, suppress_blank, max_initial_tid, nosp_id;
};
/* TokOut (csrc/kernels.h) without its pad word. */
struct mwx_test_logits_out {
  int id, tid;
  float p, plog, pt, ptsum, nosp;
};

/* One logits_process(..., pick = true) call (lp_filter_kernel, lp_probs_kernel,
 * lp_pick_kernel) on R rows of V raw logits [R][V], the static mask smask [V]
 * (< 0: suppressed), ctl [R] and *lc. Out: flt, probs, logprobs [R][V] and
 * out [R]. The hook owns every device buffer (probs and logprobs included).
 * Every output starts as all-ones bits (NaN; id = tid = -1), so a row whose
 * ctl has active = 0 or sample = 0, and probs / logprobs of a row without
 * want_probs, come back as such. Each device output, the chunk records
 * included, lies between two guard bands of sentinel words.
 * Returns 0; -1 without a launch unless 1 <= R <= 256, 1 <= V == lc->n_vocab,
 * eot, space_id and nosp_id in [0, V), beg in [0, V] and every seek_delta >= 0;
 * -4 (no launch) for V > LP_G * LP_CHUNK = 53248; -2 on a device error; -3 if
 * a launch changed a guard band. */
int mwx_test_logits_process(struct mwx_context* ctx, int R, int V, const float* logits,
                            const float* smask, const struct mwx_test_logits_ctl* ctl,
                            const struct mwx_test_logits_const* lc, float* flt, float* probs,
                            float* logprobs, struct mwx_test_logits_out* out);

/* The engine's own LogitsConst and static suppression mask for a call with
 * *params (the functions the decode driver calls; host code, no device work):
 * *lc and smask [n_vocab] (0 or -inf). Returns 0, or -1 on a null argument. */
int mwx_test_logits_setup(struct mwx_context* ctx, const struct mwx_full_params* params,
                          struct mwx_test_logits_const* lc, float* smask);

/* --- transcript scoring on given data (tests/test_gpu_score_kernel.py) ----- */

/* One score_rows launch (csrc/k_score.hip) on R rows of V raw
 * logits [R][V] with target [R] and active [R]. Out, [R] each: plog, p, top_id,
 * top_plog. The hook owns the device buffers; the output records start as
 * all-ones bits (NaN; top_id = -1), so an inactive row comes back as such, and
 * lie between two guard bands of sentinel words. Returns 0; -1 without a
 * launch unless 1 <= R <= 4096, 1 <= V <= 53248 and every target in [0, V);
 * -2 on a device error; -3 if the launch changed a guard band. */
int mwx_test_score_rows(struct mwx_context* ctx, int R, int V, const float* logits,
                        const int* target, const int* active, float* plog, float* p, int* top_id,
                        float* top_plog);

/* Rows per block of mwx_align_batch's logits buffer (default 256; 0 restores
 * it). Returns the previous value. The result of mwx_align_batch does not
 * depend on it. */
int mwx_test_set_score_rows_cap(int rows);

/* --- language identification (tests/test_gpu_lang_kernel.py, _detect.py) --- */

/* One lang_probs launch (csrc/k_lang.hip, DESIGN.md "Language identification")
 * on R rows of V raw logits [R][V], over the n entries from t0 of each row.
 * Out: probs [R][n], best [R]. The hook owns the device buffers; both outputs
 * lie between two guard bands of sentinel words. Returns 0; -1 without a
 * launch, the outputs untouched, for a null argument, R <= 0, n outside
 * 1..128, t0 < 0 or t0 + n > V; -2 on a device error; -3 if the launch changed
 * a guard band. */
int mwx_test_lang_probs(struct mwx_context* ctx, int R, int V, const float* logits, int t0, int n,
                        float* probs, int* best);

/* A state keeps (on != 0) the language-logit row that the detection pass of
 * its next mwx_full* / mwx_align_batch calls feeds lang_probs for it. Returns
 * the previous setting. */
int mwx_test_lang_keep(struct mwx_state* state, int on);
/* That row of the state's last call: mwx_lang_max_id() + 1 raw logits into
 * logits_out (room for n). Returns their number; 0 when the call kept none
 * (no detection for this state, or keeping off); -1 bad arguments. */
int mwx_test_lang_last(struct mwx_state* state, float* logits_out, int n);

/* --- contextual biasing (tests/test_bias_ref.py, test_gpu_bias_kernel.py) -- */

/* The matcher tables of n phrases (csrc/bias.h) and the host
 * transition: needs no context and does no device work. Walks hist [n_hist]
 * from the root and writes the state's (token, bias) set, tokens ascending,
 * into tokens_out / boosts_out (room for cap each; nullable with cap 0) and
 * the tables' size in bytes into *table_bytes_out (nullable). Returns the
 * set's size (which may exceed cap: then only cap pairs are written), or the
 * code mwx_full_batch would refuse the phrases with (-1; -3 for a negative id: no
 * vocabulary is known here), or -1 for n_hist < 0 or
 * hist == NULL with n_hist > 0. */
int mwx_test_bias_match(const struct mwx_bias_phrase* phrases, int n,
                        const mwx_token* hist, int n_hist, mwx_token* tokens_out,
                        float* boosts_out, int cap, long long* table_bytes_out);

/* The id of that state (root = 0; ids are breadth-first over the phrases'
 * trie), as the host's walk gives it; the refusal codes of mwx_test_bias_match. */
int mwx_test_bias_state(const struct mwx_bias_phrase* phrases, int n, const mwx_token* hist,
                        int n_hist);

/* One logits_bias launch (csrc/k_bias.hip) on R rows of V logits [R][V]. Rows
 * start at the root; a small kernel walks row r's history hist[r][0 ..
 * hist_len[r]) (hist is [R][H]) with the __device__ transition the advance
 * kernels use, then logits_bias runs once with active [R] and sample [R].
 * Out: logits_out [R][V], state_out [R]. The hook owns the device buffers;
 * both outputs lie between two guard bands of sentinel words. Returns 0; -1
 * without a launch for a null argument, R outside 1..256, V < 1, H < 0, a
 * hist_len outside 0..H, or phrases mwx_full_batch would refuse (ids checked
 * against V); -2 on a device error; -3 if a launch changed a guard band. */
int mwx_test_logits_bias(struct mwx_context* ctx, const struct mwx_bias_phrase* phrases, int n,
                         int R, int V, const float* logits, const mwx_token* hist, int H,
                         const int* hist_len, const int* active, const int* sample,
                         float* logits_out, int* state_out);

/* --- constrained decoding (tests/test_constraint_ref.py,
 * test_gpu_constraint_kernel.py) ----------------------------------------- */

/* A constraint (csrc/constraint.h) built from choices (texts !=
 * NULL: mwx_constraint_from_choices(texts, n, flags)) or else from a DFA
 * (mwx_constraint_from_dfa(n_states, start, trans, accepting)), walked with the
 * class-compressed table over bytes [n_bytes] from state `from` (< 0: the
 * start). Needs no context and does no device work. Returns the state reached
 * (0 = dead), or -1 when the constraint is refused or for n_bytes < 0 or
 * bytes == NULL with n_bytes > 0. Nullable outputs: the state's accepting flag,
 * the number of states (the dead one included), the number of byte classes,
 * and the size in bytes of the block the device reads. */
int mwx_test_constraint_walk(const char* const* texts, int n, int flags, int n_states, int start,
                             const uint16_t* trans, const uint8_t* accepting, int from,
                             const uint8_t* bytes, int n_bytes, int* accepting_out,
                             int* n_states_out, int* n_classes_out, long long* table_bytes_out);

/* One logits_constrain launch (csrc/k_constrain.hip) on R rows with the given
 * constraint states, active [R] and sample [R]. The token byte table is the
 * context's own vocabulary (tok_off == NULL: V must be mwx_n_vocab, eot is
 * ignored) or a supplied one: the bytes of token t < eot are tok_bytes[
 * tok_off[t] .. tok_off[t + 1]), tok_off [eot + 1] ascending from 0, eot <= V.
 * Out: mask_out [R][ceil(V / 64)] 64-bit words, bit t % 64 of word t / 64 set
 * = token t rejected. The hook owns the device buffers; the words start as
 * all-ones bits, so a row the kernel does not write comes back as such, and lie
 * between two guard bands of sentinel words. Returns 0; -1 without a launch
 * for a null argument, R outside 1..256, V outside 1..53248, a state outside
 * [0, n_states) or a malformed table; -2 on a device error; -3 if the launch
 * changed a guard band. */
int mwx_test_constraint_mask(struct mwx_context* ctx, const struct mwx_constraint* c, int R, int V,
                             int eot, const uint32_t* tok_off, const uint8_t* tok_bytes,
                             const int* state, const int* active, const int* sample,
                             uint64_t* mask_out);

/* mwx_test_logits_process with the filter's constrained-decoding arguments:
 * cmask [R][ceil(V / 64)] rejection words and the penalty (finite, > 0; else
 * -1 without a launch). Everything else as mwx_test_logits_process. */
int mwx_test_logits_process_masked(struct mwx_context* ctx, int R, int V, const float* logits,
                                   const float* smask, const struct mwx_test_logits_ctl* ctl,
                                   const struct mwx_test_logits_const* lc, const uint64_t* cmask,
                                   float penalty, float* flt, float* probs, float* logprobs,
                                   struct mwx_test_logits_out* out);

#ifdef __cplusplus
}
#endif

#endif /* MWX_TEST_H */
