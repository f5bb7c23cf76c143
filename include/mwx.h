/*
 * mwx.h — C ABI of the MI355X-native Whisper engine.
 *
 * This is the drop-in boundary for the hot path of sentiric-stt-whisper-service.
 * The service's SttEngine (src/stt_engine.cpp) binds the whisper.h subset listed
 * below; every entry point here replaces exactly one of those symbols with the
 * same argument meaning, ownership and error behaviour. Reference call sites
 * (paths relative to the reference repository):
 *
 *   mwx_context_default_params            <- whisper_context_default_params      src/stt_engine.cpp:28
 *   mwx_init_from_file_with_params        <- whisper_init_from_file_with_params  src/stt_engine.cpp:33
 *   mwx_init_state                        <- whisper_init_state                  src/stt_engine.cpp:39
 *   mwx_free_state / mwx_free             <- whisper_free_state / whisper_free   src/stt_engine.cpp:56-57
 *   mwx_full_default_params               <- whisper_full_default_params         src/stt_engine.cpp:214
 *   mwx_full_with_state                   <- whisper_full_with_state             src/stt_engine.cpp:245-246
 *   mwx_full_n_segments_from_state        <- whisper_full_n_segments_from_state  src/stt_engine.cpp:261
 *   mwx_full_get_segment_text_from_state  <- whisper_full_get_segment_text_from_state   :267
 *   mwx_full_get_segment_t0/t1_from_state <- whisper_full_get_segment_t0/t1_from_state  :278-279
 *   mwx_full_get_segment_speaker_turn_next_from_state <- whisper_..._speaker_turn_next  :280-281
 *   mwx_full_n_tokens_from_state          <- whisper_full_n_tokens_from_state    src/stt_engine.cpp:284
 *   mwx_full_get_token_data_from_state    <- whisper_full_get_token_data_from_state :288
 *   mwx_token_to_str                      <- whisper_token_to_str                src/stt_engine.cpp:289
 *   mwx_token_eot                         <- whisper_token_eot                   src/stt_engine.cpp:290
 *   mwx_log_set                           <- whisper_log_set                     src/main.cpp:71
 *   mwx_resample                          <- SttEngine::resample_audio (libsamplerate
 *                                            src_simple, SRC_SINC_FASTEST) src/stt_engine.cpp:87-106
 *
 * New (no whisper.h counterpart): mwx_full_batch runs B independent clips in one
 * batched GPU pass (the data-parallel unit of this engine), and
 * mwx_write_synthetic_model writes a seeded model in the ggml .bin layout that
 * src/model_manager.cpp provisions (no real checkpoints exist offline).
 * whisper_context_params.dtw_token_timestamps / dtw_aheads_preset / dtw_n_top /
 * dtw_aheads / dtw_mem_size map to the mwx_context_params fields of the same
 * names, whisper_aheads / whisper_ahead / whisper_alignment_heads_preset to
 * mwx_aheads / mwx_ahead / mwx_alignment_heads_preset, and
 * whisper_token_data.t_dtw to mwx_token_data.t_dtw.
 * The whisper_vad_* family (src/stt_engine.cpp:44-55, :108-115) maps to
 * mwx_vad_*: see the voice-activity section below. whisper_vad_segments_* and
 * whisper_full's params.vad map to mwx_vad_segments_*, mwx_vad_trim_batch and
 * mwx_full_batch_trimmed ("VAD speech segments and silence trimming" below):
 * segments, the gather of the speech into a dense buffer and the transcription
 * of that buffer with times on the caller's timeline, all on the GPU with one
 * upload of the audio. The segment rule is this project's definition.
 *
 * Conventions: plain C, no exceptions cross this boundary, all functions return
 * NULL / negative on failure (0 = success), strings returned by getters stay
 * valid until the next mwx_full* call on the same state.
 */
#ifndef MWX_H
#define MWX_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MWX_SAMPLE_RATE 16000
#define MWX_N_FFT 400
#define MWX_HOP_LENGTH 160
#define MWX_CHUNK_SIZE 30
#define MWX_MAX_DECODERS 8

typedef int32_t mwx_token;
struct mwx_context;
struct mwx_state;

/* ggml_log_level-compatible levels (src/main.cpp:37-55 switches on these). */
enum mwx_log_level {
  MWX_LOG_LEVEL_NONE = 0,
  MWX_LOG_LEVEL_DEBUG = 1,
  MWX_LOG_LEVEL_INFO = 2,
  MWX_LOG_LEVEL_WARN = 3,
  MWX_LOG_LEVEL_ERROR = 4,
  MWX_LOG_LEVEL_CONT = 5,
};
typedef void (*mwx_log_callback)(enum mwx_log_level level, const char* text,
                                 void* user_data);

/* whisper_ahead / whisper_aheads: one alignment head, a list of them */
struct mwx_ahead {
  int n_text_layer;
  int n_head;
};
struct mwx_aheads {
  size_t n_heads;
  const struct mwx_ahead* heads;
};

struct mwx_context_params {
  bool use_gpu;     /* must be true: the engine has no CPU path */
  bool flash_attn;  /* accepted for API parity; attention is always fused */
  int gpu_device;   /* HIP device ordinal */
  /* Engine extension: MWX_COMPUTE_MXFP8 runs the encoder and cross-K/V GEMMs
   * on MX-fp8 operands (e4m3 + one E8M0 scale per 32 k; weights quantized at
   * load, activations by the producer step) with gfx950's block-scaled fp8
   * MFMA. MWX_COMPUTE_MODEL (default) computes in the model's 16-bit type. */
  int compute;
  /* DTW token timestamps (whisper.h dtw_token_timestamps and the fields after
   * it): when set, mwx_token_data.t_dtw of every text token of every emitted
   * segment is the time (10-ms units, the clip's timeline, like t0 / t1) a
   * dynamic-time-warping path through the alignment heads' cross-attention
   * assigns to it; otherwise t_dtw is -1. The rule is this project's
   * definition (a teacher-forced pass per 30-s window after its
   * result is final, HF transformers' normalisation, median filter and DTW).
   * Ids, text, t0 / t1, p and plog do not depend on the setting.
   * dtw_aheads_preset: enum mwx_alignment_heads_preset. N_TOP_MOST takes every
   * head of the last dtw_n_top decoder layers (1 .. n_text_layer); CUSTOM the
   * dtw_aheads list (n_text_layer = decoder layer, n_head = head); the model
   * presets name a fixed list and require the model's geometry. Init fails on
   * a layer or head outside the model. dtw_mem_size is accepted and unused. */
  bool dtw_token_timestamps;
  int dtw_aheads_preset;
  int dtw_n_top;
  struct mwx_aheads dtw_aheads;
  size_t dtw_mem_size;
};
/* whisper_alignment_heads_preset (same order) */
enum mwx_alignment_heads_preset {
  MWX_AHEADS_NONE = 0,
  MWX_AHEADS_N_TOP_MOST,
  MWX_AHEADS_CUSTOM,
  MWX_AHEADS_TINY_EN,
  MWX_AHEADS_TINY,
  MWX_AHEADS_BASE_EN,
  MWX_AHEADS_BASE,
  MWX_AHEADS_SMALL_EN,
  MWX_AHEADS_SMALL,
  MWX_AHEADS_MEDIUM_EN,
  MWX_AHEADS_MEDIUM,
  MWX_AHEADS_LARGE_V1,
  MWX_AHEADS_LARGE_V2,
  MWX_AHEADS_LARGE_V3,
  MWX_AHEADS_LARGE_V3_TURBO,
};
enum mwx_compute {
  MWX_COMPUTE_MODEL = 0,
  MWX_COMPUTE_MXFP8 = 1,
};

enum mwx_sampling_strategy {
  MWX_SAMPLING_GREEDY = 0,
  MWX_SAMPLING_BEAM_SEARCH = 1,
};

typedef bool (*mwx_abort_callback)(void* user_data);

/* Same fields and meaning as whisper_token_data. */
typedef struct mwx_token_data {
  mwx_token id;  /* token id */
  mwx_token tid; /* forced timestamp token id */
  float p;       /* probability of the token */
  float plog;    /* log probability of the token */
  float pt;      /* probability of the timestamp token */
  float ptsum;   /* sum of probabilities of all timestamp tokens */
  int64_t t0;    /* token-level timestamps (10 ms units), -1 if unset */
  int64_t t1;
  int64_t t_dtw; /* DTW timestamp (mwx_context_params.dtw_token_timestamps), else -1 */
  float vlen; /* voice length of the token */
} mwx_token_data;

/* Contextual biasing (INTEGRATION.md "Contextual biasing"): one
 * boosted phrase. tokens: n_tokens (1 .. MWX_BIAS_MAX_TOKENS) text-token ids,
 * each in [0, mwx_token_eot); boost: finite, may be negative or zero. */
#define MWX_BIAS_MAX_TOKENS 16
#define MWX_BIAS_MAX_PHRASES 1024
struct mwx_bias_phrase {
  const mwx_token* tokens;
  int n_tokens;
  float boost;
};

/* Mirrors the whisper_full_params fields the service sets or relies on
 * (src/stt_engine.cpp:214-243) plus the upstream defaults it inherits. */
struct mwx_full_params {
  int strategy;
  int n_threads;
  int n_max_text_ctx;
  int offset_ms;
  int duration_ms;

  bool translate;
  bool no_context;
  bool no_timestamps;
  bool single_segment;
  bool print_special;
  bool print_progress;
  bool print_realtime;
  bool print_timestamps;

  bool token_timestamps;
  float thold_pt;
  float thold_ptsum;
  int max_len;
  bool split_on_word;
  int max_tokens;

  /* Audio context (INTEGRATION.md "Audio context"). 0 (the
   * default; negative values count as 0): every window is encoded to
   * n_audio_ctx frames. 1 .. n_audio_ctx: every window of every clip of the
   * call is encoded from the first 2 * audio_ctx mel frames at its seek (a
   * real frame past them counts as zero) to audio_ctx frames, and the decoder
   * attends over audio_ctx keys; timestamp tokens stay 20-ms units and the
   * window loop is unchanged. audio_ctx == n_audio_ctx is bit-identical to 0;
   * more than n_audio_ctx: the call returns -5. See also audio_ctx_fit. */
  int audio_ctx;
  bool tdrz_enable;

  const char* initial_prompt;
  const mwx_token* prompt_tokens;
  int prompt_n_tokens;

  const char* language;
  bool detect_language;

  bool suppress_blank;
  bool suppress_nst;

  float temperature;
  float max_initial_ts;
  float length_penalty;
  float temperature_inc;
  float entropy_thold;
  float logprob_thold;
  float no_speech_thold;

  struct {
    int best_of;
  } greedy;
  struct {
    int beam_size;
    float patience;
  } beam_search;

  mwx_abort_callback abort_callback;
  void* abort_callback_user_data;

  /* Engine extension (benchmark workload only): when > 0 every 30-s window of
   * every clip is decoded for exactly this many steps (greedy or beam) with EOT
   * and timestamp tokens suppressed, and the clip then advances by a whole
   * window, so each window costs the same fixed number of decode steps and a
   * long clip runs window after window. */
  int bench_fixed_steps;

  /* Engine extension (appended field), off by default: every window of every
   * clip gets its own audio context, fitted to the audio left in the clip:
   * mwx_audio_ctx_for(ctx, n_samples, seek, audio_ctx, true), with audio_ctx
   * (> 0) as the floor. A clip's result is bit-identical to the clip run alone
   * with audio_ctx set to that value, whatever else is in the batch. The
   * effect of a short context on recognition quality is unmeasured (no real
   * checkpoint has been run with it): opt-in. */
  bool audio_ctx_fit;

  /* Engine extension (appended field): NULL (default), or one language id per
   * batch entry. Entry b with lang_ids[b] >= 0 is transcribed in that language
   * (mwx_lang_str(lang_ids[b])): it takes no part in the detection pass and is
   * not encoded for it, and its result is bit-identical to the same clip run
   * alone with that language, whatever else is in the batch. Entry b with
   * lang_ids[b] < 0 follows `language`. An id above mwx_lang_max_id(): the
   * call returns -3 before any GPU work. A non-multilingual model ignores the
   * field, as it ignores `language`. Honoured by mwx_full_batch, _pcm16,
   * _trimmed, _chunked (every chunk of entry b gets lang_ids[b]) and
   * mwx_align_batch; mwx_full_with_state reads lang_ids[0]. */
  const int* lang_ids;

  /* Engine extension (appended field), read by mwx_full_batch_chunked only and
   * only for entries whose language is to be detected: MWX_CHUNK_LANG_PER_CHUNK
   * (0, default) detects per chunk; MWX_CHUNK_LANG_RECORDING (1) detects once
   * per recording (rule at mwx_full_batch_chunked). */
  int chunk_language;

  /* Engine extension (appended fields; this project's rule):
   * contextual biasing. NULL / 0 (default): off, and the call is bit-identical
   * to one made before the fields existed (same kernels, same step graph).
   * Else n_bias_phrases (0 .. MWX_BIAS_MAX_PHRASES) phrases the decoders
   * should prefer. For a decoder, h is the ids it has generated so far in the
   * current attempt of the current window, oldest first (prompt and sot
   * sequence excluded; timestamp tokens included, and as no phrase can hold
   * one they end a match; a temperature-fallback attempt and a new window
   * start from the empty h; in beam search and best-of a decoder that takes
   * over another's candidate takes over its h). The matches of h are the pairs
   * (p, k), 0 <= k < len_p, k <= |h|, with the last k ids of h equal to the
   * first k ids of phrase p (k = 0 always matches: a phrase's first token is
   * boosted at every step). bias[t] = the largest boost_p over the matches
   * with p[k] == t; a sampling row's raw logits become x'[t] = x[t] + bias[t]
   * (one float add; tokens no match points at keep their bits) before anything
   * else reads them. Everything downstream sees x': the temperature division,
   * the suppression and timestamp rules, p / plog, the draws, and the
   * no-speech probability of a window's first step (a boost can therefore move
   * no_speech_prob). A failed match retracts nothing. The matcher tables are
   * built and uploaded once per call; the state is carried on the device.
   * Honoured by mwx_full_with_state, mwx_full_batch, _pcm16, _trimmed and
   * _chunked (every chunk); ignored by mwx_align_batch, the DTW pass and
   * language detection. Refused before any GPU work and before any state
   * changes: -3 for an id outside [0, mwx_token_eot); -1 (logged) for
   * n_bias_phrases outside its range, a non-zero count with a NULL array,
   * n_tokens outside 1 .. MWX_BIAS_MAX_TOKENS, or a NaN / infinite boost.
   * mwx_perf_enable class "logits_bias": the kernel's launches. The effect on
   * recognition and a sensible boost range are unmeasured (no real checkpoint
   * has been run with it). */
  const struct mwx_bias_phrase* bias_phrases;
  int n_bias_phrases;

  /* Engine extension (appended fields; this project's rule):
   * constrained decoding. NULL (default): off, and the call is bit-identical to
   * one made before the fields existed (same kernels, same step graph). Else a
   * byte-level automaton (mwx_constraint_from_dfa / _from_choices, below) that
   * every sampling step of every decoder is held to. A decoder carries a state
   * s: the start state at the beginning of every attempt of every window (in
   * beam search and best-of a decoder that takes over another's candidate
   * takes over its state); after it generates id < mwx_token_eot, s becomes
   * delta*(s, bytes(id)), bytes(id) being mwx_token_to_str's string; any other
   * id leaves s as it is. At a sampling step in state s != 0 a text token
   * t < eot is rejected iff bytes(t) is empty or delta*(s, bytes(t)) == 0; eot
   * is rejected iff s is not accepting; ids above eot (specials, timestamps)
   * are never rejected. In state 0 (the constraint has failed) nothing is
   * rejected and decoding goes on unconstrained. A rejected token's logit
   * becomes y - constraint_penalty, y = x / T (or x): after the temperature
   * division, before the suppression and timestamp rules. Everything
   * downstream sees it (p / plog, the timestamp-versus-text rule, the draws);
   * the no-speech probability, computed from the raw logits, does not. Tokens
   * that are not rejected keep their bits. The penalty is finite (default 100,
   * whisper.cpp's grammar_penalty), so the constraint alone never leaves a row
   * without a finite logit. bias_phrases may be used with it (the boosts add to
   * the raw logits first). Honoured by mwx_full_with_state, mwx_full_batch,
   * _pcm16, _trimmed and _chunked (every chunk); ignored by mwx_align_batch,
   * the DTW pass and language detection. Refused (-1, logged) before any GPU
   * work and before any state changes: a NaN, infinite or <= 0 penalty with a
   * non-NULL constraint; bench_fixed_steps > 0 with a constraint.
   * mwx_perf_enable class "logits_constrain": the mask kernel's launches. One
   * constraint per call: per-entry constraints, a grammar or regex compiler
   * and Unicode case folding are not provided. The effect on recognition with
   * a real checkpoint is unmeasured. */
  const struct mwx_constraint* constraint;
  float constraint_penalty;
};
#define MWX_CHUNK_LANG_PER_CHUNK 0
#define MWX_CHUNK_LANG_RECORDING 1

/* --- lifecycle --------------------------------------------------------- */
struct mwx_context_params mwx_context_default_params(void);
struct mwx_context* mwx_init_from_file_with_params(
    const char* path_model, struct mwx_context_params params);
struct mwx_state* mwx_init_state(struct mwx_context* ctx);
void mwx_free_state(struct mwx_state* state);
void mwx_free(struct mwx_context* ctx);

/* --- inference --------------------------------------------------------- */
struct mwx_full_params mwx_full_default_params(int strategy);

/* Returns 0 on success, <0 on failure (same codes as whisper_full_with_state). */
int mwx_full_with_state(struct mwx_context* ctx, struct mwx_state* state,
                        struct mwx_full_params params, const float* samples,
                        int n_samples);

/* Batched variant: clip b (f32 PCM @16 kHz, n_samples[b] samples) is decoded
 * into states[b]. All clips share params. Returns 0 or the first error.
 * samples[b] may be host memory or device memory of the context's GPU
 * (HBM-resident input: copied device-to-device, no PCIe transfer). */
int mwx_full_batch(struct mwx_context* ctx, struct mwx_state* const* states,
                   struct mwx_full_params params,
                   const float* const* samples, const int* n_samples,
                   int n_clips);

/* As mwx_full_batch with 16-bit PCM (host or device memory), converted on
 * the device exactly as SttEngine::transcribe_pcm16 converts it (x / 32768,
 * src/stt_engine.cpp:123): half the bytes over PCIe. */
int mwx_full_batch_pcm16(struct mwx_context* ctx, struct mwx_state* const* states,
                         struct mwx_full_params params, const int16_t* const* samples,
                         const int* n_samples, int n_clips);

/* Device input buffers on the context's GPU (for mwx_full_batch over
 * HBM-resident PCM): allocate n floats, upload n floats from host memory
 * (synchronous), free. NULL / <0 on failure. */
float* mwx_device_buffer(struct mwx_context* ctx, size_t n);
int mwx_device_upload(struct mwx_context* ctx, float* dst, const float* src, size_t n);
void mwx_device_buffer_free(struct mwx_context* ctx, float* p);

/* --- results ------------------------------------------------------------ */
int mwx_full_n_segments_from_state(struct mwx_state* state);
const char* mwx_full_get_segment_text_from_state(struct mwx_state* state,
                                                 int i_segment);
int64_t mwx_full_get_segment_t0_from_state(struct mwx_state* state,
                                           int i_segment);
int64_t mwx_full_get_segment_t1_from_state(struct mwx_state* state,
                                           int i_segment);
bool mwx_full_get_segment_speaker_turn_next_from_state(struct mwx_state* state,
                                                       int i_segment);
float mwx_full_get_segment_no_speech_prob_from_state(struct mwx_state* state,
                                                     int i_segment);
int mwx_full_n_tokens_from_state(struct mwx_state* state, int i_segment);
mwx_token_data mwx_full_get_token_data_from_state(struct mwx_state* state,
                                                  int i_segment, int i_token);
int mwx_full_lang_id_from_state(struct mwx_state* state);
/* Per-language probabilities of the detection pass of the last call on this
 * state (language auto / detect_language), probs[id] for id < the return value
 * (mwx_lang_max_id() + 1); 0 when that call did not detect; -1 bad arguments
 * (n smaller than that). The softmax runs over the language logits only, as
 * whisper_lang_auto_detect's does; the language used is the first maximum of
 * those logits. */
int mwx_full_lang_probs_from_state(struct mwx_state* state, float* probs, int n);

/* --- segment prosody -----------------------------------------------------
 * The reference's per-segment affect / speaker features
 * (src/prosody_extractor.h:6-31 AffectiveTags, ProsodyOptions; computed by
 * extract_prosody for every kept segment, src/stt_engine.cpp:313-337) on the
 * GPU, bit-identical to the reference's CPU build. */
typedef struct mwx_prosody_params { /* ProsodyOptions, same defaults */
  float lpf_alpha;                  /* 0.07 */
  float gender_threshold;           /* 170 Hz */
  float min_pitch;                  /* 60 Hz */
  float max_pitch;                  /* 500 Hz */
} mwx_prosody_params;

enum mwx_gender { MWX_GENDER_UNKNOWN = 0 /* "?" */, MWX_GENDER_M = 1, MWX_GENDER_F = 2 };
enum mwx_emotion {
  MWX_EMOTION_NEUTRAL = 0,
  MWX_EMOTION_EXCITED = 1,
  MWX_EMOTION_ANGRY = 2,
  MWX_EMOTION_SAD = 3
};

typedef struct mwx_prosody { /* AffectiveTags */
  float pitch_mean, pitch_std, energy_mean, energy_std, spectral_centroid,
      zero_crossing_rate, arousal, valence;
  float speaker_vec[8];
  int gender;      /* enum mwx_gender (gender_proxy) */
  int emotion;     /* enum mwx_emotion (emotion_proxy) */
  int serial_runs; /* diagnostics: filter runs recomputed serially */
  int reserved;
} mwx_prosody;

mwx_prosody_params mwx_prosody_default_params(void);

/* Prosody of n_seg segments [seg_start[i], seg_start[i] + seg_len[i]) of one
 * PCM buffer (host or device memory, n_pcm samples at sample_rate, 100 <=
 * sample_rate <= 160000). A segment shorter than 160 samples gets the
 * reference's empty-input result (extract_prosody(nullptr, 0, ...)). Runs on
 * the state's stream; synchronous. 0 on success, <0 on bad arguments or a
 * device error. */
int mwx_prosody_batch(struct mwx_context* ctx, struct mwx_state* state, const float* pcm,
                      int64_t n_pcm, const int64_t* seg_start, const int64_t* seg_len,
                      int n_seg, int sample_rate, const mwx_prosody_params* params,
                      mwx_prosody* out);

/* As mwx_prosody_batch with every array in device memory (no host copies, no
 * synchronization: the results are ready when the state's stream is). For
 * throughput measurement over HBM-resident inputs. d_desc holds n_seg int64
 * triples {start, len, frame_offset}: frame_offset = the sum of
 * len / (sample_rate / 100) over the segments before it; total_frames = that
 * sum over all n_seg. */
int mwx_prosody_batch_device(struct mwx_context* ctx, struct mwx_state* state,
                             const float* d_pcm, const int64_t* d_desc, int n_seg,
                             int64_t total_frames, int sample_rate,
                             const mwx_prosody_params* params, mwx_prosody* d_out);

/* --- resampling -------------------------------------------------------------
 * SttEngine::resample_audio (src/stt_engine.cpp:87-106, called for every
 * request whose sample rate is not 16 kHz, :138-145): libsamplerate's
 * src_simple(SRC_SINC_FASTEST, mono, end_of_input = 0) restated on the GPU —
 * the same output count (the converter holds back the last filter half-width
 * of input) and alignment; the coefficient table is a reconstruction of the
 * "fastest" table's geometry (libsamplerate is absent, parity unpinned).
 * `in` / `out` may be host or device memory of the context's GPU. Returns the
 * frames generated (the reference's output_frames_gen; 0 when
 * src_rate == dst_rate or n_in == 0, where the reference keeps the input), or
 * < 0 on bad arguments / a ratio outside libsamplerate's [1/256, 256] / a
 * device error. Runs on the state's stream; synchronous. */
long mwx_resample_max_frames(int n_in, int src_rate, int dst_rate); /* (long)(n_in*ratio)+100 */
int mwx_resample(struct mwx_context* ctx, struct mwx_state* state, const float* in, int n_in,
                 int src_rate, int dst_rate, float* out, int out_cap);

/* --- voice-activity detection ---------------------------------------------
 * The whisper_vad_* calls behind SttEngine::is_speech_detected
 * (src/stt_engine.cpp:44-55 load, :108-115 call), on the GPU:
 *
 *   mwx_vad_default_context_params     <- whisper_vad_default_context_params
 *   mwx_vad_init_from_file_with_params <- whisper_vad_init_from_file_with_params
 *   mwx_vad_detect_speech              <- whisper_vad_detect_speech
 *   mwx_vad_n_probs / mwx_vad_probs    <- whisper_vad_n_probs / whisper_vad_probs
 *   mwx_vad_free                       <- whisper_vad_free
 *
 * The model is a Silero-v5-shaped net over 512-sample chunks of 16 kHz f32
 * PCM (the last chunk zero-padded): one speech probability per chunk, the
 * LSTM state zero at the start of every clip of every call. The network and
 * the file layout are written down in INTEGRATION.md ("VAD model"); upstream
 * whisper.cpp is not available to this project, so parity with its VAD is
 * unpinned.
 *
 * One call at a time per context (the host SttEngine holds a mutex, as the
 * reference does, src/stt_engine.cpp:110). `samples` may be host memory or
 * device memory of the context's GPU, as for mwx_full_batch. */
struct mwx_vad_context;
struct mwx_vad_context_params {
  int n_threads;  /* accepted for API parity; unused */
  bool use_gpu;   /* must be true: there is no CPU path */
  int gpu_device; /* HIP device ordinal */
};
struct mwx_vad_context_params mwx_vad_default_context_params(void);
/* NULL (with a logged reason) on a bad magic, a truncated file, a missing or
 * mis-shaped tensor, hyper-parameters other than the supported shape, or a
 * device error. */
struct mwx_vad_context* mwx_vad_init_from_file_with_params(
    const char* path_model, struct mwx_vad_context_params params);
void mwx_vad_free(struct mwx_vad_context* vctx);

/* Computes the chunk probabilities of one clip. Returns true when they were
 * computed and false on an error. The return value is NOT a speech decision:
 * read the probabilities and apply a rule (SttEngine: any chunk >=
 * vad_threshold). n_samples = 0 succeeds with 0 probabilities. */
bool mwx_vad_detect_speech(struct mwx_vad_context* vctx, const float* samples, int n_samples);
int mwx_vad_n_probs(struct mwx_vad_context* vctx);
/* Valid until the next call on the same context. */
const float* mwx_vad_probs(struct mwx_vad_context* vctx);

/* Engine extension: all clips in one pass (the front end over every chunk of
 * every clip at once, the recurrences of the clips side by side). Clip b's
 * mwx_vad_n_chunks(n_samples[b]) probabilities are written to
 * probs_out + probs_offset[b] (host memory, sized by the caller); bit for bit
 * what mwx_vad_detect_speech gives for the clip alone. Leaves
 * mwx_vad_n_probs / mwx_vad_probs unchanged. Returns 0, or < 0 on bad
 * arguments or a device error. */
int mwx_vad_n_chunks(int n_samples); /* ceil(n_samples / 512) */
int mwx_vad_detect_speech_batch(struct mwx_vad_context* vctx, const float* const* samples,
                                const int* n_samples, int n_clips, float* probs_out,
                                const int* probs_offset);
/* Device time of the last call's two kernels (front end; recurrence + head)
 * in milliseconds, from HIP events on the context's stream. 0 on success. */
int mwx_vad_last_kernel_ms(struct mwx_vad_context* vctx, float* frontend_ms, float* lstm_ms);

/* --- VAD speech segments and silence trimming --------------------------------
 *   mwx_vad_default_params             <- whisper_vad_default_params
 *   mwx_vad_segments_from_probs        <- whisper_vad_segments_from_probs
 *   mwx_vad_segments_from_samples      <- whisper_vad_segments_from_samples
 *   mwx_vad_segments_n_segments        <- whisper_vad_segments_n_segments
 *   mwx_vad_segments_get_segment_t0/t1 <- whisper_vad_segments_get_segment_t0/t1
 *   mwx_vad_free_segments              <- whisper_vad_free_segments
 *   mwx_vad_trim_batch + mwx_full_batch_trimmed  ~ whisper_full with params.vad
 *
 * The rule that turns chunk probabilities into segments is this project's
 * definition (Silero's get_speech_timestamps restated; DESIGN.md deviation D7,
 * written out in INTEGRATION.md "VAD speech segments"): parity with
 * whisper.cpp's whisper_vad_segments_from_probs / whisper_vad is unpinned. It
 * runs on the GPU (csrc/k_vad.hip, vad_segments_kernel) over the probabilities
 * the network kernels left there. */
struct mwx_vad_params {           /* whisper_vad_params: same names and defaults */
  float threshold;                /* 0.5: p >= threshold is speech */
  int min_speech_duration_ms;     /* 250 */
  int min_silence_duration_ms;    /* 100 */
  float max_speech_duration_s;    /* FLT_MAX */
  int speech_pad_ms;              /* 30 */
  float samples_overlap;          /* 0.1 s kept after a segment in the trimmed audio */
};
struct mwx_vad_params mwx_vad_default_params(void);

/* NULL (with a logged reason) on invalid parameters (threshold outside (0, 1),
 * a negative duration, max_speech_duration_s <= 0, samples_overlap < 0, NaN) or
 * a device error. from_probs uses the probabilities and the clip length of the
 * context's last mwx_vad_detect_speech; from_samples runs that call first. */
struct mwx_vad_segments;
struct mwx_vad_segments* mwx_vad_segments_from_probs(struct mwx_vad_context* vctx,
                                                     struct mwx_vad_params params);
struct mwx_vad_segments* mwx_vad_segments_from_samples(struct mwx_vad_context* vctx,
                                                       struct mwx_vad_params params,
                                                       const float* samples, int n_samples);
int mwx_vad_segments_n_segments(struct mwx_vad_segments* segments);
/* centiseconds = samples / 160.0f */
float mwx_vad_segments_get_segment_t0(struct mwx_vad_segments* segments, int i_segment);
float mwx_vad_segments_get_segment_t1(struct mwx_vad_segments* segments, int i_segment);
void mwx_vad_free_segments(struct mwx_vad_segments* segments);

/* Engine extension: VAD, segments and compaction of n_clips clips (host or
 * device memory) in one pass. Host clips are uploaded once, for the VAD, and
 * compacted from that copy; the speech of every clip (each segment followed by
 * samples_overlap of audio, 0.1 s of zeros between pieces that are not adjacent)
 * lands in one device buffer that the returned object owns. The object does not
 * depend on vctx afterwards. NULL on invalid parameters or a device error. */
struct mwx_vad_trimmed;
struct mwx_vad_trimmed* mwx_vad_trim_batch(struct mwx_vad_context* vctx,
                                           struct mwx_vad_params params,
                                           const float* const* samples, const int* n_samples,
                                           int n_clips);
int mwx_vad_trimmed_n_clips(const struct mwx_vad_trimmed* t);
int mwx_vad_trimmed_n_segments(const struct mwx_vad_trimmed* t, int clip);
/* Segment i of the clip in samples of the caller's clip; 0, or < 0 out of range. */
int mwx_vad_trimmed_segment(const struct mwx_vad_trimmed* t, int clip, int i, int64_t* s0,
                            int64_t* s1);
int64_t mwx_vad_trimmed_n_samples(const struct mwx_vad_trimmed* t, int clip); /* compacted */
/* Device pointer to the clip's compacted PCM (NULL when it has no samples). */
const float* mwx_vad_trimmed_pcm(const struct mwx_vad_trimmed* t, int clip);
/* A time of the compacted clip, in centiseconds, on the caller's timeline.
 * is_end: the value ends something (t1) and maps to the end of the speech
 * before a gap rather than to the start of the speech after it. A value < 0
 * stays as it is. */
int64_t mwx_vad_trimmed_map_time(const struct mwx_vad_trimmed* t, int clip, int64_t t_cs,
                                 bool is_end);
void mwx_vad_trimmed_free(struct mwx_vad_trimmed* t);
/* Device time of the last mwx_vad_trim_batch's two kernels (segments;
 * compaction) in milliseconds. 0 on success, -1 if nothing was compacted. */
int mwx_vad_last_trim_kernel_ms(struct mwx_vad_context* vctx, float* segments_ms,
                                float* compact_ms);

/* As mwx_full_batch over trimmed audio: batch entry b is clip clip_index[b] of
 * trimmed[b] (one object for the whole batch, or one single-clip object per
 * queued request). A clip without segments is left out of the Whisper pass and
 * its state ends with 0 segments; the others run through mwx_full_batch on
 * their compacted device PCM, and every segment and token time stored in their
 * states is then mapped, so the mwx_full_get_* getters return times of the
 * caller's clip. An object of another device than ctx is an error. */
int mwx_full_batch_trimmed(struct mwx_context* ctx, struct mwx_state* const* states,
                           struct mwx_full_params params,
                           const struct mwx_vad_trimmed* const* trimmed, const int* clip_index,
                           int n_clips);

/* --- vocabulary / model ------------------------------------------------- */
const char* mwx_token_to_str(struct mwx_context* ctx, mwx_token token);
mwx_token mwx_token_eot(struct mwx_context* ctx);
mwx_token mwx_token_sot(struct mwx_context* ctx);
mwx_token mwx_token_beg(struct mwx_context* ctx);
mwx_token mwx_token_not(struct mwx_context* ctx);
mwx_token mwx_token_nosp(struct mwx_context* ctx);
mwx_token mwx_token_transcribe(struct mwx_context* ctx);
mwx_token mwx_token_translate(struct mwx_context* ctx);
mwx_token mwx_token_lang(struct mwx_context* ctx, int lang_id);
int mwx_n_vocab(struct mwx_context* ctx);
int mwx_n_text_ctx(struct mwx_context* ctx);
int mwx_n_audio_ctx(struct mwx_context* ctx);
/* The audio context of the window at `seek` (mel frames, 10 ms) of a clip of
 * n_samples samples under mwx_full_params.audio_ctx / audio_ctx_fit (a host
 * function). With N = n_audio_ctx: fit off: audio_ctx > 0 ? audio_ctx : N. fit on, rem =
 * max(0, n_len_org - seek) real mel frames left and floor = audio_ctx > 0 ?
 * audio_ctx : 64: min(N, max(floor, 64 * ceil((ceil(rem / 2) + 32) / 64))),
 * i.e. 0.64 s of trailing context, rounded up to the attention key tile.
 * ctx may be NULL: N = 1500, every Whisper model's. -1: audio_ctx > N. */
int mwx_audio_ctx_for(struct mwx_context* ctx, int n_samples, int seek, int audio_ctx, bool fit);
int mwx_n_mels(struct mwx_context* ctx);
int mwx_is_multilingual(struct mwx_context* ctx);
int mwx_model_wtype(struct mwx_context* ctx); /* 1 = f16, 30 = bf16 */
int mwx_lang_id(const char* lang);
const char* mwx_lang_str(int id);
int mwx_lang_max_id(void);
/* Greedy longest-match tokenizer (whisper_tokenize semantics). Returns the
 * number of tokens, or -(needed) if n_max_tokens is too small. */
int mwx_tokenize(struct mwx_context* ctx, const char* text, mwx_token* tokens,
                 int n_max_tokens);

void mwx_log_set(mwx_log_callback log_callback, void* user_data);

/* --- measurement ------------------------------------------------------------
 * Times every launch of one kernel class with a pair of HIP events recorded on
 * the state's stream (the stream the kernels run on). Classes: "mel",
 * "enc_gemm", "enc_attn", "cross_gemm", "dec_gemm", "dec_attn_self",
 * "dec_attn_cross", "logits_gemm", "logits_bias" (contextual biasing: launched
 * only by calls with bias_phrases), "logits_constrain" (constrained decoding:
 * only by calls with a constraint), "logits_proc", "prosody". NULL disables.
 * mwx_perf_read synchronizes, returns the summed milliseconds and the launch
 * count since the last read, and resets them. */
void mwx_perf_enable(struct mwx_state* state, const char* kernel_class);
int mwx_perf_read(struct mwx_state* state, double* total_ms, int* launches);
/* Several classes may be enabled at once as a comma-separated list;
 * mwx_perf_read reads the first, mwx_perf_read_class any of them. Launches
 * inside the decode-step graph are timed on every 8th step (MWX_PERF_PERIOD). */
int mwx_perf_read_class(struct mwx_state* state, const char* kernel_class, double* total_ms,
                        int* launches);

/* --- model tooling --------------------------------------------------------
 * Writes a model in the ggml .bin layout read by whisper.cpp and by
 * mwx_init_from_file_with_params: magic, 11 hparams, mel filterbank, vocab,
 * tensors. Weights are splitmix64-seeded; wtype 1 = f16, 30 = bf16 for the 2-D
 * tensors (1-D tensors, conv biases and positional embeddings are f32, as in
 * the upstream converter). arch: "tiny.en", "tiny", "base.en", "base",
 * "small", "medium", "large-v3", or "micro" (test-sized).
 * Returns 0 on success. */
int mwx_write_synthetic_model(const char* path, const char* arch, int wtype,
                              uint64_t seed);

/* Writes a seeded VAD model in the layout mwx_vad_init_from_file_with_params
 * reads ("VAD model"): the STFT basis is the Hann-windowed
 * DFT, every other weight is uniform in +-g / sqrt(fan_in) (g = 2 encoder,
 * 3 LSTM, 16 head: at g = 1 a random net barely reacts to its input). The
 * basis and the convolution weights are f16, the rest f32. Returns 0 on
 * success. */
int mwx_write_synthetic_vad_model(const char* path, uint64_t seed);

/* Quantizes a whisper ggml .bin (f32 / f16 / bf16) into a ggml block type
 * (q4_0 = 2, q4_1 = 3, q5_0 = 6, q5_1 = 7, q8_0 = 8; the 256-element K types
 * q2_K = 10, q3_K = 11, q4_K = 12, q5_K = 13, q6_K = 14) with the rules of
 * whisper.cpp's `quantize` tool: 2-D tensors except the positional
 * embeddings are quantized, everything else is copied; ftype becomes
 * 2000 + ftype. Legacy blocks are ggml's quantize_row_q*_ref bit for bit; K
 * blocks come from a plain min/max encoder (valid blocks, not ggml's scale
 * search). A row length that is not a multiple of the block (tiny's 384 for
 * K types) fails with -8, as ggml's quantizer does. Returns 0 on success. */
int mwx_model_quantize(const char* in_path, const char* out_path, int type);

/* --- chunked long-form transcription ------------------------------------------
 * One long recording as a batch (the rule is written out in
 * INTEGRATION.md "Chunked long-form transcription"): the clip's pieces are
 * packed, in order, into chunks of at most chunk_s seconds of compacted audio
 * (csrc/k_vad.hip, vad_chunks_kernel), a piece longer than that being a chunk
 * of its own, and every chunk is decoded as an independent batch entry. This
 * project's definition: parity with faster-whisper's or WhisperX's batched
 * pipelines is not claimed. */

/* As mwx_vad_trim_batch, plus a chunk plan (rule D10). chunk_s in [1, 30];
 * anything else, NaN included, is refused (NULL, logged). Segments, pieces and
 * the compacted PCM are those of mwx_vad_trim_batch. */
struct mwx_vad_trimmed* mwx_vad_trim_batch_chunked(struct mwx_vad_context* vctx,
                                                   struct mwx_vad_params params, float chunk_s,
                                                   const float* const* samples,
                                                   const int* n_samples, int n_clips);
/* The chunks of a clip. An object made by mwx_vad_trim_batch reports one chunk
 * per clip that has segments: the whole compacted clip. */
int mwx_vad_trimmed_n_chunks(const struct mwx_vad_trimmed* t, int clip);
/* Chunk j: its first segment and segment count, its start and length in
 * samples of the compacted clip (the gap zeros after its last piece are not
 * part of it). 0, or < 0 out of range. Outputs are nullable. */
int mwx_vad_trimmed_chunk(const struct mwx_vad_trimmed* t, int clip, int j, int* first_segment,
                          int* n_segments, int64_t* start, int64_t* len);
/* As mwx_vad_trimmed_map_time for a time counted from the start of chunk j. A
 * value past the chunk's end maps to the end of its last piece. */
int64_t mwx_vad_trimmed_chunk_map_time(const struct mwx_vad_trimmed* t, int clip, int j,
                                       int64_t t_cs, bool is_end);
/* Device time of the last mwx_vad_trim_batch_chunked's vad_chunks_kernel in
 * milliseconds. 0 on success, -1 if no plan was made. */
int mwx_vad_last_chunk_kernel_ms(struct mwx_vad_context* vctx, float* chunks_ms);

/* Batch entry b = clip clip_index[b] of trimmed[b]; every chunk of every entry is one
 * entry of an internal mwx_full_batch run, at most max_batch (>= 1) per run, in
 * (entry, chunk) order. Entry 0 of every run works on states[0]; the others on
 * scratch states that states[0] owns (created on first use, at most
 * max_batch - 1, freed with it). states[b] ends with the segments of its
 * clip's chunks in chunk order, every segment and token time on the caller's
 * timeline (mwx_vad_trimmed_chunk_map_time), and its first chunk's language
 * id; a clip without chunks ends with 0 segments. Every chunk is an
 * independent clip to the engine: the prompt parameters apply to each one and
 * language = "auto" detects per chunk; a chunk shorter than 0.1 s decodes to
 * nothing, as a clip that short does. The result does not depend on
 * max_batch. params.offset_ms and params.duration_ms must be 0 (-1, logged).
 * On an error or an abort (polled between runs too) the code is returned and
 * every state of the call holds 0 segments. For an object made by
 * mwx_vad_trim_batch this is mwx_full_batch_trimmed.
 *
 * params.chunk_language = MWX_CHUNK_LANG_RECORDING (this project's definition,
 * DESIGN.md D13): for every entry whose language is to be detected, its
 * leading chunks 0..k, k the smallest index at which their summed length
 * reaches 480000 samples (all chunks if they never do), those shorter than
 * 0.1 s left out, first go through a detection-only pass (runs of at most
 * max_batch, in (entry, chunk) order). Their probabilities are pooled,
 * P = sum_j len_j p_j / sum_j len_j (double, in chunk order); the recording's
 * language is the lowest id among the maxima of P, and every chunk of the
 * entry is then transcribed in it (lang_ids). states[b] ends with that
 * language id and with P, rounded to float, as its lang_probs. An entry with
 * no chunk of at least 0.1 s ends as with MWX_CHUNK_LANG_PER_CHUNK. At most
 * about 30 s of speech per recording is encoded twice. */
int mwx_full_batch_chunked(struct mwx_context* ctx, struct mwx_state* const* states,
                           struct mwx_full_params params,
                           const struct mwx_vad_trimmed* const* trimmed, const int* clip_index,
                           int n_clips, int max_batch);

/* --- streaming VAD ---------------------------------------------------------------
 * A stream is fed a piece of 16 kHz audio at a time and carries the network's
 * recurrent state, the samples that do not fill a 512-sample chunk yet and the
 * segment scan across the calls (csrc/k_vad.hip,
 * vad_stream_stage_kernel / vad_lstm_stream_kernel / vad_stream_scan_kernel).
 * Two invariants:
 *   1. After any sequence of feeds, mwx_vad_stream_probs holds the bits that
 *      mwx_vad_detect_speech returns for everything fed since the last reset,
 *      the last chunk included when it is partial: that one is computed
 *      zero-padded as a provisional step whose state is not kept, replaced when
 *      the chunk completes, and not seen by the scan.
 *   2. The raw segments closed so far, followed by mwx_vad_stream_finish, are
 *      the segments of rule D7 over those probabilities before its padding
 *      pass; padded as D7 pads they are mwx_vad_segments_from_samples of the
 *      whole audio. The stream does not pad: padding looks ahead.
 * A stream belongs to its context and shares the context's rule of one call at
 * a time (init, free, reset and feed count as calls). Free the streams before
 * the context; a stream that outlives it accepts only mwx_vad_stream_free. */
struct mwx_vad_stream;
/* NULL (logged) on the parameter errors mwx_vad_segments_from_probs refuses, or
 * a device error. */
struct mwx_vad_stream* mwx_vad_stream_init(struct mwx_vad_context* vctx,
                                           struct mwx_vad_params params);
void mwx_vad_stream_free(struct mwx_vad_stream* s);
/* As new: h = c = 0, position 0, no tail, scan cleared, no probabilities or
 * segments. 0, or < 0 without a stream or a context. */
int mwx_vad_stream_reset(struct mwx_vad_stream* s);
/* Appends n_samples[i] samples (host or device memory; 0 allowed; at most
 * 480000 per stream per call) to streams[i], all streams in one pass of the
 * kernels and one copy back. A stream may appear once per call. The result of
 * a stream does not depend on which others share the call. 0, or < 0 on bad
 * arguments, a finished stream or a stream of another context (no stream of
 * the call has changed) or a device error (reset the streams of the call). */
int mwx_vad_stream_feed_batch(struct mwx_vad_context* vctx, struct mwx_vad_stream* const* streams,
                              const float* const* samples, const int* n_samples, int n_streams);
/* Applies rule D7's tail rule with N = the samples fed: speech still open
 * closes at N if it is long enough. Afterwards only reset and free. */
int mwx_vad_stream_finish(struct mwx_vad_stream* s);
int64_t mwx_vad_stream_n_samples(const struct mwx_vad_stream* s);
int mwx_vad_stream_n_probs(const struct mwx_vad_stream* s); /* mwx_vad_n_chunks(n_samples) */
/* All probabilities since reset; valid until the stream's next call. */
const float* mwx_vad_stream_probs(const struct mwx_vad_stream* s);
float mwx_vad_stream_max_prob(const struct mwx_vad_stream* s); /* over those; 0 when none */
int mwx_vad_stream_n_segments(const struct mwx_vad_stream* s); /* raw segments closed since reset */
/* Raw (unpadded) segment i in samples since reset. closed_at = 512 * (index of
 * the chunk whose step closed it + 1), or n_samples for the one
 * mwx_vad_stream_finish closes. 0, or < 0 out of range. Outputs are nullable. */
int mwx_vad_stream_segment(const struct mwx_vad_stream* s, int i, int64_t* s0, int64_t* s1,
                           int64_t* closed_at);
bool mwx_vad_stream_in_speech(const struct mwx_vad_stream* s); /* the scan's `triggered` */
/* Device time of the last mwx_vad_stream_feed_batch in milliseconds: staging,
 * front end, recurrence + head (the scan kernel behind them is not timed). 0 on
 * success, -1 if the last call was none or launched nothing. */
int mwx_vad_stream_last_kernel_ms(struct mwx_vad_context* vctx, float* stage_ms,
                                  float* frontend_ms, float* lstm_ms);

/* --- transcript alignment and scoring ---------------------------
 * Text the caller already has (a script, a corrected transcript, a subtitle
 * line, a hypothesis of another pass) is teacher-forced through the decoder
 * against the clip's audio: a log-probability per token and, in a context
 * created with dtw_token_timestamps, a DTW time per token. Clip b is at most
 * 30 s of 16 kHz audio (host or device memory, as mwx_full_batch) and
 * n_tokens[b] text tokens, 0 .. MWX_ALIGN_MAX_TOKENS, every id below
 * mwx_token_eot (no special, no timestamp token).
 *
 * The decoded sequence is the clip's sot sequence ([SOT], or [SOT, language,
 * task] for a multilingual model), <|notimestamps|>, the tokens, EOT. Row i
 * (0 <= i <= n) is the position that predicts token i (row n: EOT, "the text
 * ends here"; with n = 0 the only row). From the raw logits x of that position
 * (no suppression mask, no temperature, no timestamp rule):
 *   plog = x[target] - logsumexp(x), p = expf(plog),
 *   top_id = argmax x (lowest index among bit-equal values),
 *   top_plog = x[top_id] - logsumexp(x).
 * The logits are the bits a decode step gives for that row and position.
 *
 * Read from params: language ("auto" / NULL / "" runs the detection pass of
 * mwx_full_batch), translate, audio_ctx, audio_ctx_fit (as mwx_full_batch) and
 * the abort callback (polled before the encode: -6, and before the pass: -9).
 * offset_ms and duration_ms must be 0 (-1, logged). Every other field is
 * ignored: there is no previous-text prompt (initial_prompt / prompt_tokens
 * are not used), no sampling, no fallback and no threshold.
 *
 * Refused before any state changes: -3 a token id outside [0, mwx_token_eot)
 * or an unknown language; -1 (logged) n_tokens[b] > MWX_ALIGN_MAX_TOKENS,
 * n_samples[b] > 30 * 16000, a null pointer or n_clips < 1; -5 audio_ctx >
 * n_audio_ctx.
 *
 * states[b] ends with one segment: t0 = 0, t1 = the clip's length in
 * centiseconds, the text the concatenated token strings, the tokens the given
 * ids with p, plog, t_dtw (2 x the DTW frame, or -1 without DTW or with n = 0),
 * tid = id, pt = ptsum = 0, t0 = t1 = -1, vlen = 0;
 * mwx_full_lang_id_from_state returns the language used. A clip too short for
 * mwx_full_batch to decode (under 0.1 s) ends with 0 segments and no rows. A
 * clip's result does not depend on the other clips of the call. The decode
 * state of a following mwx_full_batch is not affected.
 * mwx_perf_enable class "score": the scoring kernel's launches. */
#define MWX_ALIGN_MAX_TOKENS 224
int mwx_align_batch(struct mwx_context* ctx, struct mwx_state* const* states,
                    struct mwx_full_params params, const float* const* samples,
                    const int* n_samples, const mwx_token* const* tokens, const int* n_tokens,
                    int n_clips);
/* Row i of the state's last mwx_align_batch, 0 <= i <= n (row n: EOT). 0, or -1
 * out of range or without rows. Outputs are nullable. */
int mwx_align_row(struct mwx_state* state, int i, float* plog, mwx_token* top_id,
                  float* top_plog);

/* --- constrained decoding -------------------------------
 * A constraint is a deterministic automaton over bytes: states 0 .. S - 1
 * (2 <= S <= MWX_CONSTRAINT_MAX_STATES), state 0 dead (not accepting, every
 * transition to 0), a start state >= 1, trans [S][256] state ids and an
 * accepting flag per state. The object is immutable once built, usable from
 * any thread and with any context, and freed by mwx_constraint_free (not
 * while a call that uses it runs).
 *
 * mwx_constraint_from_dfa returns NULL (reason logged) for n_states outside
 * 2 .. MWX_CONSTRAINT_MAX_STATES, a null table, a target >= n_states, a state
 * 0 that is accepting or has a transition away from 0, start outside
 * 1 .. n_states - 1, or a state other than 0 that is reachable from the start
 * and cannot reach an accepting state (so a viable prefix can always be
 * completed over a vocabulary that holds every single byte).
 *
 * mwx_constraint_from_choices builds the byte trie of n texts: the accepted
 * strings are the texts, each with (MWX_CONSTRAINT_LEADING_SPACE) one optional
 * ' ' before it and (MWX_CONSTRAINT_TRAILING_PUNCT) one optional '.', '!' or
 * '?' after it; with MWX_CONSTRAINT_FOLD_CASE an ASCII letter matches either
 * case. NULL for n < 1, a null or empty text, unknown flag bits, or more than
 * MWX_CONSTRAINT_MAX_STATES - 1 live states. */
#define MWX_CONSTRAINT_MAX_STATES 4096
#define MWX_CONSTRAINT_FOLD_CASE 1
#define MWX_CONSTRAINT_LEADING_SPACE 2
#define MWX_CONSTRAINT_TRAILING_PUNCT 4
struct mwx_constraint;
struct mwx_constraint* mwx_constraint_from_dfa(int n_states, int start, const uint16_t* trans,
                                               const uint8_t* accepting);
struct mwx_constraint* mwx_constraint_from_choices(const char* const* texts, int n, int flags);
void mwx_constraint_free(struct mwx_constraint* c);
/* Host-only queries. _accepting: 1 / 0 (0 for s out of range). _walk: the state
 * after n bytes from s (0 for s out of range or a null argument). */
int mwx_constraint_n_states(const struct mwx_constraint* c);
int mwx_constraint_start(const struct mwx_constraint* c);
int mwx_constraint_accepting(const struct mwx_constraint* c, int s);
int mwx_constraint_walk(const struct mwx_constraint* c, int s, const uint8_t* bytes, int n);
/* The last mwx_full* call on the state: -1 it had no constraint; 1 every
 * decoded window's final sequence ended in an accepting state; 0 otherwise (a
 * dead state, or a window that ended in a non-accepting state). */
int mwx_full_constraint_status_from_state(struct mwx_state* state);

#ifdef __cplusplus
}
#endif

#endif /* MWX_H */
