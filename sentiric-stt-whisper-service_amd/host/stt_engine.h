// SttEngine on the mwx C ABI — the drop-in for the reference's
// src/stt_engine.h:16-115 (same class, method names, argument meaning, result
// types and error behaviour), with whisper.h replaced by include/mwx.h.
//
// Kept from the reference: the state pool with a queue timeout that throws
// EngineBusyException (src/stt_engine.cpp:63-85), the request-option defaults
// (:204-212), the whisper_full parameter mapping (:214-243), the too-short
// audio gate (:153-167), and the result post-filters (:261-311: hallucination
// phrases, tokens with id >= eot skipped, average token p < 0.40 drops the
// segment), per-segment prosody (src/stt_engine.cpp:313-337: computed on the
// GPU by mwx_prosody_batch, bit-identical to src/prosody_extractor.cpp) and
// speaker clustering (src/speaker_cluster.cpp, restated below), and
// resampling of non-16 kHz input (resample_audio, :87-106, :138-145: on the
// GPU by mwx_resample; the input is kept when resampling yields nothing, as
// the reference keeps it when libsamplerate fails, :141), and the VAD speech
// gate (is_speech_detected, :108-115, :169-194: on the GPU by mwx_vad_*; a clip
// with no speech comes back as one empty result and never takes a state).
// The gate's decision rule is this engine's own (deviation D6): any
// chunk probability >= Settings::vad_threshold. Settings::vad_trim (off by
// default) replaces the gate by silence trimming: mwx_vad_trim_batch +
// mwx_full_batch_trimmed (deviation D7). Settings::stream_vad and
// stream_endpoint_silence_ms (off by default) give the stream sessions a VAD
// that is fed incrementally (mwx_vad_stream_*; deviation D11).
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "mwx.h"

namespace mwx_host {

// The Settings fields SttEngine reads (reference src/config.h:10-80 defaults).
struct Settings {
  std::string model_dir = "/models";
  std::string model_filename = "ggml-medium.bin";
  // The reference defaults to true (src/config.h:30); off here so that an
  // engine built without a VAD model file behaves as before.
  bool enable_vad = false;
  std::string vad_model_filename = "ggml-silero-vad.bin";  // src/config.h:25
  float vad_threshold = 0.75f;                             // src/config.h:34
  // Engine extension (whisper.cpp's params.vad): with enable_vad
  // and a loaded VAD model, the clip's speech segments are cut out on the GPU
  // (threshold = vad_threshold, the other mwx_vad_params at their defaults) and
  // only they are decoded; times are reported on the clip's own timeline. A
  // clip without segments gets the gate's empty result. Replaces the gate
  // pass: a clip still goes through the VAD once.
  bool vad_trim = false;
  int vad_ms_min_duration = 500;
  int n_threads = 4;
  int parallel_requests = 2;
  int request_queue_timeout_ms = 5000;
  std::string language = "auto";
  bool no_timestamps = false;
  int beam_size = 5;
  float temperature = 0.0f;
  int best_of = 5;
  float logprob_threshold = -0.7f;
  float no_speech_threshold = 0.85f;
  bool flash_attn = true;
  bool suppress_nst = true;
  int gpu_device = 0;
  int stream_buffer_samples = 8000;
  float cluster_threshold = 0.88f;  // src/config.h:71
  // Engine extension (no reference counterpart): dynamic request batching.
  // max_batch > 1: concurrent transcribe() calls with the same decoding
  // options are gathered (up to max_batch, waiting at most batch_window_us
  // for more) and run as one mwx_full_batch by one of parallel_requests
  // batcher threads. max_batch = 1 keeps the reference's one-request-per-
  // state path.
  int max_batch = 1;
  int batch_window_us = 2000;
  // Engine extension (whisper.h dtw_token_timestamps): the
  // context computes mwx_token_data.t_dtw from the alignment heads'
  // cross-attention, and TokenData.t0 / t1 (the service's words[].start / end)
  // come from it instead of the token_timestamps heuristic: t0 = the token's
  // t_dtw, t1 = the next kept token's t_dtw, the segment's t1 for its last
  // token. dtw_aheads_preset is an enum mwx_alignment_heads_preset value;
  // N_TOP_MOST reads dtw_n_top, CUSTOM dtw_aheads ((decoder layer, head)).
  bool dtw_token_timestamps = false;
  int dtw_aheads_preset = 0;
  int dtw_n_top = -1;
  std::vector<std::pair<int, int>> dtw_aheads;
  // Audio context (mwx_full_params.audio_ctx / audio_ctx_fit; DESIGN.md D9,
  // INTEGRATION.md "Audio context"), for every request path. audio_ctx > 0:
  // every window is encoded to that many frames; audio_ctx_fit: every window
  // to the frames its remaining audio needs (audio_ctx the floor). Both off
  // by default: the effect of a short context on recognition quality is
  // unmeasured.
  int audio_ctx = 0;
  bool audio_ctx_fit = false;
  // Chunked long-form transcription (INTEGRATION.md "Chunked
  // long-form transcription"), on top of vad_trim: vad_chunk_s in [1, 30] packs
  // a clip's speech into chunks of at most that many seconds
  // (mwx_vad_trim_batch_chunked, with max_speech_duration_s = min(its value,
  // vad_chunk_s) so that uninterrupted speech is still cut) and decodes them
  // side by side, at most vad_chunk_batch per engine run
  // (mwx_full_batch_chunked). 0 = off. Active only with vad_trim active and a
  // library that has the calls; otherwise the path is vad_trim's. Streaming
  // sessions do not chunk.
  float vad_chunk_s = 0.0f;
  int vad_chunk_batch = 32;
  // One language per recording on the chunked path: with
  // language "auto", the language is detected once over the recording's
  // leading chunks (about 30 s of speech, pooled by length) and every chunk is
  // transcribed in it (mwx_full_params.chunk_language =
  // MWX_CHUNK_LANG_RECORDING). Off: every chunk detects its own language.
  bool chunk_language_recording = false;
  // Contextual biasing (mwx_full_params.bias_phrases; DESIGN.md D14,
  // INTEGRATION.md "Contextual biasing"): the boost of a request's hotwords
  // when the request does not give one. 0 (default): biasing off. The effect
  // on recognition and a sensible range are unmeasured.
  float hotword_boost = 0.0f;
  // Constrained decoding (mwx_full_params.constraint; DESIGN.md D15,
  // INTEGRATION.md "Constrained decoding"): the penalty of a request's choices
  // when the request does not give one. Finite and > 0; default 100.
  float choice_penalty = 100.0f;
  // Streaming VAD for StreamSession (INTEGRATION.md "Streaming"),
  // both off by default and inert without a loaded VAD model or against a
  // library that lacks the mwx_vad_stream_* calls.
  // stream_vad: with the gate path active (enable_vad, a VAD model, vad_trim not
  // active) a session feeds every sample it buffers to a VAD stream of its own
  // and hands the gate decision (max probability >= vad_threshold: rule D6 on
  // the buffer, bit for bit) to its transcriptions instead of running the gate
  // over the whole buffer again for every partial. The events do not change.
  bool stream_vad = false;
  // stream_endpoint_silence_ms = S > 0: server-side endpointing. The session's
  // VAD stream runs the segment rule with threshold = vad_threshold and
  // min_silence_duration_ms = S (the other mwx_vad_params at their defaults);
  // when a feed closes a speech segment the buffer up to the end of the chunk
  // that closed it is transcribed and finalized as the client's empty chunk
  // finalizes it, and the buffer goes on with the rest.
  int stream_endpoint_silence_ms = 0;
};

// Reads the DTW settings from the environment, as the service reads its other
// settings: STT_WHISPER_SERVICE_DTW_TOKEN_TIMESTAMPS (true / 1),
// STT_WHISPER_SERVICE_DTW_AHEADS_PRESET (n_top_most, custom, tiny.en, tiny,
// base.en, base, small.en, small, medium.en, medium, large-v1, large-v2,
// large-v3, large-v3-turbo), STT_WHISPER_SERVICE_DTW_N_TOP and
// STT_WHISPER_SERVICE_DTW_AHEADS ("layer:head,layer:head,..."). Unset
// variables leave the fields as they are.
void settings_dtw_from_env(Settings& s);
// STT_WHISPER_SERVICE_HOTWORD_BOOST (a finite number >= 0) into
// Settings::hotword_boost; unset or malformed leaves the field as it is.
void settings_hotwords_from_env(Settings& s);
// STT_WHISPER_SERVICE_CHOICE_PENALTY (a finite number > 0) into
// Settings::choice_penalty; unset or malformed leaves the field as it is.
void settings_choices_from_env(Settings& s);

// Owner of one mwx_vad_trimmed (vad_trim; defined in stt_engine.cpp).
struct TrimmedAudio;
// Owner of one mwx_vad_stream (stream_vad / stream_endpoint_silence_ms; defined
// in stt_engine.cpp). Must not outlive its engine.
struct VadStreamHandle;

struct TokenData {
  std::string text;
  float p;
  int64_t t0;
  int64_t t1;
};

// src/prosody_extractor.h:6-27
struct AffectiveTags {
  std::string gender_proxy;   // "M" / "F" / "?"
  std::string emotion_proxy;  // "excited" | "neutral" | "sad" | "angry"
  float arousal = 0.0f;
  float valence = 0.0f;
  float pitch_mean = 0.0f;
  float pitch_std = 0.0f;
  float energy_mean = 0.0f;
  float energy_std = 0.0f;
  float spectral_centroid = 0.0f;
  float zero_crossing_rate = 0.0f;
  std::vector<float> speaker_vec;  // 8-D
};

struct ProsodyOptions {
  float lpf_alpha = 0.07f;
  float gender_threshold = 170.0f;
  float min_pitch = 60.0f;
  float max_pitch = 500.0f;
};

// Online speaker clustering of segment speaker vectors (the reference's
// SpeakerClusterer, src/speaker_cluster.h:45-66 / .cpp:5-40): each vector
// joins the cluster of highest cosine similarity if that is >= threshold
// (running-mean centroid), else opens "spk_<n>". Clusters live in an
// std::unordered_map keyed by id, scanned in the map's order with ties kept
// by the first — the same container as the reference, hence the same order.
class SpeakerClusterer {
 public:
  explicit SpeakerClusterer(float threshold = 0.88f) : threshold_(threshold) {}
  std::string assign_or_add(const std::vector<float>& vec);

 private:
  struct Cluster {
    std::string id;
    std::vector<float> centroid;
    size_t count = 0;
  };
  float threshold_;
  std::unordered_map<std::string, Cluster> clusters_;
  int next_id_ = 0;
};

struct RequestOptions {
  std::string language;
  std::string prompt;
  bool translate = false;
  bool enable_diarization = false;
  float temperature = -1.0f;
  int beam_size = -1;
  int best_of = -1;
  ProsodyOptions prosody_opts;
  std::function<bool()> should_abort = nullptr;
  // Contextual biasing: words or short phrases the recogniser should prefer.
  // Each becomes two boosted phrases (" word" and "word", through
  // mwx_tokenize); one that tokenizes to nothing or to more than
  // MWX_BIAS_MAX_TOKENS tokens is dropped with a warning. hotword_boost < 0:
  // Settings::hotword_boost. A boost of 0 passes nothing to the engine.
  std::vector<std::string> hotwords;
  float hotword_boost = -1.0f;
  // Constrained decoding: the closed set of answers the transcript is held to
  // (one per window). An empty choice, or one with a NUL byte, is dropped with
  // a warning; with none left, or a set the engine refuses (more than 4095
  // states), the request runs unconstrained. choice_flags: MWX_CONSTRAINT_*.
  // A request with choices decodes with no_timestamps (a closed answer is one
  // untimed piece of text; timestamp tokens are outside the constraint).
  // choice_penalty < 0: Settings::choice_penalty.
  std::vector<std::string> choices;
  int choice_flags = MWX_CONSTRAINT_FOLD_CASE | MWX_CONSTRAINT_LEADING_SPACE |
                     MWX_CONSTRAINT_TRAILING_PUNCT;
  float choice_penalty = -1.0f;
};

struct TranscriptionResult {
  std::string text;
  std::string language;
  float prob;
  int64_t t0;
  int64_t t1;
  bool speaker_turn_next;
  std::vector<TokenData> tokens;
  int token_count = 0;
  std::string gender_proxy;
  std::string emotion_proxy;
  float arousal = 0.0f;
  float valence = 0.0f;
  AffectiveTags affective;
  std::string speaker_id;
  // the probability the detection pass gave the language used (language
  // "auto"), -1 when the call did not detect
  float language_probability = -1.0f;
  // mwx_full_constraint_status_from_state of the call: -1 no choices, 1 every
  // window ended on one of them, 0 otherwise
  int choice_match = -1;
};

// Transcript alignment (SttEngine::align; mwx.h mwx_align_batch, rule D12):
// the caller's text, teacher-forced against the audio. One entry per text
// token: its log-probability given the audio and the text before it, its DTW
// time (10 ms units; -1 unless Settings::dtw_token_timestamps) and the model's
// own first choice at that position.
struct AlignedToken {
  std::string text;
  int id;
  float p, plog;
  int64_t t;  // t_dtw or -1
  int top_id;
  std::string top_text;
  float top_plog;
};
struct AlignmentResult {
  bool ok = false;
  std::string text, language;
  float avg_logprob = 0;  // mean plog of the tokens (0 without tokens)
  float eot_logprob = 0;  // log-probability that the text ends after its last token
  int n_agree = 0;        // tokens with top_id == id
  std::vector<AlignedToken> tokens;
};

class EngineBusyException : public std::runtime_error {
 public:
  explicit EngineBusyException(const std::string& msg) : std::runtime_error(msg) {}
};

class SttEngine {
 public:
  explicit SttEngine(const Settings& settings);  // throws std::runtime_error on load failure
  ~SttEngine();
  SttEngine(const SttEngine&) = delete;
  SttEngine& operator=(const SttEngine&) = delete;

  // Everything the engine parameters read from the request: requests with
  // equal keys share one batched engine call. Hotwords and their boost are
  // part of it only when there are hotwords.
  std::string options_key(const RequestOptions& o) const;

  bool is_ready() const { return ctx_ != nullptr; }
  const Settings& get_settings() const { return settings_; }
  // Settings::audio_ctx / audio_ctx_fit of the requests that start after the
  // call (not synchronized with requests in flight: set it before serving).
  // false, and nothing changed, for more than kMaxAudioCtx frames.
  static constexpr int kMaxAudioCtx = 1500;  // every Whisper model's n_audio_ctx
  bool set_audio_ctx(int audio_ctx, bool fit) {
    if (audio_ctx > kMaxAudioCtx) return false;
    settings_.audio_ctx = audio_ctx > 0 ? audio_ctx : 0;
    settings_.audio_ctx_fit = fit;
    return true;
  }

  // Settings::vad_chunk_s / vad_chunk_batch of the requests that start after
  // the call (as set_audio_ctx: set it before serving). chunk_s = 0 switches
  // chunking off; false, and nothing changed, for a chunk_s outside [1, 30]
  // or a batch < 1. Whether chunking then runs: chunk_active().
  bool set_vad_chunk(float chunk_s, int chunk_batch) {
    if (chunk_s != chunk_s || chunk_batch < 1) return false;
    if (chunk_s != 0.0f && !(chunk_s >= 1.0f && chunk_s <= 30.0f)) return false;
    settings_.vad_chunk_s = chunk_s;
    settings_.vad_chunk_batch = chunk_batch;
    return true;
  }
  // Settings::chunk_language_recording of the requests that start after the
  // call (as set_audio_ctx: set it before serving)
  void set_chunk_language_recording(bool on) { settings_.chunk_language_recording = on; }
  bool chunk_active() const { return trim_active_ && chunk_bound_ && settings_.vad_chunk_s > 0.0f; }

  struct PerformanceMetrics {
    double queue_time_ms;
    double processing_time_ms;
    int token_count;
  };

  std::vector<TranscriptionResult> transcribe(const std::vector<float>& pcmf32,
                                              int input_sample_rate,
                                              const RequestOptions& options,
                                              PerformanceMetrics* out_metrics = nullptr);
  std::vector<TranscriptionResult> transcribe_pcm16(const std::vector<int16_t>& pcm16,
                                                    int input_sample_rate,
                                                    const RequestOptions& options,
                                                    PerformanceMetrics* out_metrics = nullptr);

  // Batched entry (no reference counterpart): B independent 16 kHz clips in
  // one GPU pass, each result list filtered exactly as transcribe() filters
  // it. Runs on states kept for batch calls (grown on demand, reused; one
  // batch call at a time).
  std::vector<std::vector<TranscriptionResult>> transcribe_batch(
      const std::vector<std::vector<float>>& clips, const RequestOptions& options);

  // Transcript alignment (no reference counterpart): scores and DTW times of
  // `text` against at most 30 s of audio. The audio is resampled as
  // transcribe() resamples it; the text is trimmed, prefixed with one space and
  // tokenised (at most 224 tokens). No VAD gate, no minimum-duration gate, no
  // post-filter, no prompt (RequestOptions::prompt is not used); language as in
  // transcribe() ("auto" detects), the result's language is the one used. Any
  // failure (too many tokens, audio over 30 s, an engine error, a library
  // without the alignment calls) is logged and gives ok = false; the state
  // pool's timeout throws EngineBusyException as transcribe() does. The
  // request batcher is not involved.
  AlignmentResult align(const std::vector<float>& pcm, int sample_rate, const std::string& text,
                        const RequestOptions& options);
  AlignmentResult align_pcm16(const std::vector<int16_t>& pcm16, int sample_rate,
                              const std::string& text, const RequestOptions& options);
  // Language identification (no reference counterpart): the clip's top_k
  // languages (code, probability), by probability descending, then by language
  // id; top_k < 1 or above the number of languages: all of them. The audio is
  // resampled and the minimum-duration gate applied as transcribe() does
  // (too short: empty); no VAD gate. One detection-only engine call
  // (detect_language) on a pooled state; only the first 30 s are looked at.
  // Empty on any failure or against a library without the call.
  std::vector<std::pair<std::string, float>> detect_language(const std::vector<float>& pcm,
                                                             int sample_rate, int top_k);
  std::vector<std::pair<std::string, float>> detect_language_pcm16(
      const std::vector<int16_t>& pcm16, int sample_rate, int top_k);

  // B independent 16 kHz clips and their texts in one GPU pass, on the states
  // kept for batch calls; clips.size() != texts.size() fails every entry.
  std::vector<AlignmentResult> align_batch(const std::vector<std::vector<float>>& clips16k,
                                           const std::vector<std::string>& texts,
                                           const RequestOptions& options);
  bool align_available() const { return align_bound_; }

  // SttEngine::resample_audio (src/stt_engine.cpp:87-106) on the GPU
  // (mwx_resample): empty when src_rate == target_rate, the input is empty or
  // resampling fails — the caller then keeps its input, as the reference does.
  std::vector<float> resample_audio(const float* input, size_t input_size, int src_rate,
                                    int target_rate);

  // src/stt_engine.cpp:108-115. True when there is no VAD context or the call
  // failed (the gate stays open); otherwise true when at least one chunk
  // probability is >= Settings::vad_threshold.
  bool is_speech_detected(const float* pcm, size_t n_samples);

  // Batches run by the request batcher so far (max_batch > 1).
  long batches_run() const { return batches_run_.load(); }

  // ---- streaming VAD (Settings::stream_vad / stream_endpoint_silence_ms) ----
  // Whether a StreamSession of this engine takes its gate decisions from a VAD
  // stream / endpoints on the server side.
  bool stream_vad_active() const { return stream_gate_active_; }
  bool stream_endpoint_active() const { return stream_endpoint_active_; }
  // Clips that went through the whole-buffer VAD gate so far (is_speech_detected
  // and transcribe_batch's batched gate pass).
  long vad_gate_runs() const { return vad_gate_runs_.load(); }
  // transcribe_pcm16 at 16 kHz with the gate's decision supplied by the caller
  // (`speech`) wherever transcribe() would run the gate over the clip.
  std::vector<TranscriptionResult> transcribe_pcm16_gated(const std::vector<int16_t>& pcm16,
                                                          const RequestOptions& options,
                                                          bool speech,
                                                          PerformanceMetrics* out_metrics = nullptr);
  // A VAD stream for one session; null when neither setting is active or the
  // library refuses. Every call below takes the VAD mutex for one
  // mwx_vad_stream_* call (n = 1); false = the call failed.
  std::shared_ptr<VadStreamHandle> vad_stream_open();
  bool vad_stream_feed(VadStreamHandle& h, const float* pcm, size_t n);
  bool vad_stream_reset(VadStreamHandle& h);
  // The two queries below read what the stream's last call left on the host
  // and take no lock: a stream is used by its one session.
  // Rule D6 over the first n_chunks probabilities of the stream (< 0: all of
  // them, the provisional one of a partial last chunk included).
  bool vad_stream_speech(const VadStreamHandle& h, long n_chunks = -1) const;
  // closed_at of the last raw segment the stream has closed; 0 when none.
  int64_t vad_stream_last_closed_at(const VadStreamHandle& h) const;

 private:
  // ---- dynamic request batching (Settings::max_batch > 1) ----
  struct Pending {
    const std::vector<float>* pcm;
    RequestOptions options;
    std::string key;  // requests with equal keys share mwx_full_params
    std::chrono::steady_clock::time_point t_enq;
    bool started = false, done = false, cancelled = false;
    int ret = 0;
    double t_start_ms = 0.0, t_proc_ms = 0.0;
    int token_count = 0;
    std::vector<TranscriptionResult> results;
    std::shared_ptr<TrimmedAudio> trimmed;  // vad_trim: the request's single-clip object
  };
  std::vector<TranscriptionResult> transcribe_batched(const std::vector<float>& pcmf32,
                                                      const RequestOptions& options,
                                                      PerformanceMetrics* out_metrics,
                                                      std::shared_ptr<TrimmedAudio> trimmed);
  void batcher_loop(std::vector<mwx_state*> states);
  std::deque<std::shared_ptr<Pending>> queue_;
  std::mutex q_mutex_;
  std::condition_variable q_cv_;     // batcher: new work / stop
  std::condition_variable done_cv_;  // callers: started / done
  std::vector<std::thread> batchers_;
  bool stop_ = false;
  std::atomic<long> batches_run_{0};

  mwx_state* acquire_state();
  void release_state(mwx_state* state);
  // the arrays mwx_full_params.bias_phrases points into: alive as long as the
  // parameters are in use
  struct BiasKeep {
    std::vector<std::vector<mwx_token>> toks;
    std::vector<mwx_bias_phrase> phrases;
    std::shared_ptr<const mwx_constraint> constraint;  // (RequestOptions::choices)
  };
  // Constrained decoding: the penalty the request resolves to, the choices it
  // keeps, and their constraint (built once per distinct (flags, choices) and
  // kept: requests of one batch key share it)
  float choice_penalty_of(const RequestOptions& o) const;
  static std::vector<std::string> kept_choices(const RequestOptions& o, bool warn);
  std::shared_ptr<const mwx_constraint> constraint_of(const RequestOptions& o) const;
  mutable std::mutex con_mutex_;
  mutable std::map<std::string, std::shared_ptr<const mwx_constraint>> con_cache_;
  float hotword_boost_of(const RequestOptions& o) const;
  void make_bias(const RequestOptions& options, BiasKeep& keep) const;
  mwx_full_params make_params(const RequestOptions& options, std::string& target_lang,
                              std::function<bool()>& abort_fn, BiasKeep& bias) const;
  std::vector<TranscriptionResult> collect(mwx_state* state, const std::string& lang,
                                           const float* pcm, size_t pcm_size,
                                           const ProsodyOptions& popts, int* token_count) const;

  // vad_trim: VAD, segments and compaction of the clips in one pass under the
  // VAD mutex; null when trimming is off or the call failed (the clips then
  // take the untrimmed path)
  std::shared_ptr<TrimmedAudio> trim_clips(const float* const* pcm, const int* n_samples,
                                              int n_clips);
  bool trim_active_ = false;  // vad_trim, a VAD context and a library that has the calls
  bool chunk_bound_ = false;  // the library has the chunked calls
  bool lang_bound_ = false;   // the library has the language-probability calls
  bool align_bound_ = false;  // the library has the alignment calls
  // mwx_align_batch on `states` and the results of its clips
  std::vector<AlignmentResult> align_run(mwx_state* const* states,
                                         const std::vector<const std::vector<float>*>& clips,
                                         const std::vector<std::string>& texts,
                                         const RequestOptions& options);
  bool stream_gate_active_ = false;      // stream_vad, the gate path and the stream calls
  bool stream_endpoint_active_ = false;  // stream_endpoint_silence_ms, a VAD context, the calls
  std::atomic<long> vad_gate_runs_{0};
  friend struct VadStreamHandle;
  // transcribe() with the gate decision optionally supplied (gate != nullptr)
  std::vector<TranscriptionResult> transcribe_impl(const std::vector<float>& pcmf32,
                                                   int input_sample_rate,
                                                   const RequestOptions& options,
                                                   PerformanceMetrics* out_metrics,
                                                   const bool* gate);
  // the chunk batch of the engine call over trimmed audio: > 0 with chunking
  // active (mwx_full_batch_chunked), 0 for mwx_full_batch_trimmed
  int chunk_batch() const { return chunk_active() ? settings_.vad_chunk_batch : 0; }

  // the one result of a clip the VAD gate holds back (src/stt_engine.cpp:172-183)
  static TranscriptionResult empty_result(size_t pcm_size);

  Settings settings_;
  mwx_context* ctx_ = nullptr;
  mwx_vad_context* vad_ctx_ = nullptr;
  std::mutex vad_mutex_;
  std::queue<mwx_state*> state_pool_;
  std::mutex pool_mutex_;
  std::condition_variable pool_cv_;
  std::vector<mwx_state*> all_states_;
  mwx_state* aux_state_ = nullptr;  // resampling (its own stream)
  std::mutex aux_mutex_;
  std::vector<mwx_state*> batch_states_;  // transcribe_batch
  std::mutex batch_mutex_;

  struct StateGuard {
    SttEngine& engine;
    mwx_state* state;
    explicit StateGuard(SttEngine& e) : engine(e) { state = engine.acquire_state(); }
    ~StateGuard() {
      if (state) engine.release_state(state);
    }
    mwx_state* get() { return state; }
  };
};

}  // namespace mwx_host
