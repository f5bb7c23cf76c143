// SttEngine over the mwx C ABI. See stt_engine.h for what is kept from the
// reference (file:line citations there and below).
#include "stt_engine.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "text_filters.h"

// The VAD entry points are bound weakly: a library without them (an older
// libmwx, the CPU stub of the sanitizer builds) still links, and enable_vad
// then behaves as "the VAD model failed to load" (gate open).
#pragma weak mwx_vad_default_context_params
#pragma weak mwx_vad_init_from_file_with_params
#pragma weak mwx_vad_free
#pragma weak mwx_vad_detect_speech
#pragma weak mwx_vad_n_probs
#pragma weak mwx_vad_probs
#pragma weak mwx_vad_n_chunks
#pragma weak mwx_vad_detect_speech_batch
// ... and so are the trimming calls: without them vad_trim falls back to the gate
#pragma weak mwx_vad_default_params
#pragma weak mwx_vad_trim_batch
#pragma weak mwx_vad_trimmed_n_segments
#pragma weak mwx_vad_trimmed_free
#pragma weak mwx_full_batch_trimmed
// ... and the chunked calls: without them vad_chunk_s leaves the path vad_trim's
#pragma weak mwx_vad_trim_batch_chunked
#pragma weak mwx_vad_trimmed_n_chunks
#pragma weak mwx_full_batch_chunked
// ... and the stream calls: without them stream_vad and
// stream_endpoint_silence_ms are inert
#pragma weak mwx_vad_stream_init
#pragma weak mwx_vad_stream_free
#pragma weak mwx_vad_stream_reset
#pragma weak mwx_vad_stream_feed_batch
#pragma weak mwx_vad_stream_n_probs
#pragma weak mwx_vad_stream_probs
#pragma weak mwx_vad_stream_max_prob
#pragma weak mwx_vad_stream_n_segments
#pragma weak mwx_vad_stream_segment
// ... and the alignment calls (with the three lookups only align() uses):
// without them align() returns ok = false
#pragma weak mwx_align_batch
#pragma weak mwx_align_row
#pragma weak mwx_tokenize
#pragma weak mwx_constraint_from_choices
#pragma weak mwx_constraint_free
#pragma weak mwx_full_constraint_status_from_state
#pragma weak mwx_full_lang_id_from_state
#pragma weak mwx_lang_str
// ... and the language-probability calls: without them detect_language()
// returns nothing and language_probability stays -1
#pragma weak mwx_full_lang_probs_from_state
#pragma weak mwx_lang_max_id

namespace mwx_host {

// One session's VAD stream. Freeing it is a call on the engine's VAD context,
// so it takes the engine's VAD mutex.
struct VadStreamHandle {
  SttEngine& engine;
  mwx_vad_stream* s;
  VadStreamHandle(SttEngine& e, mwx_vad_stream* stream) : engine(e), s(stream) {}
  ~VadStreamHandle() {
    std::lock_guard<std::mutex> lock(engine.vad_mutex_);
    mwx_vad_stream_free(s);
  }
  VadStreamHandle(const VadStreamHandle&) = delete;
  VadStreamHandle& operator=(const VadStreamHandle&) = delete;
};

// The trimmed audio of one trim pass, and the object array of one
// mwx_full_batch_trimmed call. Plain structs rather than standard containers
// of the C type: the library's type then appears in no symbol of the host.
struct TrimmedAudio {
  mwx_vad_trimmed* t = nullptr;
  ~TrimmedAudio() {
    if (t) mwx_vad_trimmed_free(t);
  }
};

namespace {

struct TrimList {
  const mwx_vad_trimmed** p;
  explicit TrimList(size_t n) : p(new const mwx_vad_trimmed*[n]) {}
  ~TrimList() { delete[] p; }
  TrimList(const TrimList&) = delete;
  TrimList& operator=(const TrimList&) = delete;
};

// mwx_full_batch_trimmed, or with chunking active (chunk_batch > 0)
// mwx_full_batch_chunked. An object of a plain trim pass is one chunk per clip,
// so a setting changed between the trim pass and this call is harmless.
int full_trimmed(mwx_context* ctx, int chunk_batch, mwx_state* const* states,
                 const mwx_full_params& p, const TrimList& objs, const int* clip_index, int n) {
  if (chunk_batch > 0)
    return mwx_full_batch_chunked(ctx, states, p, objs.p, clip_index, n, chunk_batch);
  return mwx_full_batch_trimmed(ctx, states, p, objs.p, clip_index, n);
}

bool abort_trampoline(void* user_data) {
  auto* fn = static_cast<std::function<bool()>*>(user_data);
  return fn && *fn && (*fn)();
}

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

constexpr float kMinAvgTokenProb = 0.40f;  // src/stt_engine.cpp:264

float cosine_sim(const std::vector<float>& a, const std::vector<float>& b) {
  float dot = 0.0f, na = 0.0f, nb = 0.0f;  // one pass, in index order
  for (size_t i = 0; i < a.size(); ++i) {
    dot += a[i] * b[i];
    na += a[i] * a[i];
    nb += b[i] * b[i];
  }
  if (na == 0.0f || nb == 0.0f) return 0.0f;
  return dot / (std::sqrt(na) * std::sqrt(nb));
}

AffectiveTags to_tags(const mwx_prosody& p) {
  static const char* kGender[] = {"?", "M", "F"};
  static const char* kEmotion[] = {"neutral", "excited", "angry", "sad"};
  AffectiveTags t;
  t.gender_proxy = kGender[p.gender];
  t.emotion_proxy = kEmotion[p.emotion];
  t.arousal = p.arousal;
  t.valence = p.valence;
  t.pitch_mean = p.pitch_mean;
  t.pitch_std = p.pitch_std;
  t.energy_mean = p.energy_mean;
  t.energy_std = p.energy_std;
  t.spectral_centroid = p.spectral_centroid;
  t.zero_crossing_rate = p.zero_crossing_rate;
  t.speaker_vec.assign(p.speaker_vec, p.speaker_vec + 8);
  return t;
}

}  // namespace

std::string SpeakerClusterer::assign_or_add(const std::vector<float>& vec) {
  const Cluster* best = nullptr;
  float best_sim = 0.0f;
  for (const auto& kv : clusters_) {
    const float sim = cosine_sim(vec, kv.second.centroid);
    if (sim > best_sim) {
      best_sim = sim;
      best = &kv.second;
    }
  }
  if (best && best_sim >= threshold_) {
    Cluster& c = clusters_[best->id];
    const size_t n = c.count;
    for (size_t i = 0; i < c.centroid.size(); ++i)
      c.centroid[i] = (c.centroid[i] * n + vec[i]) / (n + 1);
    c.count = n + 1;
    return c.id;
  }
  Cluster fresh;
  fresh.id = "spk_" + std::to_string(next_id_++);
  fresh.centroid = vec;
  fresh.count = 1;
  const std::string id = fresh.id;
  clusters_[id] = std::move(fresh);
  return id;
}

void settings_hotwords_from_env(Settings& s) {
  if (const char* v = std::getenv("STT_WHISPER_SERVICE_HOTWORD_BOOST")) {
    char* end = nullptr;
    const float b = std::strtof(v, &end);
    if (end != v && std::isfinite(b) && b >= 0.0f) s.hotword_boost = b;
  }
}

void settings_choices_from_env(Settings& s) {
  if (const char* v = std::getenv("STT_WHISPER_SERVICE_CHOICE_PENALTY")) {
    char* end = nullptr;
    const float b = std::strtof(v, &end);
    if (end != v && std::isfinite(b) && b > 0.0f) s.choice_penalty = b;
  }
}

void settings_dtw_from_env(Settings& s) {
  static const char* const kPresets[] = {"none", "n_top_most", "custom", "tiny.en", "tiny",
                                         "base.en", "base", "small.en", "small", "medium.en",
                                         "medium", "large-v1", "large-v2", "large-v3",
                                         "large-v3-turbo"};  // enum mwx_alignment_heads_preset
  if (const char* v = std::getenv("STT_WHISPER_SERVICE_DTW_TOKEN_TIMESTAMPS"))
    s.dtw_token_timestamps = std::string(v) == "true" || std::string(v) == "1";
  if (const char* v = std::getenv("STT_WHISPER_SERVICE_DTW_AHEADS_PRESET")) {
    s.dtw_aheads_preset = -1;  // (an unknown name fails the context's check)
    for (int i = 0; i < (int)(sizeof(kPresets) / sizeof(kPresets[0])); ++i)
      if (std::string(v) == kPresets[i]) s.dtw_aheads_preset = i;
  }
  if (const char* v = std::getenv("STT_WHISPER_SERVICE_DTW_N_TOP")) s.dtw_n_top = std::atoi(v);
  if (const char* v = std::getenv("STT_WHISPER_SERVICE_DTW_AHEADS")) {
    s.dtw_aheads.clear();
    const std::string str(v);
    size_t p = 0;
    while (p < str.size()) {
      size_t q = str.find(',', p);
      if (q == std::string::npos) q = str.size();
      const std::string item = str.substr(p, q - p);
      const size_t c = item.find(':');
      if (c != std::string::npos)
        s.dtw_aheads.emplace_back(std::atoi(item.substr(0, c).c_str()),
                                  std::atoi(item.substr(c + 1).c_str()));
      p = q + 1;
    }
  }
}

SttEngine::SttEngine(const Settings& settings) : settings_(settings) {
  const std::string path = settings_.model_dir + "/" + settings_.model_filename;
  mwx_context_params cp = mwx_context_default_params();
  cp.use_gpu = true;
  cp.flash_attn = settings_.flash_attn;
  cp.gpu_device = settings_.gpu_device;
  std::vector<mwx_ahead> aheads;
  for (const auto& a : settings_.dtw_aheads) aheads.push_back({a.first, a.second});
  cp.dtw_token_timestamps = settings_.dtw_token_timestamps;
  cp.dtw_aheads_preset = settings_.dtw_aheads_preset;
  cp.dtw_n_top = settings_.dtw_n_top;
  cp.dtw_aheads.n_heads = aheads.size();
  cp.dtw_aheads.heads = aheads.empty() ? nullptr : aheads.data();
  cp.dtw_mem_size = 0;
  ctx_ = mwx_init_from_file_with_params(path.c_str(), cp);
  if (!ctx_) throw std::runtime_error("Whisper model initialization failed");
  aux_state_ = mwx_init_state(ctx_);
  if (!aux_state_) throw std::runtime_error("Whisper state initialization failed");
  all_states_.push_back(aux_state_);
  align_bound_ = mwx_align_batch && mwx_align_row && mwx_tokenize && mwx_full_lang_id_from_state &&
                 mwx_lang_str;
  lang_bound_ = mwx_full_lang_probs_from_state && mwx_lang_max_id && mwx_lang_str &&
                mwx_full_lang_id_from_state;
  // src/stt_engine.cpp:44-55: a VAD model that does not load is logged and the
  // engine carries on without the gate
  if (settings_.enable_vad) {
    const std::string vad_path = settings_.model_dir + "/" + settings_.vad_model_filename;
    if (mwx_vad_default_context_params && mwx_vad_init_from_file_with_params &&
        mwx_vad_detect_speech && mwx_vad_n_probs && mwx_vad_probs && mwx_vad_free) {
      mwx_vad_context_params vp = mwx_vad_default_context_params();
      vp.n_threads = settings_.n_threads;
      vp.use_gpu = true;
      vp.gpu_device = settings_.gpu_device;
      vad_ctx_ = mwx_vad_init_from_file_with_params(vad_path.c_str(), vp);
    }
    if (!vad_ctx_)
      std::fprintf(stderr, "SttEngine: VAD model %s not loaded, VAD disabled\n", vad_path.c_str());
    trim_active_ = settings_.vad_trim && vad_ctx_ && mwx_vad_default_params &&
                   mwx_vad_trim_batch && mwx_vad_trimmed_n_segments && mwx_vad_trimmed_free &&
                   mwx_full_batch_trimmed;
    chunk_bound_ = mwx_vad_trim_batch_chunked && mwx_vad_trimmed_n_chunks && mwx_full_batch_chunked;
    if (settings_.vad_chunk_s != 0.0f &&
        !set_vad_chunk(settings_.vad_chunk_s, settings_.vad_chunk_batch)) {
      std::fprintf(stderr, "SttEngine: vad_chunk_s %g / vad_chunk_batch %d invalid, chunking off\n",
                   settings_.vad_chunk_s, settings_.vad_chunk_batch);
      settings_.vad_chunk_s = 0.0f;
    }
    const bool stream_bound = mwx_vad_stream_init && mwx_vad_stream_free && mwx_vad_stream_reset &&
                              mwx_vad_stream_feed_batch && mwx_vad_stream_n_probs &&
                              mwx_vad_stream_probs && mwx_vad_stream_max_prob &&
                              mwx_vad_stream_n_segments && mwx_vad_stream_segment &&
                              mwx_vad_default_params;
    stream_gate_active_ = settings_.stream_vad && vad_ctx_ && !trim_active_ && stream_bound;
    stream_endpoint_active_ = settings_.stream_endpoint_silence_ms > 0 && vad_ctx_ && stream_bound;
  }
  const int pool = std::max(1, settings_.parallel_requests);
  if (settings_.max_batch > 1) {
    // one batcher thread per pool slot, each with its own max_batch states
    for (int i = 0; i < pool; ++i) {
      std::vector<mwx_state*> sts;
      for (int b = 0; b < settings_.max_batch; ++b) {
        mwx_state* st = mwx_init_state(ctx_);
        if (!st) throw std::runtime_error("Whisper state initialization failed");
        sts.push_back(st);
        all_states_.push_back(st);
      }
      batchers_.emplace_back(&SttEngine::batcher_loop, this, sts);
    }
    return;
  }
  for (int i = 0; i < pool; ++i) {
    mwx_state* st = mwx_init_state(ctx_);
    if (!st) throw std::runtime_error("Whisper state initialization failed");
    state_pool_.push(st);
    all_states_.push_back(st);
  }
}

SttEngine::~SttEngine() {
  {
    std::lock_guard<std::mutex> lock(q_mutex_);
    stop_ = true;
  }
  q_cv_.notify_all();
  for (auto& t : batchers_) t.join();
  for (mwx_state* st : all_states_) mwx_free_state(st);
  if (vad_ctx_) mwx_vad_free(vad_ctx_);
  if (ctx_) mwx_free(ctx_);
}

// Everything make_params reads from the request: equal keys -> identical
// mwx_full_params, so those requests can share one mwx_full_batch.
std::string SttEngine::options_key(const RequestOptions& o) const {
  const int beam = o.beam_size >= 0 ? o.beam_size : settings_.beam_size;
  const float temp = o.temperature >= 0.0f ? o.temperature : settings_.temperature;
  const int best_of = o.best_of >= 0 ? o.best_of : settings_.best_of;
  const std::string lang = o.language.empty() ? settings_.language : o.language;
  char buf[96];
  std::snprintf(buf, sizeof buf, "%d|%.9g|%d|%d|%d|", beam, temp, best_of, (int)o.translate,
                (int)o.enable_diarization);
  std::string key = std::string(buf) + lang + "|" + o.prompt;
  if (!o.hotwords.empty()) {  // (no hotwords: the key as it always was)
    char hb[48];
    std::snprintf(hb, sizeof hb, "|hw%.9g", hotword_boost_of(o));
    key += hb;
    for (const std::string& w : o.hotwords) key += "|" + std::to_string(w.size()) + ":" + w;
  }
  if (!o.choices.empty()) {  // (no choices: the key as it always was)
    char cb[64];
    std::snprintf(cb, sizeof cb, "|ch%d,%.9g", o.choice_flags, choice_penalty_of(o));
    key += cb;
    for (const std::string& w : o.choices) key += "|" + std::to_string(w.size()) + ":" + w;
  }
  return key;
}

std::vector<TranscriptionResult> SttEngine::transcribe_batched(
    const std::vector<float>& pcmf32, const RequestOptions& options,
    PerformanceMetrics* out_metrics, std::shared_ptr<TrimmedAudio> trimmed) {
  auto req = std::make_shared<Pending>();
  req->pcm = &pcmf32;
  req->options = options;
  // trimmed and untrimmed requests (a failed trim pass) never share a batch
  req->key = options_key(options) + (trimmed ? "|trimmed" : "");
  req->trimmed = std::move(trimmed);
  req->t_enq = std::chrono::steady_clock::now();
  std::unique_lock<std::mutex> lock(q_mutex_);
  queue_.push_back(req);
  // every batcher: one already gathering another key would swallow a single
  // wakeup while an idle batcher sleeps
  q_cv_.notify_all();
  // EngineBusyException when no batcher picks the request up in time
  // (the state-pool queue timeout of src/stt_engine.cpp:63-85)
  if (!done_cv_.wait_for(lock, std::chrono::milliseconds(settings_.request_queue_timeout_ms),
                         [&] { return req->started; })) {
    req->cancelled = true;
    for (auto it = queue_.begin(); it != queue_.end(); ++it)
      if (*it == req) {
        queue_.erase(it);
        break;
      }
    throw EngineBusyException("Server is busy (Queue timeout)");
  }
  done_cv_.wait(lock, [&] { return req->done; });
  if (out_metrics) *out_metrics = {req->t_start_ms, req->t_proc_ms, req->token_count};
  if (req->ret != 0) {
    std::fprintf(stderr, "Whisper processing failed: %d\n", req->ret);
    return {};
  }
  return std::move(req->results);
}

void SttEngine::batcher_loop(std::vector<mwx_state*> states) {
  const int max_b = (int)states.size();
  while (true) {
    std::vector<std::shared_ptr<Pending>> batch;
    {
      std::unique_lock<std::mutex> lock(q_mutex_);
      q_cv_.wait(lock, [&] { return stop_ || !queue_.empty(); });
      if (stop_) return;
      // gather: wait up to batch_window_us for more requests of this key
      const auto deadline = queue_.front()->t_enq +
                            std::chrono::microseconds(settings_.batch_window_us);
      const std::string key = queue_.front()->key;
      auto count = [&] {
        int c = 0;
        for (auto& r : queue_) c += r->key == key;
        return c;
      };
      while (!stop_ && count() < max_b &&
             q_cv_.wait_until(lock, deadline) != std::cv_status::timeout) {
      }
      if (stop_) return;
      for (auto it = queue_.begin(); it != queue_.end() && (int)batch.size() < max_b;) {
        if ((*it)->key == key) {
          (*it)->started = true;
          batch.push_back(*it);
          it = queue_.erase(it);
        } else {
          ++it;
        }
      }
      // requests left behind (other keys, or beyond max_batch) go to an idle
      // batcher now rather than after this batch
      if (!queue_.empty()) q_cv_.notify_all();
    }
    done_cv_.notify_all();
    if (batch.empty()) continue;
    const auto t0 = std::chrono::steady_clock::now();
    std::string lang;
    // the batch is aborted only when every request in it asks to abort
    std::function<bool()> abort_fn = nullptr;
    bool any_abort = false;
    for (auto& r : batch) any_abort |= (bool)r->options.should_abort;
    if (any_abort)
      abort_fn = [&batch] {
        for (auto& r : batch)
          if (!r->options.should_abort || !r->options.should_abort()) return false;
        return true;
      };
    BiasKeep bias_keep;  // (the hotword phrases' arrays, alive for the call)
    const mwx_full_params p = make_params(batch[0]->options, lang, abort_fn, bias_keep);
    std::vector<const float*> ptrs;
    std::vector<int> lens;
    for (auto& r : batch) {
      ptrs.push_back(r->pcm->data());
      lens.push_back((int)r->pcm->size());
    }
    int ret;
    if (batch[0]->trimmed) {
      TrimList objs(batch.size());
      for (size_t b = 0; b < batch.size(); ++b) objs.p[b] = batch[b]->trimmed->t;
      const std::vector<int> first(batch.size(), 0);
      ret = full_trimmed(ctx_, chunk_batch(), states.data(), p, objs, first.data(),
                         (int)batch.size());
    } else {
      ret = mwx_full_batch(ctx_, states.data(), p, ptrs.data(), lens.data(), (int)batch.size());
    }
    const auto t1 = std::chrono::steady_clock::now();
    batches_run_++;
    for (size_t b = 0; b < batch.size(); ++b) {
      auto& r = *batch[b];
      r.ret = ret;
      r.t_start_ms = ms_between(r.t_enq, t0);
      r.t_proc_ms = ms_between(t0, t1);
      if (ret == 0) {
        try {
          r.results = collect(states[b], lang, r.pcm->data(), r.pcm->size(),
                              r.options.prosody_opts, &r.token_count);
        } catch (const std::exception& e) {
          std::fprintf(stderr, "SttEngine: %s\n", e.what());
          r.ret = -100;
        }
      }
    }
    {
      std::lock_guard<std::mutex> lock(q_mutex_);
      for (auto& r : batch) r->done = true;
    }
    done_cv_.notify_all();
  }
}

mwx_state* SttEngine::acquire_state() {
  std::unique_lock<std::mutex> lock(pool_mutex_);
  const bool ok = pool_cv_.wait_for(lock,
                                    std::chrono::milliseconds(settings_.request_queue_timeout_ms),
                                    [this] { return !state_pool_.empty(); });
  if (!ok) throw EngineBusyException("Server is busy (Queue timeout)");
  mwx_state* st = state_pool_.front();
  state_pool_.pop();
  return st;
}

void SttEngine::release_state(mwx_state* state) {
  std::lock_guard<std::mutex> lock(pool_mutex_);
  state_pool_.push(state);
  pool_cv_.notify_one();
}

std::vector<TranscriptionResult> SttEngine::transcribe_pcm16(const std::vector<int16_t>& pcm16,
                                                             int input_sample_rate,
                                                             const RequestOptions& options,
                                                             PerformanceMetrics* out_metrics) {
  std::vector<float> f(pcm16.size());
  for (size_t i = 0; i < pcm16.size(); ++i) f[i] = static_cast<float>(pcm16[i]) / 32768.0f;
  return transcribe(f, input_sample_rate, options, out_metrics);
}

// Parameter mapping of src/stt_engine.cpp:204-243.
// Contextual biasing (mwx_full_params.bias_phrases): the boost
// the request resolves to, and its hotwords as phrases.
float SttEngine::hotword_boost_of(const RequestOptions& o) const {
  if (o.hotwords.empty()) return 0.0f;
  const float b = o.hotword_boost >= 0.0f ? o.hotword_boost : settings_.hotword_boost;
  return std::isfinite(b) ? b : 0.0f;
}

void SttEngine::make_bias(const RequestOptions& options, BiasKeep& keep) const {
  keep.toks.clear();
  keep.phrases.clear();
  const float boost = hotword_boost_of(options);
  if (boost == 0.0f) return;  // (off: nothing is passed)
  if (!mwx_tokenize) {
    std::fprintf(stderr, "SttEngine: hotwords ignored: the library has no mwx_tokenize\n");
    return;
  }
  for (const std::string& w : options.hotwords) {
    if (w.empty()) continue;
    // two phrases per hotword: after a space (mid-sentence) and bare
    std::vector<std::vector<mwx_token>> forms;
    bool ok = true;
    for (const std::string& text : {" " + w, w}) {
      std::vector<mwx_token> t(MWX_BIAS_MAX_TOKENS + 1);
      const int n = mwx_tokenize(ctx_, text.c_str(), t.data(), (int)t.size());
      if (n < 1 || n > MWX_BIAS_MAX_TOKENS) {
        ok = false;
        break;
      }
      t.resize(n);
      forms.push_back(std::move(t));
    }
    if (!ok || keep.toks.size() + 2 > (size_t)MWX_BIAS_MAX_PHRASES) {
      std::fprintf(stderr,
                   "SttEngine: hotword \"%s\" dropped (no tokens, more than %d tokens, or more "
                   "than %d phrases)\n", w.c_str(), MWX_BIAS_MAX_TOKENS, MWX_BIAS_MAX_PHRASES);
      continue;
    }
    for (auto& t : forms) keep.toks.push_back(std::move(t));
  }
  for (const auto& t : keep.toks) keep.phrases.push_back({t.data(), (int)t.size(), boost});
}

// Constrained decoding (mwx_full_params.constraint).
float SttEngine::choice_penalty_of(const RequestOptions& o) const {
  const float p = o.choice_penalty >= 0.0f ? o.choice_penalty : settings_.choice_penalty;
  return (std::isfinite(p) && p > 0.0f) ? p : 100.0f;
}

std::vector<std::string> SttEngine::kept_choices(const RequestOptions& o, bool warn) {
  std::vector<std::string> kept;
  for (const std::string& c : o.choices) {
    if (c.empty() || c.find('\0') != std::string::npos) {
      if (warn) std::fprintf(stderr, "SttEngine: a choice dropped (empty, or it holds a NUL)\n");
      continue;
    }
    kept.push_back(c);
  }
  return kept;
}

std::shared_ptr<const mwx_constraint> SttEngine::constraint_of(const RequestOptions& o) const {
  if (o.choices.empty()) return nullptr;
  if (!mwx_constraint_from_choices || !mwx_constraint_free) {
    std::fprintf(stderr, "SttEngine: choices ignored: the library has no mwx_constraint_*\n");
    return nullptr;
  }
  std::string key = std::to_string(o.choice_flags);
  for (const std::string& c : o.choices) key += "|" + std::to_string(c.size()) + ":" + c;
  std::lock_guard<std::mutex> lock(con_mutex_);
  auto it = con_cache_.find(key);
  if (it != con_cache_.end()) return it->second;
  const std::vector<std::string> kept = kept_choices(o, true);
  std::shared_ptr<const mwx_constraint> con;
  if (!kept.empty()) {
    std::vector<const char*> texts;
    for (const std::string& c : kept) texts.push_back(c.c_str());
    if (mwx_constraint* raw =
            mwx_constraint_from_choices(texts.data(), (int)texts.size(), o.choice_flags))
      con = std::shared_ptr<const mwx_constraint>(
          raw, [](const mwx_constraint* p) { mwx_constraint_free(const_cast<mwx_constraint*>(p)); });
    else
      std::fprintf(stderr, "SttEngine: choices refused by the engine; running unconstrained\n");
  }
  if (con_cache_.size() >= 64) con_cache_.clear();  // (callers in flight hold their own reference)
  con_cache_[key] = con;
  return con;
}

mwx_full_params SttEngine::make_params(const RequestOptions& options, std::string& target_lang,
                                       std::function<bool()>& abort_fn, BiasKeep& bias) const {
  const int beam = options.beam_size >= 0 ? options.beam_size : settings_.beam_size;
  const float temp = options.temperature >= 0.0f ? options.temperature : settings_.temperature;
  const int best_of = options.best_of >= 0 ? options.best_of : settings_.best_of;
  const int strategy = beam > 1 ? MWX_SAMPLING_BEAM_SEARCH : MWX_SAMPLING_GREEDY;
  mwx_full_params p = mwx_full_default_params(strategy);
  if (abort_fn) {
    p.abort_callback = abort_trampoline;
    p.abort_callback_user_data = &abort_fn;
  }
  p.print_realtime = false;
  p.print_progress = false;
  p.print_timestamps = !settings_.no_timestamps;
  p.print_special = false;
  p.token_timestamps = true;
  p.suppress_nst = settings_.suppress_nst;
  p.no_speech_thold = settings_.no_speech_threshold;
  p.translate = options.translate;
  p.tdrz_enable = options.enable_diarization;
  target_lang = options.language.empty() ? settings_.language : options.language;
  p.language = target_lang.c_str();
  if (!options.prompt.empty()) p.initial_prompt = options.prompt.c_str();
  p.temperature = temp;
  if (strategy == MWX_SAMPLING_BEAM_SEARCH)
    p.beam_search.beam_size = beam;
  else
    p.greedy.best_of = best_of;
  p.entropy_thold = 2.40f;
  p.logprob_thold = settings_.logprob_threshold;
  p.n_threads = settings_.n_threads;
  p.audio_ctx = settings_.audio_ctx;
  p.audio_ctx_fit = settings_.audio_ctx_fit;
  p.chunk_language =
      settings_.chunk_language_recording ? MWX_CHUNK_LANG_RECORDING : MWX_CHUNK_LANG_PER_CHUNK;
  make_bias(options, bias);
  if (!bias.phrases.empty()) {
    p.bias_phrases = bias.phrases.data();
    p.n_bias_phrases = (int)bias.phrases.size();
  }
  bias.constraint = constraint_of(options);
  if (bias.constraint) {
    p.constraint = bias.constraint.get();
    p.constraint_penalty = choice_penalty_of(options);
    // a closed answer is one untimed piece of text: timestamp tokens are never
    // rejected (D15), and left on, their probability mass can outweigh every
    // allowed text token (the timestamp-versus-text rule) and end a window empty
    p.no_timestamps = true;
  }
  return p;
}

// Segment / token extraction and post-filters of src/stt_engine.cpp:258-337.
std::vector<TranscriptionResult> SttEngine::collect(mwx_state* state, const std::string& lang,
                                                    const float* pcm, size_t pcm_size,
                                                    const ProsodyOptions& popts,
                                                    int* token_count) const {
  std::vector<TranscriptionResult> results;
  std::vector<int64_t> seg_start, seg_len;
  // the used language's probability, when the call's detection pass ran
  float lang_prob = -1.0f;
  if (lang_bound_) {
    std::vector<float> probs((size_t)mwx_lang_max_id() + 1);
    const int n = mwx_full_lang_probs_from_state(state, probs.data(), (int)probs.size());
    const int id = mwx_full_lang_id_from_state(state);
    if (n > 0 && id >= 0 && id < n) lang_prob = probs[id];
  }
  const int eot = mwx_token_eot(ctx_);
  const int n_seg = mwx_full_n_segments_from_state(state);
  for (int i = 0; i < n_seg; ++i) {
    const char* tc = mwx_full_get_segment_text_from_state(state, i);
    std::string text = tc ? std::string(tc) : "";
    if (is_hallucination(text)) continue;
    const int64_t t0 = mwx_full_get_segment_t0_from_state(state, i);
    const int64_t t1 = mwx_full_get_segment_t1_from_state(state, i);
    const bool turn = mwx_full_get_segment_speaker_turn_next_from_state(state, i);
    std::vector<TokenData> tokens;
    std::vector<int64_t> t_dtw;
    double total_p = 0.0;
    int valid = 0;
    const int nt = mwx_full_n_tokens_from_state(state, i);
    for (int j = 0; j < nt; ++j) {
      const mwx_token_data d = mwx_full_get_token_data_from_state(state, i, j);
      if (d.id >= eot) continue;
      const char* ts = mwx_token_to_str(ctx_, d.id);
      tokens.push_back({std::string(ts ? ts : ""), d.p, d.t0, d.t1});
      t_dtw.push_back(d.t_dtw);
      total_p += d.p;
      ++valid;
    }
    // dtw_token_timestamps: a kept token starts at its t_dtw and ends where
    // the next kept token starts, the segment's last one at the segment's end
    // (a token the context gave no t_dtw keeps its t0 / t1)
    if (settings_.dtw_token_timestamps)
      for (size_t k = 0; k < tokens.size(); ++k) {
        if (t_dtw[k] < 0) continue;
        tokens[k].t0 = t_dtw[k];
        tokens[k].t1 = k + 1 < tokens.size() && t_dtw[k + 1] >= 0 ? t_dtw[k + 1] : t1;
      }
    if (token_count) *token_count += valid;
    const float avg = valid > 0 ? static_cast<float>(total_p / valid) : 0.0f;
    if (avg < kMinAvgTokenProb && valid > 0) continue;
    // segment sample range (src/stt_engine.cpp:313-321)
    int64_t s0 = static_cast<int64_t>((static_cast<double>(t0) / 100.0) * 16000.0);
    int64_t s1 = static_cast<int64_t>((static_cast<double>(t1) / 100.0) * 16000.0);
    s0 = std::max<int64_t>(0, std::min<int64_t>(s0, (int64_t)pcm_size));
    s1 = std::max<int64_t>(s0, std::min<int64_t>(s1, (int64_t)pcm_size));
    seg_start.push_back(s0);
    seg_len.push_back(s1 - s0);
    TranscriptionResult r;
    r.text = text;
    r.language = lang;
    r.language_probability = lang_prob;
    r.prob = avg;
    r.t0 = t0;
    r.t1 = t1;
    r.speaker_turn_next = turn;
    r.tokens = std::move(tokens);
    r.token_count = valid;
    results.push_back(std::move(r));
  }
  // prosody of every kept segment in one GPU launch, then speaker clustering
  // in segment order (src/stt_engine.cpp:323-337); segments shorter than 160
  // samples get the empty-input tags and speaker "?"
  std::vector<mwx_prosody> pros(results.size());
  if (!results.empty()) {
    mwx_prosody_params pp;
    pp.lpf_alpha = popts.lpf_alpha;
    pp.gender_threshold = popts.gender_threshold;
    pp.min_pitch = popts.min_pitch;
    pp.max_pitch = popts.max_pitch;
    const int rc = mwx_prosody_batch(ctx_, state, pcm, (int64_t)pcm_size, seg_start.data(),
                                     seg_len.data(), (int)results.size(), 16000, &pp, pros.data());
    if (rc != 0) throw std::runtime_error("mwx_prosody_batch failed");
  }
  SpeakerClusterer clusterer(settings_.cluster_threshold);
  for (size_t i = 0; i < results.size(); ++i) {
    TranscriptionResult& r = results[i];
    r.affective = to_tags(pros[i]);
    r.gender_proxy = r.affective.gender_proxy;
    r.emotion_proxy = r.affective.emotion_proxy;
    r.arousal = r.affective.arousal;
    r.valence = r.affective.valence;
    r.speaker_id = seg_len[i] < 160 ? "?" : clusterer.assign_or_add(r.affective.speaker_vec);
  }
  if (mwx_full_constraint_status_from_state) {  // (RequestOptions::choices)
    const int match = mwx_full_constraint_status_from_state(state);
    for (TranscriptionResult& r : results) r.choice_match = match;
  }
  return results;
}

bool SttEngine::is_speech_detected(const float* pcm, size_t n_samples) {
  if (!vad_ctx_) return true;
  vad_gate_runs_++;
  std::lock_guard<std::mutex> lock(vad_mutex_);
  if (!mwx_vad_detect_speech(vad_ctx_, pcm, static_cast<int>(n_samples))) return true;
  const int n = mwx_vad_n_probs(vad_ctx_);
  const float* probs = mwx_vad_probs(vad_ctx_);
  for (int i = 0; i < n; ++i)
    if (probs[i] >= settings_.vad_threshold) return true;
  return false;
}

std::shared_ptr<TrimmedAudio> SttEngine::trim_clips(const float* const* pcm, const int* n_samples,
                                                    int n_clips) {
  if (!trim_active_) return nullptr;
  mwx_vad_params vp = mwx_vad_default_params();
  vp.threshold = settings_.vad_threshold;
  auto out = std::make_shared<TrimmedAudio>();
  std::lock_guard<std::mutex> lock(vad_mutex_);
  if (chunk_active()) {
    const float chunk_s = settings_.vad_chunk_s;
    vp.max_speech_duration_s = std::min(vp.max_speech_duration_s, chunk_s);
    out->t = mwx_vad_trim_batch_chunked(vad_ctx_, vp, chunk_s, pcm, n_samples, n_clips);
  } else {
    out->t = mwx_vad_trim_batch(vad_ctx_, vp, pcm, n_samples, n_clips);
  }
  return out->t ? out : nullptr;
}


TranscriptionResult SttEngine::empty_result(size_t pcm_size) {
  TranscriptionResult r;
  r.text = "";
  r.language = "unknown";
  r.prob = 0.0f;
  r.t0 = 0;
  r.t1 = static_cast<int64_t>(pcm_size / 16.0);
  r.speaker_turn_next = false;
  r.token_count = 0;
  // extract_prosody(nullptr, 0, ...): src/prosody_extractor.cpp:35-48
  r.affective.gender_proxy = "?";
  r.affective.emotion_proxy = "neutral";
  r.affective.speaker_vec.assign(8, 0.0f);
  r.speaker_id = "unknown";
  return r;
}

std::vector<TranscriptionResult> SttEngine::transcribe(const std::vector<float>& pcmf32,
                                                       int input_sample_rate,
                                                       const RequestOptions& options,
                                                       PerformanceMetrics* out_metrics) {
  return transcribe_impl(pcmf32, input_sample_rate, options, out_metrics, nullptr);
}

std::vector<TranscriptionResult> SttEngine::transcribe_pcm16_gated(
    const std::vector<int16_t>& pcm16, const RequestOptions& options, bool speech,
    PerformanceMetrics* out_metrics) {
  std::vector<float> f(pcm16.size());
  for (size_t i = 0; i < pcm16.size(); ++i) f[i] = static_cast<float>(pcm16[i]) / 32768.0f;
  return transcribe_impl(f, 16000, options, out_metrics, &speech);
}

// ---- VAD streams of the sessions --------------------------------------------
std::shared_ptr<VadStreamHandle> SttEngine::vad_stream_open() {
  if (!stream_gate_active_ && !stream_endpoint_active_) return nullptr;
  mwx_vad_params vp = mwx_vad_default_params();
  vp.threshold = settings_.vad_threshold;
  if (stream_endpoint_active_) vp.min_silence_duration_ms = settings_.stream_endpoint_silence_ms;
  std::lock_guard<std::mutex> lock(vad_mutex_);
  mwx_vad_stream* s = mwx_vad_stream_init(vad_ctx_, vp);
  if (!s) return nullptr;
  return std::make_shared<VadStreamHandle>(*this, s);
}

bool SttEngine::vad_stream_feed(VadStreamHandle& h, const float* pcm, size_t n) {
  constexpr size_t kMaxFeed = 480000;  // mwx_vad_stream_feed_batch's limit per call
  for (size_t at = 0; at < n; at += kMaxFeed) {
    const float* p = pcm + at;
    const int k = static_cast<int>(std::min(kMaxFeed, n - at));
    std::lock_guard<std::mutex> lock(vad_mutex_);
    if (mwx_vad_stream_feed_batch(vad_ctx_, &h.s, &p, &k, 1) != 0) return false;
  }
  return true;
}

bool SttEngine::vad_stream_reset(VadStreamHandle& h) {
  std::lock_guard<std::mutex> lock(vad_mutex_);
  return mwx_vad_stream_reset(h.s) == 0;
}

bool SttEngine::vad_stream_speech(const VadStreamHandle& h, long n_chunks) const {
  if (n_chunks < 0) return mwx_vad_stream_max_prob(h.s) >= settings_.vad_threshold;
  const long n = std::min<long>(n_chunks, mwx_vad_stream_n_probs(h.s));
  const float* probs = mwx_vad_stream_probs(h.s);
  for (long i = 0; i < n; ++i)
    if (probs[i] >= settings_.vad_threshold) return true;
  return false;
}

int64_t SttEngine::vad_stream_last_closed_at(const VadStreamHandle& h) const {
  const int n = mwx_vad_stream_n_segments(h.s);
  int64_t at = 0;
  if (n <= 0 || mwx_vad_stream_segment(h.s, n - 1, nullptr, nullptr, &at) != 0) return 0;
  return at;
}

std::vector<TranscriptionResult> SttEngine::transcribe_impl(const std::vector<float>& pcmf32,
                                                            int input_sample_rate,
                                                            const RequestOptions& options,
                                                            PerformanceMetrics* out_metrics,
                                                            const bool* gate) {
  const auto t_start = std::chrono::steady_clock::now();
  if (!ctx_) return {};
  if (options.should_abort && options.should_abort()) return {};
  // src/stt_engine.cpp:136-145: non-16 kHz input is resampled; an empty
  // result (failure) keeps the original buffer. One pass, as the reference
  // swaps its pcm pointer: the abort callback is polled once above and
  // processing_time_ms includes the resampling.
  std::vector<float> resampled;
  if (input_sample_rate != 16000)
    resampled = resample_audio(pcmf32.data(), pcmf32.size(), input_sample_rate, 16000);
  const std::vector<float>& pcm = resampled.empty() ? pcmf32 : resampled;
  const size_t pcm_size = pcm.size();
  const size_t min_samples = static_cast<size_t>((settings_.vad_ms_min_duration * 16000) / 1000);
  if (pcm_size < min_samples) {
    if (out_metrics) *out_metrics = {0.0, 0.0, 0};
    return {};
  }
  // src/stt_engine.cpp:169-194: silence never reaches Whisper. With vad_trim
  // the trim pass is the gate (no segments = no speech); if it fails the clip
  // goes on untrimmed, as a failed gate call leaves the gate open.
  std::shared_ptr<TrimmedAudio> trimmed;
  bool speech = true;
  if (trim_active_) {
    const float* p = pcm.data();
    const int n = static_cast<int>(pcm_size);
    trimmed = trim_clips(&p, &n, 1);
    speech = !trimmed || mwx_vad_trimmed_n_segments(trimmed->t, 0) != 0;
  } else if (settings_.enable_vad) {
    // (a session with a VAD stream has the decision already)
    speech = gate ? *gate : is_speech_detected(pcm.data(), pcm_size);
  }
  if (!speech) {
    if (out_metrics)
      *out_metrics = {0.0, ms_between(t_start, std::chrono::steady_clock::now()), 0};
    return {empty_result(pcm_size)};
  }
  if (settings_.max_batch > 1) return transcribe_batched(pcm, options, out_metrics, trimmed);
  StateGuard guard(*this);
  mwx_state* state = guard.get();
  const auto t_acq = std::chrono::steady_clock::now();
  std::string lang;
  std::function<bool()> abort_fn = options.should_abort;
  BiasKeep bias_keep;  // (the hotword phrases' arrays, alive for the call)
  const mwx_full_params p = make_params(options, lang, abort_fn, bias_keep);
  int ret;
  if (trimmed) {
    TrimList obj(1);
    obj.p[0] = trimmed->t;
    const int first = 0;
    ret = full_trimmed(ctx_, chunk_batch(), &state, p, obj, &first, 1);
  } else {
    ret = mwx_full_with_state(ctx_, state, p, pcm.data(), static_cast<int>(pcm_size));
  }
  const auto t_end = std::chrono::steady_clock::now();
  if (out_metrics) *out_metrics = {ms_between(t_start, t_acq), ms_between(t_acq, t_end), 0};
  if (ret != 0) {
    std::fprintf(stderr, options.should_abort && options.should_abort()
                             ? "Whisper processing aborted.\n"
                             : "Whisper processing failed: %d\n",
                 ret);
    return {};
  }
  return collect(state, lang, pcm.data(), pcm_size, options.prosody_opts,
                 out_metrics ? &out_metrics->token_count : nullptr);
}

// ---- transcript alignment ---------------------------------------------------
std::vector<AlignmentResult> SttEngine::align_run(mwx_state* const* states,
                                                  const std::vector<const std::vector<float>*>& clips,
                                                  const std::vector<std::string>& texts,
                                                  const RequestOptions& options) {
  const size_t B = clips.size();
  std::vector<AlignmentResult> out(B);
  std::vector<std::vector<mwx_token>> toks(B);
  for (size_t b = 0; b < B; ++b) {
    // trimmed, one leading space (the form Whisper's text tokens take after a
    // special token)
    const size_t a = texts[b].find_first_not_of(" \t\r\n");
    const size_t z = texts[b].find_last_not_of(" \t\r\n");
    const std::string t = a == std::string::npos ? "" : " " + texts[b].substr(a, z - a + 1);
    if (!t.empty()) {
      toks[b].resize(MWX_ALIGN_MAX_TOKENS);
      const int n = mwx_tokenize(ctx_, t.c_str(), toks[b].data(), MWX_ALIGN_MAX_TOKENS);
      if (n < 0) {
        std::fprintf(stderr, "SttEngine: align: %d tokens, at most %d\n", -n, MWX_ALIGN_MAX_TOKENS);
        return out;
      }
      toks[b].resize(static_cast<size_t>(n));
    }
    if (clips[b]->size() > static_cast<size_t>(MWX_CHUNK_SIZE) * MWX_SAMPLE_RATE) {
      std::fprintf(stderr, "SttEngine: align: %zu samples, at most %d s\n", clips[b]->size(),
                   MWX_CHUNK_SIZE);
      return out;
    }
  }
  std::string lang;
  std::function<bool()> abort_fn = options.should_abort;
  BiasKeep bias_keep;  // (the hotword phrases' arrays, alive for the call)
  const mwx_full_params p = make_params(options, lang, abort_fn, bias_keep);
  std::vector<const float*> ptrs;
  std::vector<int> lens, ntok;
  std::vector<const mwx_token*> tptr;
  for (size_t b = 0; b < B; ++b) {
    ptrs.push_back(clips[b]->data());
    lens.push_back(static_cast<int>(clips[b]->size()));
    tptr.push_back(toks[b].data());
    ntok.push_back(static_cast<int>(toks[b].size()));
  }
  const int ret = mwx_align_batch(ctx_, states, p, ptrs.data(), lens.data(), tptr.data(),
                                  ntok.data(), static_cast<int>(B));
  if (ret != 0) {
    std::fprintf(stderr, "SttEngine: align failed: %d\n", ret);
    return out;
  }
  for (size_t b = 0; b < B; ++b) {
    AlignmentResult& r = out[b];
    const int n = ntok[b];
    if (mwx_full_n_segments_from_state(states[b]) != 1 ||
        mwx_full_n_tokens_from_state(states[b], 0) != n) {
      std::fprintf(stderr, "SttEngine: align: clip %zu too short to align\n", b);
      continue;
    }
    const char* tc = mwx_full_get_segment_text_from_state(states[b], 0);
    r.text = tc ? tc : "";
    const char* ls = mwx_lang_str(mwx_full_lang_id_from_state(states[b]));
    r.language = ls ? ls : "";
    double sum = 0.0;
    bool rows = true;
    for (int j = 0; j < n && rows; ++j) {
      const mwx_token_data d = mwx_full_get_token_data_from_state(states[b], 0, j);
      AlignedToken t;
      const char* ts = mwx_token_to_str(ctx_, d.id);
      t.text = ts ? ts : "";
      t.id = d.id;
      t.p = d.p;
      t.plog = d.plog;
      t.t = d.t_dtw;
      mwx_token top = 0;
      rows = mwx_align_row(states[b], j, nullptr, &top, &t.top_plog) == 0;
      t.top_id = top;
      const char* tt = mwx_token_to_str(ctx_, top);
      t.top_text = tt ? tt : "";
      r.n_agree += t.top_id == t.id;
      sum += d.plog;
      r.tokens.push_back(std::move(t));
    }
    rows = rows && mwx_align_row(states[b], n, &r.eot_logprob, nullptr, nullptr) == 0;
    if (!rows) {
      std::fprintf(stderr, "SttEngine: align: clip %zu has no score rows\n", b);
      r = AlignmentResult();
      continue;
    }
    r.avg_logprob = n > 0 ? static_cast<float>(sum / n) : 0.0f;
    r.ok = true;
  }
  return out;
}

std::vector<AlignmentResult> SttEngine::align_batch(const std::vector<std::vector<float>>& clips16k,
                                                    const std::vector<std::string>& texts,
                                                    const RequestOptions& options) {
  std::vector<AlignmentResult> out(clips16k.size());
  if (!ctx_ || clips16k.empty()) return out;
  if (!align_bound_) {
    std::fprintf(stderr, "SttEngine: align: the library has no alignment calls\n");
    return out;
  }
  if (clips16k.size() != texts.size()) {
    std::fprintf(stderr, "SttEngine: align: %zu clips, %zu texts\n", clips16k.size(), texts.size());
    return out;
  }
  std::lock_guard<std::mutex> batch_lock(batch_mutex_);
  while (batch_states_.size() < clips16k.size()) {
    mwx_state* st = mwx_init_state(ctx_);
    if (!st) return out;
    batch_states_.push_back(st);
    all_states_.push_back(st);
  }
  std::vector<const std::vector<float>*> clips;
  for (const auto& c : clips16k) clips.push_back(&c);
  return align_run(batch_states_.data(), clips, texts, options);
}

AlignmentResult SttEngine::align(const std::vector<float>& pcmf32, int sample_rate,
                                 const std::string& text, const RequestOptions& options) {
  if (!ctx_) return {};
  if (!align_bound_) {
    std::fprintf(stderr, "SttEngine: align: the library has no alignment calls\n");
    return {};
  }
  if (options.should_abort && options.should_abort()) return {};
  std::vector<float> resampled;
  if (sample_rate != 16000)
    resampled = resample_audio(pcmf32.data(), pcmf32.size(), sample_rate, 16000);
  const std::vector<float>& pcm = resampled.empty() ? pcmf32 : resampled;
  // (with the request batcher on, the pool's states belong to the batchers:
  // the states kept for batch calls serve instead)
  if (settings_.max_batch > 1) {
    std::vector<AlignmentResult> r = align_batch({pcm}, {text}, options);
    return r.empty() ? AlignmentResult() : std::move(r[0]);
  }
  StateGuard guard(*this);
  mwx_state* state = guard.get();
  std::vector<AlignmentResult> r = align_run(&state, {&pcm}, {text}, options);
  return r.empty() ? AlignmentResult() : std::move(r[0]);
}

// ---- language identification ------------------------------------------------
std::vector<std::pair<std::string, float>> SttEngine::detect_language(
    const std::vector<float>& pcmf32, int sample_rate, int top_k) {
  if (!ctx_) return {};
  if (!lang_bound_) {
    std::fprintf(stderr, "SttEngine: detect_language: the library has no language-probability calls\n");
    return {};
  }
  std::vector<float> resampled;
  if (sample_rate != 16000)
    resampled = resample_audio(pcmf32.data(), pcmf32.size(), sample_rate, 16000);
  const std::vector<float>& pcm = resampled.empty() ? pcmf32 : resampled;
  const size_t min_samples = static_cast<size_t>((settings_.vad_ms_min_duration * 16000) / 1000);
  if (pcm.size() < min_samples) return {};
  const int n_lang = mwx_lang_max_id() + 1;
  std::vector<float> probs((size_t)n_lang);
  auto run = [&](mwx_state* state) -> int {
    std::string lang;
    std::function<bool()> abort_fn = nullptr;
    BiasKeep bias_keep;  // (the hotword phrases' arrays, alive for the call)
    mwx_full_params p = make_params(RequestOptions(), lang, abort_fn, bias_keep);
    p.language = "auto";
    p.detect_language = true;
    const int ret = mwx_full_with_state(ctx_, state, p, pcm.data(), static_cast<int>(pcm.size()));
    if (ret != 0) {
      std::fprintf(stderr, "SttEngine: detect_language failed: %d\n", ret);
      return 0;
    }
    return mwx_full_lang_probs_from_state(state, probs.data(), n_lang);
  };
  int n = 0;
  if (settings_.max_batch > 1) {
    // (the pool's states belong to the batchers: a batch-call state serves)
    std::lock_guard<std::mutex> batch_lock(batch_mutex_);
    if (batch_states_.empty()) {
      mwx_state* st = mwx_init_state(ctx_);
      if (!st) return {};
      batch_states_.push_back(st);
      all_states_.push_back(st);
    }
    n = run(batch_states_[0]);
  } else {
    StateGuard guard(*this);
    n = run(guard.get());
  }
  if (n <= 0) return {};
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return probs[a] > probs[b]; });
  if (top_k >= 1 && top_k < n) order.resize((size_t)top_k);
  std::vector<std::pair<std::string, float>> out;
  for (int id : order) {
    const char* s = mwx_lang_str(id);
    out.emplace_back(s ? s : "", probs[id]);
  }
  return out;
}

std::vector<std::pair<std::string, float>> SttEngine::detect_language_pcm16(
    const std::vector<int16_t>& pcm16, int sample_rate, int top_k) {
  std::vector<float> f(pcm16.size());
  for (size_t i = 0; i < pcm16.size(); ++i) f[i] = static_cast<float>(pcm16[i]) / 32768.0f;
  return detect_language(f, sample_rate, top_k);
}

AlignmentResult SttEngine::align_pcm16(const std::vector<int16_t>& pcm16, int sample_rate,
                                       const std::string& text, const RequestOptions& options) {
  std::vector<float> f(pcm16.size());
  for (size_t i = 0; i < pcm16.size(); ++i) f[i] = static_cast<float>(pcm16[i]) / 32768.0f;
  return align(f, sample_rate, text, options);
}

std::vector<float> SttEngine::resample_audio(const float* input, size_t input_size, int src_rate,
                                             int target_rate) {
  if (src_rate == target_rate || input_size == 0) return {};
  const long cap = mwx_resample_max_frames(static_cast<int>(input_size), src_rate, target_rate);
  if (cap <= 0) return {};
  std::vector<float> out(static_cast<size_t>(cap));
  int n = 0;
  {
    std::lock_guard<std::mutex> lock(aux_mutex_);
    n = mwx_resample(ctx_, aux_state_, input, static_cast<int>(input_size), src_rate, target_rate,
                     out.data(), static_cast<int>(cap));
  }
  if (n <= 0) {
    std::fprintf(stderr, "SttEngine: resampling %d -> %d Hz failed (%d)\n", src_rate, target_rate, n);
    return {};
  }
  out.resize(static_cast<size_t>(n));
  return out;
}

std::vector<std::vector<TranscriptionResult>> SttEngine::transcribe_batch(
    const std::vector<std::vector<float>>& clips, const RequestOptions& options) {
  std::vector<std::vector<TranscriptionResult>> out(clips.size());
  if (!ctx_ || clips.empty()) return out;
  const size_t min_samples = static_cast<size_t>((settings_.vad_ms_min_duration * 16000) / 1000);
  // VAD gate: one batched pass over the clips that pass the minimum duration;
  // a silent clip gets the empty result and is left out of the Whisper batch
  std::vector<size_t> run;  // indices of the clips that go to mwx_full_batch
  // vad_trim: one trim pass over those clips instead; a clip without segments
  // gets the empty result, the others are decoded from their trimmed audio.
  // Shorter clips end with no result either way and are left out here.
  std::shared_ptr<TrimmedAudio> trimmed;
  std::vector<int> trim_index;  // run[i]'s clip in `trimmed`
  if (trim_active_) {
    std::vector<size_t> gated;
    std::vector<const float*> vptrs;
    std::vector<int> vlens;
    for (size_t b = 0; b < clips.size(); ++b)
      if (clips[b].size() >= min_samples) {
        gated.push_back(b);
        vptrs.push_back(clips[b].data());
        vlens.push_back(static_cast<int>(clips[b].size()));
      }
    if (gated.empty()) return out;
    trimmed = trim_clips(vptrs.data(), vlens.data(), static_cast<int>(gated.size()));
    if (trimmed) {
      for (size_t g = 0; g < gated.size(); ++g) {
        if (mwx_vad_trimmed_n_segments(trimmed->t, static_cast<int>(g)) != 0) {
          run.push_back(gated[g]);
          trim_index.push_back(static_cast<int>(g));
        } else {
          out[gated[g]] = {empty_result(clips[gated[g]].size())};
        }
      }
    } else {
      for (size_t b = 0; b < clips.size(); ++b) run.push_back(b);  // failed: untrimmed
    }
  } else if (vad_ctx_ && mwx_vad_detect_speech_batch && mwx_vad_n_chunks) {
    std::vector<size_t> gated;
    std::vector<const float*> vptrs;
    std::vector<int> vlens, voff;
    int total = 0;
    for (size_t b = 0; b < clips.size(); ++b) {
      if (clips[b].size() < min_samples) {
        run.push_back(b);  // as before: decoded with the batch, result dropped
        continue;
      }
      gated.push_back(b);
      vptrs.push_back(clips[b].data());
      vlens.push_back(static_cast<int>(clips[b].size()));
      voff.push_back(total);
      total += mwx_vad_n_chunks(vlens.back());
    }
    std::vector<float> probs(static_cast<size_t>(std::max(total, 1)));
    int rc = 0;
    if (!gated.empty()) {
      vad_gate_runs_ += static_cast<long>(gated.size());
      std::lock_guard<std::mutex> lock(vad_mutex_);
      rc = mwx_vad_detect_speech_batch(vad_ctx_, vptrs.data(), vlens.data(),
                                       static_cast<int>(gated.size()), probs.data(), voff.data());
    }
    for (size_t g = 0; g < gated.size(); ++g) {
      bool speech = rc != 0;  // a failed call leaves the gate open
      const int n = mwx_vad_n_chunks(vlens[g]);
      for (int i = 0; i < n && !speech; ++i) speech = probs[voff[g] + i] >= settings_.vad_threshold;
      if (speech)
        run.push_back(gated[g]);
      else
        out[gated[g]] = {empty_result(clips[gated[g]].size())};
    }
    std::sort(run.begin(), run.end());
  } else {
    for (size_t b = 0; b < clips.size(); ++b) run.push_back(b);
  }
  if (run.empty()) return out;
  std::lock_guard<std::mutex> batch_lock(batch_mutex_);
  while (batch_states_.size() < run.size()) {
    mwx_state* st = mwx_init_state(ctx_);
    if (!st) return out;
    batch_states_.push_back(st);
    all_states_.push_back(st);
  }
  std::vector<mwx_state*> states(batch_states_.begin(), batch_states_.begin() + run.size());
  std::vector<const float*> ptrs;
  std::vector<int> lens;
  for (size_t b : run) {
    ptrs.push_back(clips[b].data());
    lens.push_back(static_cast<int>(clips[b].size()));
  }
  std::string lang;
  std::function<bool()> abort_fn = options.should_abort;
  BiasKeep bias_keep;  // (the hotword phrases' arrays, alive for the call)
  const mwx_full_params p = make_params(options, lang, abort_fn, bias_keep);
  int ret;
  if (trimmed) {
    TrimList objs(run.size());
    for (size_t i = 0; i < run.size(); ++i) objs.p[i] = trimmed->t;
    ret = full_trimmed(ctx_, chunk_batch(), states.data(), p, objs, trim_index.data(),
                       static_cast<int>(run.size()));
  } else {
    ret = mwx_full_batch(ctx_, states.data(), p, ptrs.data(), lens.data(),
                         static_cast<int>(run.size()));
  }
  if (ret == 0) {
    for (size_t i = 0; i < run.size(); ++i) {
      const size_t b = run[i];
      if (clips[b].size() >= min_samples)
        out[b] = collect(states[i], lang, clips[b].data(), clips[b].size(), options.prosody_opts,
                         nullptr);
    }
  }
  return out;
}

}  // namespace mwx_host
