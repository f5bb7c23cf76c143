// Plain-C entry points over mwx_host::SttEngine for the Python tests (ctypes).
// Results are returned as JSON with every string hex-encoded (token text may
// be a partial UTF-8 sequence).
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "stt_engine.h"
#include "stt_stream.h"
#include "text_filters.h"

using namespace mwx_host;

namespace {

std::string hex(const std::string& s) {
  static const char* d = "0123456789abcdef";
  std::string o;
  o.reserve(s.size() * 2);
  for (unsigned char c : s) {
    o.push_back(d[c >> 4]);
    o.push_back(d[c & 15]);
  }
  return o;
}

std::string to_json(const std::vector<TranscriptionResult>& rs) {
  std::string o = "[";
  char buf[1024];
  for (size_t i = 0; i < rs.size(); ++i) {
    const TranscriptionResult& r = rs[i];
    std::snprintf(buf, sizeof buf, "%s{\"prob\":%.9g,\"t0\":%lld,\"t1\":%lld,\"turn\":%d,\"n\":%d,",
                  i ? "," : "", r.prob, (long long)r.t0, (long long)r.t1, (int)r.speaker_turn_next,
                  r.token_count);
    o += buf;
    o += "\"text\":\"" + hex(r.text) + "\",\"language\":\"" + hex(r.language) + "\",";
    std::snprintf(buf, sizeof buf, "\"language_probability\":%.9g,", r.language_probability);
    o += buf;
    const AffectiveTags& a = r.affective;
    std::snprintf(buf, sizeof buf,
                  "\"gender\":\"%s\",\"emotion\":\"%s\",\"speaker\":\"%s\",\"arousal\":%.9g,"
                  "\"valence\":%.9g,\"pitch_mean\":%.9g,\"pitch_std\":%.9g,\"energy_mean\":%.9g,"
                  "\"energy_std\":%.9g,\"spectral_centroid\":%.9g,\"zero_crossing_rate\":%.9g,",
                  r.gender_proxy.c_str(), r.emotion_proxy.c_str(), r.speaker_id.c_str(), r.arousal,
                  r.valence, a.pitch_mean, a.pitch_std, a.energy_mean, a.energy_std,
                  a.spectral_centroid, a.zero_crossing_rate);
    o += buf;
    o += "\"speaker_vec\":[";
    for (size_t j = 0; j < a.speaker_vec.size(); ++j) {
      std::snprintf(buf, sizeof buf, "%s%.9g", j ? "," : "", a.speaker_vec[j]);
      o += buf;
    }
    o += "],\"tokens\":[";
    for (size_t j = 0; j < r.tokens.size(); ++j) {
      const TokenData& t = r.tokens[j];
      std::snprintf(buf, sizeof buf, "%s{\"p\":%.9g,\"t0\":%lld,\"t1\":%lld,\"text\":\"", j ? "," : "",
                    t.p, (long long)t.t0, (long long)t.t1);
      o += buf;
      o += hex(t.text) + "\"}";
    }
    o += "]}";
  }
  return o + "]";
}

// AlignmentResult: floats as their f32 bit patterns (a log-probability may be
// -inf, which JSON cannot carry)
unsigned f32_bits(float v) {
  unsigned u;
  std::memcpy(&u, &v, 4);
  return u;
}
std::string to_json(const AlignmentResult& r) {
  char buf[256];
  std::snprintf(buf, sizeof buf, "{\"ok\":%d,\"avg_logprob\":%u,\"eot_logprob\":%u,\"n_agree\":%d,",
                (int)r.ok, f32_bits(r.avg_logprob), f32_bits(r.eot_logprob), r.n_agree);
  std::string o = buf;
  o += "\"text\":\"" + hex(r.text) + "\",\"language\":\"" + hex(r.language) + "\",\"tokens\":[";
  for (size_t j = 0; j < r.tokens.size(); ++j) {
    const AlignedToken& t = r.tokens[j];
    std::snprintf(buf, sizeof buf, "%s{\"id\":%d,\"p\":%u,\"plog\":%u,\"t\":%lld,\"top_id\":%d,"
                  "\"top_plog\":%u,\"text\":\"", j ? "," : "", t.id, f32_bits(t.p), f32_bits(t.plog),
                  (long long)t.t, t.top_id, f32_bits(t.top_plog));
    o += buf;
    o += hex(t.text) + "\",\"top_text\":\"" + hex(t.top_text) + "\"}";
  }
  return o + "]}";
}

int emit(const std::string& s, char* out, int cap) {
  if ((int)s.size() + 1 > cap) return -(int)(s.size() + 1);
  std::memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

}  // namespace

extern "C" {

int mwx_stt_is_hallucination(const char* text) { return is_hallucination(text ? text : "") ? 1 : 0; }

void* mwx_stt_new(const char* model_dir, const char* model_filename, int parallel_requests,
                  int queue_timeout_ms, int beam_size, const char* language, int vad_ms_min,
                  int gpu_device) {
  Settings s;
  s.model_dir = model_dir;
  s.model_filename = model_filename;
  s.parallel_requests = parallel_requests;
  s.request_queue_timeout_ms = queue_timeout_ms;
  s.beam_size = beam_size;
  s.language = language;
  s.vad_ms_min_duration = vad_ms_min;
  s.gpu_device = gpu_device;
  try {
    settings_dtw_from_env(s);
    settings_hotwords_from_env(s);
    settings_choices_from_env(s);
    return new SttEngine(s);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "SttEngine: %s\n", e.what());
    return nullptr;
  }
}

// As mwx_stt_new, with dynamic request batching (Settings::max_batch /
// batch_window_us).
void* mwx_stt_new_batched(const char* model_dir, const char* model_filename,
                          int parallel_requests, int queue_timeout_ms, int beam_size,
                          const char* language, int vad_ms_min, int gpu_device, int max_batch,
                          int batch_window_us) {
  Settings s;
  s.model_dir = model_dir;
  s.model_filename = model_filename;
  s.parallel_requests = parallel_requests;
  s.request_queue_timeout_ms = queue_timeout_ms;
  s.beam_size = beam_size;
  s.language = language;
  s.vad_ms_min_duration = vad_ms_min;
  s.gpu_device = gpu_device;
  s.max_batch = max_batch;
  s.batch_window_us = batch_window_us;
  try {
    settings_dtw_from_env(s);
    settings_hotwords_from_env(s);
    settings_choices_from_env(s);
    return new SttEngine(s);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "SttEngine: %s\n", e.what());
    return nullptr;
  }
}

// SpeakerClusterer over n 8-D vectors in order: writes the ids, one per line.
int mwx_stt_cluster_ids(const float* vecs, int n, float threshold, char* out, int cap) {
  SpeakerClusterer c(threshold);
  std::string o;
  for (int i = 0; i < n; ++i)
    o += c.assign_or_add(std::vector<float>(vecs + 8 * i, vecs + 8 * i + 8)) + "\n";
  return emit(o, out, cap);
}

// As mwx_stt_new_batched, with Settings::stream_buffer_samples.
void* mwx_stt_new_ex(const char* model_dir, const char* model_filename, int parallel_requests,
                     int queue_timeout_ms, int beam_size, const char* language, int vad_ms_min,
                     int gpu_device, int max_batch, int batch_window_us,
                     int stream_buffer_samples) {
  Settings s;
  s.model_dir = model_dir;
  s.model_filename = model_filename;
  s.parallel_requests = parallel_requests;
  s.request_queue_timeout_ms = queue_timeout_ms;
  s.beam_size = beam_size;
  s.language = language;
  s.vad_ms_min_duration = vad_ms_min;
  s.gpu_device = gpu_device;
  s.max_batch = max_batch;
  s.batch_window_us = batch_window_us;
  s.stream_buffer_samples = stream_buffer_samples;
  try {
    settings_dtw_from_env(s);
    settings_hotwords_from_env(s);
    settings_choices_from_env(s);
    return new SttEngine(s);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "SttEngine: %s\n", e.what());
    return nullptr;
  }
}

// As mwx_stt_new_ex, with the VAD speech gate (Settings::enable_vad,
// vad_model_filename under model_dir, vad_threshold).
void* mwx_stt_new_vad(const char* model_dir, const char* model_filename, int parallel_requests,
                      int queue_timeout_ms, int beam_size, const char* language, int vad_ms_min,
                      int gpu_device, int max_batch, int batch_window_us,
                      int stream_buffer_samples, int enable_vad, const char* vad_model_filename,
                      float vad_threshold) {
  Settings s;
  s.model_dir = model_dir;
  s.model_filename = model_filename;
  s.parallel_requests = parallel_requests;
  s.request_queue_timeout_ms = queue_timeout_ms;
  s.beam_size = beam_size;
  s.language = language;
  s.vad_ms_min_duration = vad_ms_min;
  s.gpu_device = gpu_device;
  s.max_batch = max_batch;
  s.batch_window_us = batch_window_us;
  s.stream_buffer_samples = stream_buffer_samples;
  s.enable_vad = enable_vad != 0;
  if (vad_model_filename) s.vad_model_filename = vad_model_filename;
  s.vad_threshold = vad_threshold;
  try {
    settings_dtw_from_env(s);
    settings_hotwords_from_env(s);
    settings_choices_from_env(s);
    return new SttEngine(s);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "SttEngine: %s\n", e.what());
    return nullptr;
  }
}

// As mwx_stt_new_vad, with silence trimming (Settings::vad_trim).
void* mwx_stt_new_vad_trim(const char* model_dir, const char* model_filename,
                           int parallel_requests, int queue_timeout_ms, int beam_size,
                           const char* language, int vad_ms_min, int gpu_device, int max_batch,
                           int batch_window_us, int stream_buffer_samples, int enable_vad,
                           const char* vad_model_filename, float vad_threshold, int vad_trim) {
  Settings s;
  s.model_dir = model_dir;
  s.model_filename = model_filename;
  s.parallel_requests = parallel_requests;
  s.request_queue_timeout_ms = queue_timeout_ms;
  s.beam_size = beam_size;
  s.language = language;
  s.vad_ms_min_duration = vad_ms_min;
  s.gpu_device = gpu_device;
  s.max_batch = max_batch;
  s.batch_window_us = batch_window_us;
  s.stream_buffer_samples = stream_buffer_samples;
  s.enable_vad = enable_vad != 0;
  if (vad_model_filename) s.vad_model_filename = vad_model_filename;
  s.vad_threshold = vad_threshold;
  s.vad_trim = vad_trim != 0;
  try {
    settings_dtw_from_env(s);
    settings_hotwords_from_env(s);
    settings_choices_from_env(s);
    return new SttEngine(s);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "SttEngine: %s\n", e.what());
    return nullptr;
  }
}

// As mwx_stt_new_vad_trim, with the streaming-VAD settings of the sessions
// (Settings::stream_vad, stream_endpoint_silence_ms).
void* mwx_stt_new_stream_vad(const char* model_dir, const char* model_filename,
                             int parallel_requests, int queue_timeout_ms, int beam_size,
                             const char* language, int vad_ms_min, int gpu_device, int max_batch,
                             int batch_window_us, int stream_buffer_samples, int enable_vad,
                             const char* vad_model_filename, float vad_threshold, int vad_trim,
                             int stream_vad, int stream_endpoint_silence_ms) {
  Settings s;
  s.model_dir = model_dir;
  s.model_filename = model_filename;
  s.parallel_requests = parallel_requests;
  s.request_queue_timeout_ms = queue_timeout_ms;
  s.beam_size = beam_size;
  s.language = language;
  s.vad_ms_min_duration = vad_ms_min;
  s.gpu_device = gpu_device;
  s.max_batch = max_batch;
  s.batch_window_us = batch_window_us;
  s.stream_buffer_samples = stream_buffer_samples;
  s.enable_vad = enable_vad != 0;
  if (vad_model_filename) s.vad_model_filename = vad_model_filename;
  s.vad_threshold = vad_threshold;
  s.vad_trim = vad_trim != 0;
  s.stream_vad = stream_vad != 0;
  s.stream_endpoint_silence_ms = stream_endpoint_silence_ms;
  try {
    settings_dtw_from_env(s);
    settings_hotwords_from_env(s);
    settings_choices_from_env(s);
    return new SttEngine(s);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "SttEngine: %s\n", e.what());
    return nullptr;
  }
}

// Clips that went through the whole-buffer VAD gate so far.
long mwx_stt_vad_gate_runs(void* eng) { return static_cast<SttEngine*>(eng)->vad_gate_runs(); }

// Bit 0: the engine's sessions take the gate decision from a VAD stream
// (stream_vad active); bit 1: they endpoint (stream_endpoint_silence_ms active).
int mwx_stt_stream_vad_active(void* eng) {
  SttEngine* e = static_cast<SttEngine*>(eng);
  return (e->stream_vad_active() ? 1 : 0) | (e->stream_endpoint_active() ? 2 : 0);
}

// SttEngine::transcribe_batch over n_clips f32 clips at 16 kHz: a JSON list
// with one result list per clip (as mwx_stt_transcribe_pcm16 writes one).
// Return codes as mwx_stt_transcribe_pcm16.
int mwx_stt_transcribe_batch_f32(void* eng, const float* const* pcm, const int* n, int n_clips,
                                 const char* language, int beam_size, float temperature, char* out,
                                 int cap) {
  RequestOptions o;
  o.language = language ? language : "";
  o.beam_size = beam_size;
  o.temperature = temperature;
  try {
    std::vector<std::vector<float>> clips;
    for (int b = 0; b < n_clips; ++b) clips.emplace_back(pcm[b], pcm[b] + n[b]);
    const auto rs = static_cast<SttEngine*>(eng)->transcribe_batch(clips, o);
    std::string j = "[";
    for (size_t b = 0; b < rs.size(); ++b) j += (b ? "," : "") + to_json(rs[b]);
    j += "]";
    const int r = emit(j, out, cap);
    return r < -1 ? r - 2 : r;
  } catch (const EngineBusyException&) {
    return -2;
  } catch (...) {
    return -1;
  }
}

// SttEngine::align_pcm16 / align: one AlignmentResult as JSON (strings
// hex-encoded, floats as f32 bit patterns). Return codes as
// mwx_stt_transcribe_pcm16.
int mwx_stt_align_pcm16(void* eng, const int16_t* pcm, int n, int sample_rate, const char* text,
                        const char* language, int translate, char* out, int cap) {
  RequestOptions o;
  o.language = language ? language : "";
  o.translate = translate != 0;
  try {
    const AlignmentResult r = static_cast<SttEngine*>(eng)->align_pcm16(
        std::vector<int16_t>(pcm, pcm + n), sample_rate, text ? text : "", o);
    const int rc = emit(to_json(r), out, cap);
    return rc < -1 ? rc - 2 : rc;
  } catch (const EngineBusyException&) {
    return -2;
  } catch (...) {
    return -1;
  }
}

// SttEngine::align_batch over n_clips f32 clips at 16 kHz and their texts: a
// JSON list with one AlignmentResult per clip.
int mwx_stt_align_batch_f32(void* eng, const float* const* pcm, const int* n,
                            const char* const* texts, int n_clips, const char* language,
                            int translate, char* out, int cap) {
  RequestOptions o;
  o.language = language ? language : "";
  o.translate = translate != 0;
  try {
    std::vector<std::vector<float>> clips;
    std::vector<std::string> tx;
    for (int b = 0; b < n_clips; ++b) {
      clips.emplace_back(pcm[b], pcm[b] + n[b]);
      tx.emplace_back(texts[b] ? texts[b] : "");
    }
    const auto rs = static_cast<SttEngine*>(eng)->align_batch(clips, tx, o);
    std::string j = "[";
    for (size_t b = 0; b < rs.size(); ++b) j += (b ? "," : "") + to_json(rs[b]);
    j += "]";
    const int rc = emit(j, out, cap);
    return rc < -1 ? rc - 2 : rc;
  } catch (const EngineBusyException&) {
    return -2;
  } catch (...) {
    return -1;
  }
}

// StreamSession over an engine: feed one chunk (len 0 = end of speech);
// returns the events as JSON (strings hex-encoded) like mwx_stt_transcribe_pcm16.
// If `cap` is too small the chunk is still consumed: the events are kept and
// -(needed + 2) is returned; mwx_stt_stream_drain then delivers them (never
// feed the chunk again). While such events are undelivered, a feed returns
// -3 (MWX_STT_PENDING) WITHOUT consuming its chunk: drain, then feed the same
// chunk again. -1 = error, -2 = EngineBusyException.
struct StreamHandle {
  explicit StreamHandle(SttEngine& e) : session(e) {}
  StreamSession session;
  std::string pending;  // undelivered events JSON
};
void* mwx_stt_stream_new(void* eng) { return new StreamHandle(*static_cast<SttEngine*>(eng)); }
void mwx_stt_stream_free(void* s) { delete static_cast<StreamHandle*>(s); }

int mwx_stt_stream_drain(void* s, char* out, int cap) {
  StreamHandle* h = static_cast<StreamHandle*>(s);
  const int r = emit(h->pending.empty() ? std::string("[]") : h->pending, out, cap);
  if (r >= 0) h->pending.clear();
  return r < -1 ? r - 2 : r;
}

int mwx_stt_stream_feed(void* s, const uint8_t* data, int len, char* out, int cap) {
  StreamHandle* h = static_cast<StreamHandle*>(s);
  if (!h->pending.empty()) return -3;  // MWX_STT_PENDING: drain first, chunk not consumed
  try {
    const auto evs = h->session.feed(data, len > 0 ? (size_t)len : 0);
    std::string o = "[";
    char buf[512];
    for (size_t i = 0; i < evs.size(); ++i) {
      const StreamEvent& e = evs[i];
      std::snprintf(buf, sizeof buf,
                    "%s{\"final\":%d,\"arousal\":%.9g,\"valence\":%.9g,\"pitch_mean\":%.9g,"
                    "\"pitch_std\":%.9g,\"energy_mean\":%.9g,\"energy_std\":%.9g,"
                    "\"spectral_centroid\":%.9g,\"zero_crossing_rate\":%.9g,",
                    i ? "," : "", (int)e.is_final, e.arousal, e.valence, e.pitch_mean, e.pitch_std,
                    e.energy_mean, e.energy_std, e.spectral_centroid, e.zero_crossing_rate);
      o += buf;
      o += "\"text\":\"" + hex(e.transcription) + "\",\"gender\":\"" + e.gender_proxy +
           "\",\"emotion\":\"" + e.emotion_proxy + "\",\"speaker\":\"" + e.speaker_id +
           "\",\"speaker_vec\":[";
      for (size_t j = 0; j < e.speaker_vec.size(); ++j) {
        std::snprintf(buf, sizeof buf, "%s%.9g", j ? "," : "", e.speaker_vec[j]);
        o += buf;
      }
      o += "],\"words\":[";
      for (size_t j = 0; j < e.words.size(); ++j) {
        const StreamWord& w = e.words[j];
        std::snprintf(buf, sizeof buf, "%s{\"start\":%.9g,\"end\":%.9g,\"p\":%.9g,\"word\":\"",
                      j ? "," : "", w.start, w.end, w.probability);
        o += buf;
        o += hex(w.word) + "\"}";
      }
      o += "]}";
    }
    o += "]";
    const int r = emit(o, out, cap);
    if (r < -1) h->pending = o;
    return r < -1 ? r - 2 : r;
  } catch (const EngineBusyException&) {
    return -2;
  } catch (...) {
    return -1;
  }
}

long mwx_stt_batches(void* eng) { return static_cast<SttEngine*>(eng)->batches_run(); }

void mwx_stt_free(void* eng) { delete static_cast<SttEngine*>(eng); }

// Settings::audio_ctx / audio_ctx_fit of the requests that start after the
// call, on every request path of the engine. 0; -1 without an engine or for
// an audio_ctx above 1500 frames (nothing changes).
int mwx_stt_set_audio_ctx(void* eng, int audio_ctx, int fit) {
  if (!eng) return -1;
  return static_cast<SttEngine*>(eng)->set_audio_ctx(audio_ctx, fit != 0) ? 0 : -1;
}

// Settings::vad_chunk_s / vad_chunk_batch (chunked long-form transcription,
// DESIGN.md D10) of the requests that start after the call. chunk_s = 0 switches
// it off. 1 = chunking now runs, 0 = set but inactive (vad_trim is not active,
// or the library lacks the calls: the path stays vad_trim's); -1 without an
// engine, for a chunk_s outside [1, 30] or a chunk_batch < 1 (nothing changes).
int mwx_stt_set_vad_chunk(void* eng, float chunk_s, int chunk_batch) {
  if (!eng) return -1;
  SttEngine* e = static_cast<SttEngine*>(eng);
  if (!e->set_vad_chunk(chunk_s, chunk_batch)) return -1;
  return e->chunk_active() ? 1 : 0;
}

// Settings::chunk_language_recording (one language per recording on the
// chunked path) of the requests that start after the call. 0;
// -1 without an engine.
int mwx_stt_set_chunk_language_recording(void* eng, int on) {
  if (!eng) return -1;
  static_cast<SttEngine*>(eng)->set_chunk_language_recording(on != 0);
  return 0;
}

// SttEngine::detect_language_pcm16 / detect_language: a JSON list of
// {"language": hex, "p": f32 bits}, best first. Return codes as
// mwx_stt_transcribe_pcm16.
static int detect_any(void* eng, const float* f, const int16_t* s, int n, int sample_rate,
                      int top_k, char* out, int cap) {
  try {
    SttEngine* e = static_cast<SttEngine*>(eng);
    const auto r = f ? e->detect_language(std::vector<float>(f, f + n), sample_rate, top_k)
                     : e->detect_language_pcm16(std::vector<int16_t>(s, s + n), sample_rate, top_k);
    std::string j = "[";
    char buf[64];
    for (size_t i = 0; i < r.size(); ++i) {
      std::snprintf(buf, sizeof buf, "\",\"p\":%u}", f32_bits(r[i].second));
      j += std::string(i ? "," : "") + "{\"language\":\"" + hex(r[i].first) + buf;
    }
    j += "]";
    const int rc = emit(j, out, cap);
    return rc < -1 ? rc - 2 : rc;
  } catch (const EngineBusyException&) {
    return -2;
  } catch (...) {
    return -1;
  }
}
int mwx_stt_detect_language(void* eng, const float* pcm, int n, int sample_rate, int top_k,
                            char* out, int cap) {
  if (!eng || !pcm || n < 0) return -1;
  return detect_any(eng, pcm, nullptr, n, sample_rate, top_k, out, cap);
}
int mwx_stt_detect_language_pcm16(void* eng, const int16_t* pcm, int n, int sample_rate, int top_k,
                                  char* out, int cap) {
  if (!eng || !pcm || n < 0) return -1;
  return detect_any(eng, nullptr, pcm, n, sample_rate, top_k, out, cap);
}

// 0.. = JSON length written; -1 = error; -2 = EngineBusyException;
// < -2 = -(needed capacity). abort_after >= 0: RequestOptions::should_abort
// answers true from its (abort_after + 1)-th call on (the service's abort
// hook, src/stt_engine.cpp:17-23,215-219); < 0: no abort callback.
static int transcribe_any(void* eng, const int16_t* pcm16, const float* pcmf, int n,
                          int sample_rate, const char* language, int beam_size, float temperature,
                          char* out, int cap, double* metrics3, int abort_after, int* abort_calls);

int mwx_stt_transcribe_pcm16_ex(void* eng, const int16_t* pcm, int n, int sample_rate,
                                const char* language, int beam_size, float temperature, char* out,
                                int cap, double* metrics3, int abort_after, int* abort_calls) {
  return transcribe_any(eng, pcm, nullptr, n, sample_rate, language, beam_size, temperature, out,
                        cap, metrics3, abort_after, abort_calls);
}

// As mwx_stt_transcribe_pcm16_ex over f32 PCM (SttEngine::transcribe).
int mwx_stt_transcribe_f32_ex(void* eng, const float* pcm, int n, int sample_rate,
                              const char* language, int beam_size, float temperature, char* out,
                              int cap, double* metrics3, int abort_after, int* abort_calls) {
  return transcribe_any(eng, nullptr, pcm, n, sample_rate, language, beam_size, temperature, out,
                        cap, metrics3, abort_after, abort_calls);
}

static int transcribe_any(void* eng, const int16_t* pcm16, const float* pcmf, int n,
                          int sample_rate, const char* language, int beam_size, float temperature,
                          char* out, int cap, double* metrics3, int abort_after, int* abort_calls) {
  RequestOptions o;
  o.language = language ? language : "";
  o.beam_size = beam_size;
  o.temperature = temperature;
  auto calls = std::make_shared<int>(0);
  if (abort_after >= 0)
    o.should_abort = [calls, abort_after] { return (*calls)++ >= abort_after; };
  SttEngine::PerformanceMetrics m{0, 0, 0};
  try {
    SttEngine* e = static_cast<SttEngine*>(eng);
    const auto rs = pcm16 ? e->transcribe_pcm16(std::vector<int16_t>(pcm16, pcm16 + n), sample_rate, o, &m)
                          : e->transcribe(std::vector<float>(pcmf, pcmf + n), sample_rate, o, &m);
    if (metrics3) {
      metrics3[0] = m.queue_time_ms;
      metrics3[1] = m.processing_time_ms;
      metrics3[2] = m.token_count;
    }
    if (abort_calls) *abort_calls = *calls;
    const int r = emit(to_json(rs), out, cap);
    return r < -1 ? r - 2 : r;
  } catch (const EngineBusyException&) {
    return -2;
  } catch (...) {
    return -1;
  }
}

// SttEngine::transcribe over f32 PCM with RequestOptions::choices (constrained
// decoding; choice_flags < 0 and choice_penalty < 0 keep the defaults):
// {"choice_match": k, "results": [...]} with the results as
// mwx_stt_transcribe_pcm16 writes them and k the results' choice_match (-1
// when there is no result to carry it). Return codes as
// mwx_stt_transcribe_pcm16.
int mwx_stt_transcribe_choices_f32(void* eng, const float* pcm, int n, int sample_rate,
                                   const char* const* choices, int n_choices, int choice_flags,
                                   float choice_penalty, const char* language, int beam_size,
                                   float temperature, char* out, int cap) {
  RequestOptions o;
  o.language = language ? language : "";
  o.beam_size = beam_size;
  o.temperature = temperature;
  for (int i = 0; i < n_choices && choices; ++i) o.choices.emplace_back(choices[i] ? choices[i] : "");
  if (choice_flags >= 0) o.choice_flags = choice_flags;
  o.choice_penalty = choice_penalty;
  try {
    const auto rs = static_cast<SttEngine*>(eng)->transcribe(std::vector<float>(pcm, pcm + n),
                                                             sample_rate, o);
    const int match = rs.empty() ? -1 : rs[0].choice_match;
    const int r = emit("{\"choice_match\":" + std::to_string(match) + ",\"results\":" +
                           to_json(rs) + "}", out, cap);
    return r < -1 ? r - 2 : r;
  } catch (const EngineBusyException&) {
    return -2;
  } catch (...) {
    return -1;
  }
}

int mwx_stt_transcribe_pcm16(void* eng, const int16_t* pcm, int n, int sample_rate,
                             const char* language, int beam_size, float temperature, char* out,
                             int cap, double* metrics3) {
  RequestOptions o;
  o.language = language ? language : "";
  o.beam_size = beam_size;
  o.temperature = temperature;
  SttEngine::PerformanceMetrics m{0, 0, 0};
  try {
    const auto rs = static_cast<SttEngine*>(eng)->transcribe_pcm16(
        std::vector<int16_t>(pcm, pcm + n), sample_rate, o, &m);
    if (metrics3) {
      metrics3[0] = m.queue_time_ms;
      metrics3[1] = m.processing_time_ms;
      metrics3[2] = m.token_count;
    }
    const int r = emit(to_json(rs), out, cap);
    return r < -1 ? r - 2 : r;
  } catch (const EngineBusyException&) {
    return -2;
  } catch (...) {
    return -1;
  }
}

}  // extern "C"
