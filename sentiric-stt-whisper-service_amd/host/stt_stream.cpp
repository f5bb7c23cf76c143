// StreamSession: see stt_stream.h (src/grpc_server.cpp:98-309 semantics).
#include "stt_stream.h"

#include <cstdio>
#include <cstring>

namespace mwx_host {

namespace {

bool is_wav(const uint8_t* p, size_t n) {  // src/utils.h:101-105
  return n >= 12 && std::memcmp(p, "RIFF", 4) == 0 && std::memcmp(p + 8, "WAVE", 4) == 0;
}

void set_affect(StreamEvent& ev, const TranscriptionResult& r, bool detail) {
  const AffectiveTags& a = r.affective;
  ev.gender_proxy = a.gender_proxy;
  ev.emotion_proxy = a.emotion_proxy;
  ev.arousal = a.arousal;
  ev.valence = a.valence;
  if (detail) {
    ev.pitch_mean = a.pitch_mean;
    ev.pitch_std = a.pitch_std;
    ev.energy_mean = a.energy_mean;
    ev.energy_std = a.energy_std;
    ev.spectral_centroid = a.spectral_centroid;
    ev.zero_crossing_rate = a.zero_crossing_rate;
  }
  ev.speaker_vec = a.speaker_vec;
  ev.speaker_id = r.speaker_id;
}

// the finals of the empty-chunk path (src/grpc_server.cpp:150-190)
void push_finals(std::vector<StreamEvent>& out, const std::vector<TranscriptionResult>& results) {
  for (const auto& r : results) {
    if (r.text.empty()) continue;
    StreamEvent ev;
    ev.transcription = r.text;
    ev.is_final = true;
    set_affect(ev, r, true);
    for (const auto& t : r.tokens)
      ev.words.push_back({t.text, (float)t.t0 / 100.0f, (float)t.t1 / 100.0f, t.p});
    out.push_back(std::move(ev));
  }
}

}  // namespace

StreamSession::StreamSession(SttEngine& engine)
    : engine_(engine),
      vad_(engine.vad_stream_open()),
      step_((size_t)engine.get_settings().stream_buffer_samples) {
  gate_from_stream_ = vad_ && engine.stream_vad_active();
  endpoint_ = vad_ && engine.stream_endpoint_active();
}

void StreamSession::drop_vad() {
  std::fprintf(stderr, "Streaming: VAD stream call failed, session continues without it\n");
  vad_.reset();
  gate_from_stream_ = endpoint_ = false;
}

void StreamSession::vad_feed(size_t from) {
  if (!vad_ || from >= buffer_.size()) return;
  std::vector<float> f(buffer_.size() - from);
  for (size_t i = 0; i < f.size(); ++i) f[i] = static_cast<float>(buffer_[from + i]) / 32768.0f;
  if (!engine_.vad_stream_feed(*vad_, f.data(), f.size())) drop_vad();
}

void StreamSession::restart_buffer(size_t keep_from) {
  buffer_.erase(buffer_.begin(), buffer_.begin() + (std::ptrdiff_t)keep_from);
  last_processed_ = 0;
  if (!vad_) return;
  if (!engine_.vad_stream_reset(*vad_)) return drop_vad();
  vad_feed(0);
}

std::vector<TranscriptionResult> StreamSession::transcribe(const std::vector<int16_t>& pcm,
                                                           SttEngine::PerformanceMetrics* perf) {
  const RequestOptions& options = options_;  // default request options (+ set_hotwords)
  if (!gate_from_stream_) return engine_.transcribe_pcm16(pcm, 16000, options, perf);
  // the whole buffer: every probability, the provisional one included; a
  // prefix that ends on a chunk boundary: its whole chunks (rule D6 either way)
  const bool speech = pcm.size() == buffer_.size()
                          ? engine_.vad_stream_speech(*vad_)
                          : engine_.vad_stream_speech(*vad_, (long)(pcm.size() / 512));
  return engine_.transcribe_pcm16_gated(pcm, options, speech, perf);
}

std::vector<StreamEvent> StreamSession::feed(const uint8_t* data, size_t len) {
  std::vector<StreamEvent> out;
  if (len == 0) {          // end of speech: finalize the buffered sentence
    if (!buffer_.empty()) {
      push_finals(out, transcribe(buffer_, nullptr));
      restart_buffer(buffer_.size());
    }
    return out;
  }
  if (first_chunk_) {
    if (is_wav(data, len)) {
      wav_container_ = true;
      if (len > 44) header_skip_ = 44;
    }
    first_chunk_ = false;
  }
  if (wav_container_ && header_skip_ > 0) {
    if (len >= header_skip_) {
      data += header_skip_;
      len -= header_skip_;
      header_skip_ = 0;
    } else {
      header_skip_ -= len;
      len = 0;
    }
  }
  if (len > 0) {
    const size_t samples = len / 2;
    const size_t cur = buffer_.size();
    buffer_.resize(cur + samples);
    std::memcpy(buffer_.data() + cur, data, samples * 2);
    vad_feed(cur);
  }
  // server-side endpointing: a closed speech segment finalizes the buffer up
  // to the end of the chunk that closed it
  while (endpoint_) {
    const int64_t cut = engine_.vad_stream_last_closed_at(*vad_);
    if (cut <= 0 || (size_t)cut > buffer_.size()) break;
    const std::vector<int16_t> head(buffer_.begin(), buffer_.begin() + (std::ptrdiff_t)cut);
    push_finals(out, transcribe(head, nullptr));
    restart_buffer((size_t)cut);
  }
  if (buffer_.size() - last_processed_ >= step_) {
    try {
      SttEngine::PerformanceMetrics perf;
      const auto results = transcribe(buffer_, &perf);
      last_processed_ = buffer_.size();
      StreamEvent partial;
      bool any = false;
      for (const auto& r : results) {
        if (r.text.empty()) continue;
        partial.transcription += r.text + " ";
        set_affect(partial, r, true);  // the last non-empty segment's
        any = true;
      }
      if (any) out.push_back(std::move(partial));
      if (buffer_.size() > kMaxBufferSamples) {  // 30 s without a pause
        for (const auto& r : results) {
          if (r.text.empty()) continue;
          StreamEvent ev;
          ev.transcription = r.text;
          ev.is_final = true;
          set_affect(ev, r, false);
          out.push_back(std::move(ev));
        }
        restart_buffer(buffer_.size());
      }
    } catch (const std::exception& e) {
      std::fprintf(stderr, "Streaming error: %s\n", e.what());
    }
  }
  return out;
}

}  // namespace mwx_host
