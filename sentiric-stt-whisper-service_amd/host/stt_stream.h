// Streaming re-transcription session: the reference's
// per-stream buffer loop of WhisperTranscribeStream (src/grpc_server.cpp:98-309)
// without the gRPC transport, over the GPU SttEngine.
//
// Kept from the reference, chunk by chunk:
//  * the first chunk may carry a WAV container: "RIFF"...."WAVE" at bytes 0-11
//    (src/utils.h:101-105); then 44 header bytes are skipped — only when that
//    first chunk is longer than 44 bytes, as the reference does (:195-212);
//  * chunk bytes are appended as little-endian int16 (an odd trailing byte is
//    dropped, :214-219);
//  * every `stream_buffer_samples` new samples (Settings, default 8000 =
//    0.5 s) the WHOLE buffer is re-transcribed and one partial event carries
//    the non-empty segment texts joined with trailing spaces plus the affect
//    fields and speaker of the last such segment (:222-262);
//  * past 30 s of buffer the segments of that transcription are forced final
//    (text, gender, emotion, arousal, valence, speaker, speaker vector) and the
//    buffer restarts (:264-290); a transcription error on this path is
//    swallowed, as the reference logs it and carries on (:292-295);
//  * an empty chunk is the end-of-speech signal: a non-empty buffer is
//    transcribed once more and every non-empty segment becomes a final event
//    with all affect fields and its words (token text, t0 / 100, t1 / 100, p),
//    then the buffer restarts (:150-190).
//
// Engine extensions, both off by default (the reference has
// neither):
//  * Settings::stream_vad: the session feeds every sample it buffers
//    (s / 32768.0f, as transcribe_pcm16 converts) to a VAD stream of its own,
//    restarted whenever the buffer restarts, and its transcriptions take the
//    gate's decision from it. The events are those of the whole-buffer gate.
//  * Settings::stream_endpoint_silence_ms = S > 0, server-side endpointing:
//    after a chunk whose samples close at least one raw speech segment of the
//    VAD stream (rule D7 with min_silence_duration_ms = S), cut = the last
//    one's closed_at; buffer_[0, cut) is transcribed and its non-empty
//    segments become final events exactly as the empty chunk finalizes them;
//    the buffer becomes buffer_[cut:], the VAD stream restarts and is fed the
//    remainder, and the same test runs again on what that closes. Then the
//    partial cadence test runs on the new buffer.
//
// GPU-side, concurrent sessions of an engine built with Settings::max_batch > 1
// have their re-transcriptions gathered into shared mwx_full_batch calls by
// the engine's request batcher: many live streams, one decode loop.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "stt_engine.h"

namespace mwx_host {

// The fields of one WhisperTranscribeStreamResponse; fields the reference
// leaves unset in a given message keep their protobuf defaults (0 / empty).
struct StreamWord {
  std::string word;
  float start = 0.0f;  // seconds
  float end = 0.0f;
  float probability = 0.0f;
};

struct StreamEvent {
  std::string transcription;
  bool is_final = false;
  std::string gender_proxy;
  std::string emotion_proxy;
  float arousal = 0.0f;
  float valence = 0.0f;
  float pitch_mean = 0.0f;
  float pitch_std = 0.0f;
  float energy_mean = 0.0f;
  float energy_std = 0.0f;
  float spectral_centroid = 0.0f;
  float zero_crossing_rate = 0.0f;
  std::vector<float> speaker_vec;
  std::string speaker_id;
  std::vector<StreamWord> words;
};

class StreamSession {
 public:
  explicit StreamSession(SttEngine& engine);

  // One received audio chunk (bytes as sent by the client); an empty chunk is
  // the end-of-speech signal. Returns the events the reference would write.
  std::vector<StreamEvent> feed(const uint8_t* data, size_t len);

  size_t buffered_samples() const { return buffer_.size(); }

  // The request options of the session's transcriptions (default: none set).
  // The stream path reads the contextual-biasing fields (hotwords,
  // hotword_boost); the rest stay at the reference's stream defaults.
  void set_hotwords(const std::vector<std::string>& hotwords, float hotword_boost = -1.0f) {
    options_.hotwords = hotwords;
    options_.hotword_boost = hotword_boost;
  }

  // ... and the constrained-decoding fields (choices, choice_flags, choice_penalty)
  void set_choices(const std::vector<std::string>& choices, int choice_flags = -1,
                   float choice_penalty = -1.0f) {
    options_.choices = choices;
    if (choice_flags >= 0) options_.choice_flags = choice_flags;
    options_.choice_penalty = choice_penalty;
  }

  static constexpr size_t kMaxBufferSamples = 16000 * 30;  // src/grpc_server.cpp:132

 private:
  // the engine's transcription of `pcm` = buffer_[0, pcm.size()): through the
  // gate decision of the VAD stream when the session has one for that
  std::vector<TranscriptionResult> transcribe(const std::vector<int16_t>& pcm,
                                              SttEngine::PerformanceMetrics* perf);
  void vad_feed(size_t from);    // buffer_[from, end) -> the VAD stream
  void restart_buffer(size_t keep_from);  // buffer_ = buffer_[keep_from:], VAD stream anew
  void drop_vad();               // a failed VAD stream call: the session goes on as without one

  SttEngine& engine_;
  RequestOptions options_;  // default request options (+ set_hotwords)
  std::shared_ptr<VadStreamHandle> vad_;  // Settings::stream_vad / stream_endpoint_silence_ms
  bool gate_from_stream_ = false;
  bool endpoint_ = false;
  std::vector<int16_t> buffer_;
  size_t last_processed_ = 0;
  size_t step_;  // Settings::stream_buffer_samples
  bool first_chunk_ = true;
  bool wav_container_ = false;
  size_t header_skip_ = 0;
};

}  // namespace mwx_host
