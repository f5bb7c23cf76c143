// TEST INFRASTRUCTURE ONLY — the host SttEngine's VAD gate over CPU stand-ins
// (tests/san/mwx_stub.cpp for Whisper, vad_stub.cpp for the VAD), built with
// AddressSanitizer + UBSan (tests/vad/Makefile) and run by
// tests/test_vad_host.py. Checks, from several threads: the gate rule (a
// probability equal to the threshold passes, anything below is held back, a
// failing VAD call leaves the gate open), the fields of the empty result, the
// batched gate, and the open gate after a VAD model that does not load.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "stt_engine.h"

using namespace mwx_host;

extern std::atomic<int> g_vad_single_calls, g_vad_batch_calls, g_vad_overlaps;

namespace {

std::atomic<int> failures{0};
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

// a 2-s clip whose chunk probabilities (vad_stub.cpp) are all `base` except
// chunk `at`, which is `peak`
std::vector<float> clip(float base, int at, float peak, int n = 32000) {
  std::vector<float> x((size_t)n, 0.01f);
  for (int i = 0; i * 512 < n; ++i) x[(size_t)i * 512] = i == at ? peak : base;
  return x;
}

void check_empty(const std::vector<TranscriptionResult>& rs, size_t n) {
  CHECK(rs.size() == 1);
  if (rs.size() != 1) return;
  const TranscriptionResult& r = rs[0];
  CHECK(r.text.empty());
  CHECK(r.language == "unknown");
  CHECK(r.prob == 0.0f);
  CHECK(r.t0 == 0);
  CHECK(r.t1 == (int64_t)(n / 16.0));
  CHECK(!r.speaker_turn_next);
  CHECK(r.tokens.empty());
  CHECK(r.token_count == 0);
  CHECK(r.speaker_id == "unknown");
  CHECK(r.affective.gender_proxy == "?");
  CHECK(r.affective.emotion_proxy == "neutral");
  CHECK(r.affective.speaker_vec.size() == 8);
  for (float v : r.affective.speaker_vec) CHECK(v == 0.0f);
  CHECK(r.affective.pitch_mean == 0.0f && r.affective.energy_mean == 0.0f);
}

bool same(const std::vector<TranscriptionResult>& a, const std::vector<TranscriptionResult>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].text != b[i].text || a[i].t0 != b[i].t0 || a[i].t1 != b[i].t1 ||
        a[i].token_count != b[i].token_count || a[i].language != b[i].language)
      return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ofstream(dir + "/ggml-micro.bin") << "stub";
  std::ofstream(dir + "/vad.bin") << "stub";
  Settings base;
  base.model_dir = dir;
  base.model_filename = "ggml-micro.bin";
  base.parallel_requests = 4;
  base.language = "en";
  base.beam_size = 1;
  Settings with_vad = base;
  with_vad.enable_vad = true;
  with_vad.vad_model_filename = "vad.bin";
  with_vad.vad_threshold = 0.75f;
  Settings missing = with_vad;
  missing.vad_model_filename = "no-such-file.bin";
  CHECK(!Settings().enable_vad);  // off by default
  CHECK(Settings().vad_model_filename == "ggml-silero-vad.bin" && Settings().vad_threshold == 0.75f);

  const float below = std::nextafter(0.75f, 0.0f);
  const auto at_threshold = clip(0.1f, 40, 0.75f);  // one chunk equal to the threshold
  const auto just_below = clip(below, 3, below);    // every chunk a hair below it
  const auto silent = clip(0.0f, 0, 0.0f, 32000 + 137);
  auto failing = clip(0.0f, 0, 0.0f);
  failing[0] = -1.0f;  // the stub's detect_speech returns false
  RequestOptions opt;

  SttEngine plain(base), gated(with_vad), open(missing);
  const auto ref_at = plain.transcribe(at_threshold, 16000, opt);
  const auto ref_below = plain.transcribe(just_below, 16000, opt);
  const auto ref_failing = plain.transcribe(failing, 16000, opt);
  CHECK(!ref_at.empty());
  CHECK(g_vad_single_calls == 0);  // VAD off: never called

  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&] {
      for (int rep = 0; rep < 8; ++rep) {
        SttEngine::PerformanceMetrics m{-1, -1, -1};
        CHECK(same(gated.transcribe(at_threshold, 16000, opt), ref_at));  // p == threshold passes
        check_empty(gated.transcribe(just_below, 16000, opt, &m), just_below.size());
        CHECK(m.queue_time_ms == 0.0 && m.processing_time_ms >= 0.0 && m.token_count == 0);
        check_empty(gated.transcribe(silent, 16000, opt), silent.size());
        CHECK(same(gated.transcribe(failing, 16000, opt), ref_failing));  // failed call: gate open
        CHECK(gated.is_speech_detected(at_threshold.data(), at_threshold.size()));
        CHECK(!gated.is_speech_detected(silent.data(), silent.size()));
        // the model did not load: everything is transcribed
        CHECK(same(open.transcribe(just_below, 16000, opt), ref_below));
        CHECK(open.is_speech_detected(silent.data(), silent.size()));
        // shorter than vad_ms_min_duration: dropped before the gate
        CHECK(gated.transcribe(std::vector<float>(4000, 0.9f), 16000, opt).empty());
      }
    });
  for (auto& t : th) t.join();
  CHECK(g_vad_overlaps == 0);  // the host serialises calls on the VAD context
  CHECK(g_vad_single_calls > 0);

  // batched gate: one VAD pass, silent clips left out of the Whisper batch
  const std::vector<std::vector<float>> clips = {at_threshold, silent, just_below, at_threshold,
                                                 std::vector<float>(4000, 0.9f)};
  const int before = g_vad_batch_calls;
  const auto off_rs = plain.transcribe_batch(clips, opt);
  CHECK(g_vad_batch_calls == before);
  const auto on_rs = gated.transcribe_batch(clips, opt);
  CHECK(g_vad_batch_calls == before + 1);
  CHECK(on_rs.size() == clips.size());
  if (on_rs.size() == clips.size()) {
    CHECK(same(on_rs[0], off_rs[0]) && same(on_rs[3], off_rs[3]));
    check_empty(on_rs[1], clips[1].size());
    check_empty(on_rs[2], clips[2].size());
    CHECK(on_rs[4].empty() && off_rs[4].empty());
  }
  const auto open_rs = open.transcribe_batch(clips, opt);
  CHECK(open_rs.size() == off_rs.size());
  for (size_t b = 0; b < open_rs.size() && b < off_rs.size(); ++b) CHECK(same(open_rs[b], off_rs[b]));
  // every clip silent: no Whisper batch at all
  const auto all_silent = gated.transcribe_batch({silent, just_below}, opt);
  CHECK(all_silent.size() == 2);
  if (all_silent.size() == 2) {
    check_empty(all_silent[0], silent.size());
    check_empty(all_silent[1], just_below.size());
  }

  std::printf("host_vad_check: %d failure(s)\n", failures.load());
  return failures ? 1 : 0;
}
