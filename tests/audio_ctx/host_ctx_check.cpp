// TEST INFRASTRUCTURE ONLY — Settings::audio_ctx / audio_ctx_fit reach the
// mwx_full_params of every request path of the host SttEngine: transcribe(),
// transcribe_pcm16(), the request batcher (max_batch > 1), vad_trim (single
// and transcribe_batch), and a StreamSession's re-transcriptions; and the C
// shim's setter changes them for the requests after it. Runs over CPU stand-ins
// (tests/audio_ctx/Makefile: AddressSanitizer + UBSan, a stand-alone program),
// started by tests/test_audio_ctx_ref.py.
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "stt_engine.h"
#include "stt_stream.h"

using namespace mwx_host;

extern std::atomic<int> g_ctx_calls, g_ctx_batch_calls, g_ctx_last_audio_ctx, g_ctx_last_fit,
    g_ctx_mismatch, g_ctx_want_audio_ctx, g_ctx_want_fit;
extern "C" int mwx_stt_set_audio_ctx(void* eng, int audio_ctx, int fit);

namespace {

int failures = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

// chunks [a0, a1) are speech for the VAD stand-in (their first sample 0.9)
std::vector<float> clip(int n, int a0, int a1) {
  std::vector<float> x((size_t)n);
  for (int i = 0; i < n; ++i) x[(size_t)i] = 0.001f * (float)((i / 512) % 37);
  for (int i = 0; i * 512 < n; ++i) x[(size_t)i * 512] = i >= a0 && i < a1 ? 0.9f : 0.1f;
  return x;
}

// every decode call from here on must carry (audio_ctx, fit)
void expect(int audio_ctx, bool fit) {
  g_ctx_want_audio_ctx = audio_ctx;
  g_ctx_want_fit = fit ? 1 : 0;
}

void run_paths(const Settings& base, int audio_ctx, bool fit, bool by_setter) {
  Settings s = base;
  if (!by_setter) {
    s.audio_ctx = audio_ctx;
    s.audio_ctx_fit = fit;
  }
  Settings queued = s;
  queued.max_batch = 3;
  queued.parallel_requests = 2;
  Settings trim = s;
  trim.enable_vad = true;
  trim.vad_model_filename = "vad.bin";
  trim.vad_threshold = 0.75f;
  trim.vad_trim = true;
  const auto a = clip(3 * 16000 + 11, 0, 80);
  const auto b = clip(2 * 16000, 5, 40);
  std::vector<int16_t> a16(a.size());
  for (size_t i = 0; i < a.size(); ++i) a16[i] = (int16_t)(a[i] * 32767.0f);
  RequestOptions opt;
  SttEngine plain(s), batched(queued), trimmed(trim);
  if (by_setter) {
    for (SttEngine* e : {&plain, &batched, &trimmed}) {
      CHECK(e->get_settings().audio_ctx == 0 && !e->get_settings().audio_ctx_fit);
      CHECK(mwx_stt_set_audio_ctx(e, 1501, 1) == -1);  // refused: nothing changes
      CHECK(e->get_settings().audio_ctx == 0 && !e->get_settings().audio_ctx_fit);
      CHECK(mwx_stt_set_audio_ctx(e, audio_ctx, fit ? 1 : 0) == 0);
      CHECK(e->get_settings().audio_ctx == audio_ctx && e->get_settings().audio_ctx_fit == fit);
    }
  }
  expect(audio_ctx, fit);
  const int m0 = g_ctx_mismatch;
  int calls = g_ctx_calls + g_ctx_batch_calls;
  auto more_calls = [&] {
    const int now = g_ctx_calls + g_ctx_batch_calls;
    const bool more = now > calls;
    calls = now;
    return more;
  };
  CHECK(!plain.transcribe(a, 16000, opt).empty() && more_calls());
  CHECK(!plain.transcribe_pcm16(a16, 16000, opt).empty() && more_calls());
  CHECK(!batched.transcribe(a, 16000, opt).empty() && more_calls());
  CHECK(batched.batches_run() > 0);
  CHECK(!trimmed.transcribe(a, 16000, opt).empty() && more_calls());
  CHECK(trimmed.transcribe_batch({a, b}, opt).size() == 2 && more_calls());
  CHECK(plain.transcribe_batch({a, b}, opt).size() == 2 && more_calls());
  {
    // a stream: two partial re-transcriptions and the final one
    StreamSession ss(batched);
    std::vector<uint8_t> bytes(a16.size() * 2);
    for (size_t i = 0; i < a16.size(); ++i) {
      bytes[2 * i] = (uint8_t)(a16[i] & 0xff);
      bytes[2 * i + 1] = (uint8_t)((a16[i] >> 8) & 0xff);
    }
    const size_t half = bytes.size() / 4 * 2;
    ss.feed(bytes.data(), half);
    ss.feed(bytes.data() + half, bytes.size() - half);
    ss.feed(nullptr, 0);
    CHECK(more_calls());
  }
  CHECK(g_ctx_mismatch == m0);
  CHECK(g_ctx_last_audio_ctx == audio_ctx && g_ctx_last_fit == (fit ? 1 : 0));
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
  CHECK(Settings().audio_ctx == 0 && !Settings().audio_ctx_fit);  // off by default
  const mwx_full_params dp = mwx_full_default_params(MWX_SAMPLING_GREEDY);
  CHECK(dp.audio_ctx == 0 && !dp.audio_ctx_fit);
  run_paths(base, 0, false, false);
  run_paths(base, 192, false, false);
  run_paths(base, 0, true, false);
  run_paths(base, 100, true, false);
  run_paths(base, 256, true, true);
  run_paths(base, 96, false, true);
  CHECK(mwx_stt_set_audio_ctx(nullptr, 1, 1) == -1);
  std::printf("host_ctx_check: %d failure(s), %d + %d decode calls\n", failures, g_ctx_calls.load(),
              g_ctx_batch_calls.load());
  return failures ? 1 : 0;
}
