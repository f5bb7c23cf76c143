// TEST INFRASTRUCTURE ONLY — the host SttEngine's detect_language() /
// detect_language_pcm16() and TranscriptionResult::language_probability over
// the CPU stand-in lang_stub.cpp (tests/lang/Makefile; AddressSanitizer +
// UBSan), run by tests/test_lang_host.py: the list is sorted by probability
// descending, then by language id, and clipped to top_k; the engine call is a
// detection-only one with language "auto"; the minimum-duration gate and the
// resampler apply as in transcribe(); language_probability is the used
// language's probability after "auto" and -1 after a fixed language, on the
// pooled path and through the request batcher; Settings::chunk_language_recording
// reaches mwx_full_params. Built with -DLANG_UNBOUND against the plain
// stand-in (no language-probability calls): detect_language() returns nothing
// and language_probability stays -1.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "stt_engine.h"

using namespace mwx_host;

#ifndef LANG_UNBOUND
extern int g_lang_calls, g_lang_detect_calls;
extern mwx_full_params g_lang_params;
extern std::string g_lang_language;
#endif
extern "C" int mwx_stt_detect_language_pcm16(void* eng, const int16_t* pcm, int n, int sample_rate,
                                             int top_k, char* out, int cap);
extern "C" int mwx_stt_detect_language(void* eng, const float* pcm, int n, int sample_rate,
                                       int top_k, char* out, int cap);
extern "C" int mwx_stt_set_chunk_language_recording(void* eng, int on);

namespace {

int failures = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

Settings base(const std::string& dir) {
  Settings s;
  s.model_dir = dir;
  s.model_filename = "ggml-micro.bin";
  s.parallel_requests = 1;
  s.request_queue_timeout_ms = 1000;
  s.language = "auto";
  s.enable_vad = false;
  return s;
}

typedef std::vector<std::pair<std::string, float>> Langs;
bool same(const Langs& a, const Langs& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].first != b[i].first || a[i].second != b[i].second) return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ofstream(dir + "/ggml-micro.bin") << "stub";
  std::vector<float> pcm(16000 * 4);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = 0.01f * (float)((i / 160) % 23);
  std::vector<float> loud = pcm;
  loud[0] = 0.9f;  // the stand-in's second distribution
  RequestOptions opt;

#ifdef LANG_UNBOUND
  {
    SttEngine e(base(dir));
    CHECK(e.detect_language(pcm, 16000, 3).empty());
    CHECK(e.detect_language_pcm16(std::vector<int16_t>(32000, 100), 16000, 0).empty());
    const auto rs = e.transcribe(pcm, 16000, opt);
    CHECK(!rs.empty());
    for (const auto& r : rs) CHECK(r.language_probability == -1.0f && r.language == "auto");
    char buf[256];
    CHECK(mwx_stt_detect_language(&e, pcm.data(), (int)pcm.size(), 16000, 3, buf, sizeof buf) == 2);
    CHECK(std::string(buf) == "[]");
  }
  std::printf("host_lang_unbound: %d failure(s)\n", failures);
#else
  for (int max_batch : {1, 4}) {
    Settings s = base(dir);
    s.max_batch = max_batch;
    SttEngine e(s);
    // ordering: probability descending, ties by id; {0.1, 0.4, 0.1, 0.4, 0}
    const Langs all = {{"de", 0.4f}, {"fr", 0.4f}, {"en", 0.1f}, {"tr", 0.1f}, {"es", 0.0f}};
    const int calls = g_lang_calls, det = g_lang_detect_calls;
    const Langs top3 = e.detect_language(pcm, 16000, 3);
    CHECK(same(top3, Langs(all.begin(), all.begin() + 3)));
    // one detection-only engine call with language "auto"
    CHECK(g_lang_calls == calls + 1 && g_lang_detect_calls == det + 1);
    CHECK(g_lang_params.detect_language && g_lang_language == "auto");
    CHECK(g_lang_params.lang_ids == nullptr);
    // top_k clipping: < 1 and above the number of languages give all
    CHECK(same(e.detect_language(pcm, 16000, 1), Langs(all.begin(), all.begin() + 1)));
    CHECK(same(e.detect_language(pcm, 16000, 5), all));
    CHECK(same(e.detect_language(pcm, 16000, 0), all));
    CHECK(same(e.detect_language(pcm, 16000, -7), all));
    CHECK(same(e.detect_language(pcm, 16000, 99), all));
    const Langs b = e.detect_language(loud, 16000, 2);
    CHECK(same(b, Langs{{"tr", 0.7f}, {"fr", 0.2f}}));
    // the pcm16 twin converts as transcribe_pcm16 does
    std::vector<int16_t> p16(pcm.size());
    for (size_t i = 0; i < pcm.size(); ++i) p16[i] = (int16_t)(pcm[i] * 32768.0f);
    CHECK(same(e.detect_language_pcm16(p16, 16000, 3), top3));
    // minimum duration as transcribe(): too short gives nothing and no engine call
    const int calls2 = g_lang_calls;
    const size_t min_samples = (size_t)e.get_settings().vad_ms_min_duration * 16;
    if (min_samples > 0) {
      CHECK(e.detect_language(std::vector<float>(min_samples - 1, 0.1f), 16000, 3).empty());
      CHECK(g_lang_calls == calls2);
    }
    CHECK(e.detect_language(std::vector<float>(), 16000, 3).empty() || min_samples == 0);
    // resampled input reaches the engine
    CHECK(e.detect_language(std::vector<float>(32000, 0.1f), 8000, 2).size() == 2);
    CHECK(e.detect_language(std::vector<float>(4 * 44100, 0.1f), 44100, 0).size() == 5);

    // language_probability: the used language's probability after "auto"
    auto rs = e.transcribe(pcm, 16000, opt);
    CHECK(!rs.empty());
    for (const auto& r : rs) CHECK(r.language_probability == 0.4f && r.language == "auto");
    rs = e.transcribe(loud, 16000, opt);
    CHECK(!rs.empty());
    for (const auto& r : rs) CHECK(r.language_probability == 0.7f);
    // ... and -1 after a fixed language
    RequestOptions fixed;
    fixed.language = "tr";
    rs = e.transcribe(pcm, 16000, fixed);
    CHECK(!rs.empty());
    for (const auto& r : rs) CHECK(r.language_probability == -1.0f && r.language == "tr");
    CHECK(!g_lang_params.detect_language && g_lang_params.chunk_language == MWX_CHUNK_LANG_PER_CHUNK);
    // a detection between two transcriptions leaves no trace in the next one
    (void)e.detect_language(pcm, 16000, 1);
    rs = e.transcribe(pcm, 16000, fixed);
    for (const auto& r : rs) CHECK(r.language_probability == -1.0f);
    if (max_batch == 1) {
      const auto rb = e.transcribe_batch({pcm, loud}, opt);
      CHECK(rb.size() == 2 && !rb[0].empty() && !rb[1].empty());
      if (rb.size() == 2) {
        for (const auto& r : rb[0]) CHECK(r.language_probability == 0.4f);
        for (const auto& r : rb[1]) CHECK(r.language_probability == 0.7f);
      }
    }
    // Settings::chunk_language_recording reaches the engine's parameters
    CHECK(mwx_stt_set_chunk_language_recording(&e, 1) == 0);
    (void)e.transcribe(pcm, 16000, opt);
    CHECK(g_lang_params.chunk_language == MWX_CHUNK_LANG_RECORDING);
    CHECK(mwx_stt_set_chunk_language_recording(&e, 0) == 0);
    (void)e.transcribe(pcm, 16000, opt);
    CHECK(g_lang_params.chunk_language == MWX_CHUNK_LANG_PER_CHUNK);
    CHECK(mwx_stt_set_chunk_language_recording(nullptr, 1) == -1);

    // the C glue: JSON out, hex strings, f32 bit patterns (0.4f = 1053609165)
    char buf[512];
    const int n = mwx_stt_detect_language_pcm16(&e, p16.data(), (int)p16.size(), 16000, 2, buf,
                                                sizeof buf);
    CHECK(n > 0 && (int)std::strlen(buf) == n);
    CHECK(std::string(buf) == "[{\"language\":\"6465\",\"p\":1053609165},"
                              "{\"language\":\"6672\",\"p\":1053609165}]");
    CHECK(mwx_stt_detect_language(&e, pcm.data(), (int)pcm.size(), 16000, 5, buf, 8) < -2);
    CHECK(mwx_stt_detect_language(nullptr, pcm.data(), 4, 16000, 5, buf, 8) == -1);
  }
  std::printf("host_lang_check: %d failure(s)\n", failures);
#endif
  return failures ? 1 : 0;
}
