// TEST INFRASTRUCTURE ONLY — the host SttEngine's contextual biasing
// (RequestOptions::hotwords / hotword_boost, Settings::hotword_boost) over the
// CPU stand-in bias_stub.cpp (tests/bias/Makefile; AddressSanitizer + UBSan),
// run by tests/test_bias_host.py: two phrases per hotword (" word", "word")
// through mwx_tokenize, the boost's resolution order (request, then setting,
// then the environment's default of 0), dropped hotwords, the batching key
// (unchanged without hotwords, different with them), nothing passed when the
// boost resolves to 0, the request batcher and a streaming session.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "stt_engine.h"
#include "stt_stream.h"

using namespace mwx_host;

struct BiasSeen {
  std::vector<mwx_token> ids;
  float boost;
};
extern int g_bias_calls, g_bias_clips;
extern bool g_bias_null;
extern std::vector<BiasSeen> g_bias_seen;

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
  s.language = "en";
  s.enable_vad = false;
  return s;
}

std::vector<mwx_token> bytes(const std::string& s) {
  std::vector<mwx_token> v;
  for (char c : s) v.push_back((unsigned char)c);
  return v;
}

// the last call carried exactly " w", "w" for every word, all at `boost`
bool saw(const std::vector<std::string>& words, float boost) {
  if (g_bias_seen.size() != 2 * words.size() || g_bias_null != words.empty()) return false;
  for (size_t i = 0; i < words.size(); ++i) {
    if (g_bias_seen[2 * i].ids != bytes(" " + words[i]) || g_bias_seen[2 * i].boost != boost)
      return false;
    if (g_bias_seen[2 * i + 1].ids != bytes(words[i]) || g_bias_seen[2 * i + 1].boost != boost)
      return false;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ofstream(dir + "/ggml-micro.bin") << "stub";
  std::vector<float> pcm(16000 * 4);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = 0.01f * (float)((i / 160) % 23);

  // the environment: unset leaves 0 (off); a number sets it; junk is ignored
  {
    unsetenv("STT_WHISPER_SERVICE_HOTWORD_BOOST");
    Settings s;
    CHECK(s.hotword_boost == 0.0f);
    settings_hotwords_from_env(s);
    CHECK(s.hotword_boost == 0.0f);
    setenv("STT_WHISPER_SERVICE_HOTWORD_BOOST", "2.5", 1);
    settings_hotwords_from_env(s);
    CHECK(s.hotword_boost == 2.5f);
    for (const char* junk : {"abc", "-1", "nan", "inf", ""}) {
      setenv("STT_WHISPER_SERVICE_HOTWORD_BOOST", junk, 1);
      settings_hotwords_from_env(s);
      CHECK(s.hotword_boost == 2.5f);
    }
    unsetenv("STT_WHISPER_SERVICE_HOTWORD_BOOST");
  }

  for (int max_batch : {1, 4}) {
    Settings s = base(dir);
    s.max_batch = max_batch;
    s.hotword_boost = 1.5f;
    SttEngine e(s);
    RequestOptions none;
    // no hotwords: nothing passed, the key as it always was
    const int calls = g_bias_calls;
    CHECK(!e.transcribe(pcm, 16000, none).empty());
    CHECK(g_bias_calls == calls + 1 && g_bias_null && g_bias_seen.empty());
    CHECK(e.options_key(none) == "5|0|5|0|0|en|");
    RequestOptions boosted_only = none;
    boosted_only.hotword_boost = 9.0f;  // a boost without hotwords changes nothing
    CHECK(e.options_key(boosted_only) == e.options_key(none));
    CHECK(!e.transcribe(pcm, 16000, boosted_only).empty());
    CHECK(g_bias_null);

    // two phrases per hotword, the setting's boost
    RequestOptions hw;
    hw.hotwords = {"Sentiric", "gfx950"};
    CHECK(!e.transcribe(pcm, 16000, hw).empty());
    CHECK(saw(hw.hotwords, 1.5f));
    // the request's boost wins over the setting's
    RequestOptions hw2 = hw;
    hw2.hotword_boost = 4.0f;
    CHECK(!e.transcribe(pcm, 16000, hw2).empty());
    CHECK(saw(hw.hotwords, 4.0f));
    // a request boost of 0: off, nothing passed
    RequestOptions hw0 = hw;
    hw0.hotword_boost = 0.0f;
    CHECK(!e.transcribe(pcm, 16000, hw0).empty());
    CHECK(g_bias_null && g_bias_seen.empty());
    // keys: different with hotwords, by the words and by the resolved boost
    CHECK(e.options_key(hw) != e.options_key(none));
    CHECK(e.options_key(hw) != e.options_key(hw2));
    CHECK(e.options_key(hw).compare(0, e.options_key(none).size(), e.options_key(none)) == 0);
    RequestOptions hw3 = hw;
    hw3.hotwords = {"Sentiric", "gfx95", "0"};
    CHECK(e.options_key(hw3) != e.options_key(hw));
    RequestOptions hw4 = hw;
    hw4.hotwords = {"Sentiric|6:gfx950"};  // (lengths in the key: no way to forge a separator)
    CHECK(e.options_key(hw4) != e.options_key(hw));
    RequestOptions same = hw;
    same.hotword_boost = 1.5f;  // resolves to what the setting gives
    CHECK(e.options_key(same) == e.options_key(hw));
    // dropped: empty, and more than 16 tokens (" " + 16 bytes = 17)
    RequestOptions drop;
    drop.hotwords = {"", "sixteen_bytes_ok", "ok", "seventeen_bytes_no"};
    CHECK(!e.transcribe(pcm, 16000, drop).empty());
    CHECK(saw({"ok"}, 1.5f));
    RequestOptions all_dropped;
    all_dropped.hotwords = {"", "this_hotword_is_far_too_long"};
    CHECK(!e.transcribe(pcm, 16000, all_dropped).empty());
    CHECK(g_bias_null && g_bias_seen.empty());
    // the pcm16 entry point and the batch entry point
    std::vector<int16_t> p16(pcm.size(), 300);
    CHECK(!e.transcribe_pcm16(p16, 16000, hw2).empty());
    CHECK(saw(hw.hotwords, 4.0f));
    if (max_batch == 1) {
      const auto rb = e.transcribe_batch({pcm, pcm}, hw);
      CHECK(rb.size() == 2 && g_bias_clips == 2 && saw(hw.hotwords, 1.5f));
    }
    // a streaming session passes its hotwords through
    {
      StreamSession ss(e);
      ss.set_hotwords({"stream"}, 3.0f);
      std::vector<uint8_t> chunk(2 * 16000, 0);
      for (size_t i = 0; i < chunk.size(); i += 2) chunk[i + 1] = (uint8_t)((i / 320) % 9);
      const int c0 = g_bias_calls;
      (void)ss.feed(chunk.data(), chunk.size());
      (void)ss.feed(nullptr, 0);
      CHECK(g_bias_calls > c0 && saw({"stream"}, 3.0f));
    }
  }
  // the setting's default: off, hotwords or not
  {
    SttEngine e(base(dir));
    RequestOptions hw;
    hw.hotwords = {"word"};
    CHECK(!e.transcribe(pcm, 16000, hw).empty());
    CHECK(g_bias_null && g_bias_seen.empty());
    hw.hotword_boost = 2.0f;
    CHECK(!e.transcribe(pcm, 16000, hw).empty());
    CHECK(saw({"word"}, 2.0f));
  }
  std::printf("host_bias_check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
