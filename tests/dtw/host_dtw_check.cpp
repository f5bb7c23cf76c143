// TEST INFRASTRUCTURE ONLY — the host SttEngine's DTW token times over the CPU
// stand-in dtw_stub.cpp (tests/dtw/Makefile; AddressSanitizer + UBSan), run by
// tests/test_dtw_host.py: Settings::dtw_* reach mwx_context_params, and with
// dtw_token_timestamps a kept token's t0 is its t_dtw and its t1 the next kept
// token's t_dtw (the segment's t1 for the last one); with it off the tokens
// keep the heuristic t0 / t1. Segment times never change.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "stt_engine.h"

using namespace mwx_host;

extern mwx_context_params g_dtw_params;
extern std::vector<mwx_ahead> g_dtw_heads;

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
  s.language = "en";
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ofstream(dir + "/ggml-micro.bin") << "stub";
  std::vector<float> pcm(16000 * 9);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = 0.01f * (float)((i / 160) % 23);
  RequestOptions opt;
  opt.language = "en";

  std::vector<TranscriptionResult> plain;
  {
    SttEngine off(base(dir));
    CHECK(!g_dtw_params.dtw_token_timestamps);
    plain = off.transcribe(pcm, 16000, opt);
    CHECK(!plain.empty());
    // the stand-in's heuristic times: 50 units per token from the segment start
    for (const auto& r : plain)
      for (size_t k = 0; k < r.tokens.size(); ++k)
        CHECK(r.tokens[k].t1 - r.tokens[k].t0 == 50);
  }
  {
    Settings s = base(dir);
    s.dtw_token_timestamps = true;
    s.dtw_aheads_preset = MWX_AHEADS_CUSTOM;
    s.dtw_aheads = {{0, 1}, {1, 0}};
    SttEngine on(s);
    CHECK(g_dtw_params.dtw_token_timestamps);
    CHECK(g_dtw_params.dtw_aheads_preset == MWX_AHEADS_CUSTOM);
    CHECK(g_dtw_params.dtw_aheads.n_heads == 2 && g_dtw_heads.size() == 2);
    CHECK(g_dtw_heads.size() == 2 && g_dtw_heads[0].n_text_layer == 0 &&
          g_dtw_heads[0].n_head == 1 && g_dtw_heads[1].n_text_layer == 1 &&
          g_dtw_heads[1].n_head == 0);
    const auto got = on.transcribe(pcm, 16000, opt);
    CHECK(got.size() == plain.size());
    size_t n_tok = 0;
    for (size_t i = 0; i < got.size() && i < plain.size(); ++i) {
      const auto &g = got[i], &p = plain[i];
      CHECK(g.text == p.text && g.t0 == p.t0 && g.t1 == p.t1 && g.prob == p.prob);
      CHECK(g.tokens.size() == p.tokens.size());
      // every kept segment of the stand-in keeps its three text tokens, so a
      // token's index among the kept ones is its index in the segment
      for (size_t k = 0; k < g.tokens.size() && k < p.tokens.size(); ++k, ++n_tok) {
        const int64_t want0 = p.tokens[k].t0 + 7 + 3 * (int64_t)k;
        const int64_t want1 =
            k + 1 < g.tokens.size() ? p.tokens[k + 1].t0 + 7 + 3 * (int64_t)(k + 1) : g.t1;
        CHECK(g.tokens[k].t0 == want0);
        CHECK(g.tokens[k].t1 == want1);
        CHECK(g.tokens[k].text == p.tokens[k].text && g.tokens[k].p == p.tokens[k].p);
      }
    }
    CHECK(n_tok >= 6);
    const auto batch = on.transcribe_batch({pcm, pcm}, opt);
    CHECK(batch.size() == 2);
    for (const auto& b : batch) {
      CHECK(b.size() == got.size());
      for (size_t i = 0; i < b.size() && i < got.size(); ++i)
        for (size_t k = 0; k < b[i].tokens.size() && k < got[i].tokens.size(); ++k)
          CHECK(b[i].tokens[k].t0 == got[i].tokens[k].t0 && b[i].tokens[k].t1 == got[i].tokens[k].t1);
    }
  }
  {
    Settings s = base(dir);
    s.dtw_token_timestamps = true;
    s.dtw_aheads_preset = MWX_AHEADS_N_TOP_MOST;
    s.dtw_n_top = 2;
    SttEngine top(s);
    CHECK(g_dtw_params.dtw_aheads_preset == MWX_AHEADS_N_TOP_MOST && g_dtw_params.dtw_n_top == 2);
    CHECK(g_dtw_params.dtw_aheads.n_heads == 0 && g_dtw_heads.empty());
  }
  {  // the environment
    Settings s = base(dir);
    settings_dtw_from_env(s);
    CHECK(!s.dtw_token_timestamps && s.dtw_aheads_preset == 0 && s.dtw_aheads.empty());
    setenv("STT_WHISPER_SERVICE_DTW_TOKEN_TIMESTAMPS", "true", 1);
    setenv("STT_WHISPER_SERVICE_DTW_AHEADS_PRESET", "custom", 1);
    setenv("STT_WHISPER_SERVICE_DTW_AHEADS", "3:1,5:7", 1);
    setenv("STT_WHISPER_SERVICE_DTW_N_TOP", "4", 1);
    settings_dtw_from_env(s);
    CHECK(s.dtw_token_timestamps && s.dtw_aheads_preset == MWX_AHEADS_CUSTOM && s.dtw_n_top == 4);
    CHECK(s.dtw_aheads.size() == 2 && s.dtw_aheads[0] == std::make_pair(3, 1) &&
          s.dtw_aheads[1] == std::make_pair(5, 7));
    setenv("STT_WHISPER_SERVICE_DTW_AHEADS_PRESET", "large-v3", 1);
    settings_dtw_from_env(s);
    CHECK(s.dtw_aheads_preset == MWX_AHEADS_LARGE_V3);
    setenv("STT_WHISPER_SERVICE_DTW_AHEADS_PRESET", "no-such-model", 1);
    settings_dtw_from_env(s);
    CHECK(s.dtw_aheads_preset == -1);
  }
  std::printf("host_dtw_check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
