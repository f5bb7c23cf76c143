// TEST INFRASTRUCTURE ONLY — the host SttEngine's align() / align_pcm16() /
// align_batch() over the CPU stand-in align_stub.cpp (tests/align/Makefile;
// AddressSanitizer + UBSan), run by tests/test_align_host.py: the text is
// trimmed and tokenised with one leading space, the limits and engine errors
// give ok = false without a throw, n_agree / avg_logprob / eot_logprob are
// formed from the rows, the state pool's timeout throws EngineBusyException,
// and the request batcher is not involved. Built with -DALIGN_UNBOUND against
// the plain stand-in (no alignment calls): align() returns ok = false.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "stt_engine.h"

using namespace mwx_host;

#ifndef ALIGN_UNBOUND
extern std::string g_align_text;
extern int g_align_calls, g_align_clips, g_align_sleep_ms;
extern mwx_full_params g_align_params;
#endif

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
  s.request_queue_timeout_ms = 100;
  s.language = "en";
  return s;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ofstream(dir + "/ggml-micro.bin") << "stub";
  std::vector<float> pcm(16000 * 4);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = 0.01f * (float)((i / 160) % 23);
  RequestOptions opt;

#ifdef ALIGN_UNBOUND
  {
    SttEngine e(base(dir));
    CHECK(!e.align_available());
    const AlignmentResult r = e.align(pcm, 16000, "hello world", opt);
    CHECK(!r.ok && r.tokens.empty() && r.text.empty());
    const auto rs = e.align_batch({pcm, pcm}, {"hello", "world"}, opt);
    CHECK(rs.size() == 2 && !rs[0].ok && !rs[1].ok);
    CHECK(!e.align_pcm16(std::vector<int16_t>(16000, 100), 16000, "hello", opt).ok);
    CHECK(!e.transcribe(pcm, 16000, opt).empty());  // the rest of the engine works
  }
  std::printf("host_align_unbound: %d failure(s)\n", failures);
#else
  {
    SttEngine e(base(dir));
    CHECK(e.align_available());
    // trimmed, one leading space; words of the stand-in's vocabulary
    const AlignmentResult r = e.align(pcm, 16000, "  hello world this is \n", opt);
    CHECK(g_align_text == " hello world this is");
    CHECK(r.ok && r.tokens.size() == 4 && r.text == " hello world this is");
    CHECK(r.language == "en");
    CHECK(!g_align_params.translate && g_align_params.initial_prompt == nullptr);
    double sum = 0.0;
    int agree = 0;
    for (size_t j = 0; j < r.tokens.size(); ++j) {
      const AlignedToken& t = r.tokens[j];
      CHECK(t.id == (int)j && t.text == std::string(mwx_token_to_str(nullptr, t.id)));
      CHECK(t.p == 0.5f + 0.01f * (float)j && t.plog == std::log(t.p) && t.t == -1);
      CHECK(t.top_id == (j % 2 == 0 ? t.id : (t.id + 1) % 16));
      CHECK(t.top_plog == (j % 2 == 0 ? t.plog : -0.1f));
      CHECK(t.top_text == std::string(mwx_token_to_str(nullptr, t.top_id)));
      sum += t.plog;
      agree += t.top_id == t.id;
    }
    CHECK(r.n_agree == agree && agree == 2);
    CHECK(r.avg_logprob == (float)(sum / 4) && r.eot_logprob == -0.25f);
    // requested language, translate; "auto" reports what the engine used
    RequestOptions de;
    de.language = "de";
    de.translate = true;
    CHECK(e.align(pcm, 16000, "hello", de).language == "de" && g_align_params.translate);
    RequestOptions au;
    au.language = "auto";
    CHECK(e.align(pcm, 16000, "hello", au).language == "tr");
    // empty text: no tokens, only the EOT row
    const AlignmentResult none = e.align(pcm, 16000, " \t ", opt);
    CHECK(none.ok && none.tokens.empty() && none.avg_logprob == 0.0f && none.eot_logprob == -0.25f);
    // pcm16 at another rate goes through the resampler
    const int calls0 = g_align_calls;
    const AlignmentResult p16 = e.align_pcm16(std::vector<int16_t>(8000 * 3, 300), 8000, "world", opt);
    CHECK(p16.ok && p16.tokens.size() == 1 && p16.tokens[0].id == 1 && g_align_calls == calls0 + 1);
    // no minimum-duration gate: 0.2 s still reaches the engine ...
    CHECK(e.align(std::vector<float>(3200, 0.1f), 16000, "hello", opt).ok);
    // ... which has no result for a clip under 0.1 s
    CHECK(!e.align(std::vector<float>(800, 0.1f), 16000, "hello", opt).ok);
    // limits: 225 words, 30 s + 1 sample; an engine error (-3: the stand-in
    // refuses nothing the tokeniser makes, so the abort path stands in)
    std::string many;
    for (int i = 0; i < 225; ++i) many += " hello";
    const int calls1 = g_align_calls;
    CHECK(!e.align(pcm, 16000, many, opt).ok && g_align_calls == calls1);
    CHECK(!e.align(std::vector<float>(480001, 0.0f), 16000, "hello", opt).ok);
    CHECK(g_align_calls == calls1);
    std::string most;
    for (int i = 0; i < 224; ++i) most += " hello";
    CHECK(e.align(pcm, 16000, most, opt).tokens.size() == 224);
    RequestOptions ab;
    int polls = 0;
    ab.should_abort = [&polls] { return ++polls > 1; };
    CHECK(!e.align(pcm, 16000, "hello", ab).ok && polls == 2);
    // batch: one engine call, results per clip; a size mismatch fails all
    const int calls2 = g_align_calls;
    const auto rs = e.align_batch({pcm, pcm, pcm}, {"hello", "", "a test"}, opt);
    CHECK(g_align_calls == calls2 + 1 && g_align_clips == 3);
    CHECK(rs.size() == 3 && rs[0].ok && rs[1].ok && rs[2].ok);
    CHECK(rs.size() == 3 && rs[0].tokens.size() == 1 && rs[1].tokens.empty() &&
          rs[2].tokens.size() == 2 && rs[2].text == " a test");
    const auto bad = e.align_batch({pcm, pcm}, {"hello"}, opt);
    CHECK(bad.size() == 2 && !bad[0].ok && !bad[1].ok && g_align_calls == calls2 + 1);
    // pool: the one state is held by a running align; the second caller gets
    // EngineBusyException after the queue timeout, as transcribe() does
    g_align_sleep_ms = 600;
    std::atomic<bool> first_ok{false};
    std::thread th([&] { first_ok = e.align(pcm, 16000, "hello", opt).ok; });
    std::this_thread::sleep_for(std::chrono::milliseconds(150));
    bool busy = false;
    try {
      e.align(pcm, 16000, "world", opt);
    } catch (const EngineBusyException&) {
      busy = true;
    }
    th.join();
    g_align_sleep_ms = 0;
    CHECK(busy && first_ok.load());
    CHECK(e.align(pcm, 16000, "hello", opt).ok);  // the state is back in the pool
    CHECK(e.batches_run() == 0);
  }
  {  // with the request batcher on, align() runs on the batch states, not the batcher
    Settings s = base(dir);
    s.max_batch = 4;
    SttEngine e(s);
    CHECK(e.align(pcm, 16000, "hello world", opt).ok);
    CHECK(e.batches_run() == 0);
    CHECK(!e.transcribe(pcm, 16000, opt).empty() && e.batches_run() == 1);
  }
  std::printf("host_align_check: %d failure(s)\n", failures);
#endif
  return failures ? 1 : 0;
}
