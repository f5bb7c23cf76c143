// TEST INFRASTRUCTURE ONLY — the host SttEngine's vad_trim plumbing over CPU
// stand-ins (tests/san/mwx_stub.cpp, tests/vad/vad_stub.cpp and, unless built
// with -DNO_TRIM_SYMBOLS, trim_stub.cpp), built with AddressSanitizer + UBSan
// (tests/vad_trim/Makefile) and run by tests/test_vad_trim_host.py.
//
// With the trimming calls present: from several threads, transcribe() (direct
// and through the request batcher) and transcribe_batch() decode the kept
// samples only, a clip without segments gets the empty result, a failing trim
// call leaves the clip untrimmed, the gate calls are never made (a clip goes
// through the VAD once), calls on the VAD context never overlap, and every
// trimmed object is freed. Without them (NO_TRIM_SYMBOLS): vad_trim behaves as
// the gate.
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "stt_engine.h"

using namespace mwx_host;

extern std::atomic<int> g_vad_single_calls, g_vad_batch_calls, g_vad_overlaps;
#ifndef NO_TRIM_SYMBOLS
extern std::atomic<int> g_trim_calls, g_trim_clips, g_trim_live, g_trimmed_decodes;
#endif

namespace {

std::atomic<int> failures{0};
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

// chunk i has probability `hi` inside [a0, a1) or [b0, b1) and `lo` elsewhere;
// the other samples differ per chunk so that the kept audio decides the result
std::vector<float> clip(int n, int a0, int a1, int b0, int b1, float hi = 0.9f, float lo = 0.1f) {
  std::vector<float> x((size_t)n);
  for (int i = 0; i < n; ++i) x[(size_t)i] = 0.001f * (float)((i / 512) % 37);
  for (int i = 0; i * 512 < n; ++i)
    x[(size_t)i * 512] = (i >= a0 && i < a1) || (i >= b0 && i < b1) ? hi : lo;
  return x;
}

// what the stand-in rule keeps at `thr`
std::vector<float> kept(const std::vector<float>& x, float thr) {
  std::vector<float> out;
  const int n = (int)x.size();
  for (int i = 0; i * 512 < n; ++i)
    if (x[(size_t)i * 512] >= thr)
      out.insert(out.end(), x.begin() + 512 * i, x.begin() + std::min(n, 512 * i + 512));
  return out;
}

bool is_empty_result(const std::vector<TranscriptionResult>& rs, size_t n) {
  return rs.size() == 1 && rs[0].text.empty() && rs[0].language == "unknown" && rs[0].t0 == 0 &&
         rs[0].t1 == (int64_t)(n / 16.0) && rs[0].tokens.empty() && rs[0].speaker_id == "unknown";
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
  Settings gate = base;
  gate.enable_vad = true;
  gate.vad_model_filename = "vad.bin";
  gate.vad_threshold = 0.75f;
  Settings trim = gate;
  trim.vad_trim = true;
  Settings queued = trim;
  queued.max_batch = 3;
  queued.parallel_requests = 2;
  Settings no_model = trim;
  no_model.vad_model_filename = "no-such-file.bin";
  Settings no_vad = trim;
  no_vad.enable_vad = false;
  CHECK(!Settings().vad_trim);  // off by default

  const auto two = clip(5 * 16000 + 77, 10, 60, 100, 140);  // 50 + 40 of 157 chunks kept
  const auto one = clip(3 * 16000, 0, 80, 0, 0);
  const auto at_thr = clip(2 * 16000, 5, 40, 0, 0, 0.75f);  // equal to the threshold: speech
  const auto silent = clip(2 * 16000 + 5, 0, 0, 0, 0);
  auto failing = two;
  failing[0] = -1.0f;  // the stand-ins' calls fail on it
  const std::vector<float> tiny(4000, 0.9f);
  RequestOptions opt;

  {
    SttEngine plain(base), gated(gate), trimmed(trim), batched(queued), open(no_model), off(no_vad);
    const auto ref_two = plain.transcribe(two, 16000, opt);
    const auto ref_failing = plain.transcribe(failing, 16000, opt);
    const auto cut_two = plain.transcribe(kept(two, 0.75f), 16000, opt);
    const auto cut_one = plain.transcribe(kept(one, 0.75f), 16000, opt);
    const auto cut_at = plain.transcribe(kept(at_thr, 0.75f), 16000, opt);
    CHECK(!cut_two.empty() && !same(cut_two, ref_two));  // trimming shows in the result
    const int gate_calls = g_vad_single_calls + g_vad_batch_calls;
    CHECK(gate_calls == 0);

#ifndef NO_TRIM_SYMBOLS
    // one engine after the other: the stand-ins count overlapping VAD calls
    // over all contexts, and each engine has a context and a mutex of its own
    for (SttEngine* e : {&trimmed, &batched}) {
      std::vector<std::thread> th;
      for (int t = 0; t < 4; ++t)
        th.emplace_back([&] {
          for (int rep = 0; rep < 6; ++rep) {
            SttEngine::PerformanceMetrics m{-1, -1, -1};
            CHECK(same(e->transcribe(two, 16000, opt), cut_two));
            CHECK(same(e->transcribe(one, 16000, opt), cut_one));
            CHECK(same(e->transcribe(at_thr, 16000, opt), cut_at));
            CHECK(is_empty_result(e->transcribe(silent, 16000, opt, &m), silent.size()));
            CHECK(m.queue_time_ms == 0.0 && m.processing_time_ms >= 0.0 && m.token_count == 0);
            CHECK(same(e->transcribe(failing, 16000, opt), ref_failing));  // failed: untrimmed
            CHECK(e->transcribe(tiny, 16000, opt).empty());  // under vad_ms_min_duration
          }
        });
      for (auto& t : th) t.join();
    }
    CHECK(g_vad_overlaps == 0);
    CHECK(g_vad_single_calls + g_vad_batch_calls == 0);  // the trim pass is the only VAD pass
    CHECK(g_trim_calls == 4 * 6 * 2 * 5 && g_trim_clips == g_trim_calls);
    CHECK(batched.batches_run() > 0);

    // transcribe_batch: one trim pass over the clips long enough, one trimmed decode
    const int calls = g_trim_calls, clips_seen = g_trim_clips, decodes = g_trimmed_decodes;
    const auto rs = trimmed.transcribe_batch({two, silent, tiny, one, at_thr}, opt);
    CHECK(g_trim_calls == calls + 1 && g_trim_clips == clips_seen + 4);
    CHECK(g_trimmed_decodes == decodes + 1);
    CHECK(rs.size() == 5);
    if (rs.size() == 5) {
      CHECK(same(rs[0], cut_two) && same(rs[3], cut_one) && same(rs[4], cut_at));
      CHECK(is_empty_result(rs[1], silent.size()));
      CHECK(rs[2].empty());
    }
    const auto all_silent = trimmed.transcribe_batch({silent, silent}, opt);
    CHECK(all_silent.size() == 2 && g_trimmed_decodes == decodes + 1);  // no Whisper batch
    for (const auto& r : all_silent) CHECK(is_empty_result(r, silent.size()));
    // the failing clip fails the pass: every clip of the batch goes on untrimmed
    const auto mixed = trimmed.transcribe_batch({two, failing}, opt);
    CHECK(mixed.size() == 2);
    if (mixed.size() == 2) CHECK(same(mixed[0], ref_two) && same(mixed[1], ref_failing));
    // no VAD model, or VAD off: untrimmed, and no VAD call at all
    const int trims = g_trim_calls;
    CHECK(same(open.transcribe(two, 16000, opt), ref_two));
    CHECK(same(off.transcribe(two, 16000, opt), ref_two));
    CHECK(g_trim_calls == trims && g_vad_single_calls + g_vad_batch_calls == 0);
#else
    // a library without the trimming calls: vad_trim is the gate
    CHECK(same(trimmed.transcribe(two, 16000, opt), gated.transcribe(two, 16000, opt)));
    CHECK(same(trimmed.transcribe(two, 16000, opt), ref_two));
    CHECK(same(batched.transcribe(two, 16000, opt), ref_two));
    CHECK(is_empty_result(trimmed.transcribe(silent, 16000, opt), silent.size()));
    CHECK(g_vad_single_calls == 5);
    const auto rs = trimmed.transcribe_batch({two, silent, one}, opt);
    const auto gs = gated.transcribe_batch({two, silent, one}, opt);
    CHECK(g_vad_batch_calls == 2 && rs.size() == 3 && gs.size() == 3);
    for (size_t b = 0; b < rs.size() && b < gs.size(); ++b) CHECK(same(rs[b], gs[b]));
    if (rs.size() == 3) CHECK(is_empty_result(rs[1], silent.size()) && same(rs[0], ref_two));
#endif
  }
#ifndef NO_TRIM_SYMBOLS
  CHECK(g_trim_live == 0);  // every trimmed object was freed
#endif
  std::printf("host_trim_check: %d failure(s)\n", failures.load());
  return failures ? 1 : 0;
}
