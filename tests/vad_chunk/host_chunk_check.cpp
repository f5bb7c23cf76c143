// TEST INFRASTRUCTURE ONLY — the host SttEngine's chunked-transcription plumbing
// (Settings::vad_chunk_s / vad_chunk_batch, mwx_stt_set_vad_chunk) over CPU
// stand-ins (tests/san/mwx_stub.cpp, tests/vad/vad_stub.cpp,
// tests/vad_trim/trim_stub.cpp and, unless built with -DNO_CHUNK_SYMBOLS,
// chunk_stub.cpp), built with AddressSanitizer + UBSan (tests/vad_chunk/Makefile)
// and run by tests/test_vad_chunk_host.py.
//
// With the chunked calls present: from several threads, with the request
// batcher on and off, vad_chunk_s > 0 sends the trim pass through
// mwx_vad_trim_batch_chunked with max_speech_duration_s clamped to vad_chunk_s
// and every decode through mwx_full_batch_chunked with vad_chunk_batch; the
// setter switches an existing engine over and back and refuses invalid values;
// without vad_trim nothing chunks. Without them (NO_CHUNK_SYMBOLS): the path is
// vad_trim's and the setter reports chunking inactive.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "stt_engine.h"

using namespace mwx_host;

extern "C" int mwx_stt_set_vad_chunk(void* eng, float chunk_s, int chunk_batch);

extern std::atomic<int> g_vad_single_calls, g_vad_batch_calls, g_vad_overlaps;
extern std::atomic<int> g_trim_calls, g_trim_clips, g_trim_live, g_trimmed_decodes;
#ifndef NO_CHUNK_SYMBOLS
extern std::atomic<int> g_chunk_trim_calls, g_chunked_decodes, g_chunk_bad_args;
extern std::atomic<int> g_chunk_last_s_milli, g_chunk_last_max_speech_milli, g_chunk_last_batch;
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
  CHECK(Settings().vad_chunk_s == 0.0f && Settings().vad_chunk_batch == 32);  // off by default
  Settings trim = base;
  trim.enable_vad = true;
  trim.vad_model_filename = "vad.bin";
  trim.vad_threshold = 0.75f;
  trim.vad_trim = true;
  Settings chunk = trim;
  chunk.vad_chunk_s = 5.0f;
  chunk.vad_chunk_batch = 7;
  Settings queued = chunk;
  queued.max_batch = 3;
  queued.parallel_requests = 2;
  Settings gate_only = chunk;  // vad_chunk_s without vad_trim: nothing chunks
  gate_only.vad_trim = false;
  Settings bad = trim;  // an invalid setting is dropped at construction
  bad.vad_chunk_s = 0.5f;

  const auto two = clip(5 * 16000 + 77, 10, 60, 100, 140);
  const auto one = clip(3 * 16000, 0, 80, 0, 0);
  const auto silent = clip(2 * 16000 + 5, 0, 0, 0, 0);
  auto failing = two;
  failing[0] = -1.0f;  // the stand-ins' calls fail on it
  const std::vector<float> tiny(4000, 0.9f);
  RequestOptions opt;

  {
    SttEngine plain(base), trimmed(trim), chunked(chunk), batched(queued), gated(gate_only),
        dropped(bad);
    const auto ref_two = plain.transcribe(two, 16000, opt);
    const auto ref_failing = plain.transcribe(failing, 16000, opt);
    const auto cut_two = plain.transcribe(kept(two, 0.75f), 16000, opt);
    const auto cut_one = plain.transcribe(kept(one, 0.75f), 16000, opt);
    CHECK(!cut_two.empty() && !same(cut_two, ref_two));
    CHECK(!trimmed.chunk_active() && !gated.chunk_active() && !dropped.chunk_active());
    CHECK(dropped.get_settings().vad_chunk_s == 0.0f);
    CHECK(mwx_stt_set_vad_chunk(nullptr, 1.0f, 32) == -1);

#ifndef NO_CHUNK_SYMBOLS
    CHECK(chunked.chunk_active() && batched.chunk_active());
    // one engine after the other: the stand-ins count overlapping VAD calls
    // over all contexts, and each engine has a context and a mutex of its own
    for (SttEngine* e : {&chunked, &batched}) {
      std::vector<std::thread> th;
      for (int t = 0; t < 4; ++t)
        th.emplace_back([&] {
          for (int rep = 0; rep < 6; ++rep) {
            CHECK(same(e->transcribe(two, 16000, opt), cut_two));
            CHECK(same(e->transcribe(one, 16000, opt), cut_one));
            CHECK(is_empty_result(e->transcribe(silent, 16000, opt), silent.size()));
            CHECK(same(e->transcribe(failing, 16000, opt), ref_failing));  // failed: untrimmed
            CHECK(e->transcribe(tiny, 16000, opt).empty());  // under vad_ms_min_duration
          }
        });
      for (auto& t : th) t.join();
    }
    CHECK(g_vad_overlaps == 0);
    CHECK(g_vad_single_calls + g_vad_batch_calls == 0);  // the trim pass is the only VAD pass
    CHECK(g_chunk_trim_calls == 4 * 6 * 2 * 4 && g_trim_calls == g_chunk_trim_calls);
    CHECK(g_trimmed_decodes == 0 && g_chunked_decodes > 0 && g_chunk_bad_args == 0);
    CHECK(batched.batches_run() > 0);
    CHECK(g_chunk_last_s_milli == 5000 && g_chunk_last_batch == 7);
    CHECK(g_chunk_last_max_speech_milli == 5000);  // min(FLT_MAX, vad_chunk_s)

    // transcribe_batch: one chunked trim pass, one chunked decode
    {
      const int calls = g_chunk_trim_calls, decodes = g_chunked_decodes;
      const auto rs = chunked.transcribe_batch({two, silent, tiny, one}, opt);
      CHECK(g_chunk_trim_calls == calls + 1 && g_chunked_decodes == decodes + 1);
      CHECK(g_trimmed_decodes == 0);
      CHECK(rs.size() == 4);
      if (rs.size() == 4) {
        CHECK(same(rs[0], cut_two) && same(rs[3], cut_one));
        CHECK(is_empty_result(rs[1], silent.size()) && rs[2].empty());
      }
    }

    // the setter on an engine that trims: over, refused values, and back
    {
      const int calls = g_chunk_trim_calls, decodes = g_chunked_decodes;
      CHECK(same(trimmed.transcribe(two, 16000, opt), cut_two));
      CHECK(g_chunk_trim_calls == calls && g_chunked_decodes == decodes && g_trimmed_decodes == 1);
      CHECK(mwx_stt_set_vad_chunk(&trimmed, 2.0f, 4) == 1);
      CHECK(mwx_stt_set_vad_chunk(&trimmed, 0.5f, 4) == -1);
      CHECK(mwx_stt_set_vad_chunk(&trimmed, 31.0f, 4) == -1);
      CHECK(mwx_stt_set_vad_chunk(&trimmed, std::nanf(""), 4) == -1);
      CHECK(mwx_stt_set_vad_chunk(&trimmed, 2.0f, 0) == -1);
      CHECK(trimmed.get_settings().vad_chunk_s == 2.0f &&
            trimmed.get_settings().vad_chunk_batch == 4);  // refused: nothing changed
      CHECK(same(trimmed.transcribe(two, 16000, opt), cut_two));
      CHECK(g_chunk_trim_calls == calls + 1 && g_chunked_decodes == decodes + 1);
      CHECK(g_chunk_last_s_milli == 2000 && g_chunk_last_max_speech_milli == 2000 &&
            g_chunk_last_batch == 4 && g_trimmed_decodes == 1);
      CHECK(mwx_stt_set_vad_chunk(&trimmed, 0.0f, 32) == 0);
      CHECK(same(trimmed.transcribe(two, 16000, opt), cut_two));
      CHECK(g_chunk_trim_calls == calls + 1 && g_chunked_decodes == decodes + 1 &&
            g_trimmed_decodes == 2 && g_chunk_bad_args == 0);
    }

    // vad_chunk_s without vad_trim: the gate, and no trimming or chunked call
    {
      const int trims = g_trim_calls, decodes = g_chunked_decodes;
      CHECK(mwx_stt_set_vad_chunk(&gated, 3.0f, 8) == 0);  // set, inactive
      CHECK(same(gated.transcribe(two, 16000, opt), ref_two));
      CHECK(g_trim_calls == trims && g_chunked_decodes == decodes && g_vad_single_calls == 1);
    }
#else
    // a library without the chunked calls: the path is vad_trim's
    CHECK(!chunked.chunk_active() && !batched.chunk_active());
    CHECK(mwx_stt_set_vad_chunk(&chunked, 5.0f, 7) == 0);  // set, inactive
    CHECK(mwx_stt_set_vad_chunk(&chunked, 0.5f, 7) == -1);
    for (SttEngine* e : {&chunked, &batched}) {
      std::vector<std::thread> th;
      for (int t = 0; t < 4; ++t)
        th.emplace_back([&] {
          for (int rep = 0; rep < 3; ++rep) {
            CHECK(same(e->transcribe(two, 16000, opt), cut_two));
            CHECK(is_empty_result(e->transcribe(silent, 16000, opt), silent.size()));
            CHECK(same(e->transcribe(failing, 16000, opt), ref_failing));
          }
        });
      for (auto& t : th) t.join();
    }
    CHECK(g_trim_calls == 4 * 3 * 2 * 3 && g_trimmed_decodes > 0);
    CHECK(g_vad_overlaps == 0 && g_vad_single_calls + g_vad_batch_calls == 0);
    const int decodes = g_trimmed_decodes;
    const auto rs = chunked.transcribe_batch({two, silent, one}, opt);
    CHECK(g_trimmed_decodes == decodes + 1 && rs.size() == 3);
    if (rs.size() == 3)
      CHECK(same(rs[0], cut_two) && is_empty_result(rs[1], silent.size()) && same(rs[2], cut_one));
#endif
  }
  CHECK(g_trim_live == 0);  // every trimmed object was freed
  std::printf("host_chunk_check: %d failure(s)\n", failures.load());
  return failures ? 1 : 0;
}
