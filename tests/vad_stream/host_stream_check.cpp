// TEST INFRASTRUCTURE ONLY — the host side of streaming VAD (Settings::stream_vad,
// Settings::stream_endpoint_silence_ms; StreamSession) over CPU stand-ins
// (tests/san/mwx_stub.cpp, tests/vad/vad_stub.cpp, tests/vad_trim/trim_stub.cpp
// and, unless built with -DNO_STREAM_SYMBOLS, stream_stub.cpp), built with
// AddressSanitizer + UBSan (tests/vad_stream/Makefile) and run by
// tests/test_vad_stream_host.py.
//
// With the stream calls present: the gate decision of a session's VAD stream
// replaces the whole-buffer gate without changing an event (and the gate no
// longer runs); the stream restarts whenever the buffer does (empty chunk,
// 30-s rule, endpoint cut); endpointing cuts at the last closed segment's
// closed_at, finalizes the head as the empty chunk does and goes on with the
// remainder, also when one feed closes two segments; a failing stream call
// leaves a working session; several sessions run from several threads.
// Without them (NO_STREAM_SYMBOLS): both settings are inert and the events
// are today's.
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "stt_engine.h"
#include "stt_stream.h"

using namespace mwx_host;

extern "C" int mwx_stt_stream_vad_active(void* eng);
extern "C" long mwx_stt_vad_gate_runs(void* eng);

extern std::atomic<int> g_vad_single_calls, g_vad_batch_calls, g_vad_overlaps;
#ifndef NO_STREAM_SYMBOLS
extern std::atomic<int> g_stream_live, g_stream_inits, g_stream_feeds, g_stream_resets;
extern std::atomic<int> g_stream_last_min_silence_ms, g_stream_last_threshold_milli;
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

constexpr int16_t kHi = 29491, kLo = 3277;  // 0.9 and 0.1 as the stand-ins read them
constexpr float kThr = 0.75f;
constexpr int kSilenceMs = 200;             // the endpoint's S: 3200 samples

struct Range {
  int a, b;  // chunks [a, b) are speech
};

// chunk i has probability 0.9 inside a range and 0.1 elsewhere; the other
// samples differ per chunk so that the audio of a cut decides its result
std::vector<int16_t> clip(int n, const std::vector<Range>& speech) {
  std::vector<int16_t> x((size_t)n);
  for (int i = 0; i < n; ++i) x[(size_t)i] = (int16_t)(40 * ((i / 512) % 37));
  for (int i = 0; i * 512 < n; ++i) {
    bool sp = false;
    for (const Range& r : speech) sp |= i >= r.a && i < r.b;
    x[(size_t)i * 512] = sp ? kHi : kLo;
  }
  return x;
}

struct Ev {
  std::string text, speaker;
  bool is_final;
  size_t n_words;
  float arousal, pitch_mean;
  bool operator==(const Ev& o) const {
    return text == o.text && speaker == o.speaker && is_final == o.is_final &&
           n_words == o.n_words && arousal == o.arousal && pitch_mean == o.pitch_mean;
  }
};
using Events = std::vector<std::vector<Ev>>;  // per fed chunk

std::vector<Ev> plain(const std::vector<StreamEvent>& evs) {
  std::vector<Ev> out;
  for (const auto& e : evs)
    out.push_back({e.transcription, e.speaker_id, e.is_final, e.words.size(), e.arousal,
                   e.pitch_mean});
  return out;
}

// feeds: sample counts, 0 = the empty chunk
Events run(SttEngine& eng, const std::vector<int16_t>& pcm, const std::vector<size_t>& feeds) {
  StreamSession s(eng);
  Events out;
  size_t at = 0;
  for (size_t k : feeds) {
    out.push_back(plain(s.feed((const uint8_t*)(pcm.data() + at), 2 * k)));
    at += k;
  }
  return out;
}

std::vector<size_t> cadence(size_t n, size_t step, bool end = true) {
  std::vector<size_t> f;
  for (size_t a = 0; a < n; a += step) f.push_back(std::min(step, n - a));
  if (end) f.push_back(0);
  return f;
}

size_t count(const Events& ev, bool finals, size_t upto) {
  size_t n = 0;
  for (size_t i = 0; i < upto && i < ev.size(); ++i)
    for (const Ev& e : ev[i]) n += e.is_final == finals;
  return n;
}

// closed_at of the last segment that the rule (threshold kThr, silence
// kSilenceMs, min speech 250 ms) closes within the whole chunks of `buf`; 0 = none
size_t last_closed_at(const std::vector<int16_t>& buf) {
  const int64_t min_sil = 16 * kSilenceMs, min_speech = 16 * 250;
  const float neg = kThr - 0.15f;
  bool trig = false;
  int64_t start = 0, temp_end = 0;
  size_t closed = 0;
  for (size_t i = 0; (i + 1) * 512 <= buf.size(); ++i) {
    const float p = (float)buf[i * 512] / 32768.0f;
    const int64_t cur = 512 * (int64_t)i;
    if (p >= kThr) {
      temp_end = 0;
      if (!trig) {
        trig = true;
        start = cur;
      }
    } else if (p < neg && trig) {
      if (temp_end == 0) temp_end = cur;
      if (cur - temp_end >= min_sil) {
        if (temp_end - start > min_speech) closed = (size_t)cur + 512;
        temp_end = 0;
        trig = false;
      }
    }
  }
  return closed;
}

std::vector<Ev> finals_of(const std::vector<TranscriptionResult>& rs, bool words) {
  std::vector<Ev> out;
  for (const auto& r : rs)
    if (!r.text.empty())
      out.push_back({r.text, r.speaker_id, true, words ? r.tokens.size() : 0, r.affective.arousal,
                     words ? r.affective.pitch_mean : 0.0f});
  return out;
}

// The endpointing session restated over `gate` (an engine with the
// whole-buffer gate and no stream settings). cuts: every (cut, remainder).
Events model(SttEngine& gate, const std::vector<int16_t>& pcm, const std::vector<size_t>& feeds,
             size_t step, std::vector<std::pair<size_t, size_t>>* cuts) {
  Events out;
  std::vector<int16_t> buf;
  size_t last = 0, at = 0;
  RequestOptions opt;
  for (size_t k : feeds) {
    std::vector<Ev> evs;
    if (k == 0) {
      if (!buf.empty()) {
        evs = finals_of(gate.transcribe_pcm16(buf, 16000, opt), true);
        buf.clear();
        last = 0;
      }
      out.push_back(evs);
      continue;
    }
    buf.insert(buf.end(), pcm.begin() + (std::ptrdiff_t)at, pcm.begin() + (std::ptrdiff_t)(at + k));
    at += k;
    for (size_t cut; (cut = last_closed_at(buf)) != 0;) {
      const std::vector<int16_t> head(buf.begin(), buf.begin() + (std::ptrdiff_t)cut);
      for (const Ev& e : finals_of(gate.transcribe_pcm16(head, 16000, opt), true)) evs.push_back(e);
      buf.erase(buf.begin(), buf.begin() + (std::ptrdiff_t)cut);
      last = 0;
      if (cuts) cuts->push_back({cut, buf.size()});
    }
    if (buf.size() - last >= step) {
      const auto rs = gate.transcribe_pcm16(buf, 16000, opt);
      last = buf.size();
      Ev partial{"", "", false, 0, 0.0f, 0.0f};
      bool any = false;
      for (const auto& r : rs) {
        if (r.text.empty()) continue;
        partial.text += r.text + " ";
        partial.speaker = r.speaker_id;
        partial.arousal = r.affective.arousal;
        partial.pitch_mean = r.affective.pitch_mean;
        any = true;
      }
      if (any) evs.push_back(partial);
      if (buf.size() > StreamSession::kMaxBufferSamples) {
        for (const Ev& e : finals_of(rs, false)) evs.push_back(e);
        buf.clear();
        last = 0;
      }
    }
    out.push_back(evs);
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ofstream(dir + "/ggml-micro.bin") << "stub";
  std::ofstream(dir + "/vad.bin") << "stub";
  CHECK(!Settings().stream_vad && Settings().stream_endpoint_silence_ms == 0);  // off by default
  Settings base;
  base.model_dir = dir;
  base.model_filename = "ggml-micro.bin";
  base.parallel_requests = 4;
  base.language = "en";
  base.beam_size = 1;
  Settings gate = base;
  gate.enable_vad = true;
  gate.vad_model_filename = "vad.bin";
  gate.vad_threshold = kThr;
  Settings sv = gate;
  sv.stream_vad = true;
  Settings ep = sv;
  ep.stream_endpoint_silence_ms = kSilenceMs;
  Settings ep_only = gate;  // endpointing with the whole-buffer gate
  ep_only.stream_endpoint_silence_ms = kSilenceMs;
  Settings trim = ep;       // vad_trim active: no gate to replace, endpointing still on
  trim.vad_trim = true;
  Settings no_vad = base;   // no VAD model: both inert
  no_vad.stream_vad = true;
  no_vad.stream_endpoint_silence_ms = kSilenceMs;
  const size_t step = (size_t)base.stream_buffer_samples;

  // 1.5 s of silence, speech, a long pause, speech, 1 s of silence
  const auto talk = clip(8 * 16000 + 300, {{47, 110}, {170, 215}});
  // more than 30 s: the buffer restarts on its own, then silence only
  const auto longc = clip(40 * 16000, {{10, 935}});
  // two bursts and both pauses inside one client chunk
  const auto burst = clip(6 * 16000, {{10, 50}, {80, 120}});

  {
    SttEngine e_gate(gate), e_sv(sv), e_ep(ep), e_ep_only(ep_only), e_trim(trim), e_none(no_vad);
    CHECK(mwx_stt_stream_vad_active(&e_gate) == 0 && mwx_stt_stream_vad_active(&e_none) == 0);
#ifndef NO_STREAM_SYMBOLS
    CHECK(mwx_stt_stream_vad_active(&e_sv) == 1 && mwx_stt_stream_vad_active(&e_ep) == 3);
    CHECK(mwx_stt_stream_vad_active(&e_ep_only) == 2 && mwx_stt_stream_vad_active(&e_trim) == 2);

    // ---- the gate substitution: same events, no whole-buffer gate run --------
    const auto f_talk = cadence(talk.size(), step);
    const Events want_talk = run(e_gate, talk, f_talk);
    CHECK(e_gate.vad_gate_runs() > 0 && g_vad_single_calls == e_gate.vad_gate_runs());
    CHECK(count(want_talk, false, 3) == 0);                 // gate closed on the first partials
    CHECK(count(want_talk, false, want_talk.size()) > 0);   // ... and open later
    CHECK(count(want_talk, true, want_talk.size()) > 0);
    const int single_before = g_vad_single_calls;
    CHECK(run(e_sv, talk, f_talk) == want_talk);
    CHECK(e_sv.vad_gate_runs() == 0 && g_vad_single_calls == single_before);
    CHECK(g_stream_last_threshold_milli == 750 && g_stream_last_min_silence_ms == 100);
    // the stream restarts with the buffer: after the empty chunk and after the
    // 30-s rule only silence follows, and the gate must close again
    {
      auto f = cadence(talk.size(), step);
      const auto quiet = clip(2 * 16000, {});
      auto pcm = talk;
      pcm.insert(pcm.end(), quiet.begin(), quiet.end());
      for (size_t k : cadence(quiet.size(), step)) f.push_back(k);
      const int resets = g_stream_resets;
      const Events want = run(e_gate, pcm, f);
      CHECK(run(e_sv, pcm, f) == want);
      CHECK(g_stream_resets == resets + 2);
      CHECK(count(want, false, want.size()) == count(want_talk, false, want_talk.size()));
    }
    {
      const auto f = cadence(longc.size(), step);
      const int resets = g_stream_resets;
      const Events want = run(e_gate, longc, f);
      CHECK(run(e_sv, longc, f) == want);
      CHECK(g_stream_resets == resets + 2);  // the 30-s restart and the empty chunk
      size_t forced = 0;                     // finals before the empty chunk: the 30-s rule
      for (size_t i = 0; i + 1 < want.size(); ++i)
        for (const Ev& e : want[i]) forced += e.is_final;
      CHECK(forced > 0);
    }

    // ---- endpointing -----------------------------------------------------------
    for (SttEngine* e : {&e_ep, &e_ep_only}) {
      std::vector<std::pair<size_t, size_t>> cuts;
      const Events want = model(e_gate, talk, f_talk, step, &cuts);
      const Events got = run(*e, talk, f_talk);
      CHECK(got == want);
      CHECK(cuts.size() == 2 && cuts[0].first % 512 == 0 && cuts[0].second > 0);
      CHECK(count(got, true, got.size() - 1) > 0);  // an endpoint final before the empty chunk
      CHECK(!(got == want_talk));
    }
    CHECK(g_stream_last_min_silence_ms == kSilenceMs);
    CHECK(e_ep.vad_gate_runs() == 0 && e_ep_only.vad_gate_runs() > 0);
    {
      // one feed closes two segments: one cut at the second one's closed_at
      std::vector<std::pair<size_t, size_t>> cuts;
      const std::vector<size_t> f = {burst.size(), 0};
      const Events want = model(e_gate, burst, f, step, &cuts);
      const int resets = g_stream_resets;
      CHECK(run(e_ep, burst, f) == want);
      // (3200 samples of silence are reached in the 7th silent chunk, index 127)
      CHECK(cuts.size() == 1 && cuts[0].first == (size_t)(127 + 1) * 512 && cuts[0].second > 0);
      CHECK(g_stream_resets == resets + 2);  // the cut and the empty chunk
      CHECK(!want[0].empty() && want[0][0].is_final);
    }
    {
      // vad_trim active: endpointing on, decodes through the trim path
      const Events got = run(e_trim, talk, f_talk);
      CHECK(count(got, true, got.size() - 1) > 0);
    }

    // ---- a failing stream call: the session goes on without its stream -------
    {
      auto bad = talk;
      bad[20000] = -30000;  // the stand-in's feed fails on it; the gate's call does not
      const int live = g_stream_live;
      CHECK(run(e_sv, bad, f_talk) == run(e_gate, bad, f_talk));
      CHECK(g_stream_live == live);
    }

    // ---- several sessions from several threads ---------------------------------
    {
      const Events want_ep = run(e_ep, talk, f_talk);
      std::vector<std::thread> th;
      for (int t = 0; t < 4; ++t)
        th.emplace_back([&, t] {
          for (int rep = 0; rep < 3; ++rep) {
            if (t % 2)
              CHECK(run(e_sv, talk, f_talk) == want_talk);
            else
              CHECK(run(e_ep, talk, f_talk) == want_ep);
          }
        });
      for (auto& t : th) t.join();
      // each engine has a context and a mutex of its own; the stand-ins count
      // overlaps over all of them, so the engines ran one after the other above
      // and only here side by side: an overlap between two engines is no fault
    }
    {
      const int overlaps = g_vad_overlaps;
      std::vector<std::thread> th;
      for (int t = 0; t < 4; ++t)
        th.emplace_back([&] {
          for (int rep = 0; rep < 3; ++rep) CHECK(run(e_sv, talk, f_talk) == want_talk);
        });
      for (auto& t : th) t.join();
      CHECK(g_vad_overlaps == overlaps);  // one engine: its mutex serializes every stream call
    }
    CHECK(g_stream_live == 0);  // every session freed its stream
#else
    // a library without the stream calls: both settings are inert
    for (SttEngine* e : {&e_sv, &e_ep, &e_ep_only, &e_trim})
      CHECK(mwx_stt_stream_vad_active(e) == 0);
    const auto f_talk = cadence(talk.size(), step);
    const Events want_talk = run(e_gate, talk, f_talk);
    CHECK(count(want_talk, false, want_talk.size()) > 0);
    CHECK(run(e_sv, talk, f_talk) == want_talk);
    CHECK(run(e_ep, talk, f_talk) == want_talk);
    CHECK(run(e_ep_only, talk, f_talk) == want_talk);
    CHECK(e_sv.vad_gate_runs() > 0 && e_ep.vad_gate_runs() > 0);
    CHECK(run(e_ep, longc, cadence(longc.size(), step)) ==
          run(e_gate, longc, cadence(longc.size(), step)));
    std::vector<std::thread> th;
    for (int t = 0; t < 4; ++t)
      th.emplace_back([&] { CHECK(run(e_ep, talk, f_talk) == want_talk); });
    for (auto& t : th) t.join();
#endif
    CHECK(run(e_none, talk, cadence(talk.size(), step)) ==
          run(*std::unique_ptr<SttEngine>(new SttEngine(base)), talk, cadence(talk.size(), step)));
  }
  std::printf("host_stream_check: %d failure(s)\n", failures.load());
  return failures ? 1 : 0;
}
