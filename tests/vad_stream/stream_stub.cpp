// TEST INFRASTRUCTURE ONLY — CPU stand-ins for the mwx_vad_stream_* entry points,
// linked next to tests/vad/vad_stub.cpp and tests/san/mwx_stub.cpp into
// host_stream_check (tests/vad_stream/Makefile) and nowhere else. As in
// vad_stub.cpp the probability of chunk i of a stream is its sample 512 * i
// clamped to [0, 1] (so a partial last chunk has its probability from its first
// sample on, and a stream's probabilities are those of mwx_vad_detect_speech
// over the same audio); the segments are rule D7's scan over the whole chunks,
// one chunk per step. A fed sample below -0.5 makes the call fail.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "mwx.h"

extern std::atomic<int> g_vad_in_call, g_vad_overlaps;  // vad_stub.cpp: one call at a time
std::atomic<int> g_stream_live{0}, g_stream_inits{0}, g_stream_feeds{0}, g_stream_resets{0};
std::atomic<int> g_stream_last_min_silence_ms{-1};
std::atomic<int> g_stream_last_threshold_milli{-1};

struct mwx_vad_stream {
  mwx_vad_context* ctx;
  float thr, neg;
  int64_t min_speech, min_sil;
  std::vector<float> probs;
  int64_t n_samples = 0;
  size_t scanned = 0;
  bool trig = false, finished = false;
  int64_t start = 0, temp_end = 0;
  std::vector<int64_t> seg;
};

namespace {

struct CallGuard {
  CallGuard() {
    if (g_vad_in_call.fetch_add(1) != 0) ++g_vad_overlaps;
  }
  ~CallGuard() { g_vad_in_call.fetch_sub(1); }
};

void clear(mwx_vad_stream* s) {
  s->probs.clear();
  s->n_samples = 0;
  s->scanned = 0;
  s->trig = s->finished = false;
  s->start = s->temp_end = 0;
  s->seg.clear();
}

// the rule without max_speech_duration_s (the host leaves it at its default)
void scan(mwx_vad_stream* s) {
  const size_t whole = (size_t)(s->n_samples / 512);
  for (; s->scanned < whole; ++s->scanned) {
    const float p = s->probs[s->scanned];
    const int64_t cur = 512 * (int64_t)s->scanned;
    if (p >= s->thr && s->temp_end != 0) s->temp_end = 0;
    if (p >= s->thr && !s->trig) {
      s->trig = true;
      s->start = cur;
      continue;
    }
    if (p < s->neg && s->trig) {
      if (s->temp_end == 0) s->temp_end = cur;
      if (cur - s->temp_end < s->min_sil) continue;
      if (s->temp_end - s->start > s->min_speech) {
        const int64_t e[3] = {s->start, s->temp_end, cur + 512};
        s->seg.insert(s->seg.end(), e, e + 3);
      }
      s->temp_end = 0;
      s->trig = false;
    }
  }
}

}  // namespace

extern "C" {

// (mwx_vad_default_params: tests/vad_trim/trim_stub.cpp)
mwx_vad_stream* mwx_vad_stream_init(mwx_vad_context* v, mwx_vad_params p) {
  if (!v || !(p.threshold > 0.0f && p.threshold < 1.0f) || p.min_silence_duration_ms < 0)
    return nullptr;
  CallGuard g;
  mwx_vad_stream* s = new mwx_vad_stream();
  s->ctx = v;
  s->thr = p.threshold;
  s->neg = std::max(p.threshold - 0.15f, 0.01f);
  s->min_speech = 16LL * p.min_speech_duration_ms;
  s->min_sil = 16LL * p.min_silence_duration_ms;
  g_stream_last_min_silence_ms = p.min_silence_duration_ms;
  g_stream_last_threshold_milli = (int)std::lround(p.threshold * 1000.0f);
  ++g_stream_live;
  ++g_stream_inits;
  return s;
}

void mwx_vad_stream_free(mwx_vad_stream* s) {
  if (!s) return;
  CallGuard g;
  --g_stream_live;
  delete s;
}

int mwx_vad_stream_reset(mwx_vad_stream* s) {
  if (!s) return -1;
  CallGuard g;
  ++g_stream_resets;
  clear(s);
  return 0;
}

int mwx_vad_stream_feed_batch(mwx_vad_context* v, mwx_vad_stream* const* streams,
                              const float* const* x, const int* n, int n_streams) {
  if (!v || n_streams < 0) return -1;
  CallGuard g;
  ++g_stream_feeds;
  for (int i = 0; i < n_streams; ++i) {
    mwx_vad_stream* s = streams[i];
    if (!s || s->ctx != v || s->finished || n[i] < 0 || n[i] > 480000) return -2;
    for (int k = 0; k < n[i]; ++k)
      if (x[i][k] < -0.5f) return -4;
  }
  for (int i = 0; i < n_streams; ++i) {
    mwx_vad_stream* s = streams[i];
    for (int k = 0; k < n[i]; ++k, ++s->n_samples)
      if (s->n_samples % 512 == 0) s->probs.push_back(std::min(1.0f, std::max(0.0f, x[i][k])));
    scan(s);
  }
  return 0;
}

int mwx_vad_stream_n_probs(const mwx_vad_stream* s) { return s ? (int)s->probs.size() : 0; }
const float* mwx_vad_stream_probs(const mwx_vad_stream* s) {
  return s && !s->probs.empty() ? s->probs.data() : nullptr;
}
float mwx_vad_stream_max_prob(const mwx_vad_stream* s) {
  float m = 0.0f;
  if (s)
    for (float p : s->probs) m = std::max(m, p);
  return m;
}
int mwx_vad_stream_n_segments(const mwx_vad_stream* s) { return s ? (int)(s->seg.size() / 3) : 0; }
int mwx_vad_stream_segment(const mwx_vad_stream* s, int i, int64_t* s0, int64_t* s1,
                           int64_t* closed_at) {
  if (!s || i < 0 || 3 * (size_t)i + 2 >= s->seg.size()) return -1;
  if (s0) *s0 = s->seg[3 * (size_t)i];
  if (s1) *s1 = s->seg[3 * (size_t)i + 1];
  if (closed_at) *closed_at = s->seg[3 * (size_t)i + 2];
  return 0;
}

}  // extern "C"
