// TEST INFRASTRUCTURE ONLY — CPU stand-ins for the trimming entry points the host
// SttEngine binds (mwx_vad_default_params, mwx_vad_trim_batch,
// mwx_vad_trimmed_n_segments, mwx_vad_trimmed_free, mwx_full_batch_trimmed),
// linked next to tests/vad/vad_stub.cpp and tests/san/mwx_stub.cpp into
// host_trim_check (tests/vad_trim/Makefile) and nowhere else. The probability
// of chunk i is the clip's sample 512 * i, as in vad_stub.cpp; the stand-in
// "rule" keeps exactly the chunks at or above the threshold, a segment being a
// run of them, and the trimmed decode is the stub's mwx_full_batch over the
// kept samples (times are not mapped here: the map is the library's, checked on
// the GPU).
#include <algorithm>
#include <atomic>
#include <vector>

#include "mwx.h"

struct mwx_vad_trimmed {
  std::vector<std::vector<float>> pcm;
  std::vector<int> n_seg;
};

extern std::atomic<int> g_vad_in_call, g_vad_overlaps;
std::atomic<int> g_trim_calls{0}, g_trim_clips{0}, g_trim_live{0}, g_trimmed_decodes{0};

extern "C" {

mwx_vad_params mwx_vad_default_params(void) {
  mwx_vad_params p;
  p.threshold = 0.5f;
  p.min_speech_duration_ms = 250;
  p.min_silence_duration_ms = 100;
  p.max_speech_duration_s = 3.402823466e+38f;
  p.speech_pad_ms = 30;
  p.samples_overlap = 0.1f;
  return p;
}

mwx_vad_trimmed* mwx_vad_trim_batch(mwx_vad_context* v, mwx_vad_params p, const float* const* x,
                                    const int* n, int n_clips) {
  if (!v || n_clips < 0) return nullptr;
  if (g_vad_in_call.fetch_add(1) != 0) ++g_vad_overlaps;  // one call at a time per context
  ++g_trim_calls;
  g_trim_clips += n_clips;
  mwx_vad_trimmed* t = new mwx_vad_trimmed();
  bool fail = false;
  for (int b = 0; b < n_clips; ++b) {
    if (n[b] > 0 && x[b][0] < 0.0f) fail = true;  // a first sample below zero: a failing call
    std::vector<float> kept;
    int segs = 0;
    bool in = false;
    for (int i = 0; i * 512 < n[b]; ++i) {
      const bool speech = std::min(1.0f, std::max(0.0f, x[b][512 * i])) >= p.threshold;
      if (speech) kept.insert(kept.end(), x[b] + 512 * i, x[b] + std::min(n[b], 512 * i + 512));
      segs += speech && !in;
      in = speech;
    }
    t->pcm.push_back(std::move(kept));
    t->n_seg.push_back(segs);
  }
  g_vad_in_call.fetch_sub(1);
  if (fail) {
    delete t;
    return nullptr;
  }
  ++g_trim_live;
  return t;
}

int mwx_vad_trimmed_n_segments(const mwx_vad_trimmed* t, int clip) {
  return t && clip >= 0 && (size_t)clip < t->n_seg.size() ? t->n_seg[clip] : -1;
}

void mwx_vad_trimmed_free(mwx_vad_trimmed* t) {
  if (!t) return;
  --g_trim_live;
  delete t;
}

int mwx_full_batch_trimmed(mwx_context* ctx, mwx_state* const* states, mwx_full_params params,
                           const mwx_vad_trimmed* const* trimmed, const int* clip_index,
                           int n_clips) {
  if (!ctx || n_clips <= 0) return -1;
  static const float none = 0.0f;
  std::vector<const float*> ptrs;
  std::vector<int> lens;
  for (int b = 0; b < n_clips; ++b) {
    const mwx_vad_trimmed* t = trimmed[b];
    if (!t || clip_index[b] < 0 || (size_t)clip_index[b] >= t->pcm.size()) return -1;
    const std::vector<float>& c = t->pcm[clip_index[b]];
    ptrs.push_back(c.empty() ? &none : c.data());
    lens.push_back((int)c.size());
  }
  ++g_trimmed_decodes;
  return mwx_full_batch(ctx, states, params, ptrs.data(), lens.data(), n_clips);
}

}  // extern "C"
