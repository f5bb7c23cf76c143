// TEST INFRASTRUCTURE ONLY — CPU stand-ins for the chunked entry points the host
// SttEngine binds (mwx_vad_trim_batch_chunked, mwx_vad_trimmed_n_chunks,
// mwx_full_batch_chunked), linked next to tests/vad_trim/trim_stub.cpp,
// tests/vad/vad_stub.cpp and tests/san/mwx_stub.cpp into host_chunk_check
// (tests/vad_chunk/Makefile) and nowhere else. The trim pass is trim_stub.cpp's;
// the stand-in "plan" is one chunk per segment, and the chunked decode is the
// stub's mwx_full_batch over the kept samples, as trim_stub.cpp's trimmed decode
// (the plan, the stitching and the time map are the library's, checked on the
// GPU). What the host passed in is recorded for host_chunk_check.
#include <atomic>
#include <vector>

#include "mwx.h"

struct mwx_vad_trimmed {  // (trim_stub.cpp's, token for token)
  std::vector<std::vector<float>> pcm;
  std::vector<int> n_seg;
};

std::atomic<int> g_chunk_trim_calls{0}, g_chunked_decodes{0}, g_chunk_bad_args{0};
// the last values seen, in thousandths: chunk_s, max_speech_duration_s; max_batch
std::atomic<int> g_chunk_last_s_milli{0}, g_chunk_last_max_speech_milli{0}, g_chunk_last_batch{0};

extern "C" {

mwx_vad_trimmed* mwx_vad_trim_batch_chunked(mwx_vad_context* v, mwx_vad_params p, float chunk_s,
                                            const float* const* x, const int* n, int n_clips) {
  if (chunk_s != chunk_s || !(chunk_s >= 1.0f && chunk_s <= 30.0f)) {
    ++g_chunk_bad_args;
    return nullptr;
  }
  ++g_chunk_trim_calls;
  g_chunk_last_s_milli = (int)(chunk_s * 1000.0f + 0.5f);
  g_chunk_last_max_speech_milli =
      p.max_speech_duration_s > 1.0e6f ? -1 : (int)(p.max_speech_duration_s * 1000.0f + 0.5f);
  return mwx_vad_trim_batch(v, p, x, n, n_clips);
}

int mwx_vad_trimmed_n_chunks(const mwx_vad_trimmed* t, int clip) {
  return t && clip >= 0 && (size_t)clip < t->n_seg.size() ? t->n_seg[clip] : -1;
}

int mwx_full_batch_chunked(mwx_context* ctx, mwx_state* const* states, mwx_full_params params,
                           const mwx_vad_trimmed* const* trimmed, const int* clip_index,
                           int n_clips, int max_batch) {
  if (!ctx || n_clips <= 0 || max_batch < 1 || params.offset_ms != 0 || params.duration_ms != 0) {
    ++g_chunk_bad_args;
    return -1;
  }
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
  ++g_chunked_decodes;
  g_chunk_last_batch = max_batch;
  return mwx_full_batch(ctx, states, params, ptrs.data(), lens.data(), n_clips);
}

}  // extern "C"
