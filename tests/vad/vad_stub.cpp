// TEST INFRASTRUCTURE ONLY — CPU stand-ins for the mwx_vad_* entry points,
// linked next to tests/san/mwx_stub.cpp into host_vad_check (tests/vad/Makefile)
// and nowhere else. The "model" is any readable file; the probability of
// chunk i of a clip is the clip's sample 512 * i clamped to [0, 1], so a test
// dictates every probability exactly.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <vector>

#include "mwx.h"

struct mwx_vad_context {
  std::vector<float> probs;
};

std::atomic<int> g_vad_single_calls{0}, g_vad_batch_calls{0}, g_vad_in_call{0}, g_vad_overlaps{0};

namespace {

void chunk_probs(const float* x, int n, float* out) {
  for (int i = 0; i < mwx_vad_n_chunks(n); ++i) out[i] = std::min(1.0f, std::max(0.0f, x[512 * i]));
}

// one call at a time per context: the host must hold its mutex
struct CallGuard {
  CallGuard() {
    if (g_vad_in_call.fetch_add(1) != 0) ++g_vad_overlaps;
  }
  ~CallGuard() { g_vad_in_call.fetch_sub(1); }
};

}  // namespace

extern "C" {

mwx_vad_context_params mwx_vad_default_context_params(void) {
  mwx_vad_context_params p;
  p.n_threads = 4;
  p.use_gpu = true;
  p.gpu_device = 0;
  return p;
}

mwx_vad_context* mwx_vad_init_from_file_with_params(const char* path, mwx_vad_context_params params) {
  if (!path || !params.use_gpu) return nullptr;
  FILE* f = std::fopen(path, "rb");
  if (!f) return nullptr;
  std::fclose(f);
  return new mwx_vad_context();
}

void mwx_vad_free(mwx_vad_context* v) { delete v; }

int mwx_vad_n_chunks(int n_samples) { return n_samples <= 0 ? 0 : (n_samples + 511) / 512; }

bool mwx_vad_detect_speech(mwx_vad_context* v, const float* x, int n) {
  if (!v || n < 0 || (n > 0 && !x)) return false;
  CallGuard g;
  ++g_vad_single_calls;
  if (n > 0 && x[0] < 0.0f) return false;  // a first sample below zero: a failing call
  v->probs.assign((size_t)mwx_vad_n_chunks(n), 0.0f);
  chunk_probs(x, n, v->probs.data());
  return true;
}

int mwx_vad_n_probs(mwx_vad_context* v) { return v ? (int)v->probs.size() : 0; }
const float* mwx_vad_probs(mwx_vad_context* v) { return v && !v->probs.empty() ? v->probs.data() : nullptr; }

int mwx_vad_detect_speech_batch(mwx_vad_context* v, const float* const* x, const int* n, int n_clips,
                                float* out, const int* off) {
  if (!v || n_clips < 0) return -1;
  CallGuard g;
  ++g_vad_batch_calls;
  for (int b = 0; b < n_clips; ++b) chunk_probs(x[b], n[b], out + off[b]);
  return 0;
}

}  // extern "C"
