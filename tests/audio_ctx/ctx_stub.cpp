// TEST INFRASTRUCTURE ONLY — the two decode entry points of the Whisper stand-in
// (tests/san/mwx_stub.cpp, compiled with them renamed to stub_full_*:
// tests/audio_ctx/Makefile), defined here so that every call's audio-context
// params are seen: the counters say how many calls came with which
// (audio_ctx, audio_ctx_fit), the decode itself is the stand-in's.
#include <atomic>

#include "mwx.h"

std::atomic<int> g_ctx_calls{0}, g_ctx_batch_calls{0}, g_ctx_last_audio_ctx{-1},
    g_ctx_last_fit{-1}, g_ctx_mismatch{0}, g_ctx_want_audio_ctx{0}, g_ctx_want_fit{0};

extern "C" {

int stub_full_with_state(mwx_context* ctx, mwx_state* st, mwx_full_params p, const float* x, int n);
int stub_full_batch(mwx_context* ctx, mwx_state* const* states, mwx_full_params p,
                    const float* const* x, const int* n, int n_clips);

static void note(const mwx_full_params& p) {
  g_ctx_last_audio_ctx = p.audio_ctx;
  g_ctx_last_fit = p.audio_ctx_fit ? 1 : 0;
  if (p.audio_ctx != g_ctx_want_audio_ctx || (p.audio_ctx_fit ? 1 : 0) != g_ctx_want_fit)
    ++g_ctx_mismatch;
}

int mwx_full_with_state(mwx_context* ctx, mwx_state* st, mwx_full_params p, const float* x, int n) {
  ++g_ctx_calls;
  note(p);
  return stub_full_with_state(ctx, st, p, x, n);
}

int mwx_full_batch(mwx_context* ctx, mwx_state* const* states, mwx_full_params p,
                   const float* const* x, const int* n, int n_clips) {
  ++g_ctx_batch_calls;
  note(p);
  return stub_full_batch(ctx, states, p, x, n, n_clips);
}

}  // extern "C"
