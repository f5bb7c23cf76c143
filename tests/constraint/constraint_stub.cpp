// TEST INFRASTRUCTURE ONLY — the CPU stand-in tests/san/mwx_stub.cpp with its
// two transcription calls wrapped so that they record the call's constraint
// (walked during the call: reading it there is what proves the host kept it
// alive) and its penalty, and the status query the host reads afterwards. The
// constraint itself is the real one: csrc/constraint.cpp is linked in.
// Linked into tests/constraint/host_constraint_check.cpp only.
#include "mwx.h"

#define mwx_full_with_state stub_base_full_with_state
#define mwx_full_batch stub_base_full_batch
#include "../san/mwx_stub.cpp"
#undef mwx_full_with_state
#undef mwx_full_batch

#include <mutex>

int g_con_calls = 0;                       // engine calls (both entry points)
int g_con_clips = 0;                       // clips of the last call
const mwx_constraint* g_con_ptr = nullptr; // the last call's constraint
float g_con_penalty = 0.0f;                // ... and penalty
int g_con_states = 0;                      // its states (0 without one)
int g_con_yes = -1;                        // is "yes" accepted by it (-1 without one)
bool g_con_no_ts = false;                  // the last call's no_timestamps

namespace {
std::mutex g_cmu;
void record(const mwx_full_params& p, int n_clips) {
  std::lock_guard<std::mutex> lock(g_cmu);
  ++g_con_calls;
  g_con_clips = n_clips;
  g_con_ptr = p.constraint;
  g_con_penalty = p.constraint_penalty;
  g_con_no_ts = p.no_timestamps;
  g_con_states = p.constraint ? mwx_constraint_n_states(p.constraint) : 0;
  g_con_yes = -1;
  if (p.constraint) {
    const int s = mwx_constraint_walk(p.constraint, mwx_constraint_start(p.constraint),
                                      (const uint8_t*)"yes", 3);
    g_con_yes = mwx_constraint_accepting(p.constraint, s);
  }
}
}  // namespace

extern "C" {

int mwx_full_with_state(mwx_context* ctx, mwx_state* st, mwx_full_params p, const float* x, int n) {
  record(p, 1);
  return stub_base_full_with_state(ctx, st, p, x, n);
}

int mwx_full_batch(mwx_context* ctx, mwx_state* const* states, mwx_full_params p,
                   const float* const* x, const int* n, int n_clips) {
  record(p, n_clips);
  return stub_base_full_batch(ctx, states, p, x, n, n_clips);
}

// the stand-in decodes nothing: a call with a constraint reports a match
int mwx_full_constraint_status_from_state(mwx_state*) { return g_con_ptr ? 1 : -1; }

}  // extern "C"
