// TEST INFRASTRUCTURE ONLY — the CPU stand-in tests/san/mwx_stub.cpp with the
// language-probability calls (mwx_full_lang_probs_from_state, mwx_lang_max_id)
// and the two lookups the host binds with them (mwx_full_lang_id_from_state,
// mwx_lang_str). It identifies nothing: a call that detects gives one of two
// fixed five-language distributions, chosen by the clip's first sample, so
// tests/lang/host_lang_check.cpp can state what the host must make of it.
// Linked into that program only.
#include "mwx.h"

// (the stand-in's two transcription calls are wrapped below: they record the
// call's parameters and what the state then reports)
#define mwx_full_with_state stub_base_full_with_state
#define mwx_full_batch stub_base_full_batch
#include "../san/mwx_stub.cpp"
#undef mwx_full_with_state
#undef mwx_full_batch

#include <map>
#include <mutex>

int g_lang_calls = 0;          // engine calls (both entry points)
int g_lang_detect_calls = 0;   // ... with detect_language set
mwx_full_params g_lang_params; // of the last call
std::string g_lang_language;   // its language string

namespace {
const int kLangs = 5;
const char* const kLangStr[kLangs] = {"en", "de", "tr", "fr", "es"};
// ties at 0.4 (ids 1 and 3) and at 0.1 (ids 0 and 2): the order among equals
const float kProbsA[kLangs] = {0.1f, 0.4f, 0.1f, 0.4f, 0.0f};
const float kProbsB[kLangs] = {0.05f, 0.05f, 0.7f, 0.2f, 0.0f};
struct Info {
  int lang = 0;
  std::vector<float> probs;
};
std::mutex g_lmu;
std::map<mwx_state*, Info> g_info;

bool is_auto(const mwx_full_params& p) {
  return !p.language || !*p.language || std::string(p.language) == "auto";
}

int after(mwx_state* st, const mwx_full_params& p, const float* x, int n, int rc) {
  std::lock_guard<std::mutex> lock(g_lmu);
  ++g_lang_calls;
  g_lang_detect_calls += p.detect_language ? 1 : 0;
  g_lang_params = p;
  g_lang_language = p.language ? p.language : "";
  Info& in = g_info[st];
  in.probs.clear();
  if (is_auto(p) || p.detect_language) {
    const float* t = (x && n > 0 && x[0] > 0.5f) ? kProbsB : kProbsA;
    in.probs.assign(t, t + kLangs);
    in.lang = t == kProbsB ? 2 : 1;
  } else {
    in.lang = 0;
    for (int k = 0; k < kLangs; ++k)
      if (std::string(p.language) == kLangStr[k]) in.lang = k;
  }
  if (p.detect_language) st->segs.clear();  // detection only
  return rc;
}
}  // namespace

extern "C" {

int mwx_full_with_state(mwx_context* ctx, mwx_state* st, mwx_full_params p, const float* x, int n) {
  const int rc = stub_base_full_with_state(ctx, st, p, x, n);
  return st ? after(st, p, x, n, rc) : rc;
}

int mwx_full_batch(mwx_context* ctx, mwx_state* const* states, mwx_full_params p,
                   const float* const* x, const int* n, int n_clips) {
  const int rc = stub_base_full_batch(ctx, states, p, x, n, n_clips);
  for (int b = 0; b < n_clips && rc == 0; ++b) after(states[b], p, x[b], n[b], rc);
  return rc;
}

int mwx_lang_max_id(void) { return kLangs - 1; }
const char* mwx_lang_str(int id) { return id >= 0 && id < kLangs ? kLangStr[id] : nullptr; }
int mwx_full_lang_id_from_state(mwx_state* st) {
  std::lock_guard<std::mutex> lock(g_lmu);
  return g_info[st].lang;
}
int mwx_full_lang_probs_from_state(mwx_state* st, float* probs, int n) {
  if (!st || !probs || n < kLangs) return -1;
  std::lock_guard<std::mutex> lock(g_lmu);
  const Info& in = g_info[st];
  for (size_t k = 0; k < in.probs.size(); ++k) probs[k] = in.probs[k];
  return (int)in.probs.size();
}

}  // extern "C"
