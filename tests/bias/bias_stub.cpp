// TEST INFRASTRUCTURE ONLY — the CPU stand-in tests/san/mwx_stub.cpp with its
// two transcription calls wrapped so that they record the call's contextual-
// biasing phrases (a deep copy of mwx_full_params.bias_phrases: reading them
// during the call is what proves the host kept the arrays alive), and a
// tokenizer: one token per byte of the text (id = the byte), so " word" is one
// token longer than "word" and a word of more than 16 bytes has too many.
// Linked into tests/bias/host_bias_check.cpp only.
#include "mwx.h"

#define mwx_full_with_state stub_base_full_with_state
#define mwx_full_batch stub_base_full_batch
#include "../san/mwx_stub.cpp"
#undef mwx_full_with_state
#undef mwx_full_batch

#include <mutex>

struct BiasSeen {
  std::vector<mwx_token> ids;
  float boost;
};
int g_bias_calls = 0;                 // engine calls (both entry points)
int g_bias_clips = 0;                 // clips of the last call
bool g_bias_null = true;              // the last call's bias_phrases == NULL
std::vector<BiasSeen> g_bias_seen;    // the last call's phrases

namespace {
std::mutex g_bmu;
void record(const mwx_full_params& p, int n_clips) {
  std::lock_guard<std::mutex> lock(g_bmu);
  ++g_bias_calls;
  g_bias_clips = n_clips;
  g_bias_null = p.bias_phrases == nullptr;
  g_bias_seen.clear();
  for (int i = 0; i < p.n_bias_phrases && p.bias_phrases; ++i) {
    const mwx_bias_phrase& b = p.bias_phrases[i];
    g_bias_seen.push_back({std::vector<mwx_token>(b.tokens, b.tokens + b.n_tokens), b.boost});
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

int mwx_tokenize(mwx_context* ctx, const char* text, mwx_token* tokens, int n_max_tokens) {
  if (!ctx || !text) return 0;
  const int n = (int)std::strlen(text);
  if (n > n_max_tokens) return -n;
  for (int i = 0; i < n; ++i) tokens[i] = (unsigned char)text[i];
  return n;
}

}  // extern "C"
