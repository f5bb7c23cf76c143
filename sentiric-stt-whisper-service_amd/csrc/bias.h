// Contextual biasing: the matcher tables of a call's boosted
// phrases and the transition every side uses (the advance kernels in
// k_misc.hip, the host replay in driver.inc, the bias kernel in k_bias.hip).
//
// The tables are the phrases' trie with Aho-Corasick failure links, as one
// block of 32-bit words (the same block on the host and on the device):
//   [0] S = states (root = 0)   [1] E = edges = S - 1   [2], [3] = 0
//   off[S + 1]  a state's edges are off[s] .. off[s + 1], sorted by token
//   fail[S]     the state of the longest proper suffix that is a phrase prefix
//   etok[E]     the edge's token
//   edst[E]     the state it leads to
//   eboost[E]   float: the largest boost of the phrases through that state
// S <= total phrase tokens + 1, so the block is at most
// bias_table_bound(total) = 32 + 20 * total bytes: linear in the phrases'
// tokens, whatever the root's fan-out and however the phrases overlap.
//
// A row's state is the trie node of the longest suffix of its history that is
// a prefix of some phrase. Its matches (p, k >= 1) are the nodes on its
// failure chain (at most MWX_BIAS_MAX_TOKENS of them: depths fall strictly),
// and k = 0 is the root: bias[t] = max of eboost over the chain's edges on t.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MWX_BIAS_HD __host__ __device__
#else
#define MWX_BIAS_HD
#endif

namespace mwx {

constexpr int kBiasMaxChain = 17;  // MWX_BIAS_MAX_TOKENS states + the root

struct BiasView {
  int S, E;
  const int *off, *fail, *etok, *edst;
  const float* eboost;
};
MWX_BIAS_HD inline BiasView bias_view(const int* t) {
  BiasView v;
  v.S = t[0];
  v.E = t[1];
  v.off = t + 4;
  v.fail = v.off + v.S + 1;
  v.etok = v.fail + v.S;
  v.edst = v.etok + v.E;
  v.eboost = reinterpret_cast<const float*>(v.edst + v.E);
  return v;
}
// the edge of state s on token id, or -1
MWX_BIAS_HD inline int bias_find(const BiasView& v, int s, int id) {
  int lo = v.off[s], hi = v.off[s + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int t = v.etok[mid];
    if (t == id) return mid;
    if (t < id)
      lo = mid + 1;
    else
      hi = mid;
  }
  return -1;
}
// The state after `id` is appended to a history in state s. No tables (a call
// without phrases): the root, always.
MWX_BIAS_HD inline int bias_next_state(const int* tables, int s, int id) {
  if (!tables) return 0;
  const BiasView v = bias_view(tables);
  if (s < 0 || s >= v.S) s = 0;
  for (int hop = 0; hop < kBiasMaxChain; ++hop) {
    const int e = bias_find(v, s, id);
    if (e >= 0) return v.edst[e];
    if (s == 0) return 0;
    s = v.fail[s];
  }
  return 0;
}

}  // namespace mwx

#if !defined(MWX_BIAS_NO_HOST)
#include <vector>

#include "mwx.h"

namespace mwx {

inline size_t bias_table_bound(size_t total_tokens) { return 32 + 20 * total_tokens; }

// mwx_full_params.bias_phrases / n_bias_phrases: 0 when the call may run
// (also when there are none), -1 or -3 as mwx.h lists them. eot: the first id
// no phrase may hold (mwx_token_eot).
int bias_validate(const mwx_bias_phrase* phrases, int n, int eot, const char** why = nullptr);
// The table block of validated phrases (empty for n == 0).
std::vector<int32_t> bias_build(const mwx_bias_phrase* phrases, int n);
// The state after the history h[0..n) from the root. Only the last
// MWX_BIAS_MAX_TOKENS ids can matter (no phrase prefix is longer).
int bias_walk(const std::vector<int32_t>& tables, const int* h, int n);
// The (token, bias) pairs of a state, tokens ascending.
void bias_state_set(const std::vector<int32_t>& tables, int state, std::vector<int>& tokens,
                    std::vector<float>& boosts);

}  // namespace mwx
#endif
