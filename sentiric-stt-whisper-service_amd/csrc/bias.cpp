// Contextual biasing: validation of a call's phrases and the
// matcher tables (bias.h). Host only.
#include "bias.h"

#include "mwx_test.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

namespace mwx {

int bias_validate(const mwx_bias_phrase* phrases, int n, int eot, const char** why) {
  const char* dummy;
  const char*& w = why ? *why : dummy;
  w = "";
  if (n < 0 || n > MWX_BIAS_MAX_PHRASES) {
    w = "n_bias_phrases outside 0 .. MWX_BIAS_MAX_PHRASES";
    return -1;
  }
  if (n > 0 && !phrases) {
    w = "n_bias_phrases > 0 with bias_phrases == NULL";
    return -1;
  }
  for (int p = 0; p < n; ++p) {
    if (phrases[p].n_tokens < 1 || phrases[p].n_tokens > MWX_BIAS_MAX_TOKENS ||
        !phrases[p].tokens) {
      w = "a phrase's n_tokens outside 1 .. MWX_BIAS_MAX_TOKENS (or its tokens NULL)";
      return -1;
    }
    if (!std::isfinite(phrases[p].boost)) {
      w = "a phrase's boost is NaN or infinite";
      return -1;
    }
  }
  for (int p = 0; p < n; ++p)
    for (int k = 0; k < phrases[p].n_tokens; ++k)
      if (phrases[p].tokens[k] < 0 || phrases[p].tokens[k] >= eot) {
        w = "a phrase holds an id outside [0, eot)";
        return -3;
      }
  return 0;
}

std::vector<int32_t> bias_build(const mwx_bias_phrase* phrases, int n) {
  if (n <= 0 || !phrases) return {};
  // the trie, in insertion order
  struct Node {
    std::map<int, int> next;
    float boost = 0.0f;  // the largest boost of the phrases through this node
    bool seen = false;
    int fail = 0, id = 0;
  };
  std::vector<Node> nd(1);
  for (int p = 0; p < n; ++p) {
    int s = 0;
    for (int k = 0; k < phrases[p].n_tokens; ++k) {
      const int t = phrases[p].tokens[k];
      auto it = nd[s].next.find(t);
      int c;
      if (it == nd[s].next.end()) {
        c = (int)nd.size();
        nd[s].next.emplace(t, c);
        nd.emplace_back();
      } else {
        c = it->second;
      }
      Node& x = nd[c];
      x.boost = x.seen ? std::max(x.boost, phrases[p].boost) : phrases[p].boost;
      x.seen = true;
      s = c;
    }
  }
  // breadth-first order (a state's failure state comes before it) and links
  const int S = (int)nd.size(), E = S - 1;
  std::vector<int> order{0};
  order.reserve(S);
  for (size_t i = 0; i < order.size(); ++i) {
    const int s = order[i];
    nd[s].id = (int)i;
    for (const auto& kv : nd[s].next) {
      const int c = kv.second;
      int f = 0;
      if (s != 0) {
        f = nd[s].fail;
        for (;;) {
          auto it = nd[f].next.find(kv.first);
          if (it != nd[f].next.end()) {
            f = it->second;
            break;
          }
          if (f == 0) break;
          f = nd[f].fail;
        }
      }
      nd[c].fail = f;
      order.push_back(c);
    }
  }
  std::vector<int32_t> t(4 + (size_t)(S + 1) + S + 3 * (size_t)E, 0);
  t[0] = S;
  t[1] = E;
  int32_t* off = t.data() + 4;
  int32_t* fail = off + S + 1;
  int32_t* etok = fail + S;
  int32_t* edst = etok + E;
  int32_t* eb = edst + E;
  int e = 0;
  for (int i = 0; i < S; ++i) {
    const Node& x = nd[order[i]];
    off[i] = e;
    fail[i] = nd[x.fail].id;
    for (const auto& kv : x.next) {  // (std::map: tokens ascending)
      etok[e] = kv.first;
      edst[e] = nd[kv.second].id;
      memcpy(&eb[e], &nd[kv.second].boost, 4);
      ++e;
    }
  }
  off[S] = e;
  return t;
}

int bias_walk(const std::vector<int32_t>& tables, const int* h, int n) {
  if (tables.empty()) return 0;
  int s = 0;
  for (int i = std::max(0, n - MWX_BIAS_MAX_TOKENS); i < n; ++i)
    s = bias_next_state(tables.data(), s, h[i]);
  return s;
}

void bias_state_set(const std::vector<int32_t>& tables, int state, std::vector<int>& tokens,
                    std::vector<float>& boosts) {
  tokens.clear();
  boosts.clear();
  if (tables.empty()) return;
  const BiasView v = bias_view(tables.data());
  std::map<int, float> acc;
  int s = (state < 0 || state >= v.S) ? 0 : state;
  for (int hop = 0; hop < kBiasMaxChain; ++hop) {
    for (int e = v.off[s]; e < v.off[s + 1]; ++e) {
      auto it = acc.find(v.etok[e]);
      if (it == acc.end())
        acc.emplace(v.etok[e], v.eboost[e]);
      else
        it->second = std::max(it->second, v.eboost[e]);
    }
    if (s == 0) break;
    s = v.fail[s];
  }
  for (const auto& kv : acc) {
    tokens.push_back(kv.first);
    boosts.push_back(kv.second);
  }
}

}  // namespace mwx

// (include/mwx_test.h) the tables and the host transition on given phrases
extern "C" int mwx_test_bias_match(const struct mwx_bias_phrase* phrases, int n,
                                   const mwx_token* hist, int n_hist, mwx_token* tokens_out,
                                   float* boosts_out, int cap, long long* table_bytes_out) {
  if (n_hist < 0 || (n_hist > 0 && !hist) || cap < 0 || (cap > 0 && (!tokens_out || !boosts_out)))
    return -1;
  if (int rc = mwx::bias_validate(phrases, n, 0x7fffffff)) return rc;
  const std::vector<int32_t> tab = mwx::bias_build(phrases, n);
  if (table_bytes_out) *table_bytes_out = (long long)tab.size() * 4;
  std::vector<int> toks;
  std::vector<float> boosts;
  mwx::bias_state_set(tab, mwx::bias_walk(tab, hist, n_hist), toks, boosts);
  for (int i = 0; i < (int)toks.size() && i < cap; ++i) {
    tokens_out[i] = toks[i];
    boosts_out[i] = boosts[i];
  }
  return (int)toks.size();
}

// (include/mwx_test.h) the host's state id after hist, from the root
extern "C" int mwx_test_bias_state(const struct mwx_bias_phrase* phrases, int n,
                                   const mwx_token* hist, int n_hist) {
  if (n_hist < 0 || (n_hist > 0 && !hist)) return -1;
  if (int rc = mwx::bias_validate(phrases, n, 0x7fffffff)) return rc;
  return mwx::bias_walk(mwx::bias_build(phrases, n), hist, n_hist);
}
