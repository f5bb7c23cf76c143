// Constrained decoding: building and checking a constraint,
// its class-compressed table, the token byte table and the public host-only
// queries (constraint.h). Host only, no HIP.
#include "constraint.h"

#include "mwx_test.h"

#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

namespace mwx {

// cls / tab from raw: bytes with equal columns share a class
static void compress(mwx_constraint& c) {
  const int S = c.S;
  c.cls.assign(256, 0);
  std::map<std::vector<uint16_t>, int> seen;
  std::vector<std::vector<uint16_t>> cols;
  std::vector<uint16_t> col(S);
  for (int b = 0; b < 256; ++b) {
    for (int s = 0; s < S; ++s) col[s] = c.raw[(size_t)s * 256 + b];
    auto it = seen.find(col);
    if (it == seen.end()) {
      it = seen.emplace(col, (int)cols.size()).first;
      cols.push_back(col);
    }
    c.cls[b] = (uint8_t)it->second;
  }
  c.C = (int)cols.size();
  c.tab.assign((size_t)S * c.C, 0);
  for (int k = 0; k < c.C; ++k)
    for (int s = 0; s < S; ++s) c.tab[(size_t)s * c.C + k] = cols[k][s];
}

mwx_constraint* constraint_from_dfa(int n_states, int start, const uint16_t* trans,
                                    const uint8_t* accepting, const char** why) {
  const char* dummy;
  const char*& w = why ? *why : dummy;
  w = "";
  if (n_states < 2 || n_states > MWX_CONSTRAINT_MAX_STATES) {
    w = "n_states outside 2 .. MWX_CONSTRAINT_MAX_STATES";
    return nullptr;
  }
  if (!trans || !accepting) {
    w = "a null table";
    return nullptr;
  }
  if (start < 1 || start >= n_states) {
    w = "start outside 1 .. n_states - 1";
    return nullptr;
  }
  const int S = n_states;
  for (size_t i = 0; i < (size_t)S * 256; ++i)
    if (trans[i] >= S) {
      w = "a transition's target is >= n_states";
      return nullptr;
    }
  if (accepting[0]) {
    w = "state 0 is accepting";
    return nullptr;
  }
  for (int b = 0; b < 256; ++b)
    if (trans[b] != 0) {
      w = "state 0 has a transition away from 0";
      return nullptr;
    }
  // states reachable from the start (not through 0) ...
  std::vector<uint8_t> reach(S, 0), live(S, 0);
  std::vector<int> q{start};
  reach[start] = 1;
  for (size_t i = 0; i < q.size(); ++i)
    for (int b = 0; b < 256; ++b) {
      const int t = trans[(size_t)q[i] * 256 + b];
      if (t != 0 && !reach[t]) {
        reach[t] = 1;
        q.push_back(t);
      }
    }
  // ... and the states that can reach an accepting one (reverse edges)
  std::vector<std::vector<uint16_t>> rev(S);
  for (int s = 1; s < S; ++s) {
    int last = -1;
    for (int b = 0; b < 256; ++b) {
      const int t = trans[(size_t)s * 256 + b];
      if (t != 0 && t != last) rev[t].push_back((uint16_t)s);
      last = t;
    }
  }
  q.clear();
  for (int s = 1; s < S; ++s)
    if (accepting[s]) {
      live[s] = 1;
      q.push_back(s);
    }
  for (size_t i = 0; i < q.size(); ++i)
    for (uint16_t p : rev[q[i]])
      if (!live[p]) {
        live[p] = 1;
        q.push_back(p);
      }
  for (int s = 1; s < S; ++s)
    if (reach[s] && !live[s]) {
      w = "a state reachable from the start cannot reach an accepting state";
      return nullptr;
    }
  mwx_constraint* c = new mwx_constraint;
  c->S = S;
  c->start = start;
  c->raw.assign(trans, trans + (size_t)S * 256);
  c->acc.resize(S);
  for (int s = 0; s < S; ++s) c->acc[s] = accepting[s] ? 1 : 0;
  compress(*c);
  return c;
}

mwx_constraint* constraint_from_choices(const char* const* texts, int n, int flags,
                                        const char** why) {
  const char* dummy;
  const char*& w = why ? *why : dummy;
  w = "";
  const int known =
      MWX_CONSTRAINT_FOLD_CASE | MWX_CONSTRAINT_LEADING_SPACE | MWX_CONSTRAINT_TRAILING_PUNCT;
  if (n < 1 || !texts) {
    w = "n < 1 (or texts NULL)";
    return nullptr;
  }
  if (flags & ~known) {
    w = "unknown flag bits";
    return nullptr;
  }
  for (int i = 0; i < n; ++i)
    if (!texts[i] || !texts[i][0]) {
      w = "a null or empty text";
      return nullptr;
    }
  // the trie of every accepted string; node 0 = the start
  struct Node {
    std::array<int, 256> next;
    bool acc = false;
    Node() { next.fill(-1); }
  };
  std::vector<Node> nd(1);
  const int max_live = MWX_CONSTRAINT_MAX_STATES - 1;
  bool over = false;
  auto child = [&](int s, unsigned char b) {
    unsigned char lo = b, up = b;
    if ((flags & MWX_CONSTRAINT_FOLD_CASE) &&
        ((b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z'))) {
      lo = (unsigned char)(b | 0x20);
      up = (unsigned char)(b & ~0x20);
    }
    int c = nd[s].next[lo];
    if (c < 0) {
      if ((int)nd.size() >= max_live) {
        over = true;
        return s;
      }
      c = (int)nd.size();
      nd.emplace_back();
    }
    nd[s].next[lo] = nd[s].next[up] = c;
    return c;
  };
  auto insert = [&](int s, const char* text) {
    for (const char* p = text; *p && !over; ++p) s = child(s, (unsigned char)*p);
    if (over) return;
    nd[s].acc = true;
    if (flags & MWX_CONSTRAINT_TRAILING_PUNCT)
      for (const char* p = ".!?"; *p && !over; ++p) {
        const int e = child(s, (unsigned char)*p);
        if (!over) nd[e].acc = true;
      }
  };
  for (int i = 0; i < n && !over; ++i) {
    insert(0, texts[i]);
    if ((flags & MWX_CONSTRAINT_LEADING_SPACE) && !over) insert(child(0, ' '), texts[i]);
  }
  if (over) {
    w = "more than MWX_CONSTRAINT_MAX_STATES - 1 live states";
    return nullptr;
  }
  // (a node made by child() just before `over` was set cannot exist: over
  // returns before the node is added) state ids: trie node k = state k + 1
  const int S = (int)nd.size() + 1;
  std::vector<uint16_t> trans((size_t)S * 256, 0);
  std::vector<uint8_t> acc(S, 0);
  for (int k = 0; k + 1 < S; ++k) {
    acc[k + 1] = nd[k].acc ? 1 : 0;
    for (int b = 0; b < 256; ++b)
      if (nd[k].next[b] >= 0) trans[(size_t)(k + 1) * 256 + b] = (uint16_t)(nd[k].next[b] + 1);
  }
  return constraint_from_dfa(S, 1, trans.data(), acc.data(), why);
}

int constraint_walk(const mwx_constraint& c, int s, const uint8_t* bytes, size_t n) {
  if (s < 0 || s >= c.S) return 0;
  for (size_t i = 0; i < n && s != 0; ++i) s = c.tab[(size_t)s * c.C + c.cls[bytes[i]]];
  return s;
}

ConBlock constraint_block(const mwx_constraint& c) {
  ConBlock b;
  b.o_cls = c.tab.size() * 2;
  b.o_acc = b.o_cls + 256;
  b.data.resize(b.o_acc + c.acc.size());
  memcpy(b.data.data(), c.tab.data(), c.tab.size() * 2);
  memcpy(b.data.data() + b.o_cls, c.cls.data(), 256);
  memcpy(b.data.data() + b.o_acc, c.acc.data(), c.acc.size());
  return b;
}

ConTokens constraint_tokens_raw(const uint32_t* off, const uint8_t* bytes, int n_tok) {
  ConTokens t;
  t.n_tok = n_tok;
  const size_t nb = off[n_tok];
  t.o_head = ((size_t)n_tok + 1) * 4;
  t.o_bytes = t.o_head + (size_t)n_tok * 4;
  t.data.assign(t.o_bytes + nb, 0);
  memcpy(t.data.data(), off, ((size_t)n_tok + 1) * 4);
  uint32_t* head = reinterpret_cast<uint32_t*>(t.data.data() + t.o_head);
  for (int i = 0; i < n_tok; ++i) {
    uint32_t h = 0;
    const uint32_t len = off[i + 1] - off[i];
    for (uint32_t k = 0; k < len && k < (uint32_t)kConHead; ++k)
      h |= (uint32_t)bytes[off[i] + k] << (8 * k);
    head[i] = h;
  }
  if (nb) memcpy(t.data.data() + t.o_bytes, bytes, nb);
  return t;
}

ConTokens constraint_tokens(const std::vector<std::string>& id_to_token, int n_tok) {
  std::vector<uint32_t> off((size_t)n_tok + 1, 0);
  std::vector<uint8_t> bytes;
  for (int i = 0; i < n_tok; ++i) {
    const std::string& s = id_to_token[i];
    bytes.insert(bytes.end(), s.begin(), s.end());
    off[i + 1] = (uint32_t)bytes.size();
  }
  return constraint_tokens_raw(off.data(), bytes.data(), n_tok);
}

static ConView view_of(const mwx_constraint& c, const uint8_t* blk, size_t o_cls, size_t o_acc,
                       const ConTokens& t, const uint8_t* tok) {
  ConView v;
  v.tab = reinterpret_cast<const uint16_t*>(blk);
  v.cls = blk + o_cls;
  v.acc = blk + o_acc;
  v.off = reinterpret_cast<const uint32_t*>(tok);
  v.head = reinterpret_cast<const uint32_t*>(tok + t.o_head);
  v.bytes = tok + t.o_bytes;
  v.S = c.S;
  v.C = c.C;
  v.eot = t.n_tok;
  v.start = c.start;
  return v;
}
ConView constraint_view(const mwx_constraint& c, const ConTokens& t) {
  ConView v = view_of(c, nullptr, 0, 0, t, t.data.data());
  v.tab = c.tab.data();
  v.cls = c.cls.data();
  v.acc = c.acc.data();
  return v;
}
ConView constraint_view_dev(const mwx_constraint& c, const ConBlock& b, const uint8_t* d_block,
                            const ConTokens& t, const uint8_t* d_tokens) {
  return view_of(c, d_block, b.o_cls, b.o_acc, t, d_tokens);
}

int constraint_check(const mwx_full_params& P, const char** why) {
  const char* dummy;
  const char*& w = why ? *why : dummy;
  w = "";
  if (!P.constraint) return 0;
  if (!std::isfinite(P.constraint_penalty) || !(P.constraint_penalty > 0.0f)) {
    w = "constraint_penalty is NaN, infinite or <= 0";
    return -1;
  }
  if (P.bench_fixed_steps > 0) {
    w = "bench_fixed_steps > 0 with a constraint";
    return -1;
  }
  return 0;
}

}  // namespace mwx

// The log sink lives in the engine; this file also links alone (tests), so a
// refusal's reason goes through a weak hook the engine overrides.
extern "C" __attribute__((weak)) void mwx_constraint_log(const char* msg) {
  fprintf(stderr, "%s\n", msg);
}
static mwx_constraint* logged(mwx_constraint* c, const char* fn, const char* why) {
  if (!c) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", fn, why);
    mwx_constraint_log(buf);
  }
  return c;
}

extern "C" struct mwx_constraint* mwx_constraint_from_dfa(int n_states, int start,
                                                          const uint16_t* trans,
                                                          const uint8_t* accepting) {
  const char* why = "";
  mwx_constraint* c = mwx::constraint_from_dfa(n_states, start, trans, accepting, &why);
  return logged(c, "mwx_constraint_from_dfa", why);
}
extern "C" struct mwx_constraint* mwx_constraint_from_choices(const char* const* texts, int n,
                                                              int flags) {
  const char* why = "";
  mwx_constraint* c = mwx::constraint_from_choices(texts, n, flags, &why);
  return logged(c, "mwx_constraint_from_choices", why);
}
extern "C" void mwx_constraint_free(struct mwx_constraint* c) { delete c; }
extern "C" int mwx_constraint_n_states(const struct mwx_constraint* c) { return c ? c->S : 0; }
extern "C" int mwx_constraint_start(const struct mwx_constraint* c) { return c ? c->start : 0; }
extern "C" int mwx_constraint_accepting(const struct mwx_constraint* c, int s) {
  return (c && s >= 0 && s < c->S) ? c->acc[s] : 0;
}
extern "C" int mwx_constraint_walk(const struct mwx_constraint* c, int s, const uint8_t* bytes,
                                   int n) {
  if (!c || n < 0 || (n > 0 && !bytes)) return 0;
  return mwx::constraint_walk(*c, s, bytes, (size_t)n);
}

// (include/mwx_test.h) a constraint built from choices (texts != NULL) or from
// a DFA, walked over bytes from `from` (< 0: the start)
extern "C" int mwx_test_constraint_walk(const char* const* texts, int n, int flags, int n_states,
                                        int start, const uint16_t* trans,
                                        const uint8_t* accepting, int from, const uint8_t* bytes,
                                        int n_bytes, int* accepting_out, int* n_states_out,
                                        int* n_classes_out, long long* table_bytes_out) {
  if (n_bytes < 0 || (n_bytes > 0 && !bytes)) return -1;
  mwx_constraint* c = texts ? mwx_constraint_from_choices(texts, n, flags)
                            : mwx_constraint_from_dfa(n_states, start, trans, accepting);
  if (!c) return -1;
  const int s = mwx::constraint_walk(*c, from < 0 ? c->start : from, bytes, (size_t)n_bytes);
  if (accepting_out) *accepting_out = c->acc[s];
  if (n_states_out) *n_states_out = c->S;
  if (n_classes_out) *n_classes_out = c->C;
  if (table_bytes_out) *table_bytes_out = (long long)mwx::constraint_block(*c).data.size();
  delete c;
  return s;
}
