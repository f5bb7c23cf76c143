// Constrained decoding: a deterministic automaton over the
// bytes of the text, and the transition every side uses (the mask kernel in
// k_constrain.hip, the advance kernels in k_misc.hip, the host replay in
// driver.inc).
//
// A constraint (built once, immutable): S states (0 = dead), a start state, the
// raw table [S][256] it was built from, and what the device reads:
//   cls[256]   byte -> class; bytes whose columns of the raw table are equal
//              share a class, so tab[s][cls[b]] == raw[s][b] for every s, b
//   tab[S][C]  uint16 state ids
//   acc[S]     1 = accepting
// One block on the device: tab | cls | acc (tab first: 2-byte aligned).
//
// The token byte table (per context, ids below eot only):
//   off[eot + 1]  a token's bytes are bytes[off[t] .. off[t + 1])
//   head[eot]     the token's first four bytes, little-endian, zero-padded: the
//                 first transitions of lane t come from one coalesced load
//   bytes[]       every token's bytes, packed
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MWX_CON_HD __host__ __device__
#else
#define MWX_CON_HD
#endif

namespace mwx {

constexpr int kConHead = 4;  // bytes of a token held in head[]

// What a walk reads (device pointers on the device, host pointers on the
// host). tab == nullptr: no constraint, every state stays 0.
struct ConView {
  const uint16_t* tab = nullptr;
  const uint8_t* cls = nullptr;
  const uint8_t* acc = nullptr;
  const uint32_t* off = nullptr;
  const uint32_t* head = nullptr;
  const uint8_t* bytes = nullptr;
  int S = 0, C = 0, eot = 0, start = 0;
};

MWX_CON_HD inline int con_step(const ConView& v, int s, unsigned b) {
  return v.tab[(size_t)s * v.C + v.cls[b & 255u]];
}
// delta*(s, bytes(t)) for a text token t < eot and 0 < s < S; *empty: the token
// has no bytes (the state is then s itself)
MWX_CON_HD inline int con_walk_token(const ConView& v, int s, int t, bool* empty) {
  const uint32_t o = v.off[t], n = v.off[t + 1] - o;
  *empty = n == 0;
  const uint32_t h = v.head[t];
  const uint32_t nh = n < (uint32_t)kConHead ? n : (uint32_t)kConHead;
  for (uint32_t i = 0; i < nh && s != 0; ++i) s = con_step(v, s, (h >> (8 * i)) & 255u);
  for (uint32_t i = kConHead; i < n && s != 0; ++i) s = con_step(v, s, v.bytes[o + i]);
  return s;
}
// The row's state after it generated `id` in state s (D15: ids >= eot leave it).
MWX_CON_HD inline int con_next_state(const ConView& v, int s, int id) {
  if (!v.tab) return 0;
  if (s <= 0 || s >= v.S) return 0;
  if (id < 0 || id >= v.eot) return s;
  bool empty;
  return con_walk_token(v, s, id, &empty);
}
// D15's rejection of token t at a sampling step of a row in state s
MWX_CON_HD inline bool con_rejects(const ConView& v, int s, int t) {
  if (s <= 0 || s >= v.S) return false;
  if (t < v.eot) {
    bool empty;
    const int n = con_walk_token(v, s, t, &empty);
    return empty || n == 0;
  }
  return t == v.eot && !v.acc[s];
}

}  // namespace mwx

#if !defined(MWX_CON_NO_HOST)
#include <string>
#include <vector>

#include "mwx.h"

struct mwx_constraint {
  int S = 0, start = 0, C = 0;
  std::vector<uint16_t> raw;  // [S][256]
  std::vector<uint16_t> tab;  // [S][C]
  std::vector<uint8_t> cls;   // [256]
  std::vector<uint8_t> acc;   // [S]
};

namespace mwx {

// NULL with *why set when mwx.h says so
mwx_constraint* constraint_from_dfa(int n_states, int start, const uint16_t* trans,
                                    const uint8_t* accepting, const char** why);
mwx_constraint* constraint_from_choices(const char* const* texts, int n, int flags,
                                        const char** why);
// class-compressed walk of n bytes from s (s outside [0, S) counts as dead)
int constraint_walk(const mwx_constraint& c, int s, const uint8_t* bytes, size_t n);
// the device block tab | cls | acc and the offsets of its parts
struct ConBlock {
  std::vector<uint8_t> data;
  size_t o_cls = 0, o_acc = 0;
};
ConBlock constraint_block(const mwx_constraint& c);
// the token byte table of the first n_tok ids: off | head | bytes in one block
struct ConTokens {
  std::vector<uint8_t> data;
  size_t o_head = 0, o_bytes = 0;
  int n_tok = 0;
};
ConTokens constraint_tokens(const std::vector<std::string>& id_to_token, int n_tok);
ConTokens constraint_tokens_raw(const uint32_t* off, const uint8_t* bytes, int n_tok);
// a view over host copies
ConView constraint_view(const mwx_constraint& c, const ConTokens& t);
// a view over device copies laid out as the two blocks above
ConView constraint_view_dev(const mwx_constraint& c, const ConBlock& b, const uint8_t* d_block,
                            const ConTokens& t, const uint8_t* d_tokens);
// mwx_full_params.constraint / constraint_penalty: 0, or -1 with *why
int constraint_check(const mwx_full_params& P, const char** why);

}  // namespace mwx
#endif
