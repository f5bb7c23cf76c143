// TEST INFRASTRUCTURE ONLY — the contextual-biasing matcher (csrc/bias.cpp,
// DESIGN.md D14) linked directly (tests/bias/Makefile; AddressSanitizer +
// UBSan), run by tests/test_bias_host.py: seeded random phrase sets over a
// small alphabet against the rule restated naively (every phrase, every k),
// the state carried id by id against the walk from the root, the table bound,
// and the refused inputs.
#include <cmath>
#include <cstdio>
#include <limits>
#include <map>
#include <random>
#include <vector>

#include "bias.h"
#include "mwx_test.h"

namespace {

int failures = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

struct Phrase {
  std::vector<mwx_token> ids;
  float boost;
};

std::map<int, float> naive(const std::vector<Phrase>& ph, const std::vector<mwx_token>& h) {
  std::map<int, float> out;
  for (const Phrase& p : ph)
    for (size_t k = 0; k < p.ids.size() && k <= h.size(); ++k) {
      bool m = true;
      for (size_t j = 0; j < k && m; ++j) m = h[h.size() - k + j] == p.ids[j];
      if (!m) continue;
      auto it = out.find(p.ids[k]);
      if (it == out.end())
        out[p.ids[k]] = p.boost;
      else if (p.boost > it->second)
        it->second = p.boost;
    }
  return out;
}

std::vector<mwx_bias_phrase> view(const std::vector<Phrase>& ph) {
  std::vector<mwx_bias_phrase> v;
  for (const Phrase& p : ph) v.push_back({p.ids.data(), (int)p.ids.size(), p.boost});
  return v;
}

}  // namespace

int main() {
  std::mt19937 rng(20240914);
  const float boosts[] = {-3.0f, -0.5f, 0.0f, 0.25f, 1.0f, 2.5f, 7.0f};
  for (int it = 0; it < 400; ++it) {
    const int alphabet = it % 7 == 0 ? 2 : 4;
    const int max_len = it % 7 == 0 ? MWX_BIAS_MAX_TOKENS : 6;
    std::vector<Phrase> ph(1 + rng() % (it % 7 == 0 ? 40 : 12));
    size_t total = 0;
    for (Phrase& p : ph) {
      p.ids.resize(1 + rng() % max_len);
      for (auto& t : p.ids) t = (mwx_token)(rng() % alphabet);
      p.boost = boosts[rng() % 7];
      total += p.ids.size();
    }
    std::vector<mwx_token> h(rng() % 40);
    for (auto& t : h) t = (mwx_token)(rng() % (alphabet + 1));
    const std::vector<mwx_bias_phrase> v = view(ph);
    CHECK(mwx::bias_validate(v.data(), (int)v.size(), alphabet + 1) == 0);
    const std::vector<int32_t> tab = mwx::bias_build(v.data(), (int)v.size());
    CHECK(tab.size() * 4 <= mwx::bias_table_bound(total));
    int s = 0;
    for (size_t n = 0; n <= h.size(); ++n) {  // the carried state == the walk of the prefix
      if (n > 0) s = mwx::bias_next_state(tab.data(), s, h[n - 1]);
      CHECK(s == mwx::bias_walk(tab, h.data(), (int)n));
      std::vector<int> toks;
      std::vector<float> bs;
      mwx::bias_state_set(tab, s, toks, bs);
      const std::map<int, float> want =
          naive(ph, std::vector<mwx_token>(h.begin(), h.begin() + (std::ptrdiff_t)n));
      CHECK(toks.size() == want.size());
      size_t i = 0;
      for (const auto& kv : want) {
        if (i >= toks.size()) break;
        CHECK(toks[i] == kv.first && bs[i] == kv.second);
        ++i;
      }
    }
    // the hook: the same set, clipped to cap
    std::vector<mwx_token> to(3);
    std::vector<float> bo(3);
    long long bytes = 0;
    const int n = mwx_test_bias_match(v.data(), (int)v.size(), h.data(), (int)h.size(), to.data(),
                                      bo.data(), 3, &bytes);
    CHECK(n == (int)naive(ph, h).size() && bytes == (long long)tab.size() * 4);
  }
  // no tables: the root, always
  CHECK(mwx::bias_next_state(nullptr, 5, 7) == 0);
  CHECK(mwx::bias_build(nullptr, 0).empty());
  // refused inputs
  const mwx_token ok[2] = {1, 2}, neg[2] = {1, -1}, big[2] = {1, 100};
  std::vector<mwx_token> longp(MWX_BIAS_MAX_TOKENS + 1, 3);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = INFINITY;
  auto rc = [](const mwx_token* t, int n, float b, int count = 1, int eot = 100) {
    std::vector<mwx_bias_phrase> v((size_t)std::max(count, 1), mwx_bias_phrase{t, n, b});
    return mwx::bias_validate(v.data(), count, eot);
  };
  CHECK(rc(ok, 2, 1.0f) == 0);
  CHECK(rc(ok, 2, -1e30f) == 0);
  CHECK(rc(ok, 2, 1.0f, MWX_BIAS_MAX_PHRASES) == 0);
  CHECK(rc(ok, 2, 1.0f, MWX_BIAS_MAX_PHRASES + 1) == -1);
  CHECK(rc(ok, 2, 1.0f, -1) == -1);
  CHECK(rc(ok, 0, 1.0f) == -1);
  CHECK(rc(longp.data(), (int)longp.size(), 1.0f) == -1);
  CHECK(rc(longp.data(), MWX_BIAS_MAX_TOKENS, 1.0f) == 0);
  CHECK(rc(nullptr, 2, 1.0f) == -1);
  CHECK(rc(ok, 2, nan) == -1);
  CHECK(rc(ok, 2, inf) == -1);
  CHECK(rc(ok, 2, -inf) == -1);
  CHECK(rc(neg, 2, 1.0f) == -3);
  CHECK(rc(big, 2, 1.0f) == -3);
  CHECK(rc(big, 2, 1.0f, 1, 101) == 0);
  CHECK(mwx::bias_validate(nullptr, 1, 100) == -1);
  CHECK(mwx::bias_validate(nullptr, 0, 100) == 0);
  CHECK(mwx_test_bias_match(nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr) == 0);
  CHECK(mwx_test_bias_match(nullptr, 0, nullptr, 2, nullptr, nullptr, 0, nullptr) == -1);
  std::printf("matcher_check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
