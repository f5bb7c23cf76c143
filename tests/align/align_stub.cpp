// TEST INFRASTRUCTURE ONLY — the CPU stand-in tests/san/mwx_stub.cpp with the
// alignment calls (mwx_align_batch, mwx_align_row) and the three lookups the
// host's align() binds with them (mwx_tokenize, mwx_full_lang_id_from_state,
// mwx_lang_str). It aligns nothing: every value is a fixed function of the
// token ids, so tests/align/host_align_check.cpp can state what the host must
// make of it. Linked into that program only.
#include "../san/mwx_stub.cpp"

#include <map>
#include <mutex>

struct AlignRow {
  float plog;
  int top_id;
  float top_plog;
};

std::string g_align_text;       // the last text given to mwx_tokenize
int g_align_calls = 0;          // mwx_align_batch calls
int g_align_clips = 0;          // clips of the last one
int g_align_sleep_ms = 0;       // each call holds its states this long
mwx_full_params g_align_params; // of the last call

namespace {
std::mutex g_mu;
std::map<mwx_state*, std::vector<AlignRow>> g_rows;
std::map<mwx_state*, int> g_lang;
}  // namespace

extern "C" {

// words split at spaces, each with its leading space: a kWords entry is its
// index, any other word 16 + its length
int mwx_tokenize(mwx_context* ctx, const char* text, mwx_token* tokens, int n_max_tokens) {
  if (!ctx || !text) return 0;
  g_align_text = text;
  std::vector<int> ids;
  const std::string s = text;
  size_t p = 0;
  while (p < s.size()) {
    size_t q = s.find(' ', p + 1);
    if (q == std::string::npos) q = s.size();
    const std::string w = s.substr(p, q - p);
    int id = 16 + (int)w.size();
    for (int k = 0; k < 16; ++k)
      if (w == kWords[k]) id = k;
    ids.push_back(id);
    p = q;
  }
  if ((int)ids.size() > n_max_tokens) return -(int)ids.size();
  for (size_t i = 0; i < ids.size(); ++i) tokens[i] = ids[i];
  return (int)ids.size();
}

int mwx_full_lang_id_from_state(mwx_state* st) {
  std::lock_guard<std::mutex> lock(g_mu);
  return g_lang[st];
}
const char* mwx_lang_str(int id) { return id == 0 ? "en" : id == 1 ? "de" : id == 2 ? "tr" : nullptr; }

int mwx_align_batch(mwx_context* ctx, mwx_state* const* states, mwx_full_params params,
                    const float* const* samples, const int* n_samples,
                    const mwx_token* const* tokens, const int* n_tokens, int n_clips) {
  if (!ctx || !states || !samples || !n_samples || !tokens || !n_tokens || n_clips < 1) return -1;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    ++g_align_calls;
    g_align_clips = n_clips;
    g_align_params = params;
  }
  for (int b = 0; b < n_clips; ++b) {
    if (n_tokens[b] > MWX_ALIGN_MAX_TOKENS || n_samples[b] > 30 * 16000) return -1;
    for (int j = 0; j < n_tokens[b]; ++j)
      if (tokens[b][j] < 0 || tokens[b][j] >= kEot) return -3;
  }
  if (params.abort_callback && params.abort_callback(params.abort_callback_user_data)) return -6;
  if (g_align_sleep_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(g_align_sleep_ms));
  const std::string lang = params.language ? params.language : "";
  for (int b = 0; b < n_clips; ++b) {
    mwx_state* st = states[b];
    st->segs.clear();
    std::vector<AlignRow> rows;
    if (n_samples[b] >= 1600) {
      Segment s;
      s.t0 = 0;
      s.t1 = (int64_t)n_samples[b] / 160;
      s.turn = false;
      for (int j = 0; j < n_tokens[b]; ++j) {
        const int id = tokens[b][j];
        const float p = 0.5f + 0.01f * (float)(id % 16);
        s.tokens.push_back({id, p, -1, -1});
        const char* w = mwx_token_to_str(ctx, id);
        s.text += w ? w : "?";
        rows.push_back({std::log(p), j % 2 == 0 ? id : (id + 1) % 16, j % 2 == 0 ? std::log(p) : -0.1f});
      }
      rows.push_back({-0.25f, kEot, -0.125f});
      st->segs.push_back(std::move(s));
    }
    std::lock_guard<std::mutex> lock(g_mu);
    g_rows[st] = rows;
    g_lang[st] = lang == "de" ? 1 : (lang == "auto" || lang.empty()) ? 2 : 0;
  }
  return 0;
}

int mwx_align_row(mwx_state* st, int i, float* plog, mwx_token* top_id, float* top_plog) {
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_rows.find(st);
  if (it == g_rows.end() || i < 0 || i >= (int)it->second.size()) return -1;
  if (plog) *plog = it->second[i].plog;
  if (top_id) *top_id = it->second[i].top_id;
  if (top_plog) *top_plog = it->second[i].top_plog;
  return 0;
}

}  // extern "C"
