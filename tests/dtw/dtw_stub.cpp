// TEST INFRASTRUCTURE ONLY — the CPU stand-in tests/san/mwx_stub.cpp with DTW
// times: the context parameters the host passes are recorded, and when they
// ask for DTW token timestamps every text token gets t_dtw = its heuristic
// t0 + 7 + 3 j (j = token index in its segment); otherwise t_dtw stays -1.
// Linked into tests/dtw/host_dtw_check.cpp only.
#define mwx_init_from_file_with_params stub_init_from_file_with_params
#define mwx_full_get_token_data_from_state stub_get_token_data_from_state
#include "../san/mwx_stub.cpp"
#undef mwx_init_from_file_with_params
#undef mwx_full_get_token_data_from_state

mwx_context_params g_dtw_params;      // of the last context opened
std::vector<mwx_ahead> g_dtw_heads;   // its CUSTOM list

extern "C" {

mwx_context* mwx_init_from_file_with_params(const char* path, mwx_context_params params) {
  g_dtw_params = params;
  g_dtw_heads.assign(params.dtw_aheads.heads,
                     params.dtw_aheads.heads + (params.dtw_aheads.heads ? params.dtw_aheads.n_heads : 0));
  g_dtw_params.dtw_aheads.heads = nullptr;
  return stub_init_from_file_with_params(path, params);
}

mwx_token_data mwx_full_get_token_data_from_state(mwx_state* st, int i, int j) {
  mwx_token_data d = stub_get_token_data_from_state(st, i, j);
  if (g_dtw_params.dtw_token_timestamps && d.id < kEot) d.t_dtw = d.t0 + 7 + 3 * j;
  return d;
}

}  // extern "C"
