// whisper_full control flow over the batched device path (included by
// engine.cpp). Restates whisper.cpp v1.8.2 whisper_full_with_state and its
// helpers — see oracle/mwx_oracle.cpp full() for the scalar restatement this
// is tested against.
#include <cstdarg>
#include <map>

namespace mwx {

static float voice_length(const std::string& text) {
  float res = 0.0f;
  for (char c : text) {
    if (c == ' ')
      res += 0.01f;
    else if (c == ',')
      res += 2.00f;
    else if (c == '.' || c == '!' || c == '?')
      res += 3.00f;
    else if (c >= '0' && c <= '9')
      res += 3.00f;
    else
      res += 1.00f;
  }
  return res;
}
static int timestamp_to_sample(int64_t t, int n_samples) {
  return std::max(0, std::min(n_samples - 1, (int)((t * MWX_SAMPLE_RATE) / 100)));
}
static int64_t sample_to_timestamp(int i) { return (100ll * i) / MWX_SAMPLE_RATE; }

// whisper_exp_compute_token_level_timestamps
static void token_timestamps(const Context& C, TsState& st, Segment& seg, float thold_pt,
                             float thold_ptsum) {
  auto& tokens = seg.tokens;
  const int n_samples = st.n_energy;
  if (n_samples == 0 || !st.energy) return;
  const int64_t t0 = seg.t0, t1 = seg.t1;
  const int n = (int)tokens.size();
  if (n == 0) return;
  if (n == 1) {
    tokens[0].t0 = t0;
    tokens[0].t1 = t1;
    return;
  }
  const int beg = C.vocab.token_beg;
  for (int j = 0; j < n; ++j) {
    auto& token = tokens[j];
    if (j == 0) {
      if (token.id == beg) {
        tokens[j].t0 = t0;
        tokens[j].t1 = t0;
        tokens[j + 1].t0 = t0;
        st.t_beg = t0;
        st.t_last = t0;
        st.tid_last = beg;
      } else {
        tokens[j].t0 = st.t_last;
      }
    }
    const int64_t tt = st.t_beg + 2 * (token.tid - beg);
    tokens[j].vlen = voice_length(C.vocab.id_to_token[token.id]);
    if (token.pt > thold_pt && token.ptsum > thold_ptsum && token.tid > st.tid_last && tt <= t1) {
      if (j > 0) tokens[j - 1].t1 = tt;
      tokens[j].t0 = tt;
      st.tid_last = token.tid;
    }
  }
  tokens[n - 2].t1 = t1;
  tokens[n - 1].t0 = t1;
  tokens[n - 1].t1 = t1;
  st.t_last = t1;
  {
    int p0 = 0, p1 = 0;
    while (true) {
      while (p1 < n && tokens[p1].t1 < 0) p1++;
      if (p1 >= n) p1--;
      if (p1 > p0) {
        double psum = 0.0;
        for (int j = p0; j <= p1; j++) psum += tokens[j].vlen;
        const double dt = tokens[p1].t1 - tokens[p0].t0;
        for (int j = p0 + 1; j <= p1; j++) {
          const double ct = tokens[j - 1].t0 + dt * tokens[j - 1].vlen / psum;
          tokens[j - 1].t1 = (int64_t)ct;
          tokens[j].t0 = (int64_t)ct;
        }
      }
      p1++;
      p0 = p1;
      if (p1 >= n) break;
    }
  }
  for (int j = 0; j < n - 1; j++) {
    if (tokens[j].t1 < 0) tokens[j + 1].t0 = tokens[j].t1;
    if (j > 0 && tokens[j - 1].t1 > tokens[j].t0) {
      tokens[j].t0 = tokens[j - 1].t1;
      tokens[j].t1 = std::max(tokens[j].t0, tokens[j].t1);
    }
  }
  const int hw = MWX_SAMPLE_RATE / 8;
  for (int j = 0; j < n; j++) {
    if (tokens[j].id >= C.vocab.token_eot) continue;
    int s0 = timestamp_to_sample(tokens[j].t0, n_samples);
    int s1 = timestamp_to_sample(tokens[j].t1, n_samples);
    const int ss0 = std::max(s0 - hw, 0);
    const int ss1 = std::min(s1 + hw, n_samples);
    const int ns = ss1 - ss0;
    float sum = 0.0f;
    for (int k = ss0; k < ss1; k++) sum += st.energy[k];
    const float thold = 0.5 * sum / ns;
    {
      int k = s0;
      if (st.energy[k] > thold && j > 0) {
        while (k > 0 && st.energy[k] > thold) k--;
        tokens[j].t0 = sample_to_timestamp(k);
        if (tokens[j].t0 < tokens[j - 1].t1) {
          tokens[j].t0 = tokens[j - 1].t1;
        } else {
          s0 = k;
        }
      } else {
        while (st.energy[k] < thold && k < s1) k++;
        s0 = k;
        tokens[j].t0 = sample_to_timestamp(k);
      }
    }
    {
      int k = s1;
      if (st.energy[k] > thold) {
        while (k < n_samples - 1 && st.energy[k] > thold) k++;
        tokens[j].t1 = sample_to_timestamp(k);
        // upstream tests `j < ns - 1` (ns = samples, not tokens) and so reads
        // tokens[j + 1] past the end for a trailing text token (UB); guarded
        if (j < ns - 1 && j + 1 < n && tokens[j].t1 > tokens[j + 1].t0) {
          tokens[j].t1 = tokens[j + 1].t0;
        } else {
          s1 = k;
        }
      } else {
        while (st.energy[k] < thold && k > s0) k--;
        s1 = k;
        tokens[j].t1 = sample_to_timestamp(k);
      }
    }
  }
}

// whisper_sequence_score
static void sequence_score(const mwx_full_params& P, Row& s) {
  if (s.result_len == 0) return;
  double result = 0.0;
  for (int i = 0; i < s.result_len; ++i) result += s.tokens[i].plog;
  s.sum_logprobs = result;
  s.avg_logprobs = result / s.result_len;
  double penalty = s.result_len;
  if (P.length_penalty > 0.0f) penalty = pow((5.0 + penalty) / 6.0, P.length_penalty);
  s.score = result / penalty;
  const int n = 32;
  int cnt = 0;
  double entropy = 0.0;
  std::map<int, int> counts;
  for (int i = std::max(0, s.result_len - n); i < s.result_len; ++i) {
    counts[s.tokens[i].id]++;
    cnt++;
  }
  for (const auto& kv : counts) {
    const double p = kv.second / (double)cnt;
    entropy -= p * log(p);
  }
  s.entropy = entropy;
}

static bool aborted(const mwx_full_params& P) {
  return P.abort_callback && P.abort_callback(P.abort_callback_user_data);
}

// One beam-search sampling step (whisper.cpp v1.8.2 whisper_full_with_state,
// WHISPER_SAMPLING_BEAM_SEARCH): every live decoder draws beam_size candidate
// tokens with its own RNG from its probs (whisper_sample_token_topk), the
// clip's candidates are sorted by sum_logprobs_all (desc, then decoder index)
// and handed to the live decoders in order, skipping a candidate equal to the
// one just taken (from the second token on); a decoder that takes another
// decoder's candidate takes over that decoder's KV cache. Rows of a clip are
// contiguous (decoder j = row r0 + j) and step in lockstep.
static void beam_step(std::vector<Row>& rows, std::vector<ClipRun>& clips,
                      const std::vector<RowCtl>& ctl, const std::vector<TokOut>& out, State& S,
                      int n_cur, int token_beg, int beam_size, std::vector<int>& kv_moves) {
  // A candidate is its parent decoder (whose state is moved into a per-clip
  // snapshot before any decoder is overwritten) plus one drawn token: the
  // token histories are copied once per decoder that takes a candidate, not
  // once per candidate (32 clips x 25 candidates x ~220 tokens per step was
  // most of the host's per-step time)
  struct Cand {
    int dec;
    double sum_logprobs_all;
    mwx_token_data td;
  };
  struct Parent {
    int seek_delta;
    bool has_ts;
    int result_len;
    std::vector<mwx_token_data> tokens;
  };
  const int R = (int)rows.size();
  std::vector<Cand> cands;
  std::vector<Parent> par(n_cur);
  for (int r0 = 0; r0 < R; r0 += n_cur) {
    int live = -1;
    for (int j = 0; j < n_cur; ++j)
      if (!rows[r0 + j].stopped && ctl[r0 + j].sample) {
        live = r0 + j;
        break;
      }
    if (live < 0) continue;
    ClipRun& cr = clips[rows[r0].clip];
    if (ctl[live].is_initial && !rows[r0].stopped) cr.no_speech_prob = out[r0].nosp;
    const int i_step = (int)rows[live].tokens.size();
    cands.clear();
    for (int j = 0; j < n_cur; ++j) {
      const int r = r0 + j;
      const Row& w = rows[r];
      if (w.stopped) continue;
      // the beam_size draws of this decoder (device std::discrete_distribution
      // over its probs, u from its RNG: see draw_uniforms)
      const Draw* dr = S.draws_h.data() + (size_t)r * S.draw_k;
      for (int k = 0; k < beam_size; ++k) {
        mwx_token_data td;
        td.id = dr[k].id;
        td.tid = out[r].tid == 0 ? token_beg : out[r].tid;  // topk starts from token_beg
        td.p = dr[k].p;
        td.plog = dr[k].plog;
        td.pt = out[r].pt;
        td.ptsum = out[r].ptsum;
        td.t0 = td.t1 = td.t_dtw = -1;
        td.vlen = 0.0f;
        if (td.id >= token_beg) {
          td.tid = td.id;
          td.pt = td.p;
        }
        cands.push_back({j, w.sum_logprobs_all + td.plog, td});
      }
    }
    // (stable: candidates tied on both keys keep their draw order — the
    // total order the device ranking uses, beam_advance_kernel)
    std::stable_sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) {
      if (a.sum_logprobs_all != b.sum_logprobs_all) return a.sum_logprobs_all > b.sum_logprobs_all;
      return a.dec < b.dec;
    });
    for (int j = 0; j < n_cur; ++j) {
      Row& w = rows[r0 + j];
      if (w.stopped) continue;
      par[j] = Parent{w.seek_delta, w.has_ts, w.result_len, std::move(w.tokens)};
    }
    // the same token sequence: parent history + drawn token, compared from the end
    auto same = [&](const Cand& a, const Cand& b) {
      const std::vector<mwx_token_data>& pa = par[a.dec].tokens;
      const std::vector<mwx_token_data>& pb = par[b.dec].tokens;
      if (pa.size() != pb.size() || a.td.id != b.td.id) return false;
      for (int t = (int)pa.size() - 1; t >= 0; t--)
        if (pa[t].id != pb[t].id) return false;
      return true;
    };
    size_t cur_c = 0;
    for (int j = 0; j < n_cur; ++j) {
      Row& w = rows[r0 + j];
      if (w.stopped) continue;
      if (cur_c >= cands.size()) cur_c = 0;
      const Cand& cur = cands[cur_c++];
      while (cands.size() > cur_c && same(cands[cur_c], cur) && i_step > 0) ++cur_c;
      const Parent& pp = par[cur.dec];
      w.seek_delta = pp.seek_delta;
      w.has_ts = pp.has_ts;
      w.result_len = pp.result_len;
      w.sum_logprobs_all = cur.sum_logprobs_all;
      w.tokens.reserve(pp.tokens.size() + 1);
      w.tokens.assign(pp.tokens.begin(), pp.tokens.end());
      w.tokens.push_back(cur.td);
      if (cur.dec != j) {
        kv_moves.push_back(r0 + j);
        kv_moves.push_back(r0 + cur.dec);
        kv_moves.push_back(w.fed + 1);  // positions 0..fed hold this window's KV
      }
    }
  }
}

// true for device memory (e.g. PCM already resident in HBM); plain host
// memory is not known to HIP and reports an error, which is cleared
static bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}

// Incremental log-mel: point the clip's descriptor at its state's cache of
// the previous call (read) and at the other slot (this call's samples and raw
// log-mel, written by the kernel). Clips over 40 s are not cached. The state's
// cache is invalidated here and re-validated (MelCommit::apply) only once the
// mel kernel that fills the new slot has been queued: an error in between
// leaves no cache entry that claims data the kernel never wrote.
struct MelCommit {
  State* st = nullptr;
  int slot = 0, n = 0, len = 0;
  void apply() const {
    if (!st) return;
    st->melc_slot = slot;
    st->melc_n = n;
    st->melc_len = len;
  }
};
static MelCommit mel_cache_slots(State& cs, MelClip& m, int n_mels, bool on) {
  const int n_prev = cs.melc_n;
  cs.melc_n = 0;
  if (!on || m.n <= 0 || m.n > 40 * MWX_SAMPLE_RATE) return MelCommit{};
  const int p = cs.melc_slot, q = 1 - p;
  if (n_prev > 0) {
    m.n_prev = n_prev;
    m.len_prev = cs.melc_len;
    m.prev_pcm = (const float*)cs.melc_pcm[p].p;
    m.prev_raw = (const float*)cs.melc_raw[p].p;
  }
  m.save_pcm = (float*)cs.melc_pcm[q].get((size_t)m.n * 4);
  m.save_raw = (float*)cs.melc_raw[q].get((size_t)n_mels * m.n_len * 4);
  return MelCommit{&cs, q, m.n, m.n_len};
}

// pcm: f32 samples, or (pcm16) int16 samples converted on the device as
// SttEngine::transcribe_pcm16 converts them (x / 32768)
// Stream priorities for concurrent batches (the SttEngine's parallel_requests
// batchers, bench.py --lanes): by default a batch's encoder runs on a
// low-priority stream of its state, so another batch's latency-bound decode
// chain is dispatched ahead of the encoder GEMM tiles (C3 at 2 lanes: 1566 ->
// 1592 audio-s/s, same box). MWX_STREAM_PRIO: "enc_low" (default), "dec_high"
// (state streams at high priority), "both", "none" (one normal stream).
// Run-ahead safety net (a device/host disagreement redoes the attempt on the
// host loop): fault injection for the test (MWX_TEST_RA_MISMATCH=k, read once,
// or mwx_test_set_ra_mismatch) and the process's fallback count, whose first
// occurrence is logged at error level (a real rule difference would otherwise
// show only as a slowdown).
static std::atomic<long>& ra_mismatch_mode() {
  static std::atomic<long> m{-2};
  return m;
}
static long ra_fault_step_now() {
  long v = ra_mismatch_mode().load();
  if (v == -2) {
    v = getenv("MWX_TEST_RA_MISMATCH") ? atol(getenv("MWX_TEST_RA_MISMATCH")) : -1;
    long expect = -2;
    ra_mismatch_mode().compare_exchange_strong(expect, v);
  }
  return v;
}
static std::atomic<long> g_ra_fallbacks{0};
static void note_ra_fallback(State& S, const char* why) {
  ++S.n_ra_fallback;
  if (g_ra_fallbacks.fetch_add(1) == 0)
    MWX_LOG_ERROR("mwx: run-ahead decode redone on the host loop (%s); results are the host "
                  "loop's. Later occurrences are counted (mwx_runahead_fallbacks) and logged as "
                  "warnings\n", why);
}

// Token ids handed in by the caller (prompts, teacher-forced test prefixes)
// must lie in the vocabulary: the device's embedding gather clamps its
// indices (inactive rows carry stale ids and positions, and the gather
// requests them before it reads the activity flag), so an out-of-range id on
// an active row would otherwise be silently replaced, not rejected.
static bool tokens_valid(const int* t, int n, int n_vocab) {
  for (int i = 0; i < n; ++i)
    if (t[i] < 0 || t[i] >= n_vocab) return false;
  return true;
}

static bool stream_prio_has(const char* what) {
  static const std::string v = getenv("MWX_STREAM_PRIO") ? getenv("MWX_STREAM_PRIO") : "enc_low";
  return v == "both" || v.find(what) != std::string::npos;
}

// The audio context of a window (mwx.h: mwx_audio_ctx_for; DESIGN.md D9):
// n_len_org real mel frames in the clip, the window at frame `seek`.
static int audio_ctx_rule(int N, int n_len_org, int seek, int audio_ctx, bool fit) {
  const int a = std::max(0, audio_ctx);
  if (!fit) return a > 0 ? std::min(a, N) : N;
  const int rem = std::max(0, n_len_org - seek);
  const int floor_ctx = a > 0 ? a : 64;
  const int want = 64 * (((rem + 1) / 2 + 32 + 63) / 64);
  return std::min(N, std::max(floor_ctx, want));
}

// mwx_align_batch (DESIGN.md D12): run_full's mel, encode and language
// detection, then the alignment pass over the given text instead of the window
// loop
struct AlignReq {
  const mwx_token* const* tokens;
  const int* n_tokens;
};

template <typename T>
static int run_full(Context& C, mwx_state* const* states, mwx_full_params P,
                    const void* const* pcm, const int* n_samples, int n_clips,
                    bool pcm16 = false, const AlignReq* align = nullptr) {
  State& S = states[0]->s;
  const Hparams& hp = C.hp;
  const Vocab& vb = C.vocab;
  const int V = hp.n_vocab;
  hipStream_t st = S.stream;
  for (int c = 0; c < n_clips; ++c) {
    states[c]->s.result_all.clear();
    states[c]->s.dtw_dump.clear();
    states[c]->s.lang_probs.clear();
    states[c]->s.lang_last.clear();
  }
  // per-entry languages (mwx.h: lang_ids): fixed_lang[c] >= 0 is clip c's
  // language, whatever P.language says; such a clip takes no part in detection
  std::vector<int> fixed_lang(n_clips, -1);
  if (P.lang_ids && vb.is_multilingual())
    for (int c = 0; c < n_clips; ++c) {
      if (P.lang_ids[c] > lang_max_id()) return -3;
      if (P.lang_ids[c] >= 0) fixed_lang[c] = P.lang_ids[c];
    }
  if (P.audio_ctx > hp.n_audio_ctx) return -5;
  if (P.audio_ctx < 0) P.audio_ctx = 0;
  const bool beam = P.strategy == MWX_SAMPLING_BEAM_SEARCH;
  if (beam && P.beam_search.beam_size < 1) return -4;
  std::vector<ClipRun> clips(n_clips);
  const int n_mels = hp.n_mels;
  // ---------------- mel (device) ----------------
  size_t pcm_total = 0, mel_total = 0;
  long mel_stride = 0;
  for (int c = 0; c < n_clips; ++c) {
    ClipRun& cr = clips[c];
    cr.st = &states[c]->s;
    cr.pcm = pcm[c];
    cr.n = std::max(0, n_samples[c]);
    cr.pcm_off = pcm_total;
    if (cr.n > 0) {
      cr.n_len = (cr.n + MWX_SAMPLE_RATE * MWX_CHUNK_SIZE) / MWX_HOP_LENGTH;
      cr.n_len_org = 1 + (cr.n + 200 - 400) / MWX_HOP_LENGTH;
      cr.n_fft_frames = std::min((cr.n + 200) / MWX_HOP_LENGTH + 1, cr.n_len);
    }
    pcm_total += (size_t)((cr.n + 3) & ~3);  // 16-byte aligned clip starts
    mel_stride = std::max<long>(mel_stride, (long)n_mels * cr.n_len);
  }
  mel_total = (size_t)mel_stride * n_clips;
  float* d_pcm = (float*)S.pcm.get(std::max<size_t>(pcm_total, 1) * 4);
  float* d_mel = (float*)S.mel.get(std::max<size_t>(mel_total, 1) * 4);
  float* d_mx = (float*)S.melmax.get(sizeof(float) * std::max(1, n_clips));
  {
    int16_t* d_p16 = pcm16 ? (int16_t*)S.pcm16.get(std::max<size_t>(pcm_total, 1) * 2) : nullptr;
    for (int c = 0; c < n_clips; ++c) {
      ClipRun& cr = clips[c];
      if (cr.n == 0) continue;
      const size_t off = cr.pcm_off;
      const hipMemcpyKind kind =
          is_device_ptr(cr.pcm) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
      if (pcm16) {
        HIPC(hipMemcpyAsync(d_p16 + off, cr.pcm, (size_t)cr.n * 2, kind, st));
        launch_pcm16_to_f32(d_p16 + off, cr.n, d_pcm + off, st);
      } else {
        HIPC(hipMemcpyAsync(d_pcm + off, cr.pcm, (size_t)cr.n * 4, kind, st));
      }
    }
    // every clip's log-mel in one batched pass; clips of up to 40 s keep
    // their samples and raw log-mel in their state, and the next call on the
    // state recomputes only the frames whose samples changed (a stream's
    // growing buffer: the frames of audio already seen are reused exactly)
    static const bool mel_cache = getenv("MWX_NO_MEL_CACHE") == nullptr;
    std::vector<MelClip> md;
    std::vector<MelCommit> mcommit;
    int max_len = 0;
    for (int c = 0; c < n_clips; ++c) {
      const ClipRun& cr = clips[c];
      MelClip m{};
      m.pcm_off = (long)cr.pcm_off;
      m.mel_off = (long)c * mel_stride;
      m.n = cr.n;
      m.n_len = cr.n > 0 ? cr.n_len : 0;
      m.n_fft = cr.n > 0 ? cr.n_fft_frames : 0;
      max_len = std::max(max_len, m.n_len);
      mcommit.push_back(mel_cache_slots(*cr.st, m, n_mels, mel_cache));
      md.push_back(m);
    }
    MelClip* d_md = (MelClip*)S.meld.get(md.size() * sizeof(MelClip));
    float* d_part = (float*)S.melpart.get((size_t)std::max(1, n_clips) * 16 * 4);
    HIPC(hipMemcpyAsync(d_md, md.data(), md.size() * sizeof(MelClip), hipMemcpyHostToDevice, st));
    launch_mel_batch(d_pcm, d_md, n_clips, max_len, C.d_filters, n_mels, C.d_tables, d_mel, d_part,
                     d_mx, st);
    for (const MelCommit& mc : mcommit) mc.apply();
    if (P.token_timestamps) {
      float* d_en = (float*)S.energy.get(std::max<size_t>(pcm_total, 1) * 4);
      const size_t need = std::max<size_t>(pcm_total, 1);
      if (S.energy_pin_n < need) {
        std::lock_guard<std::recursive_mutex> lock(capture_mutex());
        if (S.energy_pin) (void)hipHostFree(S.energy_pin);
        S.energy_pin = nullptr;
        S.energy_pin_n = 0;
        HIPC(hipHostMalloc((void**)&S.energy_pin, need * 4, hipHostMallocDefault));
        S.energy_pin_n = need;
      }
      for (int c = 0; c < n_clips; ++c) {
        ClipRun& cr = clips[c];
        if (cr.n == 0) continue;
        const size_t off = cr.pcm_off;
        launch_signal_energy(d_pcm + off, cr.n, d_en + off, st);
        cr.ts.energy = S.energy_pin + off;
        cr.ts.n_energy = cr.n;
      }
      // one async copy of the batch's energy (read after the decode steps,
      // which synchronize the stream)
      HIPC(hipMemcpyAsync(S.energy_pin, d_en, pcm_total * 4, hipMemcpyDeviceToHost, st));
    }
  }
  Driver<T> D(C, S, P);
  D.ensure_cross(n_clips);
  D.reset_xkeys();
  // the audio context of clip c's window at `seek` (DESIGN.md D9)
  const bool actx_on = P.audio_ctx > 0 || P.audio_ctx_fit;
  auto window_ctx = [&](int c, int seek) {
    return audio_ctx_rule(hp.n_audio_ctx, clips[c].n_len_org, seek, P.audio_ctx, P.audio_ctx_fit);
  };
  // ---------------- language detection ----------------
  const bool detect = P.language == nullptr || strlen(P.language) == 0 ||
                      strcmp(P.language, "auto") == 0 || P.detect_language;
  // live: the clips whose cross slots the decode after this encode reads
  auto encode_clips = [&](const std::vector<int>& which, const std::vector<int>& seeks,
                          const std::vector<int>& live) -> int {
    if (which.empty()) return 0;
    if (aborted(P)) return -6;
    D.live_slots = live;  // (slot = clip index)
    std::vector<int> nlen, slots, nctx;
    for (size_t i = 0; i < which.size(); ++i) {
      const int c = which[i];
      nlen.push_back(clips[c].n_len);
      slots.push_back(c);
      if (actx_on) nctx.push_back(window_ctx(c, seeks[i]));
    }
    if (stream_prio_has("enc_low")) {
      // the encoder on the state's low-priority stream, between two events
      if (!S.estream) {
        int least = 0, greatest = 0;
        HIPC(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPC(hipStreamCreateWithPriority(&S.estream, hipStreamNonBlocking, least));
        HIPC(hipEventCreateWithFlags(&S.ev_e0, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&S.ev_e1, hipEventDisableTiming));
      }
      HIPC(hipEventRecord(S.ev_e0, st));
      HIPC(hipStreamWaitEvent(S.estream, S.ev_e0, 0));
      D.st = S.estream;
      D.encode(which, seeks, nlen, slots, mel_stride, nctx);
      D.st = st;
      HIPC(hipEventRecord(S.ev_e1, S.estream));
      HIPC(hipStreamWaitEvent(st, S.ev_e1, 0));
    } else {
      D.encode(which, seeks, nlen, slots, mel_stride, nctx);
    }
    for (size_t i = 0; i < which.size(); ++i) clips[which[i]].enc_seek = seeks[i];
    return 0;
  };
  std::vector<std::string> lang_of_clip(n_clips, P.language ? P.language : "");
  for (int c = 0; c < n_clips; ++c)
    if (fixed_lang[c] >= 0) {
      clips[c].lang_id = fixed_lang[c];
      lang_of_clip[c] = lang_str(fixed_lang[c]);
    }
  if (detect) {
    std::vector<int> which, seeks;
    for (int c = 0; c < n_clips; ++c) {
      if (clips[c].n_len_org <= 0 || fixed_lang[c] >= 0) continue;
      which.push_back(c);
      seeks.push_back(0);
    }
    if (int rc = encode_clips(which, seeks, which)) return rc;
    const int R = (int)which.size();
    if (R > 0) {
      D.ensure_rows(R);
      D.build_static_mask();
      std::vector<int> si(4 * R, 0);
      std::vector<RowCtl> ctl(R);
      for (int r = 0; r < R; ++r) {
        si[r] = vb.token_sot;
        si[R + r] = 0;
        si[2 * R + r] = 1;
        si[3 * R + r] = which[r];
        memset(&ctl[r], 0, sizeof(RowCtl));
        ctl[r].active = 1;
        ctl[r].sample = 0;
      }
      HIPC(hipMemcpyAsync(S.stepin.p, si.data(), si.size() * 4, hipMemcpyHostToDevice, st));
      HIPC(hipMemcpyAsync(S.ctl.p, ctl.data(), R * sizeof(RowCtl), hipMemcpyHostToDevice, st));
      D.decode_step(R, false);
      const int nl = lang_max_id() + 1;
      std::vector<float> ll((size_t)R * nl);
      for (int r = 0; r < R; ++r)
        HIPC(hipMemcpyAsync(ll.data() + (size_t)r * nl,
                            (float*)S.logits.p + (size_t)r * V + vb.token_sot + 1, nl * 4,
                            hipMemcpyDeviceToHost, st));
      // the per-language distribution of the same rows (k_lang.hip), kept per
      // clip; the language used stays the host's choice from `ll` below
      std::vector<float> lp((size_t)R * nl);
      {
        float* d_lp = (float*)S.lg_probs.get((size_t)R * nl * 4);
        int* d_lb = (int*)S.lg_best.get((size_t)R * 4);
        {
          PerfScope ps(S, "lang");
          if (!lang_probs((const float*)S.logits.p, R, V, vb.token_sot + 1, nl, d_lp, d_lb, st))
            return -1;
        }
        HIPC(hipMemcpyAsync(lp.data(), d_lp, lp.size() * 4, hipMemcpyDeviceToHost, st));
      }
      HIPC(hipStreamSynchronize(st));
      for (int r = 0; r < R; ++r) {
        State& cs = states[which[r]]->s;
        cs.lang_probs.assign(lp.begin() + (size_t)r * nl, lp.begin() + (size_t)(r + 1) * nl);
        if (cs.lang_keep)
          cs.lang_last.assign(ll.begin() + (size_t)r * nl, ll.begin() + (size_t)(r + 1) * nl);
      }
      for (int r = 0; r < R; ++r) {
        std::vector<std::pair<float, int>> lid;
        for (const auto& kv : lang_table_sorted())
          lid.emplace_back(ll[(size_t)r * nl + kv.second], kv.second);
        std::sort(lid.begin(), lid.end(),
                  [](const std::pair<float, int>& a, const std::pair<float, int>& b) {
                    return a.first > b.first;
                  });
        clips[which[r]].lang_id = lid[0].second;
        lang_of_clip[which[r]] = lang_str(lid[0].second);
      }
    }
    if (P.detect_language) {
      for (int c = 0; c < n_clips; ++c) states[c]->s.lang_id = clips[c].lang_id;
      return 0;
    }
  }
  // (the energy copy lands before any decode step completes: stream order)
  // ---------------- per-clip setup ----------------
  {
    const bool is_distil = hp.n_text_layer == 2 && hp.n_vocab != 51866;
    if (is_distil && !P.no_timestamps) P.no_timestamps = true;
  }
  D.build_static_mask();
  std::vector<float> temps;
  if (P.temperature_inc > 0.0f && P.bench_fixed_steps <= 0) {
    for (float t = P.temperature; t < 1.0f + 1e-6f; t += P.temperature_inc) temps.push_back(t);
  } else {
    temps.push_back(P.temperature);
  }
  int n_decoders = P.strategy == MWX_SAMPLING_GREEDY ? P.greedy.best_of
                                                     : std::max(P.greedy.best_of, P.beam_search.beam_size);
  n_decoders = std::max(1, n_decoders);
  if (n_decoders > MWX_MAX_DECODERS) return -4;
  std::vector<int> prompt_tokens;
  if (P.prompt_tokens && P.prompt_n_tokens > 0) {
    if (!tokens_valid(P.prompt_tokens, P.prompt_n_tokens, hp.n_vocab)) {
      MWX_LOG_ERROR("mwx: prompt_tokens holds an id outside the vocabulary (0..%d)\n", hp.n_vocab - 1);
      return -3;
    }
    prompt_tokens.assign(P.prompt_tokens, P.prompt_tokens + P.prompt_n_tokens);
  } else if (P.initial_prompt) {
    prompt_tokens = tokenize(vb, P.initial_prompt);
  }
  const int delta_min = 10;
  for (int c = 0; c < n_clips; ++c) {
    ClipRun& cr = clips[c];
    cr.rng.resize(n_decoders);
    for (int j = 1; j < n_decoders; ++j) cr.rng[j] = std::mt19937(j);
    if (!prompt_tokens.empty()) {
      cr.prompt_past = prompt_tokens;  // no_context: prompt_past starts empty
    }
    cr.prompt_init = {vb.token_sot};
    if (vb.is_multilingual()) {
      const int li = lang_id(lang_of_clip[c]);
      if (li < 0) return -3;
      cr.lang_id = li;
      cr.prompt_init.push_back(vb.token_sot + 1 + li);
      cr.prompt_init.push_back(P.translate ? vb.token_translate : vb.token_transcribe);
    }
    if (P.no_timestamps) cr.prompt_init.push_back(vb.token_not);
    cr.seek_start = P.offset_ms / 10;
    cr.seek_end = P.duration_ms == 0 ? cr.n_len_org : cr.seek_start + P.duration_ms / 10;
    cr.seek = cr.seek_start;
    if (cr.seek_end < cr.seek_start + delta_min) cr.finished = true;
  }
  const int n_max = P.bench_fixed_steps > 0 ? P.bench_fixed_steps : hp.n_text_ctx / 2 - 4;

  // ---------------- contextual biasing (D14) ----------------
  // the call's matcher tables, built and uploaded once, before the first
  // window (validated by the caller: bias_check); the alignment pass and the
  // detection above run without them. bias_state: the state after a row's
  // generated ids (only the last MWX_BIAS_MAX_TOKENS can matter), the host's
  // side of RowRun.pad / RowCtl.pad[0]
  std::vector<int32_t> bias_tab;
  if (!align && P.bias_phrases && P.n_bias_phrases > 0) {
    bias_tab = bias_build(P.bias_phrases, P.n_bias_phrases);
    int* d_bt = (int*)S.bias_tab.get(bias_tab.size() * 4);
    HIPC(hipMemcpyAsync(d_bt, bias_tab.data(), bias_tab.size() * 4, hipMemcpyHostToDevice, st));
    D.bias_dev = d_bt;
  }
  auto bias_state = [&](const std::vector<mwx_token_data>& toks) {
    if (bias_tab.empty()) return 0;
    int s = 0;
    for (size_t i = toks.size() > MWX_BIAS_MAX_TOKENS ? toks.size() - MWX_BIAS_MAX_TOKENS : 0;
         i < toks.size(); ++i)
      s = bias_next_state(bias_tab.data(), s, toks[i].id);
    return s;
  };

  // ---------------- constrained decoding (D15) ----------------
  // the context's token byte table (first constrained call only) and the
  // call's table block, uploaded once before the first window; the alignment
  // pass and the detection above run without them. con_state: the state after
  // a row's generated ids from the start state, the host's side of RowRun.con
  // / RowCtl.pad[1]
  const mwx_constraint* con = align ? nullptr : P.constraint;
  ConBlock con_blk;
  ConView con_h{};
  if (con) {
    {
      std::lock_guard<std::mutex> lock(C.con_mu);
      if (!C.con_tok_dev) {
        C.con_tok = constraint_tokens(vb.id_to_token, vb.token_eot);
        std::lock_guard<std::recursive_mutex> cap(capture_mutex());
        uint8_t* d = nullptr;
        HIPC(hipMalloc((void**)&d, C.con_tok.data.size()));
        if (hipMemcpy(d, C.con_tok.data.data(), C.con_tok.data.size(), hipMemcpyHostToDevice) !=
            hipSuccess) {
          (void)hipFree(d);
          MWX_LOG_ERROR("mwx: token byte table upload failed\n");
          return -1;
        }
        C.con_tok_dev = d;
      }
    }
    con_blk = constraint_block(*con);
    uint8_t* d_blk = (uint8_t*)S.con_blk.get(con_blk.data.size());
    HIPC(hipMemcpyAsync(d_blk, con_blk.data.data(), con_blk.data.size(), hipMemcpyHostToDevice,
                        st));
    con_h = constraint_view(*con, C.con_tok);
    D.con_dev = constraint_view_dev(*con, con_blk, d_blk, C.con_tok, C.con_tok_dev);
    D.con_penalty = P.constraint_penalty;
  }
  auto con_state = [&](const std::vector<mwx_token_data>& toks) {
    if (!con) return 0;
    int s = con->start;
    for (const mwx_token_data& t : toks) s = con_next_state(con_h, s, t.id);
    return s;
  };
  if (!align)
    for (int c = 0; c < n_clips; ++c) states[c]->s.con_status = con ? 1 : -1;

  // ---------------- transcript alignment (D12) ----------------
  if (align) {
    // the clips mwx_full_batch would decode a window of, at seek 0
    std::vector<int> act;
    for (int c = 0; c < n_clips; ++c) {
      states[c]->s.align.clear();
      if (!clips[c].finished && clips[c].seek + delta_min < clips[c].seek_end) act.push_back(c);
    }
    {
      std::vector<int> which, seeks;
      for (int c : act)
        if (clips[c].enc_seek != 0) {
          which.push_back(c);
          seeks.push_back(0);
        }
      D.live_slots = act;
      if (int rc = encode_clips(which, seeks, act)) return rc;
    }
    std::vector<typename Driver<T>::DtwClip> dc;
    for (int c : act) {
      typename Driver<T>::DtwClip x;
      x.slot = c;
      x.tokens = clips[c].prompt_init;
      if (P.no_timestamps) x.tokens.pop_back();  // (its NOT: the first scored row)
      x.pos0 = (int)x.tokens.size();
      x.tokens.push_back(vb.token_not);
      x.tokens.insert(x.tokens.end(), align->tokens[c], align->tokens[c] + align->n_tokens[c]);
      x.tokens.push_back(vb.token_eot);
      x.n_rows = (int)x.tokens.size() - x.pos0;
      x.n_cols = std::max(1, std::min(D.slot_keys(c), ((int)clips[c].seek_end + 1) / 2));
      dc.push_back(std::move(x));
    }
    if (!dc.empty()) {
      if (aborted(P)) return -9;
      std::vector<typename Driver<T>::AlignOut> out;
      D.align_pass(dc, out, C.dtw);
      for (size_t i = 0; i < dc.size(); ++i) {
        const int c = dc[i].slot, n = align->n_tokens[c];
        State& cs = states[c]->s;
        cs.align = out[i].rows;
        if ((int)cs.align.size() != n + 1) return -1;
        Segment sg{0, clips[c].seek_end, "", 0.0f, {}, false};
        for (int j = 0; j < n; ++j) {
          mwx_token_data td;
          memset(&td, 0, sizeof(td));
          td.id = td.tid = align->tokens[c][j];
          td.p = cs.align[j].p;
          td.plog = cs.align[j].plog;
          td.t0 = td.t1 = -1;
          td.t_dtw = dc[i].frames.empty() ? -1 : 2 * (int64_t)dc[i].frames[j + 1];
          sg.text += vb.id_to_token[td.id];
          sg.tokens.push_back(td);
        }
        cs.result_all.push_back(std::move(sg));
      }
    }
    for (int c = 0; c < n_clips; ++c) states[c]->s.lang_id = clips[c].lang_id;
    return 0;
  }

  // ---------------- window loop ----------------
  while (true) {
    std::vector<int> act;
    for (int c = 0; c < n_clips; ++c) {
      ClipRun& cr = clips[c];
      if (cr.finished) continue;
      if (cr.seek + delta_min >= cr.seek_end) {
        cr.finished = true;
        continue;
      }
      act.push_back(c);
    }
    if (act.empty()) break;
    {
      std::vector<int> which, seeks;
      for (int c : act)
        if (clips[c].enc_seek != clips[c].seek) {
          which.push_back(c);
          seeks.push_back(clips[c].seek);
        }
      D.live_slots = act;  // (also when nothing is encoded: the detection's encode is reused)
      if (int rc = encode_clips(which, seeks, act)) return rc;
    }
    for (int c : act) {
      ClipRun& cr = clips[c];
      if (cr.seek > cr.seek_start && cr.seek + 500 >= cr.seek_end) cr.prompt_past.clear();
    }
    // result per clip for this window
    std::vector<Row> best_row(n_clips);
    std::vector<int> pending = act;
    // whisper.cpp v1.8.2 keeps best_decoder_id across a window's attempts
    // (declared before the temperature loop), and a decoder an attempt does
    // not run (j >= n_decoders_cur: beam search's fallbacks run best_of = 1)
    // keeps what its last attempt left: when every decoder of an attempt
    // fails, the window's result is decoders[best_decoder_id] as it stands —
    // possibly an earlier attempt's decoder (oracle: mwx_oracle.cpp best_id)
    std::vector<int> best_dec(n_clips, 0);
    std::vector<std::vector<Row>> dec_last(n_clips);
    S.n_windows += (long)act.size();
    for (int it = 0; it < (int)temps.size() && !pending.empty(); ++it) {
      const float t_cur = temps[it];
      S.n_attempts += (long)pending.size();
      int n_cur = 1;
      if (beam)
        n_cur = t_cur > 0.0f ? P.greedy.best_of : P.beam_search.beam_size;
      else if (t_cur > 0.0f)
        n_cur = P.greedy.best_of;
      n_cur = std::max(1, n_cur);
      const bool sampling = t_cur >= 1e-6f;
      // rows draw from their probs with std::discrete_distribution (device
      // kernel; the uniforms come from the rows' std::mt19937 on the host)
      const bool host_probs = sampling || beam;
      const int n_draw = beam ? P.beam_search.beam_size : 1;
      if (host_probs && (n_draw < 1 || n_draw > 16)) {
        MWX_LOG_ERROR("mwx: beam_size %d unsupported (1..16)\n", n_draw);
        return -7;
      }
      // run-ahead safety net: if the device's advance and the host's replay of
      // the same rules ever disagree (or the beam grouping is one the advance
      // kernel does not take), the attempt is redone from its start on the
      // host-driven loop (the MWX_NO_RUNAHEAD path): the rows' RNGs are only
      // advanced once a run-ahead loop has finished, so the redo draws the
      // same uniforms
      bool force_host = false;
    redo_attempt:
      std::vector<Row> rows;
      for (int c : pending) {
        ClipRun& cr = clips[c];
        cr.prompt.clear();
        if (!cr.prompt_past.empty() && t_cur < 0.5f && P.n_max_text_ctx > 0) {
          const int n_take = std::min(std::min(P.n_max_text_ctx, hp.n_text_ctx / 2),
                                      (int)cr.prompt_past.size());
          cr.prompt = {vb.token_prev};
          cr.prompt.insert(cr.prompt.begin() + 1, cr.prompt_past.end() - n_take,
                           cr.prompt_past.end());
        }
        cr.prompt.insert(cr.prompt.end(), cr.prompt_init.begin(), cr.prompt_init.end());
        for (int j = 0; j < n_cur; ++j) {
          Row w;
          w.clip = c;
          w.dec = j;
          rows.push_back(w);
        }
      }
      const int R = (int)rows.size();
      D.xgroup = n_cur;
      D.ensure_rows(R);
      D.reset_kv_maps(R);  // every row starts on its own (empty) history
      // batched prompt prefill (whisper.cpp decodes the prompt in one
      // whisper_decode call): positions 0 .. P_len-2 of each clip's prompt on
      // its first decoder row in one pass of the layer stack; the clip's other
      // decoders take that history over through their position maps (no
      // copy), and every row's decode loop starts at the prompt's last
      // position, the first sampling step. MWX_PREFILL_MIN (default 2):
      // prompts with fewer positions to prefill step through them instead;
      // 0 disables the prefill.
      {
        static const int pf_min =
            getenv("MWX_PREFILL_MIN") ? atoi(getenv("MWX_PREFILL_MIN")) : 2;
        if (pf_min > 0) {
          std::vector<typename Driver<T>::PrefillRow> prs;
          std::vector<int> kv_moves;
          for (int r = 0; r < R; ++r) {
            Row& w = rows[r];
            const ClipRun& cr = clips[w.clip];
            const int n = (int)cr.prompt.size() - 1;
            if (n < pf_min || n >= D.Tctx) continue;
            if (w.dec == 0)
              prs.push_back({r, w.clip, cr.prompt.data(), n});
            else
              kv_moves.insert(kv_moves.end(), {r, r - w.dec, n});
            w.fed = n;
          }
          if (!prs.empty()) {
            if (aborted(P)) return -9;
            D.prefill(prs);
            D.copy_kv_rows(kv_moves);
          }
        }
      }
      std::vector<int> si(4 * R);
      std::vector<RowCtl> ctl(R);
      std::vector<TokOut> out(R);
      std::vector<double> uh;
      std::vector<int> ndh;
      // pinned staging: [si | ctl | out | uh | ndh | draws], 64-B aligned parts
      auto al64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
      const size_t nd_all = host_probs ? (size_t)R * n_draw : 0;
      const size_t o_si = 0, o_ctl = al64(si.size() * 4), o_out = o_ctl + al64(R * sizeof(RowCtl)),
                   o_uh = o_out + al64(R * sizeof(TokOut)), o_nd = o_uh + al64(nd_all * 8),
                   o_dr = o_nd + al64((size_t)R * 4), o_rr = o_dr + al64(nd_all * sizeof(Draw)),
                   o_rp = o_rr + al64((size_t)R * sizeof(RowRun)),
                   pin_total = o_rp + al64((size_t)R * D.Tctx * 4);
      char* pin = (char*)S.pinned(pin_total);
      auto h2d = [&](void* dst, const void* src, size_t off, size_t bytes) {
        memcpy(pin + off, src, bytes);
        HIPC(hipMemcpyAsync(dst, pin + off, bytes, hipMemcpyHostToDevice, st));
      };
      if (con) S.con_mask.get((size_t)R * ((V + 63) / 64) * 8);  // (before any graph capture)
      if (host_probs) {
        S.probs.get((size_t)R * V * 4);  // allocate before any graph capture
        S.logprobs.get((size_t)R * V * 4);
        S.draw_k = n_draw;
        S.du.get((size_t)R * n_draw * 8);
        S.dnd.get((size_t)R * 4);
        S.dneed.get((size_t)R * 4);
        S.ddraw.get((size_t)R * n_draw * sizeof(Draw));
        S.draws_h.resize((size_t)R * n_draw);
        uh.assign((size_t)R * n_draw, 0.0);
        ndh.assign(R, 0);
      }
      // every step of this loop runs the same launch sequence on the same
      // buffers: capture it once into a hipGraph and replay it per step. With
      // a perf class enabled, a second (instrumented) graph carries the
      // event-record nodes / span slots and replaces the plain one on every
      // perf_period-th step: the measurement stays live inside the timed
      // steps while its nodes (and event harvesting) cost 1/perf_period
      std::vector<hipGraph_t> graph(2, nullptr);
      std::vector<hipGraphExec_t> gexec(2, nullptr);
      const bool use_graph = getenv("MWX_NO_GRAPH") == nullptr;
      const bool perf_on = !S.perf_class.empty();
      static const int perf_period = getenv("MWX_PERF_PERIOD") ? std::max(1, atoi(getenv("MWX_PERF_PERIOD"))) : 8;
      long step_i = 0;
      struct GraphGuard {
        std::vector<hipGraph_t>& g;
        std::vector<hipGraphExec_t>& e;
        State& S;
        ~GraphGuard() {
          for (auto x : e)
            if (x) (void)hipGraphExecDestroy(x);
          for (auto x : g)
            if (x) (void)hipGraphDestroy(x);
          S.perf_gused = 0;
          S.span_gused = 0;
          S.capturing = false;
        }
      } gguard{graph, gexec, S};
      // --- one decode step: inputs from the host row states, the captured step
      // graph (+ the run-ahead advance kernel), the host token-loop rules ---
      auto fill_inputs = [&]() {
        for (int r = 0; r < R; ++r) {
          Row& w = rows[r];
          ClipRun& cr = clips[w.clip];
          const int P_len = (int)cr.prompt.size();
          RowCtl& k = ctl[r];
          memset(&k, 0, sizeof(k));
          si[r] = w.fed < P_len ? cr.prompt[w.fed] : (w.tokens.empty() ? 0 : w.tokens.back().id);
          si[R + r] = w.fed;
          si[2 * R + r] = w.stopped ? 0 : 1;
          si[3 * R + r] = w.clip;
          k.active = w.stopped ? 0 : 1;
          k.sample = (!w.stopped && w.fed >= P_len - 1) ? 1 : 0;
          k.is_initial = w.tokens.empty() ? 1 : 0;
          k.last_ts = (!w.tokens.empty() && w.tokens.back().id >= vb.token_beg) ? 1 : 0;
          k.penult_ts = (w.tokens.size() < 2 || w.tokens[w.tokens.size() - 2].id >= vb.token_beg) ? 1 : 0;
          k.has_ts = w.has_ts ? 1 : 0;
          k.seek_delta = w.seek_delta;
          k.want_probs = host_probs ? 1 : 0;
          k.temperature = t_cur;
          k.want_nosp = (k.sample && k.is_initial) ? 1 : 0;
          k.pad[0] = bias_state(w.tokens);
          k.pad[1] = con_state(w.tokens);
        }
      };
      // run-ahead (every decode mode: greedy, temperature sampling, beam
      // search at any temperature; graphs): the device applies the token
      // loop's rules after each step (row_advance / beam_advance: the beam
      // step too) so step k+1 is queued before the host has read step k; the
      // host replays the same rules on the reported tokens (and draws) and
      // checks the device chose the same inputs. Rows that draw take their
      // uniforms from a ring the host fills ahead from copies of their RNGs.
      const bool beam_ra = beam;
      const bool samp_ra = sampling && !beam;
      const bool draw_ra = beam_ra || samp_ra;  // (== host_probs)
      const bool runahead = !force_host && use_graph &&
                            (!perf_on || perf_period >= 2) && getenv("MWX_NO_RUNAHEAD") == nullptr;
      // test hook: MWX_TEST_RA_MISMATCH=k treats run-ahead step k as a mismatch
      const long ra_fault_step = ra_fault_step_now();
      RunConst rc{};
      RunReport* ring = nullptr;
      RunReport* ring_dev = nullptr;
      BeamRun brun{};
      auto advance_rows = [&](hipStream_t gs) {
        const PickIn pk = D.pick_in();
        if (beam_ra)
          beam_advance((RowRun*)S.rrun.p, (int*)((RowRun*)S.rrun.p + R), (const int*)S.rprompt.p,
                       (int*)S.stepin.p, (RowCtl*)S.ctl.p, (TokOut*)S.tokout.p, ring_dev, rc,
                       brun, pk, gs);
        else
          row_advance((RowRun*)S.rrun.p, (int*)((RowRun*)S.rrun.p + R), (const int*)S.rprompt.p,
                      (int*)S.stepin.p, (RowCtl*)S.ctl.p, (TokOut*)S.tokout.p, ring_dev, rc, brun,
                      pk, gs);
      };
      bool last_instr = false;
      auto launch_step = [&](bool advance) {
        const bool instr = perf_on && step_i % perf_period == 0;
        ++step_i;
        ++S.n_steps;
        if (use_graph) {
          const int gi = instr ? 1 : 0;
          if (!gexec[gi]) {
            std::lock_guard<std::recursive_mutex> lock(capture_mutex());
            if (instr) {
              S.perf_gused = S.span_gused = 0;
              // (graph span slots zero before the first instrumented replay)
              if (S.perf_span.p)
                HIPC(hipMemsetAsync(S.perf_span.p, 0, (size_t)State::SPAN_G * SPAN_SLOT_U64 * 8,
                                    st));
            }
            S.capturing = true;
            S.capture_perf = instr;
            HIPC(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            D.pick_in_advance = advance;  // (the advance kernel picks the tokens)
            D.decode_rows(R, host_probs, st);
            D.pick_in_advance = false;
            if (advance) advance_rows(st);
            HIPC(hipStreamEndCapture(st, &graph[gi]));
            S.capturing = false;
            S.capture_perf = true;
            HIPC(hipGraphInstantiate(&gexec[gi], graph[gi], nullptr, nullptr, 0));
          }
          HIPC(hipGraphLaunch(gexec[gi], st));
        } else {
          D.pick_in_advance = advance;
          D.decode_rows(R, host_probs, st);
          D.pick_in_advance = false;
          if (advance) advance_rows(st);
        }
        last_instr = instr;
      };
      std::vector<int> kv_moves;  // beam search: (dst row, src row, npos) of the last step
      auto process_step = [&]() -> bool {
        bool any = false;
        kv_moves.clear();
        {  // clips with a live row in this step (rows of a clip are consecutive)
          int prev = -1;
          for (int r = 0; r < R; ++r)
            if (!rows[r].stopped && rows[r].clip != prev) {
              ++S.n_clip_steps;
              prev = rows[r].clip;
            }
        }
        if (beam) beam_step(rows, clips, ctl, out, S, n_cur, vb.token_beg, P.beam_search.beam_size, kv_moves);
        for (int r = 0; r < R; ++r) {
          Row& w = rows[r];
          if (w.stopped) continue;
          ClipRun& cr = clips[w.clip];
          if (ctl[r].sample && !beam) {
            if (ctl[r].is_initial && w.dec == 0) cr.no_speech_prob = out[r].nosp;
            mwx_token_data td;
            td.tid = out[r].tid;
            td.pt = out[r].pt;
            td.ptsum = out[r].ptsum;
            td.t0 = td.t1 = td.t_dtw = -1;
            td.vlen = 0.0f;
            if (!sampling) {
              td.id = out[r].id;
              td.p = out[r].p;
              td.plog = out[r].plog;
            } else {
              const Draw& dr = S.draws_h[(size_t)r * n_draw];
              td.id = dr.id;
              td.p = dr.p;
              td.plog = dr.plog;
            }
            if (td.id >= vb.token_beg) {
              td.tid = td.id;
              td.pt = td.p;
            }
            w.tokens.push_back(td);
            w.sum_logprobs_all += td.plog;
          }
          if (ctl[r].sample) {
            const mwx_token_data td = w.tokens.back();
            const int i = (int)w.tokens.size() - 1;
            bool stop = false;
            if (td.id > vb.token_beg) {
              const int sd_new = 2 * (td.id - vb.token_beg);
              if (w.has_ts && w.seek_delta > sd_new && w.result_len < i) {
                w.failed = true;
                stop = true;
              } else {
                w.seek_delta = sd_new;
                w.result_len = i + 1;
                w.has_ts = true;
              }
            }
            if (!stop) {
              if (td.id == vb.token_eot || (P.max_tokens > 0 && i >= P.max_tokens) ||
                  (w.has_ts && cr.seek + w.seek_delta + delta_min >= cr.seek_end)) {
                stop = true;
                if (w.result_len == 0 && !P.no_timestamps) {
                  if (cr.seek + w.seek_delta + delta_min >= cr.seek_end) {
                    w.result_len = i + 1;
                  } else {
                    w.failed = true;
                  }
                }
                if (!w.failed) {
                  if (P.single_segment || P.no_timestamps) {
                    w.result_len = i + 1;
                    w.seek_delta = 100 * MWX_CHUNK_SIZE;
                  }
                  w.completed = true;
                }
              } else if (i == n_max - 1) {
                stop = true;
                if (w.result_len == 0 || w.seek_delta < 100 * MWX_CHUNK_SIZE / 2) w.failed = true;
              }
            }
            if (stop) {
              w.stopped = true;
              continue;
            }
          }
          w.fed++;
          any = true;
        }
        if (!runahead) D.copy_kv_rows(kv_moves);  // (run-ahead: beam_advance moved the maps)
        return any;
      };
      if (!runahead) {
        bool any = true;
        while (any) {
          if (aborted(P)) return -9;
          fill_inputs();
          h2d(S.stepin.p, si.data(), o_si, si.size() * 4);
          h2d(S.ctl.p, ctl.data(), o_ctl, R * sizeof(RowCtl));
          if (host_probs) {
            // the uniforms std::discrete_distribution::operator() would draw
            // (generate_canonical<double, 53> of the decoder's std::mt19937), in
            // the same per-decoder order: beam search draws beam_size per live
            // decoder of a clip (rows step in lockstep), sampling one per row
            for (int r = 0; r < R; ++r) {
              const Row& w = rows[r];
              ndh[r] = (!w.stopped && ctl[r].sample) ? n_draw : 0;
              ClipRun& cr = clips[w.clip];
              std::mt19937& rng = w.dec == 0 ? cr.st->rng0 : cr.rng[w.dec];
              for (int k = 0; k < ndh[r]; ++k)
                uh[(size_t)r * n_draw + k] =
                    std::generate_canonical<double, std::numeric_limits<double>::digits>(rng);
            }
            h2d(S.du.p, uh.data(), o_uh, uh.size() * 8);
            h2d(S.dnd.p, ndh.data(), o_nd, ndh.size() * 4);
          }
          launch_step(false);
          HIPC(hipMemcpyAsync(pin + o_out, S.tokout.p, R * sizeof(TokOut), hipMemcpyDeviceToHost, st));
          if (host_probs)
            HIPC(hipMemcpyAsync(pin + o_dr, S.ddraw.p, S.draws_h.size() * sizeof(Draw),
                                hipMemcpyDeviceToHost, st));
          HIPC(hipStreamSynchronize(st));
          memcpy(out.data(), pin + o_out, R * sizeof(TokOut));
          if (host_probs) memcpy(S.draws_h.data(), pin + o_dr, S.draws_h.size() * sizeof(Draw));
          if ((S.perf_gused || S.span_gused) && last_instr) {
            harvest_events(S.perf_gev, S.perf_gtag, S.perf_gused, S);
            harvest_spans(S, true);
          }
          any = process_step();
        }
      } else {
        fill_inputs();  // step 0 inputs
        h2d(S.stepin.p, si.data(), o_si, si.size() * 4);
        h2d(S.ctl.p, ctl.data(), o_ctl, R * sizeof(RowCtl));
        // device row states (+ the step counter after them) and prompts, built
        // in the pinned staging: async uploads, no synchronize (the host
        // captures the step graph while the window's encoder still runs)
        RowRun* rr = reinterpret_cast<RowRun*>(pin + o_rr);
        int* rp = reinterpret_cast<int*>(pin + o_rp);
        memset(rp, 0, (size_t)R * D.Tctx * 4);
        for (int r = 0; r < R; ++r) {
          const Row& w = rows[r];
          const ClipRun& cr = clips[w.clip];
          const int P_len = (int)cr.prompt.size();
          if (P_len > D.Tctx) {
            MWX_LOG_ERROR("mwx: prompt of %d tokens exceeds the text context\n", P_len);
            return -10;
          }
          RowRun& x = rr[r];
          memset(&x, 0, sizeof(x));
          x.fed = w.fed;
          x.p_len = P_len;
          x.ntok = (int)w.tokens.size();
          x.last_id = x.ntok > 0 ? w.tokens.back().id : 0;
          x.penult_id = x.ntok > 1 ? w.tokens[x.ntok - 2].id : 0;
          x.has_ts = w.has_ts ? 1 : 0;
          x.seek_delta = w.seek_delta;
          x.result_len = w.result_len;
          x.stopped = w.stopped ? 1 : 0;
          x.seek = cr.seek;
          x.seek_end = cr.seek_end;
          x.sum = w.sum_logprobs_all;
          x.pad = bias_state(w.tokens);
          x.con = con_state(w.tokens);
          std::copy(cr.prompt.begin(), cr.prompt.end(), rp + (size_t)r * D.Tctx);
        }
        constexpr int NS = State::RUN_SLOTS;
        // pinned ring: [RunReport NS][R] | beam: [BeamReport NS][R] |
        // draws (beam, sampling): [Draw NS][R][KD] | uniforms [R][RING]
        const int KD = n_draw, RING = 8 * n_draw;
        const size_t o_brep = (size_t)NS * R * sizeof(RunReport),
                     o_drep = o_brep + (beam_ra ? (size_t)NS * R * sizeof(BeamReport) : 0),
                     o_ur = o_drep + (draw_ra ? (size_t)NS * R * KD * sizeof(Draw) : 0),
                     ring_bytes = o_ur + (draw_ra ? (size_t)R * RING * 8 : 0);
        ring = S.report_ring(ring_bytes);
        HIPC(hipHostGetDevicePointer((void**)&ring_dev, ring, 0));
        // beam / sampling: the uniforms of every row's RNG stream, generated ahead into
        // the ring (from a copy of the row's std::mt19937; the row's own RNG is
        // advanced by the draws actually consumed once the loop ends)
        std::vector<std::mt19937> la;
        std::vector<long> gen, used_h;
        double* uring = reinterpret_cast<double*>(reinterpret_cast<char*>(ring) + o_ur);
        auto refill = [&]() {
          for (int r = 0; r < R; ++r)
            for (; gen[r] < used_h[r] + RING; ++gen[r])
              uring[(size_t)r * RING + gen[r] % RING] =
                  std::generate_canonical<double, std::numeric_limits<double>::digits>(la[r]);
        };
        auto row_rng = [&](int r) -> std::mt19937& {
          const Row& w = rows[r];
          return w.dec == 0 ? clips[w.clip].st->rng0 : clips[w.clip].rng[w.dec];
        };
        if (draw_ra) {
          for (int r = 0; r < R; ++r) la.push_back(row_rng(r));
          gen.assign(R, 0);
          used_h.assign(R, 0);
          refill();
          for (int r = 0; r < R; ++r) {
            ndh[r] = (!rows[r].stopped && ctl[r].sample) ? KD : 0;
            for (int k = 0; k < ndh[r]; ++k) uh[(size_t)r * KD + k] = uring[(size_t)r * RING + k];
            used_h[r] = ndh[r];
            rr[r].used = ndh[r];
          }
          h2d(S.du.p, uh.data(), o_uh, uh.size() * 8);
          h2d(S.dnd.p, ndh.data(), o_nd, ndh.size() * 4);
          char* dring = reinterpret_cast<char*>(ring_dev);
          brun.draws = (const Draw*)S.ddraw.p;
          brun.KD = KD;
          brun.n = n_cur;
          brun.du = (double*)S.du.p;
          brun.dnd = (int*)S.dnd.p;
          brun.uring = (const double*)(dring + o_ur);
          brun.ring_n = RING;
          brun.kvmap = (int*)S.kvmap.p;
          brun.kvown = (int*)S.kvown.p;
          brun.Tctx = D.Tctx;
          brun.brep = (BeamReport*)(dring + o_brep);
          brun.drep = (Draw*)(dring + o_drep);
          if (beam_ra && (R % n_cur || n_cur > 16)) {
            MWX_LOG_WARN("mwx: beam run-ahead: %d rows in groups of %d; host loop\n", R, n_cur);
            HIPC(hipStreamSynchronize(st));
            note_ra_fallback(S, "unsupported beam grouping");
            force_host = true;
            goto redo_attempt;
          }
        }
        const BeamReport* brep = reinterpret_cast<const BeamReport*>(reinterpret_cast<char*>(ring) + o_brep);
        const Draw* drep = reinterpret_cast<const Draw*>(reinterpret_cast<char*>(ring) + o_drep);
        // step counters after the row states: one (greedy) or one per clip (beam)
        const int n_ctr = beam_ra ? R / n_cur : 1;
        S.rrun.get((size_t)R * sizeof(RowRun) + (size_t)R * 4 + 64);
        S.rprompt.get((size_t)R * D.Tctx * 4);
        HIPC(hipMemcpyAsync(S.rrun.p, rr, (size_t)R * sizeof(RowRun), hipMemcpyHostToDevice, st));
        HIPC(hipMemsetAsync((RowRun*)S.rrun.p + R, 0, (size_t)n_ctr * 4, st));
        HIPC(hipMemcpyAsync(S.rprompt.p, rp, (size_t)R * D.Tctx * 4, hipMemcpyHostToDevice, st));
        rc.beg = vb.token_beg;
        rc.eot = vb.token_eot;
        rc.max_tokens = P.max_tokens;
        rc.n_max = n_max;
        rc.delta_min = delta_min;
        rc.R = R;
        rc.nslot = NS;
        rc.prompt_stride = D.Tctx;
        rc.temperature = t_cur;
        rc.want_probs = host_probs ? 1 : 0;
        rc.bias = D.bias_dev;
        rc.con = D.con_dev;
        for (int i = 0; i < NS; ++i)
          if (!S.ev_step[i]) HIPC(hipEventCreateWithFlags(&S.ev_step[i], hipEventDisableTiming));
        bool instr_of[NS] = {};
        // every row still running samples its n_max-th token (or passes
        // max_tokens) in the step just queued: no step after it is needed
        auto certain_stop_all = [&]() {
          for (int r = 0; r < R; ++r) {
            const Row& w = rows[r];
            if (w.stopped) continue;
            if (!ctl[r].sample) return false;
            const int i = (int)w.tokens.size();
            if (i == n_max - 1 || (P.max_tokens > 0 && i >= P.max_tokens)) continue;
            return false;
          }
          return true;
        };
        long k = 0;
        launch_step(true);
        instr_of[0] = last_instr;
        HIPC(hipEventRecord(S.ev_step[0], st));
        bool spec = false;  // a step past the last one needed was queued
        while (true) {
          if (aborted(P)) {
            HIPC(hipStreamSynchronize(st));
            return -9;
          }
          const bool next = !certain_stop_all();
          if (next) {
            launch_step(true);
            instr_of[(k + 1) % NS] = last_instr;
            HIPC(hipEventRecord(S.ev_step[(k + 1) % NS], st));
          }
          HIPC(hipEventSynchronize(S.ev_step[k % NS]));
          const RunReport* rpk = ring + (size_t)(k % NS) * R;
          for (int r = 0; r < R; ++r) out[r] = rpk[r].out;
          if (draw_ra)
            memcpy(S.draws_h.data(), drep + (size_t)(k % NS) * R * KD, (size_t)R * KD * sizeof(Draw));
          if ((S.perf_gused || S.span_gused) && instr_of[k % NS] && !(next && instr_of[(k + 1) % NS])) {
            harvest_events(S.perf_gev, S.perf_gtag, S.perf_gused, S);
            harvest_spans(S, true);
          }
          const bool any = process_step();
          if (beam_ra) {
            // the decoder hand-overs: the device's (src per row) == the host's
            std::vector<int> hsrc(R);
            for (int r = 0; r < R; ++r) hsrc[r] = r;
            for (size_t i = 0; i + 2 < kv_moves.size(); i += 3) hsrc[kv_moves[i]] = kv_moves[i + 1];
            for (int r = 0; r < R; ++r)
              if (brep[(size_t)(k % NS) * R + r].src != hsrc[r] || k == ra_fault_step) {
                MWX_LOG_WARN("mwx: run-ahead beam: device and host disagree on row %d's parent at "
                             "step %ld; attempt redone on the host loop\n", r, k);
                HIPC(hipStreamSynchronize(st));
                note_ra_fallback(S, "beam parent mismatch");
                force_host = true;
                goto redo_attempt;
              }
          } else if (k == ra_fault_step) {
            HIPC(hipStreamSynchronize(st));
            note_ra_fallback(S, "injected fault");
            force_host = true;
            goto redo_attempt;
          }
          if (!any) {
            spec = next;
            break;
          }
          if (!next) {
            MWX_LOG_WARN("mwx: run-ahead decode: rows still running after a certain stop; "
                         "attempt redone on the host loop\n");
            HIPC(hipStreamSynchronize(st));
            note_ra_fallback(S, "rows still running after a certain stop");
            force_host = true;
            goto redo_attempt;
          }
          fill_inputs();  // the host's inputs of step k+1
          for (int r = 0; r < R; ++r) {
            const RunReport& q = rpk[r];
            const bool same = q.act == si[2 * R + r] &&
                              (!q.act || (q.tok == si[r] && q.pos == si[R + r] &&
                                          memcmp(&q.next, &ctl[r], sizeof(RowCtl)) == 0));
            const int nd = (draw_ra && !rows[r].stopped && ctl[r].sample) ? KD : 0;
            if (!same || (beam_ra && brep[(size_t)(k % NS) * R + r].nd != nd)) {
              MWX_LOG_WARN("mwx: run-ahead decode: device and host disagree on row %d at step %ld; "
                           "attempt redone on the host loop\n", r, k + 1);
              HIPC(hipStreamSynchronize(st));
              note_ra_fallback(S, "step inputs mismatch");
              force_host = true;
              goto redo_attempt;
            }
            if (draw_ra) used_h[r] += nd;
          }
          if (draw_ra) refill();
          ++k;
        }
        // the queued step past the end ran on inactive rows only; its graph
        // must finish before the graphs are destroyed
        if (spec) HIPC(hipStreamSynchronize(st));
        if (draw_ra)  // each row's RNG past the uniforms its draws consumed
          for (int r = 0; r < R; ++r) {
            std::mt19937& rng = row_rng(r);
            for (long i = 0; i < used_h[r]; ++i)
              (void)std::generate_canonical<double, std::numeric_limits<double>::digits>(rng);
          }
      }
      // rank decoders per clip, decide fallback
      std::vector<int> still;
      for (int c : pending) {
        ClipRun& cr = clips[c];
        std::vector<Row>& dl = dec_last[c];
        if ((int)dl.size() < n_cur) dl.resize(n_cur);
        double best_score = -INFINITY;
        for (int r = 0; r < R; ++r) {
          Row& w = rows[r];
          if (w.clip != c) continue;
          if (!w.failed) {
            w.tokens.resize(w.result_len);
            sequence_score(P, w);
            if (w.result_len > 32 && w.entropy < P.entropy_thold) {
              w.failed = true;
            } else if (best_score < w.score) {
              best_score = w.score;
              best_dec[c] = w.dec;
            }
          }
          dl[w.dec] = w;
        }
        const Row& b = dl[best_dec[c]];
        bool success = true;
        if (it != (int)temps.size() - 1) {
          if (b.failed || (b.avg_logprobs < P.logprob_thold && cr.no_speech_prob < P.no_speech_thold))
            success = false;
        }
        best_row[c] = b;
        if (!success) still.push_back(c);
      }
      pending = still;
    }
    // ---------------- emit segments ----------------
    // token timestamps (whisper_exp_compute_token_level_timestamps) of the
    // emitted segments run after the loop, clips in parallel on host threads:
    // a clip's segments stay in order (its TsState carries from one to the
    // next), each token's energy sums stay sequential (same floats)
    std::vector<std::vector<size_t>> ts_todo(P.token_timestamps ? n_clips : 0);
    // DTW token timestamps: the window's seek and first segment per clip
    std::vector<int64_t> dtw_seek(C.dtw ? n_clips : 0);
    std::vector<size_t> dtw_seg0(C.dtw ? n_clips : 0);
    for (int c : act) {
      ClipRun& cr = clips[c];
      State& cs = *cr.st;
      if (C.dtw) {
        dtw_seek[c] = cr.seek;
        dtw_seg0[c] = cs.result_all.size();
      }
      const Row& best = best_row[c];
      if (con) {  // (mwx_full_constraint_status_from_state)
        const int s_end = con_state(best.tokens);
        if (!(s_end > 0 && con->acc[s_end])) cs.con_status = 0;
      }
      const int seek_delta = best.seek_delta;
      const int result_len = best.result_len;
      const auto& toks = best.tokens;
      const bool is_no_speech =
          cr.no_speech_prob > P.no_speech_thold && best.avg_logprobs < P.logprob_thold;
      const size_t n_init = cr.prompt_init.size();
      std::vector<int> new_past;
      if (!cr.prompt.empty() && cr.prompt.front() == vb.token_prev)
        new_past.insert(new_past.end(), cr.prompt.begin() + 1, cr.prompt.end() - n_init);
      for (int i = 0; i < result_len && !is_no_speech; ++i) new_past.push_back(toks[i].id);
      cr.prompt_past = new_past;
      if (!toks.empty() && !is_no_speech) {
        int i0 = 0;
        int64_t t0 = cr.seek + 2 * (toks.front().tid - vb.token_beg);
        std::string text;
        bool stn = false;
        for (int i = 0; i < (int)toks.size(); i++) {
          if (P.print_special || toks[i].id < vb.token_eot) text += vb.id_to_token[toks[i].id];
          if (P.tdrz_enable && toks[i].id == vb.token_solm) stn = true;
          if (toks[i].id > vb.token_beg && !P.single_segment) {
            const int64_t t1 = cr.seek + 2 * (toks[i].tid - vb.token_beg);
            if (!text.empty()) {
              Segment sg{t0, t1, text, cr.no_speech_prob, {}, stn};
              for (int j = i0; j <= i; j++) sg.tokens.push_back(toks[j]);
              cs.result_all.push_back(sg);
              if (P.token_timestamps) ts_todo[c].push_back(cs.result_all.size() - 1);
            }
            text = "";
            while (i < (int)toks.size() && toks[i].id > vb.token_beg) i++;
            i--;
            t0 = t1;
            i0 = i + 1;
            stn = false;
          }
        }
        if (!text.empty()) {
          const int64_t t1 = cr.seek + seek_delta;
          Segment sg{t0, t1, text, cr.no_speech_prob, {}, stn};
          for (int j = i0; j < (int)toks.size(); j++) sg.tokens.push_back(toks[j]);
          cs.result_all.push_back(sg);
          if (P.token_timestamps) ts_todo[c].push_back(cs.result_all.size() - 1);
        }
      }
      // benchmark workload (bench_fixed_steps): every window decodes the fixed
      // step count and the clip advances by a whole window (long-form clips
      // run window after window)
      cr.seek += P.bench_fixed_steps > 0 ? 100 * MWX_CHUNK_SIZE : seek_delta;
    }
    if (P.token_timestamps) {
      std::vector<int> todo;
      for (int c = 0; c < n_clips; ++c)
        if (!ts_todo[c].empty()) todo.push_back(c);
      auto run_clip = [&](int c) {
        for (size_t si : ts_todo[c])
          token_timestamps(C, clips[c].ts, clips[c].st->result_all[si], P.thold_pt, P.thold_ptsum);
      };
      static const int ts_threads =
          getenv("MWX_TS_THREADS") ? std::max(1, atoi(getenv("MWX_TS_THREADS"))) : 8;
      // small windows run inline (thread start-up would cost more than the
      // per-token energy sums); the helpers pull clips from a shared counter,
      // so if one cannot be started the calling thread does its share
      size_t n_tok = 0;
      for (int c : todo)
        for (size_t si : ts_todo[c]) n_tok += clips[c].st->result_all[si].tokens.size();
      const int nt = n_tok < 512 ? 1 : std::min<int>(ts_threads, (int)todo.size());
      if (nt <= 1) {
        for (int c : todo) run_clip(c);
      } else {
        std::atomic<int> next{0};
        auto worker = [&]() {
          for (int i; (i = next.fetch_add(1)) < (int)todo.size();) run_clip(todo[i]);
        };
        std::vector<std::thread> th;
        try {
          for (int t = 1; t < nt; ++t) th.emplace_back(worker);
        } catch (const std::system_error&) {
          MWX_LOG_WARN("mwx: token timestamps on %zu thread(s)\n", th.size() + 1);
        }
        worker();
        for (auto& t : th) t.join();
      }
    }
    // DTW token timestamps (DESIGN.md D8): one alignment pass over the windows
    // that emitted segments. It runs after the window's result is final, on
    // its own self cache, and only writes t_dtw: nothing else of the result
    // (or of the next window's decode) depends on it
    if (C.dtw) {
      std::vector<typename Driver<T>::DtwClip> dc;
      std::vector<State*> dst;
      std::vector<int64_t> dsk;
      for (int c : act) {
        State& cs = *clips[c].st;
        if (dtw_seg0[c] >= cs.result_all.size()) continue;
        typename Driver<T>::DtwClip x;
        x.slot = c;
        x.tokens = clips[c].prompt_init;
        if (P.no_timestamps) x.tokens.pop_back();  // (its NOT: the first alignment row)
        x.pos0 = (int)x.tokens.size();
        x.tokens.push_back(vb.token_not);
        for (size_t si = dtw_seg0[c]; si < cs.result_all.size(); ++si)
          for (const auto& td : cs.result_all[si].tokens)
            if (td.id < vb.token_eot) x.tokens.push_back(td.id);
        x.tokens.push_back(vb.token_eot);
        x.n_rows = (int)x.tokens.size() - x.pos0;
        if (x.n_rows <= 2 || (int)x.tokens.size() > D.Tctx || x.n_rows > DTW_MAX_ROWS) continue;
        const int rem = (int)(clips[c].seek_end - dtw_seek[c]);
        x.n_cols = std::max(1, std::min(D.slot_keys(c), (rem + 1) / 2));
        dc.push_back(std::move(x));
        dst.push_back(&cs);
        dsk.push_back(dtw_seek[c]);
      }
      if (!dc.empty()) {
        if (aborted(P)) return -9;
        D.dtw_pass(dc, dst, dsk.data());
        for (size_t i = 0; i < dc.size(); ++i) {
          State& cs = *dst[i];
          int row = 1;  // (row 0 = NOT)
          for (size_t si = dtw_seg0[dc[i].slot]; si < cs.result_all.size(); ++si)
            for (auto& td : cs.result_all[si].tokens)
              if (td.id < vb.token_eot) td.t_dtw = dsk[i] + 2 * (int64_t)dc[i].frames[row++];
        }
      }
    }
  }
  for (int c = 0; c < n_clips; ++c) states[c]->s.lang_id = clips[c].lang_id;
  return 0;
}

// DTW token timestamps: the alignment heads of a context
// (mwx_context_params.dtw_*). The presets are whisper.cpp's g_aheads tables
// (INTEGRATION.md: unpinned) with the decoder geometry they were made for.
struct AheadsPreset {
  int preset, n_text_layer, n_text_head;
  std::vector<mwx_ahead> heads;
};
static const std::vector<AheadsPreset>& aheads_presets() {
  static const std::vector<AheadsPreset> t = {
      {MWX_AHEADS_TINY_EN, 4, 6, {{1, 0}, {2, 0}, {2, 5}, {3, 0}, {3, 1}, {3, 2}, {3, 3}, {3, 4}}},
      {MWX_AHEADS_TINY, 4, 6, {{2, 2}, {3, 0}, {3, 2}, {3, 3}, {3, 4}, {3, 5}}},
      {MWX_AHEADS_BASE_EN, 6, 8, {{3, 3}, {4, 7}, {5, 1}, {5, 5}, {5, 7}}},
      {MWX_AHEADS_BASE, 6, 8, {{3, 1}, {4, 2}, {4, 3}, {4, 7}, {5, 1}, {5, 2}, {5, 4}, {5, 6}}},
      {MWX_AHEADS_SMALL_EN, 12, 12,
       {{6, 6}, {7, 0}, {7, 3}, {7, 8}, {8, 2}, {8, 5}, {8, 7}, {9, 0}, {9, 4}, {9, 8}, {9, 10},
        {10, 0}, {10, 1}, {10, 2}, {10, 3}, {10, 6}, {10, 11}, {11, 2}, {11, 4}}},
      {MWX_AHEADS_SMALL, 12, 12,
       {{5, 3}, {5, 9}, {8, 0}, {8, 4}, {8, 7}, {8, 8}, {9, 0}, {9, 7}, {9, 9}, {10, 5}}},
      {MWX_AHEADS_MEDIUM_EN, 24, 16,
       {{11, 4}, {14, 1}, {14, 12}, {14, 14}, {15, 4}, {16, 0}, {16, 4}, {16, 9}, {17, 12},
        {17, 14}, {18, 7}, {18, 10}, {18, 15}, {20, 0}, {20, 3}, {20, 9}, {20, 14}, {21, 12}}},
      {MWX_AHEADS_MEDIUM, 24, 16, {{13, 15}, {15, 4}, {15, 15}, {16, 1}, {20, 0}, {23, 4}}},
      {MWX_AHEADS_LARGE_V1, 32, 20,
       {{9, 19}, {11, 2}, {11, 4}, {11, 17}, {22, 7}, {22, 11}, {22, 17}, {23, 2}, {23, 15}}},
      {MWX_AHEADS_LARGE_V2, 32, 20,
       {{10, 12}, {13, 17}, {16, 11}, {16, 12}, {16, 13}, {17, 15}, {17, 16}, {18, 4}, {18, 11},
        {18, 19}, {19, 11}, {21, 2}, {21, 3}, {22, 3}, {22, 9}, {22, 12}, {23, 5}, {23, 7},
        {23, 13}, {25, 5}, {26, 1}, {26, 12}, {27, 15}}},
      {MWX_AHEADS_LARGE_V3, 32, 20,
       {{7, 0}, {10, 17}, {12, 18}, {13, 12}, {16, 1}, {17, 14}, {19, 11}, {21, 4}, {24, 1},
        {25, 6}}},
      {MWX_AHEADS_LARGE_V3_TURBO, 4, 20, {{2, 4}, {2, 11}, {3, 3}, {3, 6}, {3, 11}, {3, 14}}},
  };
  return t;
}

static bool dtw_setup(Context& C, const mwx_context_params& params) {
  const int L = C.hp.n_text_layer, H = C.hp.n_text_head;
  std::vector<mwx_ahead> heads;
  const int preset = params.dtw_aheads_preset;
  if (preset == MWX_AHEADS_N_TOP_MOST) {
    if (params.dtw_n_top < 1 || params.dtw_n_top > L) {
      MWX_LOG_ERROR("mwx: dtw_n_top %d outside 1..%d\n", params.dtw_n_top, L);
      return false;
    }
    for (int l = L - params.dtw_n_top; l < L; ++l)
      for (int h = 0; h < H; ++h) heads.push_back({l, h});
  } else if (preset == MWX_AHEADS_CUSTOM) {
    if (params.dtw_aheads.n_heads < 1 || !params.dtw_aheads.heads) {
      MWX_LOG_ERROR("mwx: dtw_aheads_preset CUSTOM without alignment heads\n");
      return false;
    }
    heads.assign(params.dtw_aheads.heads, params.dtw_aheads.heads + params.dtw_aheads.n_heads);
  } else {
    const AheadsPreset* ap = nullptr;
    for (const auto& a : aheads_presets())
      if (a.preset == preset) ap = &a;
    if (!ap) {
      MWX_LOG_ERROR("mwx: dtw_token_timestamps needs an alignment heads preset (got %d)\n", preset);
      return false;
    }
    if (ap->n_text_layer != L || ap->n_text_head != H) {
      MWX_LOG_ERROR("mwx: alignment heads preset %d is for %d layers x %d heads, the model has "
                    "%d x %d\n", preset, ap->n_text_layer, ap->n_text_head, L, H);
      return false;
    }
    heads = ap->heads;
  }
  for (const mwx_ahead& a : heads)
    if (a.n_text_layer < 0 || a.n_text_layer >= L || a.n_head < 0 || a.n_head >= H) {
      MWX_LOG_ERROR("mwx: alignment head (layer %d, head %d) outside the model (%d x %d)\n",
                    a.n_text_layer, a.n_head, L, H);
      return false;
    }
  C.dtw_heads.clear();
  for (const mwx_ahead& a : heads) C.dtw_heads.emplace_back(a.n_text_layer, a.n_head);
  C.dtw_off.assign(L, 0);
  C.dtw_cnt.assign(L, 0);
  std::vector<int2> dev;
  for (int l = 0; l < L; ++l) {
    C.dtw_off[l] = (int)dev.size();
    for (size_t a = 0; a < heads.size(); ++a)
      if (heads[a].n_text_layer == l) dev.push_back(int2{heads[a].n_head, (int)a});
    C.dtw_cnt[l] = (int)dev.size() - C.dtw_off[l];
  }
  std::lock_guard<std::recursive_mutex> lock(capture_mutex());  // (legacy-stream copy)
  if (hipMalloc((void**)&C.dtw_dev, dev.size() * sizeof(int2)) != hipSuccess ||
      hipMemcpy(C.dtw_dev, dev.data(), dev.size() * sizeof(int2), hipMemcpyHostToDevice) !=
          hipSuccess) {
    MWX_LOG_ERROR("mwx: alignment heads upload failed\n");
    return false;
  }
  C.dtw = true;
  return true;
}

}  // namespace mwx

// ===========================================================================
// C ABI
// ===========================================================================
using mwx::Context;
using mwx::State;

extern "C" {

struct mwx_context_params mwx_context_default_params(void) {
  mwx_context_params p;
  p.use_gpu = true;
  p.flash_attn = true;
  p.gpu_device = 0;
  p.compute = MWX_COMPUTE_MODEL;
  p.dtw_token_timestamps = false;
  p.dtw_aheads_preset = MWX_AHEADS_NONE;
  p.dtw_n_top = -1;
  p.dtw_aheads.n_heads = 0;
  p.dtw_aheads.heads = nullptr;
  p.dtw_mem_size = 1024 * 1024 * 128;
  return p;
}

struct mwx_context* mwx_init_from_file_with_params(const char* path,
                                                   struct mwx_context_params params) {
  if (!path) return nullptr;
  if (!params.use_gpu) {
    MWX_LOG_ERROR("mwx: use_gpu=false is not supported (no CPU path)\n");
    return nullptr;
  }
  try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
      MWX_LOG_ERROR("mwx: no HIP device available\n");
      return nullptr;
    }
    if (params.gpu_device < 0 || params.gpu_device >= ndev) return nullptr;
    HIPC(hipSetDevice(params.gpu_device));
    mwx::ModelFile mf;
    if (!mwx::read_model_file(path, mf)) return nullptr;
    // (read_model_file has just made this very check, so this one cannot fire
    // today; it stays so that a context never holds a vocabulary the logits
    // kernels' LP_G x LP_CHUNK split does not cover, however its Hparams come)
    if (!mwx::vocab_fits(mf.hp.n_vocab)) return nullptr;
    auto* ctx = new mwx_context();
    Context& C = ctx->c;
    C.device = params.gpu_device;
    C.hp = mf.hp;
    C.vocab = std::move(mf.vocab);
    C.filters = mf.filters;
    C.mx = params.compute == MWX_COMPUTE_MXFP8;
    if (params.compute != MWX_COMPUTE_MODEL && !C.mx) {
      delete ctx;
      return nullptr;
    }
    if (!mwx::upload_model(C, mf)) {
      if (C.arena) (void)hipFree(C.arena);
      if (C.gelu_tab) (void)hipFree(C.gelu_tab);
      delete ctx;
      return nullptr;
    }
    auto it = C.vocab.token_to_id.find(" ");
    C.space_id = it == C.vocab.token_to_id.end() ? -1 : it->second;
    for (const std::string& t : mwx::non_speech_tokens()) {
      for (const std::string& s : {t, " " + t}) {
        auto f = C.vocab.token_to_id.find(s);
        if (f != C.vocab.token_to_id.end()) C.nst_ids.push_back(f->second);
      }
    }
    for (const char* s : {" -", " '"}) {
      auto f = C.vocab.token_to_id.find(s);
      if (f != C.vocab.token_to_id.end()) C.nst_ids.push_back(f->second);
    }
    if (params.dtw_token_timestamps && !mwx::dtw_setup(C, params)) {
      mwx_free(ctx);
      return nullptr;
    }
    return ctx;
  } catch (...) {
    return nullptr;
  }
}

struct mwx_state* mwx_init_state(struct mwx_context* ctx) {
  if (!ctx) return nullptr;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    auto* s = new mwx_state();
    s->s.ctx = &ctx->c;
    if (mwx::stream_prio_has("dec_high")) {
      int least = 0, greatest = 0;
      HIPC(hipDeviceGetStreamPriorityRange(&least, &greatest));
      HIPC(hipStreamCreateWithPriority(&s->s.stream, hipStreamNonBlocking, greatest));
    } else {
      HIPC(hipStreamCreateWithFlags(&s->s.stream, hipStreamNonBlocking));
    }
    return s;
  } catch (...) {
    return nullptr;
  }
}

void mwx_free_state(struct mwx_state* state) {
  if (!state) return;
  for (mwx_state* sc : state->scratch) mwx_free_state(sc);
  state->scratch.clear();
  std::lock_guard<std::recursive_mutex> lock(mwx::capture_mutex());
  State& S = state->s;
  if (S.ctx) (void)hipSetDevice(S.ctx->device);
  mwx::DBuf* bufs[] = {&S.pcm, &S.mel,  &S.melmax, &S.melT,   &S.h1p,    &S.x,     &S.h,
                       &S.q,   &S.k,    &S.vt,     &S.o,      &S.ff,     &S.enc,   &S.cross_k,
                       &S.cross_v, &S.energy, &S.aq, &S.as, &S.ibuf, &S.xd, &S.xd2, &S.hd,     &S.qd,    &S.od,
                       &S.ffd, &S.logits, &S.kself, &S.vself, &S.stepin, &S.ctl,   &S.tokout,
                       &S.probs, &S.logprobs, &S.smask, &S.pqkv, &S.pres, &S.pq,
                       &S.du, &S.dnd, &S.ddraw, &S.dneed, &S.kvmap, &S.kvown,
                       &S.lpflt, &S.lpparts, &S.lpres, &S.pcm16, &S.pro_pcm, &S.pro_desc, &S.pro_fs,
                       &S.pro_ft, &S.pro_fc, &S.pro_out, &S.cross_ks, &S.cross_vs,
                       &S.rs_in, &S.rs_out, &S.rs_pos, &S.rs_coef, &S.rrun, &S.rprompt, &S.meld, &S.melpart,
                       &S.melc_pcm[0], &S.melc_pcm[1], &S.melc_raw[0], &S.melc_raw[1],
                       &S.pf_in, &S.pf_x, &S.pf_h, &S.pf_o, &S.pf_ff, &S.pf_pqkv,
                       &S.pf_pres, &S.pf_pq, &S.perf_span,
                       &S.dtw_kself, &S.dtw_vself, &S.dtw_w, &S.dtw_cost, &S.dtw_frames,
                       &S.dtw_meta, &S.xkeys, &S.sc_in, &S.sc_h, &S.sc_logits, &S.sc_out,
                       &S.bias_tab, &S.con_blk, &S.con_mask};
  for (auto* b : bufs) b->release();
  if (S.pin) (void)hipHostFree(S.pin);
  S.pin = nullptr;
  S.pin_n = 0;
  if (S.rep_pin) (void)hipHostFree(S.rep_pin);
  S.rep_pin = nullptr;
  for (hipEvent_t e : S.ev_step)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : S.perf_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : S.perf_gev) (void)hipEventDestroy(e);
  if (S.span_host) (void)hipHostFree(S.span_host);
  if (S.kvmap_pin) (void)hipHostFree(S.kvmap_pin);
  if (S.energy_pin) (void)hipHostFree(S.energy_pin);
  if (S.span_stream) (void)hipStreamDestroy(S.span_stream);
  if (S.ev_e0) (void)hipEventDestroy(S.ev_e0);
  if (S.ev_e1) (void)hipEventDestroy(S.ev_e1);
  if (S.estream) (void)hipStreamDestroy(S.estream);
  if (S.stream) (void)hipStreamDestroy(S.stream);
  delete state;
}

void mwx_free(struct mwx_context* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->c.device);
  if (ctx->c.arena) (void)hipFree(ctx->c.arena);
  if (ctx->c.gelu_tab) (void)hipFree(ctx->c.gelu_tab);
  if (ctx->c.dtw_dev) (void)hipFree(ctx->c.dtw_dev);
  if (ctx->c.con_tok_dev) (void)hipFree(ctx->c.con_tok_dev);
  delete ctx;
}

struct mwx_full_params mwx_full_default_params(int strategy) {
  mwx_full_params p;
  memset(&p, 0, sizeof(p));
  p.strategy = strategy;
  p.n_threads = 4;
  p.n_max_text_ctx = 16384;
  p.offset_ms = 0;
  p.duration_ms = 0;
  p.translate = false;
  p.no_context = true;
  p.no_timestamps = false;
  p.single_segment = false;
  p.print_special = false;
  p.print_progress = true;
  p.print_realtime = false;
  p.print_timestamps = true;
  p.token_timestamps = false;
  p.thold_pt = 0.01f;
  p.thold_ptsum = 0.01f;
  p.max_len = 0;
  p.split_on_word = false;
  p.max_tokens = 0;
  p.audio_ctx = 0;
  p.audio_ctx_fit = false;
  p.lang_ids = nullptr;
  p.chunk_language = MWX_CHUNK_LANG_PER_CHUNK;
  p.tdrz_enable = false;
  p.initial_prompt = nullptr;
  p.prompt_tokens = nullptr;
  p.prompt_n_tokens = 0;
  p.language = "en";
  p.detect_language = false;
  p.suppress_blank = true;
  p.suppress_nst = false;
  p.temperature = 0.0f;
  p.max_initial_ts = 1.0f;
  p.length_penalty = -1.0f;
  p.temperature_inc = 0.2f;
  p.entropy_thold = 2.4f;
  p.logprob_thold = -1.0f;
  p.no_speech_thold = 0.6f;
  p.greedy.best_of = -1;
  p.beam_search.beam_size = -1;
  p.beam_search.patience = -1.0f;
  if (strategy == MWX_SAMPLING_GREEDY) {
    p.greedy.best_of = 5;
  } else {
    p.beam_search.beam_size = 5;
    p.beam_search.patience = -1.0f;
  }
  p.abort_callback = nullptr;
  p.abort_callback_user_data = nullptr;
  p.bench_fixed_steps = 0;
  p.bias_phrases = nullptr;
  p.n_bias_phrases = 0;
  p.constraint = nullptr;
  p.constraint_penalty = 100.0f;
  return p;
}

namespace mwx {
// mwx_full_params.lang_ids of a call with n entries: no id above lang_max_id()
// (a non-multilingual model ignores the field)
// One language per recording (mwx_full_batch_chunked, DESIGN.md D13): chunks
// are pooled until their summed length reaches kLangPoolSamples; a chunk
// counts when the engine would decode it (ten mel frames: the 0.1-s rule of
// run_full's window loop)
constexpr int64_t kLangPoolSamples = 30 * MWX_SAMPLE_RATE;
static bool lang_chunk_counts(int len) {
  return len > 0 && 1 + (len + 200 - 400) / MWX_HOP_LENGTH >= 10;
}
static bool lang_ids_ok(const Vocab& vb, const int* lang_ids, int n) {
  if (!lang_ids || !vb.is_multilingual()) return true;
  for (int b = 0; b < n; ++b)
    if (lang_ids[b] > lang_max_id()) return false;
  return true;
}
// mwx_full_params.bias_phrases (mwx.h; DESIGN.md D14): 0, or the code the call
// returns before it touches a state or the device
static int bias_check(const Vocab& vb, const mwx_full_params& P, const char* fn) {
  const char* why = "";
  const int rc = bias_validate(P.bias_phrases, P.n_bias_phrases, vb.token_eot, &why);
  if (rc == -1) MWX_LOG_ERROR("%s: bias_phrases: %s\n", fn, why);
  if (rc) return rc;
  // mwx_full_params.constraint / constraint_penalty (mwx.h; DESIGN.md D15)
  const int rc2 = constraint_check(P, &why);
  if (rc2) MWX_LOG_ERROR("%s: constraint: %s\n", fn, why);
  return rc2;
}
}  // namespace mwx

static int full_batch_any(struct mwx_context* ctx, struct mwx_state* const* states,
                          struct mwx_full_params params, const void* const* samples,
                          const int* n_samples, int n_clips, bool pcm16) {
  if (!ctx || !states || n_clips <= 0) return -1;
  for (int c = 0; c < n_clips; ++c)
    if (!states[c] || (n_samples[c] > 0 && !samples[c])) return -1;
  if (!mwx::lang_ids_ok(ctx->c.vocab, params.lang_ids, n_clips)) return -3;
  if (int rc = mwx::bias_check(ctx->c.vocab, params, "mwx_full_batch")) return rc;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (ctx->c.wtype == mwx::GGML_BF16)
      return mwx::run_full<__bf16>(ctx->c, states, params, samples, n_samples, n_clips, pcm16);
    return mwx::run_full<_Float16>(ctx->c, states, params, samples, n_samples, n_clips, pcm16);
  } catch (...) {
    return -1;
  }
}

int mwx_full_batch(struct mwx_context* ctx, struct mwx_state* const* states,
                   struct mwx_full_params params, const float* const* samples,
                   const int* n_samples, int n_clips) {
  return full_batch_any(ctx, states, params, reinterpret_cast<const void* const*>(samples),
                        n_samples, n_clips, false);
}

int mwx_full_batch_pcm16(struct mwx_context* ctx, struct mwx_state* const* states,
                         struct mwx_full_params params, const int16_t* const* samples,
                         const int* n_samples, int n_clips) {
  return full_batch_any(ctx, states, params, reinterpret_cast<const void* const*>(samples),
                        n_samples, n_clips, true);
}

// Transcript alignment (mwx.h; DESIGN.md D12). Everything that can be refused
// is refused before run_full touches a state.
int mwx_align_batch(struct mwx_context* ctx, struct mwx_state* const* states,
                    struct mwx_full_params params, const float* const* samples,
                    const int* n_samples, const mwx_token* const* tokens, const int* n_tokens,
                    int n_clips) {
  if (!ctx || !states || !samples || !n_samples || !tokens || !n_tokens || n_clips < 1) {
    MWX_LOG_ERROR("mwx_align_batch: null argument or no clips\n");
    return -1;
  }
  const mwx::Hparams& hp = ctx->c.hp;
  const mwx::Vocab& vb = ctx->c.vocab;
  for (int c = 0; c < n_clips; ++c) {
    if (!states[c] || (n_samples[c] > 0 && !samples[c]) || (n_tokens[c] > 0 && !tokens[c]) ||
        n_samples[c] < 0 || n_tokens[c] < 0) {
      MWX_LOG_ERROR("mwx_align_batch: clip %d: null state, samples or tokens\n", c);
      return -1;
    }
    if (n_tokens[c] > MWX_ALIGN_MAX_TOKENS || n_tokens[c] + 5 > hp.n_text_ctx) {
      MWX_LOG_ERROR("mwx_align_batch: clip %d: %d tokens (at most %d)\n", c, n_tokens[c],
                    std::min(MWX_ALIGN_MAX_TOKENS, hp.n_text_ctx - 5));
      return -1;
    }
    if (n_samples[c] > MWX_CHUNK_SIZE * MWX_SAMPLE_RATE) {
      MWX_LOG_ERROR("mwx_align_batch: clip %d: %d samples (at most %d s)\n", c, n_samples[c],
                    MWX_CHUNK_SIZE);
      return -1;
    }
  }
  if (params.offset_ms != 0 || params.duration_ms != 0) {
    MWX_LOG_ERROR("mwx_align_batch: offset_ms and duration_ms must be 0\n");
    return -1;
  }
  for (int c = 0; c < n_clips; ++c)
    for (int j = 0; j < n_tokens[c]; ++j)
      if (tokens[c][j] < 0 || tokens[c][j] >= vb.token_eot) return -3;
  if (params.audio_ctx > hp.n_audio_ctx) return -5;
  if (!mwx::lang_ids_ok(vb, params.lang_ids, n_clips)) return -3;
  mwx_full_params P = mwx_full_default_params(MWX_SAMPLING_GREEDY);
  P.language = params.language;
  P.lang_ids = params.lang_ids;
  P.translate = params.translate;
  P.audio_ctx = params.audio_ctx;
  P.audio_ctx_fit = params.audio_ctx_fit;
  P.abort_callback = params.abort_callback;
  P.abort_callback_user_data = params.abort_callback_user_data;
  const bool detect =
      P.language == nullptr || strlen(P.language) == 0 || strcmp(P.language, "auto") == 0;
  if (!detect && vb.is_multilingual() && mwx::lang_id(P.language) < 0) return -3;
  const mwx::AlignReq req{tokens, n_tokens};
  try {
    HIPC(hipSetDevice(ctx->c.device));
    const void* const* pcm = reinterpret_cast<const void* const*>(samples);
    if (ctx->c.wtype == mwx::GGML_BF16)
      return mwx::run_full<__bf16>(ctx->c, states, P, pcm, n_samples, n_clips, false, &req);
    return mwx::run_full<_Float16>(ctx->c, states, P, pcm, n_samples, n_clips, false, &req);
  } catch (...) {
    return -1;
  }
}

int mwx_align_row(struct mwx_state* state, int i, float* plog, mwx_token* top_id,
                  float* top_plog) {
  if (!state || i < 0 || i >= (int)state->s.align.size()) return -1;
  const mwx::ScoreOut& r = state->s.align[i];
  if (plog) *plog = r.plog;
  if (top_id) *top_id = r.top_id;
  if (top_plog) *top_plog = r.top_plog;
  return 0;
}

// Trimmed audio (vad.cpp, mwx_vad_trim_batch) through the batched path: the
// clips that have speech run on their compacted device PCM, then every stored
// time moves from the compacted timeline to the caller's.
int mwx_full_batch_trimmed(struct mwx_context* ctx, struct mwx_state* const* states,
                           struct mwx_full_params params,
                           const struct mwx_vad_trimmed* const* trimmed, const int* clip_index,
                           int n_clips) {
  if (!ctx || !states || !trimmed || !clip_index || n_clips <= 0) return -1;
  if (int rc = mwx::bias_check(ctx->c.vocab, params, "mwx_full_batch_trimmed")) return rc;
  std::vector<mwx_state*> run_states;
  std::vector<const void*> ptrs;
  std::vector<int> lens;
  std::vector<const mwx_vad_trimmed::Clip*> run_clips;
  for (int b = 0; b < n_clips; ++b) {
    const mwx_vad_trimmed* t = trimmed[b];
    if (!states[b] || !t || clip_index[b] < 0 || (size_t)clip_index[b] >= t->clips.size())
      return -1;
    if (t->device != ctx->c.device) {
      MWX_LOG_ERROR("mwx_full_batch_trimmed: trimmed audio of device %d, context on device %d\n",
                    t->device, ctx->c.device);
      return -1;
    }
    if (t->clips[clip_index[b]].n_compact > 0x7fffffffLL) return -1;
  }
  if (!mwx::lang_ids_ok(ctx->c.vocab, params.lang_ids, n_clips)) return -3;
  std::vector<int> run_ids;  // (each kept entry's language id travels with it)
  for (int b = 0; b < n_clips; ++b) {
    const mwx_vad_trimmed::Clip& c = trimmed[b]->clips[clip_index[b]];
    states[b]->s.result_all.clear();
    states[b]->s.lang_probs.clear();
    states[b]->s.lang_last.clear();
    states[b]->s.con_status = params.constraint ? 1 : -1;  // (no window: nothing missed)
    if (c.seg.empty() || c.n_compact <= 0) continue;
    if (params.lang_ids) run_ids.push_back(params.lang_ids[b]);
    run_states.push_back(states[b]);
    ptrs.push_back(trimmed[b]->d_pcm + c.off);
    lens.push_back((int)c.n_compact);
    run_clips.push_back(&c);
  }
  if (run_states.empty()) return 0;
  if (params.lang_ids) params.lang_ids = run_ids.data();
  const int rc = full_batch_any(ctx, run_states.data(), params, ptrs.data(), lens.data(),
                                (int)run_states.size(), false);
  if (rc != 0) return rc;
  for (size_t r = 0; r < run_states.size(); ++r)
    for (auto& sg : run_states[r]->s.result_all) {
      sg.t0 = mwx::vad_map_time(*run_clips[r], sg.t0, false);
      sg.t1 = mwx::vad_map_time(*run_clips[r], sg.t1, true);
      for (auto& td : sg.tokens) {
        td.t0 = mwx::vad_map_time(*run_clips[r], td.t0, false);
        td.t1 = mwx::vad_map_time(*run_clips[r], td.t1, true);
        if (td.t_dtw >= 0) td.t_dtw = mwx::vad_map_time(*run_clips[r], td.t_dtw, false);
      }
    }
  return 0;
}

// A clip's chunks (vad.cpp, mwx_vad_trim_batch_chunked; DESIGN.md D10) as batch
// entries: the chunks of all entries, in (entry, chunk) order, go through
// full_batch_any in runs of at most max_batch, entry 0 of a run on states[0]
// and the rest on its scratch states; each run's segments are moved out, their
// times mapped by the chunk's map, and appended to the clip they belong to.
int mwx_full_batch_chunked(struct mwx_context* ctx, struct mwx_state* const* states,
                           struct mwx_full_params params,
                           const struct mwx_vad_trimmed* const* trimmed, const int* clip_index,
                           int n_clips, int max_batch) {
  if (!ctx || !states || !trimmed || !clip_index || n_clips <= 0 || max_batch < 1) return -1;
  if (int rc = mwx::bias_check(ctx->c.vocab, params, "mwx_full_batch_chunked")) return rc;
  struct Job {
    int entry;
    int64_t chunk;
    const mwx_vad_trimmed::Clip* clip;
    const float* pcm;
    int len;
  };
  std::vector<Job> jobs;
  for (int b = 0; b < n_clips; ++b)  // (an error below leaves every state with 0 segments)
    if (states[b]) {
      states[b]->s.result_all.clear();
      states[b]->s.lang_probs.clear();
      states[b]->s.lang_last.clear();
    }
  for (int b = 0; b < n_clips; ++b) {
    const mwx_vad_trimmed* t = trimmed[b];
    if (!states[b] || !t || clip_index[b] < 0 || (size_t)clip_index[b] >= t->clips.size())
      return -1;
    if (t->device != ctx->c.device) {
      MWX_LOG_ERROR("mwx_full_batch_chunked: trimmed audio of device %d, context on device %d\n",
                    t->device, ctx->c.device);
      return -1;
    }
    if (t->clips[clip_index[b]].n_compact > 0x7fffffffLL) return -1;
  }
  if (params.offset_ms != 0 || params.duration_ms != 0) {
    MWX_LOG_ERROR("mwx_full_batch_chunked: offset_ms and duration_ms must be 0\n");
    return -1;
  }
  if (!mwx::lang_ids_ok(ctx->c.vocab, params.lang_ids, n_clips)) return -3;
  for (int b = 0; b < n_clips; ++b) {
    const mwx_vad_trimmed::Clip& c = trimmed[b]->clips[clip_index[b]];
    if (c.seg.empty() || c.n_compact <= 0) continue;
    for (int64_t j = 0; 2 * j + 1 < (int64_t)c.chunk.size(); ++j) {
      int64_t first, n, start, len;
      if (!mwx::vad_chunk_span(c, j, first, n, start, len) || start < 0 || len < 0 ||
          start + len > c.n_compact)
        return -1;
      jobs.push_back({b, j, &c, trimmed[b]->d_pcm + c.off + start, (int)len});
    }
  }
  if (jobs.empty()) return 0;
  mwx_state* s0 = states[0];
  const size_t width = std::min((size_t)max_batch, jobs.size());
  while (s0->scratch.size() + 1 < width) {
    mwx_state* sc = mwx_init_state(ctx);
    if (!sc) return -1;
    s0->scratch.push_back(sc);
  }
  std::vector<mwx_state*> run_states{s0};
  run_states.insert(run_states.end(), s0->scratch.begin(), s0->scratch.begin() + (width - 1));
  std::vector<std::vector<mwx::Segment>> acc((size_t)n_clips);
  std::vector<int> lang((size_t)n_clips, -1);
  std::vector<std::vector<float>> lprobs((size_t)n_clips);
  int rc = 0;
  // every chunk of entry b runs with entry_lang[b] (-1: params.language)
  const bool ml = ctx->c.vocab.is_multilingual();
  std::vector<int> entry_lang((size_t)n_clips, -1);
  if (ml && params.lang_ids)
    for (int b = 0; b < n_clips; ++b) entry_lang[b] = std::max(-1, params.lang_ids[b]);
  // one language per recording (mwx.h; DESIGN.md D13): a detection-only pass
  // over each such entry's leading chunks, pooled by length
  const bool auto_lang = params.language == nullptr || strlen(params.language) == 0 ||
                         strcmp(params.language, "auto") == 0;
  std::vector<char> pooled((size_t)n_clips, 0);
  if (ml && auto_lang && !params.detect_language &&
      params.chunk_language == MWX_CHUNK_LANG_RECORDING) {
    std::vector<size_t> det;  // (indices into jobs, in (entry, chunk) order)
    std::vector<int64_t> cum((size_t)n_clips, 0);
    for (size_t i = 0; i < jobs.size(); ++i) {
      const Job& jb = jobs[i];
      if (entry_lang[jb.entry] >= 0 || cum[jb.entry] >= mwx::kLangPoolSamples) continue;
      if (!mwx::lang_chunk_counts(jb.len)) continue;
      det.push_back(i);
      cum[jb.entry] += jb.len;
    }
    const int nl = mwx::lang_max_id() + 1;
    std::vector<std::vector<double>> psum((size_t)n_clips);
    mwx_full_params pd = params;
    pd.detect_language = true;
    pd.lang_ids = nullptr;
    for (size_t r0 = 0; r0 < det.size(); r0 += width) {
      const size_t n = std::min(width, det.size() - r0);
      if (r0 > 0 && mwx::aborted(params)) {
        rc = -9;
        break;
      }
      std::vector<const void*> ptrs;
      std::vector<int> lens;
      for (size_t i = 0; i < n; ++i) {
        ptrs.push_back(jobs[det[r0 + i]].pcm);
        lens.push_back(jobs[det[r0 + i]].len);
      }
      rc = full_batch_any(ctx, run_states.data(), pd, ptrs.data(), lens.data(), (int)n, false);
      if (rc != 0) break;
      for (size_t i = 0; i < n; ++i) {
        const Job& jb = jobs[det[r0 + i]];
        const std::vector<float>& p = run_states[i]->s.lang_probs;
        if ((int)p.size() != nl) {
          rc = -1;
          break;
        }
        std::vector<double>& a = psum[jb.entry];
        a.resize((size_t)nl, 0.0);
        for (int k = 0; k < nl; ++k) a[k] += (double)jb.len * (double)p[k];
      }
      if (rc != 0) break;
    }
    if (rc == 0 && !det.empty() && mwx::aborted(params)) rc = -9;
    for (int b = 0; b < n_clips && rc == 0; ++b) {
      if (psum[b].empty()) continue;
      lprobs[b].resize((size_t)nl);
      int best = 0;
      for (int k = 0; k < nl; ++k) {
        lprobs[b][k] = (float)(psum[b][k] / (double)cum[b]);
        if (lprobs[b][k] > lprobs[b][best]) best = k;
      }
      entry_lang[b] = best;
      pooled[b] = 1;
    }
  }
  bool any_lang = false;
  for (int b = 0; b < n_clips; ++b) any_lang = any_lang || entry_lang[b] >= 0;
  // constrained decoding: an entry's status is the worst of its chunks'
  std::vector<int> con_st((size_t)n_clips, params.constraint ? 1 : -1);
  for (size_t r0 = 0; r0 < jobs.size() && rc == 0; r0 += width) {
    const size_t n = std::min(width, jobs.size() - r0);
    if (r0 > 0 && mwx::aborted(params)) {
      rc = -9;
      break;
    }
    std::vector<const void*> ptrs;
    std::vector<int> lens, ids;
    for (size_t i = 0; i < n; ++i) {
      ptrs.push_back(jobs[r0 + i].pcm);
      lens.push_back(jobs[r0 + i].len);
      ids.push_back(entry_lang[jobs[r0 + i].entry]);
    }
    mwx_full_params pr = params;
    pr.lang_ids = any_lang ? ids.data() : nullptr;
    rc = full_batch_any(ctx, run_states.data(), pr, ptrs.data(), lens.data(), (int)n, false);
    if (rc != 0) break;
    for (size_t i = 0; i < n; ++i) {
      const Job& jb = jobs[r0 + i];
      mwx::State& rs = run_states[i]->s;
      for (auto& sg : rs.result_all) {
        sg.t0 = mwx::vad_chunk_map_time(*jb.clip, jb.chunk, sg.t0, false);
        sg.t1 = mwx::vad_chunk_map_time(*jb.clip, jb.chunk, sg.t1, true);
        for (auto& td : sg.tokens) {
          td.t0 = mwx::vad_chunk_map_time(*jb.clip, jb.chunk, td.t0, false);
          td.t1 = mwx::vad_chunk_map_time(*jb.clip, jb.chunk, td.t1, true);
          if (td.t_dtw >= 0) td.t_dtw = mwx::vad_chunk_map_time(*jb.clip, jb.chunk, td.t_dtw, false);
        }
        acc[jb.entry].push_back(std::move(sg));
      }
      rs.result_all.clear();
      if (params.constraint && rs.con_status == 0) con_st[jb.entry] = 0;
      if (jb.chunk == 0) {
        lang[jb.entry] = rs.lang_id;
        if (!pooled[jb.entry]) lprobs[jb.entry] = rs.lang_probs;
      }
    }
  }
  for (mwx_state* rs : run_states) {
    rs->s.result_all.clear();
    rs->s.lang_probs.clear();
  }
  for (int b = 0; b < n_clips; ++b) states[b]->s.result_all.clear();
  if (rc != 0) return rc;
  for (int b = 0; b < n_clips; ++b) states[b]->s.con_status = con_st[b];
  for (int b = 0; b < n_clips; ++b) {
    if (lang[b] < 0) continue;
    states[b]->s.result_all = std::move(acc[b]);
    states[b]->s.lang_id = pooled[b] ? entry_lang[b] : lang[b];
    states[b]->s.lang_probs = std::move(lprobs[b]);
  }
  return 0;
}

float* mwx_device_buffer(struct mwx_context* ctx, size_t n) {
  if (!ctx || n == 0) return nullptr;
  if (hipSetDevice(ctx->c.device) != hipSuccess) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) return nullptr;
  return (float*)p;
}

int mwx_device_upload(struct mwx_context* ctx, float* dst, const float* src, size_t n) {
  if (!ctx || !dst || !src) return -1;
  if (hipSetDevice(ctx->c.device) != hipSuccess) return -1;
  std::lock_guard<std::recursive_mutex> lock(mwx::capture_mutex());  // (legacy-stream copy)
  return hipMemcpy(dst, src, n * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

void mwx_device_buffer_free(struct mwx_context* ctx, float* p) {
  if (!ctx || !p) return;
  (void)hipSetDevice(ctx->c.device);
  std::lock_guard<std::recursive_mutex> lock(mwx::capture_mutex());
  (void)hipFree(p);
}

mwx_prosody_params mwx_prosody_default_params(void) {
  mwx_prosody_params p;
  p.lpf_alpha = 0.07f;  // src/prosody_extractor.h:21-27
  p.gender_threshold = 170.0f;
  p.min_pitch = 60.0f;
  p.max_pitch = 500.0f;
  return p;
}

static_assert(sizeof(mwx_prosody) == sizeof(mwx::ProsodyOut), "mwx_prosody layout");
static_assert(sizeof(mwx::ProsodySeg) == 3 * sizeof(int64_t), "prosody descriptor layout");

static int prosody_run(mwx::State& S, const float* d_pcm, const mwx::ProsodySeg* d_desc, int n_seg,
                       int64_t total_frames, int sample_rate, const mwx_prosody_params& p,
                       mwx::ProsodyOut* d_out) {
  const size_t fr = (size_t)std::max<int64_t>(total_frames, 1);
  float* fs = (float*)S.pro_fs.get(fr * 4);
  float4* ft = (float4*)S.pro_ft.get(fr * 16);
  int* fc = (int*)S.pro_fc.get(fr * 4);
  mwx::PerfScope ps(S, "prosody");
  mwx::prosody_launch(d_pcm, d_desc, n_seg, fs, ft, fc, d_out, sample_rate / 100, sample_rate,
                      p.lpf_alpha, p.gender_threshold, p.min_pitch, p.max_pitch, S.stream);
  return 0;
}

int mwx_prosody_batch(struct mwx_context* ctx, struct mwx_state* state, const float* pcm,
                      int64_t n_pcm, const int64_t* seg_start, const int64_t* seg_len, int n_seg,
                      int sample_rate, const mwx_prosody_params* params, mwx_prosody* out) {
  if (!ctx || !state || n_seg < 0 || (n_seg > 0 && (!pcm || !seg_start || !seg_len || !out)))
    return -1;
  if (sample_rate < 100 || sample_rate > 160000 || n_pcm < 0 || n_pcm >= (int64_t)1 << 31) return -1;
  if (n_seg == 0) return 0;
  const mwx_prosody_params p = params ? *params : mwx_prosody_default_params();
  const int F = sample_rate / 100;
  std::vector<mwx::ProsodySeg> desc(n_seg);
  int64_t frames = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (seg_start[i] < 0 || seg_len[i] < 0 || seg_start[i] + seg_len[i] > n_pcm) return -1;
    desc[i] = {seg_start[i], seg_len[i], frames};
    if (seg_len[i] >= 160) frames += seg_len[i] / F;
  }
  try {
    mwx::State& S = state->s;
    HIPC(hipSetDevice(ctx->c.device));
    const float* d_pcm = pcm;
    if (!mwx::is_device_ptr(pcm)) {
      float* d = (float*)S.pro_pcm.get((size_t)std::max<int64_t>(n_pcm, 1) * 4);
      HIPC(hipMemcpyAsync(d, pcm, (size_t)n_pcm * 4, hipMemcpyHostToDevice, S.stream));
      d_pcm = d;
    }
    auto* d_desc = (mwx::ProsodySeg*)S.pro_desc.get(desc.size() * sizeof(mwx::ProsodySeg));
    HIPC(hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(mwx::ProsodySeg),
                        hipMemcpyHostToDevice, S.stream));
    auto* d_out = (mwx::ProsodyOut*)S.pro_out.get((size_t)n_seg * sizeof(mwx::ProsodyOut));
    prosody_run(S, d_pcm, d_desc, n_seg, frames, sample_rate, p, d_out);
    HIPC(hipMemcpyAsync(out, d_out, (size_t)n_seg * sizeof(mwx_prosody), hipMemcpyDeviceToHost,
                        S.stream));
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
  } catch (...) {
    return -2;
  }
}

int mwx_prosody_batch_device(struct mwx_context* ctx, struct mwx_state* state, const float* d_pcm,
                             const int64_t* d_desc, int n_seg, int64_t total_frames,
                             int sample_rate, const mwx_prosody_params* params,
                             mwx_prosody* d_out) {
  if (!ctx || !state || n_seg < 0 || (n_seg > 0 && (!d_pcm || !d_desc || !d_out))) return -1;
  if (sample_rate < 100 || sample_rate > 160000 || total_frames < 0) return -1;
  if (n_seg == 0) return 0;
  const mwx_prosody_params p = params ? *params : mwx_prosody_default_params();
  try {
    HIPC(hipSetDevice(ctx->c.device));
    return prosody_run(state->s, d_pcm, reinterpret_cast<const mwx::ProsodySeg*>(d_desc), n_seg,
                       total_frames, sample_rate, p, reinterpret_cast<mwx::ProsodyOut*>(d_out));
  } catch (...) {
    return -2;
  }
}

// ---------------------------------------------------------------------------
// resampling (SttEngine::resample_audio, src/stt_engine.cpp:87-106:
// libsamplerate src_simple with SRC_SINC_FASTEST, mono, end_of_input = 0)
// ---------------------------------------------------------------------------
namespace mwx {

constexpr int RS_INDEX_INC = 128;  // table points per zero crossing (fastest_coeffs.h geometry)
constexpr int RS_COEFFS = 2464;    // table entries; coeff_half_len = RS_COEFFS - 2
constexpr double RS_CUTOFF = 0.9;  // reconstructed: -6 dB at 0.9 of the lower Nyquist
constexpr double RS_BETA = 9.0;    // Kaiser window over the 19.25 zero crossings

static double bessel_i0(double x) {
  double sum = 1.0, term = 1.0;
  for (int k = 1; k < 64; ++k) {
    term *= (x / (2.0 * k)) * (x / (2.0 * k));
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// Reconstructed SRC_SINC_FASTEST half-filter: libsamplerate's table is not in
// the image (third-party, absent), so only its geometry is kept: 2464 points,
// 128 per input-sample period, a windowed sinc normalised to unit DC gain.
static const std::vector<float>& resample_coeffs() {
  static const std::vector<float> c = [] {
    std::vector<double> h(RS_COEFFS);
    const double span = (double)RS_COEFFS / RS_INDEX_INC;
    for (int i = 0; i < RS_COEFFS; ++i) {
      const double x = (double)i / RS_INDEX_INC;
      const double t = x / span;
      const double arg = M_PI * RS_CUTOFF * x;
      const double sinc = i == 0 ? 1.0 : std::sin(arg) / arg;
      const double w = t >= 1.0 ? 0.0 : bessel_i0(RS_BETA * std::sqrt(1.0 - t * t)) / bessel_i0(RS_BETA);
      h[i] = RS_CUTOFF * sinc * w;
    }
    double dc = h[0];
    for (int k = RS_INDEX_INC; k < RS_COEFFS; k += RS_INDEX_INC) dc += 2.0 * h[k];
    std::vector<float> f(RS_COEFFS);
    for (int i = 0; i < RS_COEFFS; ++i) f[i] = (float)(h[i] / dc);
    return f;
  }();
  return c;
}

static double rs_fmod_one(double x) {
  const double res = x - (double)std::lrint(x);
  return res < 0.0 ? res + 1.0 : res;
}

// The converter's output bookkeeping (sinc_mono_vari_process): output n is
// centred on input sample idx_n at fraction f_n; the loop stops when no more
// than `half` input samples remain beyond idx_n (end_of_input = 0: the tail
// is held back for a next call that never comes) or out_cap is reached.
struct ResamplePlan {
  int half = 0, increment = 0;
  double scale = 1.0;
  std::vector<int2> pos;  // {idx_n, start_filter_index_n}
};
static ResamplePlan resample_plan(long n_in, double ratio, long out_cap) {
  ResamplePlan R;
  const int coeff_half_len = RS_COEFFS - 2;
  double count = (coeff_half_len + 2.0) / RS_INDEX_INC;
  if (ratio < 1.0) count /= ratio;
  R.half = (int)(std::lrint(count) + 1);
  const double float_increment = RS_INDEX_INC * (ratio < 1.0 ? ratio : 1.0);
  R.increment = (int)std::lrint(float_increment * (1 << RS_SHIFT));
  R.scale = float_increment / RS_INDEX_INC;
  double input_index = 0.0;
  long idx = 0;
  while ((long)R.pos.size() < out_cap) {
    if (n_in - idx <= R.half) break;
    R.pos.push_back(int2{(int)idx, (int)std::lrint(input_index * float_increment * (1 << RS_SHIFT))});
    input_index += 1.0 / ratio;
    const double rem = rs_fmod_one(input_index);
    idx += std::lrint(input_index - rem);
    input_index = rem;
  }
  return R;
}

}  // namespace mwx

long mwx_resample_max_frames(int n_in, int src_rate, int dst_rate) {
  if (n_in < 0 || src_rate <= 0 || dst_rate <= 0) return -1;
  return (long)(n_in * ((double)dst_rate / (double)src_rate)) + 100;
}

int mwx_resample(struct mwx_context* ctx, struct mwx_state* state, const float* in, int n_in,
                 int src_rate, int dst_rate, float* out, int out_cap) {
  if (!ctx || !state || n_in < 0 || (n_in > 0 && (!in || !out)) || src_rate <= 0 || dst_rate <= 0)
    return -1;
  if (src_rate == dst_rate || n_in == 0) return 0;  // the reference returns {} (input kept)
  const double ratio = (double)dst_rate / (double)src_rate;
  if (ratio < 1.0 / 256 || ratio > 256.0) return -2;  // libsamplerate SRC_MAX_RATIO
  const mwx::ResamplePlan R = mwx::resample_plan(n_in, ratio, out_cap);
  const int n_out = (int)R.pos.size();
  if (n_out == 0) return 0;
  try {
    mwx::State& S = state->s;
    HIPC(hipSetDevice(ctx->c.device));
    const std::vector<float>& cf = mwx::resample_coeffs();
    float* d_coef = (float*)S.rs_coef.get(cf.size() * 4);
    HIPC(hipMemcpyAsync(d_coef, cf.data(), cf.size() * 4, hipMemcpyHostToDevice, S.stream));
    const float* d_in = in;
    if (!mwx::is_device_ptr(in)) {
      float* d = (float*)S.rs_in.get((size_t)n_in * 4);
      HIPC(hipMemcpyAsync(d, in, (size_t)n_in * 4, hipMemcpyHostToDevice, S.stream));
      d_in = d;
    }
    int2* d_pos = (int2*)S.rs_pos.get((size_t)n_out * sizeof(int2));
    HIPC(hipMemcpyAsync(d_pos, R.pos.data(), (size_t)n_out * sizeof(int2), hipMemcpyHostToDevice,
                        S.stream));
    const bool dev_out = mwx::is_device_ptr(out);
    float* d_out = dev_out ? out : (float*)S.rs_out.get((size_t)n_out * 4);
    {
      mwx::PerfScope ps(S, "resample");
      mwx::resample_launch(d_in, R.half, d_coef, mwx::RS_COEFFS - 2, R.increment, R.scale, d_pos,
                           n_out, d_out, S.stream);
    }
    if (!dev_out)
      HIPC(hipMemcpyAsync(out, d_out, (size_t)n_out * 4, hipMemcpyDeviceToHost, S.stream));
    HIPC(hipStreamSynchronize(S.stream));
    return n_out;
  } catch (...) {
    return -3;
  }
}

int mwx_full_with_state(struct mwx_context* ctx, struct mwx_state* state,
                        struct mwx_full_params params, const float* samples, int n_samples) {
  struct mwx_state* st[1] = {state};
  const float* pc[1] = {samples};
  int n[1] = {n_samples};
  return mwx_full_batch(ctx, st, params, pc, n, 1);
}

int mwx_full_n_segments_from_state(struct mwx_state* state) {
  return state ? (int)state->s.result_all.size() : 0;
}
const char* mwx_full_get_segment_text_from_state(struct mwx_state* state, int i) {
  return state->s.result_all.at(i).text.c_str();
}
int64_t mwx_full_get_segment_t0_from_state(struct mwx_state* state, int i) {
  return state->s.result_all.at(i).t0;
}
int64_t mwx_full_get_segment_t1_from_state(struct mwx_state* state, int i) {
  return state->s.result_all.at(i).t1;
}
bool mwx_full_get_segment_speaker_turn_next_from_state(struct mwx_state* state, int i) {
  return state->s.result_all.at(i).speaker_turn_next;
}
float mwx_full_get_segment_no_speech_prob_from_state(struct mwx_state* state, int i) {
  return state->s.result_all.at(i).no_speech_prob;
}
int mwx_full_n_tokens_from_state(struct mwx_state* state, int i) {
  return (int)state->s.result_all.at(i).tokens.size();
}
mwx_token_data mwx_full_get_token_data_from_state(struct mwx_state* state, int i, int j) {
  return state->s.result_all.at(i).tokens.at(j);
}
int mwx_full_lang_id_from_state(struct mwx_state* state) { return state ? state->s.lang_id : -1; }
int mwx_full_lang_probs_from_state(struct mwx_state* state, float* probs, int n) {
  if (!state || !probs || n < mwx::lang_max_id() + 1) return -1;
  const std::vector<float>& lp = state->s.lang_probs;
  if (lp.empty()) return 0;
  memcpy(probs, lp.data(), lp.size() * 4);
  return (int)lp.size();
}

const char* mwx_token_to_str(struct mwx_context* ctx, mwx_token token) {
  return ctx->c.vocab.id_to_token.at(token).c_str();
}
int mwx_full_constraint_status_from_state(struct mwx_state* state) {
  return state ? state->s.con_status : -1;
}
// (constraint.cpp's refusal reasons go to the engine's log sink)
extern "C" void mwx_constraint_log(const char* msg) { MWX_LOG_ERROR("%s\n", msg); }
mwx_token mwx_token_eot(struct mwx_context* ctx) { return ctx->c.vocab.token_eot; }
mwx_token mwx_token_sot(struct mwx_context* ctx) { return ctx->c.vocab.token_sot; }
mwx_token mwx_token_beg(struct mwx_context* ctx) { return ctx->c.vocab.token_beg; }
mwx_token mwx_token_not(struct mwx_context* ctx) { return ctx->c.vocab.token_not; }
mwx_token mwx_token_nosp(struct mwx_context* ctx) { return ctx->c.vocab.token_nosp; }
mwx_token mwx_token_transcribe(struct mwx_context* ctx) { return ctx->c.vocab.token_transcribe; }
mwx_token mwx_token_translate(struct mwx_context* ctx) { return ctx->c.vocab.token_translate; }
mwx_token mwx_token_lang(struct mwx_context* ctx, int lang_id) {
  return ctx->c.vocab.token_sot + 1 + lang_id;
}
int mwx_n_vocab(struct mwx_context* ctx) { return ctx->c.hp.n_vocab; }
int mwx_n_text_ctx(struct mwx_context* ctx) { return ctx->c.hp.n_text_ctx; }
int mwx_n_audio_ctx(struct mwx_context* ctx) { return ctx->c.hp.n_audio_ctx; }
int mwx_audio_ctx_for(struct mwx_context* ctx, int n_samples, int seek, int audio_ctx, bool fit) {
  const int N = ctx ? ctx->c.hp.n_audio_ctx : 1500;
  if (audio_ctx > N) return -1;
  const int n = std::max(0, n_samples);
  const int n_len_org = n > 0 ? 1 + (n + 200 - 400) / MWX_HOP_LENGTH : 0;
  return mwx::audio_ctx_rule(N, n_len_org, seek, audio_ctx, fit);
}
int mwx_n_mels(struct mwx_context* ctx) { return ctx->c.hp.n_mels; }
int mwx_is_multilingual(struct mwx_context* ctx) { return ctx->c.vocab.is_multilingual() ? 1 : 0; }
int mwx_model_wtype(struct mwx_context* ctx) { return ctx->c.wtype; }

void mwx_perf_enable(struct mwx_state* state, const char* kernel_class) {
  if (!state) return;
  State& S = state->s;
  S.perf_class = kernel_class ? kernel_class : "";
  S.perf_classes.clear();
  size_t p = 0;
  while (p < S.perf_class.size()) {
    size_t q = S.perf_class.find(',', p);
    if (q == std::string::npos) q = S.perf_class.size();
    if (q > p) S.perf_classes.push_back(S.perf_class.substr(p, q - p));
    p = q + 1;
  }
  S.perf_used = 0;
  S.perf_acc_ms.assign(S.perf_classes.size(), 0.0);
  S.perf_acc_n.assign(S.perf_classes.size(), 0);
  S.span_eused = 0;
  bool spans = false;
  for (const auto& c : S.perf_classes) spans |= c.size() > 5 && c.compare(c.size() - 5, 5, ".span") == 0;
  if (spans && !S.perf_span.p) {
    try {
      std::lock_guard<std::recursive_mutex> lock(mwx::capture_mutex());
      S.perf_span.get((size_t)(mwx::State::SPAN_G + mwx::State::SPAN_E) * mwx::SPAN_SLOT_U64 * 8, true);
      HIPC(hipHostMalloc((void**)&S.span_host,
                         (size_t)std::max(mwx::State::SPAN_G, mwx::State::SPAN_E) * mwx::SPAN_SLOT_U64 * 8,
                         hipHostMallocDefault));
      HIPC(hipStreamCreateWithFlags(&S.span_stream, hipStreamNonBlocking));
      int khz = 0;
      HIPC(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, S.ctx ? S.ctx->device : 0));
      S.span_tick_ms = khz > 0 ? 1.0 / khz : 1e-5;  // (100 MHz if unreported)
    } catch (...) {
    }
  }
}

static int perf_read_index(struct mwx_state* state, int ci, double* total_ms, int* launches) {
  State& S = state->s;
  try {
    HIPC(hipStreamSynchronize(S.stream));
    mwx::harvest_events(S.perf_ev, S.perf_tag, S.perf_used, S);
    mwx::harvest_spans(S, false);
  } catch (...) {
    return -1;
  }
  S.perf_used = 0;
  const bool ok = ci >= 0 && ci < (int)S.perf_acc_ms.size();
  if (total_ms) *total_ms = ok ? S.perf_acc_ms[ci] : 0.0;
  if (launches) *launches = ok ? (int)S.perf_acc_n[ci] : 0;
  if (ok) {
    S.perf_acc_ms[ci] = 0.0;
    S.perf_acc_n[ci] = 0;
  }
  return 0;
}

int mwx_perf_read(struct mwx_state* state, double* total_ms, int* launches) {
  if (!state) return -1;
  return perf_read_index(state, 0, total_ms, launches);
}

int mwx_perf_read_class(struct mwx_state* state, const char* kernel_class, double* total_ms,
                        int* launches) {
  if (!state || !kernel_class) return -1;
  return perf_read_index(state, mwx::perf_class_index(state->s, kernel_class), total_ms, launches);
}

int mwx_tokenize(struct mwx_context* ctx, const char* text, mwx_token* tokens, int n_max_tokens) {
  if (!ctx || !text) return 0;
  const auto res = mwx::tokenize(ctx->c.vocab, text);
  if (n_max_tokens < (int)res.size()) return -(int)res.size();
  for (size_t i = 0; i < res.size(); ++i) tokens[i] = res[i];
  return (int)res.size();
}

}  // extern "C"

// ===========================================================================
// per-stage test entry points (include/mwx_test.h)
// ===========================================================================
#include "mwx_test.h"

namespace mwx {

static int test_mel_impl(Context& C, State& S, const float* pcm, int n, long* mel_stride) {
  const int n_len = (n + MWX_SAMPLE_RATE * MWX_CHUNK_SIZE) / MWX_HOP_LENGTH;
  const int n_fft_frames = std::min((n + 200) / MWX_HOP_LENGTH + 1, n_len);
  float* d_pcm = (float*)S.pcm.get((size_t)n * 4);
  float* d_mel = (float*)S.mel.get((size_t)C.hp.n_mels * n_len * 4);
  float* d_mx = (float*)S.melmax.get(4);
  HIPC(hipMemcpyAsync(d_pcm, pcm, (size_t)n * 4, hipMemcpyHostToDevice, S.stream));
  MelClip md{};
  md.n = n;
  md.n_len = n_len;
  md.n_fft = n_fft_frames;
  const MelCommit mc = mel_cache_slots(S, md, C.hp.n_mels, getenv("MWX_NO_MEL_CACHE") == nullptr);
  MelClip* d_md = (MelClip*)S.meld.get(sizeof(MelClip));
  float* d_part = (float*)S.melpart.get(16 * 4);
  HIPC(hipMemcpyAsync(d_md, &md, sizeof(md), hipMemcpyHostToDevice, S.stream));
  launch_mel_batch(d_pcm, d_md, 1, n_len, C.d_filters, C.hp.n_mels, C.d_tables, d_mel, d_part,
                   d_mx, S.stream);
  mc.apply();
  HIPC(hipStreamSynchronize(S.stream));  // (md is on the stack)
  *mel_stride = (long)C.hp.n_mels * n_len;
  return n_len;
}

template <typename T>
static void to_f32_host(const void* dev, size_t n, float* out, hipStream_t st) {
  std::vector<T> h(n);
  HIPC(hipMemcpyAsync(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; ++i) out[i] = (float)h[i];
}

template <typename T>
static int test_encode_impl(Context& C, State& S, const float* pcm, int n, int seek, float* enc_out,
                            float* k_out, float* v_out, int audio_ctx = 0) {
  long stride = 0;
  const int n_len = test_mel_impl(C, S, pcm, n, &stride);
  mwx_full_params P = mwx_full_default_params(MWX_SAMPLING_GREEDY);
  Driver<T> D(C, S, P);
  D.ensure_cross(1);
  // Lcap: (time) rows of a cache slot; L: the rows this encode produced
  const int Lcap = C.hp.n_audio_ctx, d = C.hp.n_audio_state, H = C.hp.n_audio_head;
  const int L = audio_ctx > 0 ? audio_ctx : Lcap;
  if (audio_ctx > 0)
    D.encode({0}, {seek}, {n_len}, {0}, stride, {audio_ctx});
  else
    D.encode({0}, {seek}, {n_len}, {0}, stride);
  // (the rows of one clip are the first rows of the buffer at any row count)
  if (enc_out) to_f32_host<T>(S.enc.p, (size_t)L * d, enc_out, S.stream);
  for (int kv = 0; kv < 2; ++kv) {
    float* dst = kv == 0 ? k_out : v_out;
    if (!dst) continue;
    const size_t per_layer = (size_t)S.cross_cap * H * Lcap * 64;
    const size_t n_el = (size_t)C.hp.n_text_layer * per_layer;
    std::vector<float> f(n_el);
    if (S.cross_kv8) {  // MX-fp8 cache: codes x 2^(scale - 127)
      std::vector<uint8_t> q(n_el), sc(n_el / 32);
      HIPC(hipMemcpyAsync(q.data(), kv == 0 ? S.cross_k.p : S.cross_v.p, n_el, hipMemcpyDeviceToHost,
                          S.stream));
      HIPC(hipMemcpyAsync(sc.data(), kv == 0 ? S.cross_ks.p : S.cross_vs.p, n_el / 32,
                          hipMemcpyDeviceToHost, S.stream));
      HIPC(hipStreamSynchronize(S.stream));
      for (size_t i = 0; i < n_el; ++i) f[i] = mwx::mx_dequant(q[i], sc[i / 32]);
    } else {
      std::vector<_Float16> h(n_el);
      HIPC(hipMemcpyAsync(h.data(), kv == 0 ? S.cross_k.p : S.cross_v.p, n_el * 2,
                          hipMemcpyDeviceToHost, S.stream));
      HIPC(hipStreamSynchronize(S.stream));
      for (size_t i = 0; i < n_el; ++i) f[i] = (float)h[i];
    }
    for (int l = 0; l < C.hp.n_text_layer; ++l)
      for (int hh = 0; hh < H; ++hh)
        for (int t = 0; t < L; ++t)
          for (int e = 0; e < 64; ++e)
            dst[((size_t)l * L + t) * d + hh * 64 + e] =
                f[(size_t)l * per_layer + (((size_t)hh * Lcap + t) * 64) + e];
  }
  return 0;
}

template <typename T>
static int test_encode_dump_impl(Context& C, State& S, const float* pcm, int n, int seek,
                                 float* x_out, uint16_t* const* a_out) {
  long stride = 0;
  const int n_len = test_mel_impl(C, S, pcm, n, &stride);
  mwx_full_params P = mwx_full_default_params(MWX_SAMPLING_GREEDY);
  Driver<T> D(C, S, P);
  D.ensure_cross(1);
  typename Driver<T>::EncDump dp{x_out, {a_out[0], a_out[1], a_out[2], a_out[3]}};
  D.dump = &dp;
  D.encode({0}, {seek}, {n_len}, {0}, stride);
  HIPC(hipStreamSynchronize(S.stream));
  return 0;
}

template <typename T>
static int test_decode_impl(Context& C, State& S, const int* tokens, int n, float* logits_out,
                            bool last_only = false) {
  mwx_full_params P = mwx_full_default_params(MWX_SAMPLING_GREEDY);
  Driver<T> D(C, S, P);
  D.live_slots = {0};
  D.ensure_rows(1);
  D.build_static_mask();
  const int V = C.hp.n_vocab;
  for (int i = 0; i < n; ++i) {
    int si[4] = {tokens[i], i, 1, 0};
    RowCtl ctl;
    memset(&ctl, 0, sizeof(ctl));
    ctl.active = 1;
    HIPC(hipMemcpyAsync(S.stepin.p, si, sizeof(si), hipMemcpyHostToDevice, S.stream));
    HIPC(hipMemcpyAsync(S.ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice, S.stream));
    D.decode_step(1, false);
    if (!last_only || i == n - 1)
      HIPC(hipMemcpyAsync(logits_out + (last_only ? 0 : (size_t)i * V), S.logits.p,
                          (size_t)V * 4, hipMemcpyDeviceToHost, S.stream));
  }
  HIPC(hipStreamSynchronize(S.stream));
  return 0;
}

// As test_decode_impl(last_only) but positions 0 .. n-2 go through the
// batched prompt prefill (Driver::prefill, one row) and only the last token
// is a decode step: the prefill's K / V must give the stepwise logits bit for
// bit.
template <typename T>
static int test_decode_prefill_impl(Context& C, State& S, const int* tokens, int n,
                                    float* logits_last) {
  mwx_full_params P = mwx_full_default_params(MWX_SAMPLING_GREEDY);
  Driver<T> D(C, S, P);
  D.live_slots = {0};
  D.ensure_rows(1);
  D.build_static_mask();
  if (n > 1) {
    std::vector<typename Driver<T>::PrefillRow> prs{{0, 0, tokens, n - 1}};
    D.prefill(prs);
  }
  int si[4] = {tokens[n - 1], n - 1, 1, 0};
  RowCtl ctl;
  memset(&ctl, 0, sizeof(ctl));
  ctl.active = 1;
  HIPC(hipMemcpyAsync(S.stepin.p, si, sizeof(si), hipMemcpyHostToDevice, S.stream));
  HIPC(hipMemcpyAsync(S.ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice, S.stream));
  D.decode_step(1, false);
  HIPC(hipMemcpyAsync(logits_last, S.logits.p, (size_t)C.hp.n_vocab * 4, hipMemcpyDeviceToHost,
                      S.stream));
  HIPC(hipStreamSynchronize(S.stream));
  return 0;
}

}  // namespace mwx

extern "C" {

int mwx_test_self_kv(struct mwx_state* state, int layer, int n_pos, float* k_out, float* v_out) {
  if (!state || n_pos <= 0) return -1;
  State& S = state->s;
  try {
    const mwx::Hparams& hp = S.ctx->hp;
    const int H = hp.n_text_head, Tctx = hp.n_text_ctx;
    if (layer < 0 || layer >= hp.n_text_layer || n_pos > Tctx || S.row_cap < 1) return -1;
    const size_t layer_self = (size_t)S.row_cap * H * Tctx * 64;
    std::vector<_Float16> hk((size_t)H * Tctx * 64), hv(hk.size());
    HIPC(hipMemcpyAsync(hk.data(), (_Float16*)S.kself.p + layer * layer_self, hk.size() * 2,
                        hipMemcpyDeviceToHost, S.stream));
    HIPC(hipMemcpyAsync(hv.data(), (_Float16*)S.vself.p + layer * layer_self, hv.size() * 2,
                        hipMemcpyDeviceToHost, S.stream));
    HIPC(hipStreamSynchronize(S.stream));
    for (int h = 0; h < H; ++h)
      for (int p = 0; p < n_pos; ++p)
        for (int e = 0; e < 64; ++e) {
          const size_t src = ((size_t)h * Tctx + p) * 64 + e, dst = ((size_t)p * H + h) * 64 + e;
          k_out[dst] = (float)hk[src];
          v_out[dst] = (float)hv[src];
        }
    return 0;
  } catch (...) {
    return -1;
  }
}

int mwx_test_decode_last_prefill(struct mwx_context* ctx, struct mwx_state* state,
                                 const int* tokens, int n, float* logits_last) {
  if (!ctx || !state || !tokens || n <= 0 || n > ctx->c.hp.n_text_ctx) return -1;
  if (!mwx::tokens_valid(tokens, n, ctx->c.hp.n_vocab)) return -1;
  if (state->s.cross_cap < 1) return -2;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (ctx->c.wtype == mwx::GGML_BF16)
      return mwx::test_decode_prefill_impl<__bf16>(ctx->c, state->s, tokens, n, logits_last);
    return mwx::test_decode_prefill_impl<_Float16>(ctx->c, state->s, tokens, n, logits_last);
  } catch (...) {
    return -1;
  }
}

int mwx_test_mel(struct mwx_context* ctx, struct mwx_state* state, const float* pcm, int n,
                 float* out, long out_cap) {
  if (!ctx || !state || !pcm || n <= 0) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    long stride = 0;
    const int n_len = mwx::test_mel_impl(ctx->c, state->s, pcm, n, &stride);
    if (out && out_cap >= stride) {
      HIPC(hipMemcpyAsync(out, state->s.mel.p, (size_t)stride * 4, hipMemcpyDeviceToHost,
                          state->s.stream));
    }
    HIPC(hipStreamSynchronize(state->s.stream));
    return n_len;
  } catch (...) {
    return -1;
  }
}

int mwx_test_encode(struct mwx_context* ctx, struct mwx_state* state, const float* pcm, int n,
                    int seek, float* enc_out, float* k_out, float* v_out) {
  if (!ctx || !state || !pcm || n <= 0) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (ctx->c.wtype == mwx::GGML_BF16)
      return mwx::test_encode_impl<__bf16>(ctx->c, state->s, pcm, n, seek, enc_out, k_out, v_out);
    return mwx::test_encode_impl<_Float16>(ctx->c, state->s, pcm, n, seek, enc_out, k_out, v_out);
  } catch (...) {
    return -1;
  }
}

int mwx_test_encode_ctx(struct mwx_context* ctx, struct mwx_state* state, const float* pcm, int n,
                        int seek, int audio_ctx, float* enc_out, float* k_out, float* v_out) {
  if (!ctx || !state || !pcm || n <= 0) return -1;
  if (audio_ctx < 1 || audio_ctx > ctx->c.hp.n_audio_ctx) return -5;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (ctx->c.wtype == mwx::GGML_BF16)
      return mwx::test_encode_impl<__bf16>(ctx->c, state->s, pcm, n, seek, enc_out, k_out, v_out,
                                           audio_ctx);
    return mwx::test_encode_impl<_Float16>(ctx->c, state->s, pcm, n, seek, enc_out, k_out, v_out,
                                           audio_ctx);
  } catch (...) {
    return -1;
  }
}

int mwx_test_encode_dump(struct mwx_context* ctx, struct mwx_state* state, const float* pcm,
                         int n, int seek, float* x_out, uint16_t* const* a_out) {
  if (!ctx || !state || !pcm || n <= 0 || !x_out || !a_out) return -1;
  for (int g = 0; g < 4; ++g)
    if (!a_out[g]) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (ctx->c.wtype == mwx::GGML_BF16)
      return mwx::test_encode_dump_impl<__bf16>(ctx->c, state->s, pcm, n, seek, x_out, a_out);
    return mwx::test_encode_dump_impl<_Float16>(ctx->c, state->s, pcm, n, seek, x_out, a_out);
  } catch (...) {
    return -1;
  }
}

int mwx_test_decode(struct mwx_context* ctx, struct mwx_state* state, const int* tokens, int n,
                    float* logits_out) {
  if (!ctx || !state || !tokens || n <= 0 || n > ctx->c.hp.n_text_ctx) return -1;
  if (!mwx::tokens_valid(tokens, n, ctx->c.hp.n_vocab)) return -1;
  if (state->s.cross_cap < 1) return -2;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (ctx->c.wtype == mwx::GGML_BF16)
      return mwx::test_decode_impl<__bf16>(ctx->c, state->s, tokens, n, logits_out);
    return mwx::test_decode_impl<_Float16>(ctx->c, state->s, tokens, n, logits_out);
  } catch (...) {
    return -1;
  }
}

int mwx_test_set_xattn_mfs(int on) { return mwx::xattn_mfs_set(on); }

int mwx_test_set_dec_shared(int on) { return mwx::dec_shared_set(on); }

int mwx_test_set_gemm_8ph(int on) { return mwx::gemm_8ph_set(on); }

int mwx_test_set_ln_fold(int on) {
  return mwx::ln_fold_mode().exchange(on < 0 ? -1 : (on ? 1 : 0));
}


long mwx_test_set_ra_mismatch(long step) { return mwx::ra_mismatch_mode().exchange(step); }

int mwx_test_decode_counters(struct mwx_state* state, long* steps, long* prefill_positions,
                             int reset) {
  if (!state) return -1;
  State& S = state->s;
  if (steps) *steps = S.n_steps;
  if (prefill_positions) *prefill_positions = S.n_prefill;
  if (reset) S.n_steps = S.n_prefill = 0;
  return 0;
}

int mwx_test_window_counters(struct mwx_state* state, long* windows, long* attempts,
                             long* clip_steps, int reset) {
  if (!state) return -1;
  State& S = state->s;
  if (windows) *windows = S.n_windows;
  if (attempts) *attempts = S.n_attempts;
  if (clip_steps) *clip_steps = S.n_clip_steps;
  if (reset) S.n_windows = S.n_attempts = S.n_clip_steps = 0;
  return 0;
}

long mwx_test_runahead_fallbacks(struct mwx_state* state, int reset) {
  if (!state) return -1;
  const long n = state->s.n_ra_fallback;
  if (reset) state->s.n_ra_fallback = 0;
  return n;
}

int mwx_test_decode_last(struct mwx_context* ctx, struct mwx_state* state, const int* tokens,
                         int n, float* logits_last) {
  if (!ctx || !state || !tokens || n <= 0 || n > ctx->c.hp.n_text_ctx) return -1;
  if (!mwx::tokens_valid(tokens, n, ctx->c.hp.n_vocab)) return -1;
  if (state->s.cross_cap < 1) return -2;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (ctx->c.wtype == mwx::GGML_BF16)
      return mwx::test_decode_impl<__bf16>(ctx->c, state->s, tokens, n, logits_last, true);
    return mwx::test_decode_impl<_Float16>(ctx->c, state->s, tokens, n, logits_last, true);
  } catch (...) {
    return -1;
  }
}

}  // extern "C"

// device buffers of one test hook, freed on every exit (HIPC throws)
struct DevScratch {
  std::vector<void*> p;
  void* get(size_t bytes) {
    void* q = nullptr;
    HIPC(hipMalloc(&q, bytes));
    p.push_back(q);
    return q;
  }
  ~DevScratch() {
    for (void* q : p) (void)hipFree(q);
  }
};

extern "C" int mwx_test_gemm_mx(struct mwx_context* ctx, int M, int N, int K, const float* a,
                                const float* w, float* c) {
  if (!ctx || !a || !w || !c || M <= 0 || N <= 0 || K <= 0 || K % 128) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    std::vector<uint16_t> ab((size_t)M * K);
    for (size_t i = 0; i < ab.size(); ++i) ab[i] = mwx::f32_to_bf16(a[i]);
    std::vector<uint8_t> wq((size_t)N * K), ws((size_t)N * (K / 32));
    std::vector<float> row(K);
    for (int n = 0; n < N; ++n) {
      for (int k = 0; k < K; ++k) row[k] = mwx::bf16_to_f32(mwx::f32_to_bf16(w[(size_t)n * K + k]));
      mwx::mx_quantize_row(row.data(), K, wq.data() + (size_t)n * K, ws.data() + (size_t)n * (K / 32));
    }
    DevScratch m;
    void* da = m.get(ab.size() * 2);
    void* dq = m.get((size_t)M * K);
    void* dsa = m.get((size_t)M * (K / 32));
    void* dw = m.get(wq.size());
    void* dsw = m.get(ws.size());
    void* dc = m.get((size_t)M * N * 4);
    HIPC(hipMemcpy(da, ab.data(), ab.size() * 2, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dw, wq.data(), wq.size(), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dsw, ws.data(), ws.size(), hipMemcpyHostToDevice));
    mwx::mx_quantize<__bf16>((const __bf16*)da, K, M, K, (uint8_t*)dq, (uint8_t*)dsa, nullptr);
    mwx::EpiParams e;
    e.c32 = (float*)dc;
    e.ldc = N;
    e.sa = (const uint8_t*)dsa;
    e.sw = (const uint8_t*)dsw;
    mwx::gemm_mx<__bf16>(mwx::EPI_F32, (const uint8_t*)dq, K, 0, (const uint8_t*)dw, K, M, N, K,
                         1, e, nullptr);
    HIPC(hipMemcpy(c, dc, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return 0;
  } catch (...) {
    return -2;
  }
}


// The encoder FFN1 GEMM (gemm_big, EPI_GELU, staged epilogue) on given data:
// a [M][K], w [N][K] rounded to T (bf16 != 0: bf16, else f16), bias [N];
// out [M][N] = gelu_ggml(a.w + bias) as T, widened to f32. use_table selects
// the table lookup (the engine's path) or the per-output tanhf evaluation.
extern "C" int mwx_test_gemm_gelu(struct mwx_context* ctx, int M, int N, int K, const float* a,
                                  const float* w, const float* bias, int bf16, int use_table,
                                  float* out) {
  if (!ctx || !a || !w || !bias || !out || M <= 0 || N <= 0 || N % 64 || K <= 0 || K % 64)
    return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    auto cvt = [&](float f) { return bf16 ? mwx::f32_to_bf16(f) : mwx::f32_to_f16(f); };
    std::vector<uint16_t> ah((size_t)M * K), wh((size_t)N * K);
    for (size_t i = 0; i < ah.size(); ++i) ah[i] = cvt(a[i]);
    for (size_t i = 0; i < wh.size(); ++i) wh[i] = cvt(w[i]);
    DevScratch m;
    void* da = m.get(ah.size() * 2);
    void* dw = m.get(wh.size() * 2);
    void* db = m.get((size_t)N * 4);
    void* dc = m.get((size_t)M * N * 2);
    HIPC(hipMemcpy(da, ah.data(), ah.size() * 2, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dw, wh.data(), wh.size() * 2, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    mwx::EpiParams e;
    e.bias = (const float*)db;
    e.c16 = dc;
    e.ldc = N;
    e.gelu_tab = use_table ? ctx->c.gelu_tab : nullptr;
    if (bf16)
      mwx::gemm<__bf16>(mwx::EPI_GELU, false, (const __bf16*)da, K, 0, (const __bf16*)dw, K, M, N,
                        K, 1, e, nullptr);
    else
      mwx::gemm<_Float16>(mwx::EPI_GELU, false, (const _Float16*)da, K, 0, (const _Float16*)dw, K,
                          M, N, K, 1, e, nullptr);
    std::vector<uint16_t> ch((size_t)M * N);
    HIPC(hipMemcpy(ch.data(), dc, ch.size() * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ch.size(); ++i)
      out[i] = bf16 ? mwx::bf16_to_f32(ch[i]) : mwx::f16_to_f32(ch[i]);
    return 0;
  } catch (...) {
    return -2;
  }
}

// The MX-fp8 grouped cross-attention on given data: q [R][H*64] f32 (rounded
// to f16 by the kernel, as a decode query), K / V e4m3 codes [G][H][n][64] and
// E8M0 scales [G][H][n][2], rows r*nq .. r*nq+nq-1 on slot r; o [R][H*64] f32
// (the kernel's T output widened). MFMA or v_dot2 per mwx_test_set_xattn_mfs.
template <typename T>
static void test_xattn_mx_impl(int R, int H, int n, int nq, const float* q, const uint8_t* k8,
                               const uint8_t* ks, const uint8_t* v8, const uint8_t* vs,
                               float* o) {
  const int D = H * 64, G = R / nq;
  const size_t kvb = (size_t)G * H * n * 64, scb = (size_t)G * H * n * 2;
  const size_t R64 = (R + 63) / 64 * 64;
  DevScratch m;
  void* dq = m.get((size_t)R * D * 4);
  void* dbias = m.get((size_t)D * 4);
  void* dk = m.get(kvb);
  void* dks = m.get(scb);
  void* dv = m.get(kvb);
  void* dvs = m.get(scb);
  void* dkv = m.get((size_t)R * 4);
  void* dact = m.get((size_t)R * 4);
  void* dout = m.get(R64 * D * sizeof(T));
  std::vector<int> kvi(R), act(R, 1);
  for (int r = 0; r < R; ++r) kvi[r] = r / nq;
  HIPC(hipMemcpy(dq, q, (size_t)R * D * 4, hipMemcpyHostToDevice));
  HIPC(hipMemset(dbias, 0, (size_t)D * 4));
  HIPC(hipMemcpy(dk, k8, kvb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dks, ks, scb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dv, v8, kvb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dvs, vs, scb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dkv, kvi.data(), (size_t)R * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dact, act.data(), (size_t)R * 4, hipMemcpyHostToDevice));
  HIPC(hipMemset(dout, 0, R64 * D * sizeof(T)));
  const bool ok = mwx::dec_cross_attention_grouped<T>(
      (const float*)dq, 1, D, (const float*)dbias, dk, dv, (const int*)dkv, (const int*)dact, n,
      n, (T*)dout, R, H, powf(64.0f, -0.25f), nq, nullptr, (const uint8_t*)dks,
      (const uint8_t*)dvs);
  std::vector<T> ob(R64 * D);
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpy(ob.data(), dout, ob.size() * sizeof(T), hipMemcpyDeviceToHost));
  if (!ok) throw std::runtime_error("unsupported group");
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < D; ++c) o[(size_t)r * D + c] = (float)ob[mwx::pack_index(r, c, D)];
}

extern "C" int mwx_test_mx_widen(struct mwx_context* ctx, const uint8_t* codes,
                                 const uint8_t* e8, int n8, uint16_t* out) {
  if (!ctx || !codes || !e8 || !out || n8 <= 0) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    DevScratch m;
    void* dc = m.get((size_t)n8 * 8);
    void* de = m.get((size_t)n8);
    void* dout = m.get((size_t)n8 * 16);
    HIPC(hipMemcpy(dc, codes, (size_t)n8 * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(de, e8, (size_t)n8, hipMemcpyHostToDevice));
    mwx::mx_widen_test((const uint8_t*)dc, (const uint8_t*)de, n8, (uint16_t*)dout, nullptr);
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(out, dout, (size_t)n8 * 16, hipMemcpyDeviceToHost));
    return 0;
  } catch (...) {
    return -2;
  }
}

extern "C" int mwx_test_xattn_mx(struct mwx_context* ctx, int R, int H, int n, int nq,
                                 const float* q, const uint8_t* k8, const uint8_t* ks,
                                 const uint8_t* v8, const uint8_t* vs, float* o) {
  if (!ctx || !q || !k8 || !ks || !v8 || !vs || !o || R <= 0 || H <= 0 || nq < 1 || nq > 8 ||
      R % nq || n < 1 || n > 1536)
    return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (ctx->c.wtype == mwx::GGML_BF16)
      test_xattn_mx_impl<__bf16>(R, H, n, nq, q, k8, ks, v8, vs, o);
    else
      test_xattn_mx_impl<_Float16>(R, H, n, nq, q, k8, ks, v8, vs, o);
    return 0;
  } catch (...) {
    return -2;
  }
}

extern "C" int mwx_test_sample_draws(struct mwx_context* ctx, const float* probs,
                                     const float* logprobs, int R, int V, const double* u,
                                     const int* ndraw, int KD, int exact, int reps, int* ids,
                                     double* us) {
  if (!ctx || !probs || !logprobs || !u || !ndraw || !ids || R <= 0 || V <= 0 || KD < 1 ||
      KD > 16)
    return -1;
  for (int r = 0; r < R; ++r)
    if (ndraw[r] < 0 || ndraw[r] > KD) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    DevScratch m;
    void* dp = m.get((size_t)R * V * 4);
    void* dl = m.get((size_t)R * V * 4);
    void* du = m.get((size_t)R * KD * 8);
    void* dn = m.get((size_t)R * 4);
    void* dd = m.get((size_t)R * KD * sizeof(mwx::Draw));
    void* dneed = m.get((size_t)R * 4);
    HIPC(hipMemcpy(dp, probs, (size_t)R * V * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dl, logprobs, (size_t)R * V * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(du, u, (size_t)R * KD * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dn, ndraw, (size_t)R * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    HIPC(hipEventCreate(&e0));
    HIPC(hipEventCreate(&e1));
    const int n = std::max(1, reps);
    mwx::sample_draws((const float*)dp, (const float*)dl, V, (const double*)du, (const int*)dn, KD,
                      (mwx::Draw*)dd, (int*)dneed, R, nullptr, exact ? 1 : 0);
    HIPC(hipEventRecord(e0, nullptr));
    for (int i = 1; i < n; ++i)
      mwx::sample_draws((const float*)dp, (const float*)dl, V, (const double*)du, (const int*)dn,
                        KD, (mwx::Draw*)dd, (int*)dneed, R, nullptr, exact ? 1 : 0);
    HIPC(hipEventRecord(e1, nullptr));
    HIPC(hipEventSynchronize(e1));
    float ms = 0.0f;
    HIPC(hipEventElapsedTime(&ms, e0, e1));
    if (us) *us = n > 1 ? 1000.0 * ms / (n - 1) : 0.0;
    std::vector<mwx::Draw> h((size_t)R * KD);
    HIPC(hipMemcpy(h.data(), dd, h.size() * sizeof(mwx::Draw), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i) ids[i] = h[i].id;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return 0;
  } catch (...) {
    return -2;
  }
}

// The decode attention launchers on given data (mwx_test_dec_attn): every
// index the kernels form was checked by the caller below, so the launch stays
// inside the buffers allocated here. The output buffer starts as all-ones
// bits (NaN in f16 and bf16): a row the kernel does not write reads back NaN.
template <typename T>
static int test_dec_attn_impl(int grouped, int prefill, int R, int H, int cap, int slots, int KS,
                              int nq, int fixed_len, const float* P, const float* bias,
                              float qscale, float kscale, float scale, uint16_t* kc, uint16_t* vc,
                              const int* kv_index, const int* pos, const int* active,
                              const int* kvmap, const int* own_from, int map_row0, float* o) {
  const int D = H * 64, pcols = fixed_len ? D : 3 * D;
  const size_t R64 = (size_t)(R + 63) / 64 * 64;
  const size_t pb = (size_t)KS * R * pcols * 4, cb = (size_t)slots * H * cap * 64 * 2;
  DevScratch m;
  void* dP = m.get(pb);
  void* dbias = m.get((size_t)pcols * 4);
  void* dk = m.get(cb);
  void* dv = m.get(cb);
  void* dkvi = kv_index ? m.get((size_t)R * 4) : nullptr;
  void* dpos = m.get((size_t)R * 4);
  void* dact = m.get((size_t)R * 4);
  void* dmap = kvmap ? m.get((size_t)R * cap * 4) : nullptr;
  void* down = own_from ? m.get((size_t)R * 4) : nullptr;
  void* dout = m.get(R64 * D * sizeof(T));
  HIPC(hipMemcpy(dP, P, pb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dbias, bias, (size_t)pcols * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dk, kc, cb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dv, vc, cb, hipMemcpyHostToDevice));
  if (dkvi) HIPC(hipMemcpy(dkvi, kv_index, (size_t)R * 4, hipMemcpyHostToDevice));
  if (pos)
    HIPC(hipMemcpy(dpos, pos, (size_t)R * 4, hipMemcpyHostToDevice));
  else
    HIPC(hipMemset(dpos, 0, (size_t)R * 4));
  HIPC(hipMemcpy(dact, active, (size_t)R * 4, hipMemcpyHostToDevice));
  if (dmap) HIPC(hipMemcpy(dmap, kvmap, (size_t)R * cap * 4, hipMemcpyHostToDevice));
  if (down) HIPC(hipMemcpy(down, own_from, (size_t)R * 4, hipMemcpyHostToDevice));
  HIPC(hipMemset(dout, 0xff, R64 * D * sizeof(T)));
  bool ok = true;
  if (grouped) {
    ok = mwx::dec_cross_attention_grouped<T>((const float*)dP, KS, pcols, (const float*)dbias, dk,
                                             dv, (const int*)dkvi, (const int*)dact, fixed_len,
                                             cap, (T*)dout, R, H, scale, nq, nullptr);
  } else {
    if (prefill)
      mwx::kv_append<T>((const float*)dP, KS, pcols, (const float*)dbias, kscale, (_Float16*)dk,
                        (_Float16*)dv, (const int*)dkvi, (const int*)dpos, (const int*)dact, cap,
                        R, H, nullptr);
    mwx::dec_attention<T>((const float*)dP, KS, pcols, (const float*)dbias, qscale, kscale,
                          (_Float16*)dk, (_Float16*)dv, (const int*)dkvi, (const int*)dpos,
                          (const int*)dact, fixed_len, cap, (T*)dout, R, H, scale, nullptr,
                          (const int*)dmap, (const int*)down, map_row0, nq, prefill ? 0 : 1);
  }
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  if (!ok) return -4;
  std::vector<uint16_t> ob(R64 * D);
  static_assert(sizeof(T) == 2, "16-bit output");
  HIPC(hipMemcpy(ob.data(), dout, ob.size() * 2, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(kc, dk, cb, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(vc, dv, cb, hipMemcpyDeviceToHost));
  const bool bf = std::is_same<T, __bf16>::value;
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < D; ++c) {
      const uint16_t b = ob[mwx::pack_index(r, c, D)];
      o[(size_t)r * D + c] = bf ? mwx::bf16_to_f32(b) : mwx::f16_to_f32(b);
    }
  return 0;
}

extern "C" int mwx_test_dec_attn(struct mwx_context* ctx, int bf16, int grouped, int prefill,
                                 int R, int H, int cap, int slots, int KS, int nq, int fixed_len,
                                 const float* P, const float* bias, float qscale, float kscale,
                                 float scale, uint16_t* kcache, uint16_t* vcache,
                                 const int* kv_index, const int* pos, const int* active,
                                 const int* kvmap, const int* own_from, int map_row0, float* o) {
  if (!ctx || !P || !bias || !kcache || !vcache || !active || !o) return -1;
  if (R < 1 || R > 1024 || H < 1 || H > 32 || cap < 1 || cap > 1536 || slots < 1 || slots > 64)
    return -1;
  if (KS < 1 || KS > 8 || nq < 1 || nq > 8 || R % nq) return -1;
  if (fixed_len < 0 || fixed_len > cap || fixed_len > 1536) return -1;
  const bool self = fixed_len == 0;
  if (self && (!pos || grouped)) return -1;
  if (!self && (prefill || kvmap || own_from)) return -1;
  if ((kvmap == nullptr) != (own_from == nullptr)) return -1;
  // the grouped kernel forms q = f16(sum + bias): no query scale
  if (grouped && (nq < 2 || qscale != 1.0f)) return -1;
  if (!kv_index && R > slots) return -1;
  // every row, active or not: the kernels fetch a row's control words (and the
  // self kernel its first position-map words) before the inactive-row exit
  for (int r = 0; r < R; ++r) {
    if (kv_index && (kv_index[r] < 0 || kv_index[r] >= slots)) return -1;
    if (!self) continue;
    if (pos[r] < 0 || pos[r] >= cap) return -1;
    if (!own_from) continue;
    if (own_from[r] < 0 || own_from[r] > pos[r]) return -1;
    for (int j = 0; j < own_from[r]; ++j) {
      const long s = (long)kvmap[(size_t)r * cap + j] - map_row0;
      if (s < 0 || s >= slots) return -1;
    }
  }
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (bf16)
      return test_dec_attn_impl<__bf16>(grouped, prefill, R, H, cap, slots, KS, nq, fixed_len, P,
                                        bias, qscale, kscale, scale, kcache, vcache, kv_index, pos,
                                        active, kvmap, own_from, map_row0, o);
    return test_dec_attn_impl<_Float16>(grouped, prefill, R, H, cap, slots, KS, nq, fixed_len, P,
                                        bias, qscale, kscale, scale, kcache, vcache, kv_index, pos,
                                        active, kvmap, own_from, map_row0, o);
  } catch (...) {
    return -2;
  }
}

// The decode GEMMs on given data (mwx_test_gemm_dec / _gemm_dec_ex). Every
// device output lies between two guard bands of sentinel words and starts as
// sentinel words itself, so a store outside it (or one left out) shows.
constexpr uint32_t TEST_GUARD_WORD = 0x7fc5a5a5u;  // a NaN no kernel produces
constexpr size_t TEST_GUARD_WORDS = 1024;

// A device output of `bytes` bytes between two guard bands of TEST_GUARD_WORD
// (the slack up to the next 16 bytes belongs to the upper band). The body
// starts as `init` (in-and-out buffers) or as all-ones bits: NaN as f16, bf16
// and f32, so a word no launch wrote reads back NaN.
struct GuardedBuf {
  uint8_t* dev = nullptr;
  size_t bytes = 0, total = 0;
  static constexpr size_t G = TEST_GUARD_WORDS * 4;
  void* make(DevScratch& m, size_t n, const void* init) {
    bytes = n;
    total = 2 * G + (n + 15) / 16 * 16;
    std::vector<uint32_t> img(total / 4, TEST_GUARD_WORD);
    if (init)
      memcpy((uint8_t*)img.data() + G, init, n);
    else
      memset((uint8_t*)img.data() + G, 0xff, n);
    dev = (uint8_t*)m.get(total);
    HIPC(hipMemcpy(dev, img.data(), total, hipMemcpyHostToDevice));
    return dev + G;
  }
  // copies the body to out; false if a band changed
  bool take(void* out) const {
    std::vector<uint32_t> img(total / 4);
    HIPC(hipMemcpy(img.data(), dev, total, hipMemcpyDeviceToHost));
    std::vector<uint32_t> want(total / 4, TEST_GUARD_WORD);
    memcpy((uint8_t*)want.data() + G, (const uint8_t*)img.data() + G, bytes);
    if (memcmp(want.data(), img.data(), total)) return false;
    memcpy(out, (const uint8_t*)img.data() + G, bytes);
    return true;
  }
};

template <typename T>
static int test_gemm_dec_impl(const mwx_test_gemm_dec_args& g) {
  const bool bf = std::is_same<T, __bf16>::value;
  auto cvt = [&](float f) { return bf ? mwx::f32_to_bf16(f) : mwx::f32_to_f16(f); };
  const int M = g.M, N = g.N, K = g.K, mode = g.mode;
  const size_t M64 = (size_t)(M + 63) / 64 * 64, N16 = (size_t)(N + 15) / 16 * 16;
  const int ks_want = mode == 0 ? mwx::splitk_factor(K) : 1;
  if (ks_want < 1 || ks_want > 8) return -4;
  DevScratch m;
  auto up = [&](const void* src, size_t bytes) -> void* {
    if (!src) return nullptr;
    void* d = m.get(bytes);
    HIPC(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    return d;
  };
  const T* da = nullptr;
  if (!g.ln) {
    std::vector<uint16_t> ap(M64 * K, 0);
    for (int r = 0; r < M; ++r)
      for (int k = 0; k < K; ++k) ap[mwx::pack_index(r, k, K)] = cvt(g.a[(size_t)r * K + k]);
    da = (const T*)up(ap.data(), ap.size() * 2);
  }
  mwx::DecW<T> W;
  if (g.w8) {
    std::vector<uint8_t> qp, sp;
    mwx::mx_pack_dec_weight(g.wq, g.ws, N, K, qp, sp);
    const uint8_t* dq = (const uint8_t*)up(qp.data(), qp.size());
    W = mwx::DecW<T>(dq, (const uint8_t*)up(sp.data(), sp.size()));
  } else {
    std::vector<uint16_t> wp(N16 * K, 0);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) wp[mwx::pack_index(n, k, K)] = cvt(g.w[(size_t)n * K + k]);
    W = mwx::DecW<T>((const T*)up(wp.data(), wp.size() * 2));
  }
  // the output: f32 [ks][M][N] of sentinel words, or (mode 3) 0xFFFF T words
  const bool packed = mode == 3;
  const size_t body = packed ? M64 * N * 2 : (size_t)ks_want * M * N * 4;
  const std::vector<uint32_t> sent(std::max(body / 4, (size_t)K), TEST_GUARD_WORD);
  GuardedBuf og, xog, xig;
  void* dc = og.make(m, body, packed ? nullptr : sent.data());
  mwx::LnFuse f;
  if (g.ln) {
    const size_t kb = (size_t)K * 4;
    f.x_in = (const float*)xig.make(m, kb, g.x_in);
    f.x_out = (float*)xog.make(m, kb, sent.data());
    f.KS = g.KS;
    f.pstride = K;
    if (g.KS > 0) {
      f.P = (const float*)up(g.P, (size_t)g.KS * kb);
      f.pbias = (const float*)up(g.pbias, kb);
    }
    f.w = (const float*)up(g.ln_w, kb);
    f.b = (const float*)up(g.ln_b, kb);
    f.active = (const int*)up(g.active, 4);
  }
  int ks = 1;
  bool ok = true;
  if (mode == 0) {
    ks = g.ln ? mwx::gemm_splitk_ln<T>(f, W, N, K, (float*)dc, nullptr)
              : mwx::gemm_splitk_partials<T>(da, W, M, N, K, (float*)dc, nullptr);
    ok = ks == ks_want;
  } else {
    mwx::EpiParams e;
    e.ldc = N;
    if (packed) {
      e.c16 = dc;
      e.pack_out = true;
    } else {
      e.c32 = (float*)dc;
    }
    if (mode >= 2) e.bias = (const float*)up(g.bias, (size_t)N * 4);
    if (mode == 2) e.r32 = (const float*)up(g.res, (size_t)M * N * 4);
    const int epi = mode == 1 ? mwx::EPI_F32 : mode == 2 ? mwx::EPI_RES : mwx::EPI_GELU;
    ok = g.ln ? mwx::gemm_decode_ln<T>(epi, f, W, N, K, e, nullptr)
              : mwx::gemm_decode<T>(epi, da, W, M, N, K, e, nullptr);
  }
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  if (!ok) return -4;
  bool clean = true;
  if (packed) {
    clean = og.take(g.out16);
    if (clean)
      for (int r = 0; r < M; ++r)
        for (int n = 0; n < N; ++n) {
          const uint16_t v = g.out16[mwx::pack_index(r, n, N)];
          g.out[(size_t)r * N + n] = bf ? mwx::bf16_to_f32(v) : mwx::f16_to_f32(v);
        }
  } else {
    clean = og.take(g.out);
  }
  if (g.ln) {
    clean = xog.take(g.x_out) && clean;
    clean = xig.take(g.x_in) && clean;
  }
  if (!clean) return -3;
  if (g.ks_out) *g.ks_out = ks;
  return 0;
}

extern "C" int mwx_test_gemm_dec_ex(struct mwx_context* ctx,
                                    const struct mwx_test_gemm_dec_args* gp) {
  if (!ctx || !gp) return -1;
  const mwx_test_gemm_dec_args& g = *gp;
  if (!g.out || g.mode < 0 || g.mode > 3) return -1;
  if (g.M < 1 || g.M > 512 || g.N < 1 || g.N > 4096 || g.K < 32 || g.K > 8192 || g.K % 32)
    return -1;
  if (g.w8 ? (!g.wq || !g.ws) : !g.w) return -1;
  if (g.mode == 2 && !g.res) return -1;
  if (g.mode != 2 && g.res) return -1;
  if (g.mode < 2 && g.bias) return -1;
  // pack_index tiles of the output are 32 deep
  if (g.mode == 3 && (!g.bias || !g.out16 || g.N % 32)) return -1;
  if (g.ln) {
    if (g.M != 1 || (g.mode != 0 && g.mode != 3)) return -1;
    if (!g.x_in || !g.x_out || !g.ln_w || !g.ln_b || !g.active) return -1;
    if (g.KS < 0 || g.KS > 8 || (g.KS > 0 && (!g.P || !g.pbias))) return -1;
  } else if (!g.a) {
    return -1;
  }
  // (the engine enables MX decode weights for bf16 models only)
  if (g.w8 && !g.bf16) return -4;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    return g.bf16 ? test_gemm_dec_impl<__bf16>(g) : test_gemm_dec_impl<_Float16>(g);
  } catch (...) {
    return -2;
  }
}

extern "C" int mwx_test_gemm_dec(struct mwx_context* ctx, int bf16, int mode, int M, int N, int K,
                                 const float* a, const float* w, const float* bias,
                                 const float* res, int* ks_out, float* out) {
  if (mode < 0 || mode > 2) return -1;
  mwx_test_gemm_dec_args g{};
  g.bf16 = bf16;
  g.mode = mode;
  g.M = M;
  g.N = N;
  g.K = K;
  g.a = a;
  g.w = w;
  g.bias = bias;
  g.res = res;
  g.ks_out = ks_out;
  g.out = out;
  return mwx_test_gemm_dec_ex(ctx, &g);
}

// ---------------------------------------------------------------------------
// Encoder kernels on given data (mwx_test_enc_attn / _gemm_enc / _layer_norm)
// ---------------------------------------------------------------------------
template <typename T>
static int test_enc_attn_impl(int B, int H, int L, const int* lens, float scale,
                              const uint16_t* q, const uint16_t* k, const uint16_t* vt, float* o) {
  const int Lp = (L + 7) & ~7;
  const size_t qb = (size_t)B * H * L * 64 * 2, vb = (size_t)B * H * 64 * Lp * 2;
  const size_t on = (size_t)B * L * H * 64;
  DevScratch m;
  void* dq = m.get(qb);
  void* dk = m.get(qb);
  void* dv = m.get(vb);
  void* dl = lens ? m.get((size_t)B * 4) : nullptr;
  GuardedBuf og;
  void* dout = og.make(m, on * 2, nullptr);
  HIPC(hipMemcpy(dq, q, qb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dk, k, qb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dv, vt, vb, hipMemcpyHostToDevice));
  if (dl) HIPC(hipMemcpy(dl, lens, (size_t)B * 4, hipMemcpyHostToDevice));
  mwx::enc_attention<T>((const _Float16*)dq, (const _Float16*)dk, (const _Float16*)dv, (T*)dout, B,
                        H, L, scale, nullptr, (const int*)dl);
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  std::vector<uint16_t> ob(on);
  if (!og.take(ob.data())) return -3;
  const bool bf = std::is_same<T, __bf16>::value;
  for (size_t i = 0; i < on; ++i) o[i] = bf ? mwx::bf16_to_f32(ob[i]) : mwx::f16_to_f32(ob[i]);
  return 0;
}

extern "C" int mwx_test_enc_attn(struct mwx_context* ctx, int bf16, int B, int H, int L,
                                 const int* lens, float scale, const uint16_t* q,
                                 const uint16_t* k, const uint16_t* vt, float* o) {
  if (!ctx || !q || !k || !vt || !o) return -1;
  if (B < 1 || H < 1 || (long)B * H > 64 || L < 1 || L > 1536) return -1;
  if (lens)
    for (int b = 0; b < B; ++b)
      if (lens[b] < 1 || lens[b] > L) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (bf16) return test_enc_attn_impl<__bf16>(B, H, L, lens, scale, q, k, vt, o);
    return test_enc_attn_impl<_Float16>(B, H, L, lens, scale, q, k, vt, o);
  } catch (...) {
    return -2;
  }
}

template <typename T>
static int test_gemm_enc_impl(struct mwx_context* ctx, const mwx_test_gemm_enc_args& g) {
  const bool bf = std::is_same<T, __bf16>::value;
  auto cvt = [&](float f) { return bf ? mwx::f32_to_bf16(f) : mwx::f32_to_f16(f); };
  std::vector<uint16_t> ah((size_t)g.a_len), wh((size_t)g.N * g.K);
  for (size_t i = 0; i < ah.size(); ++i) ah[i] = cvt(g.a[i]);
  for (size_t i = 0; i < wh.size(); ++i) wh[i] = cvt(g.w[i]);
  DevScratch m;
  void* da = m.get(ah.size() * 2);
  HIPC(hipMemcpy(da, ah.data(), ah.size() * 2, hipMemcpyHostToDevice));
  mwx::EpiParams e;
  void *dw, *dq = nullptr;
  if (g.mx) {
    // w by the load-time host quantizer, a by the device kernel (dense [M][K])
    std::vector<uint8_t> wq((size_t)g.N * g.K), ws((size_t)g.N * (g.K / 32));
    std::vector<float> row(g.K);
    for (int n = 0; n < g.N; ++n) {
      for (int k = 0; k < g.K; ++k) {
        const uint16_t h = wh[(size_t)n * g.K + k];
        row[k] = bf ? mwx::bf16_to_f32(h) : mwx::f16_to_f32(h);
      }
      mwx::mx_quantize_row(row.data(), g.K, wq.data() + (size_t)n * g.K,
                           ws.data() + (size_t)n * (g.K / 32));
    }
    dw = m.get(wq.size());
    void* dsw = m.get(ws.size());
    dq = m.get((size_t)g.M * g.K);
    void* dsa = m.get((size_t)g.M * (g.K / 32));
    HIPC(hipMemcpy(dw, wq.data(), wq.size(), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dsw, ws.data(), ws.size(), hipMemcpyHostToDevice));
    mwx::mx_quantize<T>((const T*)da, g.K, g.M, g.K, (uint8_t*)dq, (uint8_t*)dsa, nullptr);
    e.sa = (const uint8_t*)dsa;
    e.sw = (const uint8_t*)dsw;
  } else {
    dw = m.get(wh.size() * 2);
    HIPC(hipMemcpy(dw, wh.data(), wh.size() * 2, hipMemcpyHostToDevice));
  }
  if (g.bias) {
    void* db = m.get((size_t)g.N * 4);
    HIPC(hipMemcpy(db, g.bias, (size_t)g.N * 4, hipMemcpyHostToDevice));
    e.bias = (const float*)db;
  }
  GuardedBuf o0, o1, o2, o3, o4;  // c16 | c32 | q, then k, v, and the MX cache's scales
  size_t qkb = 0, vb = 0;
  e.ldc = g.ldc;
  e.c_bstride = g.c_bstride;
  if (g.epi == mwx::EPI_GELU) {
    e.c16 = (uint16_t*)o0.make(m, (size_t)g.c_len * 2, g.c16) + g.c_off;
    e.gelu_tab = g.use_table ? ctx->c.gelu_tab : nullptr;
  } else if (g.epi == mwx::EPI_RES || g.epi == mwx::EPI_CONV2) {
    e.c32 = (float*)o0.make(m, (size_t)g.c_len * 4, g.c32) + g.c_off;
    if (g.epi == mwx::EPI_RES) {
      e.r32 = e.c32;
    } else {
      void* dp = m.get((size_t)g.M * g.ldc * 4);
      HIPC(hipMemcpy(dp, g.pe, (size_t)g.M * g.ldc * 4, hipMemcpyHostToDevice));
      e.pe = (const float*)dp;
    }
  } else {
    const int nb = g.M / g.L;
    e.L = g.L;
    e.H = g.H;
    e.d = g.d;
    if (g.epi == mwx::EPI_ENC_QKV) {
      qkb = (size_t)nb * g.H * g.L * 64 * 2;
      vb = (size_t)nb * g.H * 64 * g.ldv * 2;
      e.ldv = g.ldv;
      e.q = (_Float16*)o0.make(m, qkb, g.q);
    } else {
      qkb = vb = (size_t)(g.N / (2 * g.d)) * g.ncap * g.H * g.lcap * 64 * 2;
      e.lcap = g.lcap;
      e.ncap = g.ncap;
      e.kscale = g.kscale;
      void* ds = m.get((size_t)nb * 4);
      HIPC(hipMemcpy(ds, g.slot, (size_t)nb * 4, hipMemcpyHostToDevice));
      e.slot = (const int*)ds;
      if (g.kv8) {  // codes: one byte per element; two scales per row of 64
        qkb = vb = qkb / 2;
        e.ks8 = (uint8_t*)o3.make(m, qkb / 32, g.ks8);
        e.vs8 = (uint8_t*)o4.make(m, qkb / 32, g.vs8);
      }
    }
    e.k = (_Float16*)o1.make(m, qkb, g.kv8 ? (const void*)g.k8 : (const void*)g.k);
    e.v = (_Float16*)o2.make(m, vb, g.kv8 ? (const void*)g.v8 : (const void*)g.v);
  }
  if (g.mx)
    mwx::gemm_mx<T>(g.epi, (const uint8_t*)dq, g.K, 0, (const uint8_t*)dw, g.K, g.M, g.N, g.K, 1,
                    e, nullptr);
  else
    mwx::gemm<T>(g.epi, g.out16 != 0, (const T*)da, g.lda, g.a_bstride, (const T*)dw, g.K, g.M,
                 g.N, g.K, g.batch, e, nullptr);
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  bool ok = true;
  if (g.epi == mwx::EPI_GELU) {
    ok = o0.take(g.c16);
  } else if (g.epi == mwx::EPI_RES || g.epi == mwx::EPI_CONV2) {
    ok = o0.take(g.c32);
  } else {
    if (g.epi == mwx::EPI_ENC_QKV) ok = o0.take(g.q);
    ok = o1.take(g.kv8 ? (void*)g.k8 : (void*)g.k) && ok;
    ok = o2.take(g.kv8 ? (void*)g.v8 : (void*)g.v) && ok;
    if (g.kv8) {
      ok = o3.take(g.ks8) && ok;
      ok = o4.take(g.vs8) && ok;
    }
  }
  return ok ? 0 : -3;
}

extern "C" int mwx_test_gemm_enc(struct mwx_context* ctx, const struct mwx_test_gemm_enc_args* gp) {
  if (!ctx || !gp) return -1;
  const mwx_test_gemm_enc_args& g = *gp;
  if (!g.a || !g.w) return -1;
  if (g.M < 1 || g.M > 4096 || g.N < 64 || g.N > 2048 || g.N % 64 || g.K < 64 || g.K > 5120 ||
      g.K % 64 || g.batch < 1 || g.batch > 8)
    return -1;
  // 16-byte LDS-DMA reads of A: rows and batches start on 8 elements
  if (g.lda < 8 || g.lda % 8 || g.a_bstride < 0 || g.a_bstride % 8) return -1;
  if ((long)(g.batch - 1) * g.a_bstride + (long)(g.M - 1) * g.lda + g.K > g.a_len) return -1;
  if (g.mx && (g.K % 128 || g.lda != g.K || g.batch != 1 || g.epi == mwx::EPI_CONV2 || g.out16))
    return -1;
  if (g.kv8 && g.epi != mwx::EPI_CROSS_KV) return -1;
  const bool flat = g.epi == mwx::EPI_GELU || g.epi == mwx::EPI_RES || g.epi == mwx::EPI_CONV2;
  if (flat) {
    // 16-byte stores (8 16-bit words / 4 floats; 8 covers both)
    if (g.ldc < g.N || g.ldc % 8 || g.c_off < 0 || g.c_off % 8 || g.c_bstride < 0 ||
        g.c_bstride % 8)
      return -1;
    const long span = (long)(g.M - 1) * g.ldc + g.N;
    if (g.batch > 1 && g.c_bstride < span) return -1;  // batches may not overlap
    if (g.c_off + (long)(g.batch - 1) * g.c_bstride + span > g.c_len) return -1;
    if (g.epi == mwx::EPI_GELU ? !g.c16 : !g.c32) return -1;
    if (g.epi != mwx::EPI_RES && !g.bias) return -1;
    if (g.epi == mwx::EPI_CONV2 && !g.pe) return -1;
  } else if (g.epi == mwx::EPI_ENC_QKV || g.epi == mwx::EPI_CROSS_KV) {
    if (g.batch != 1 || !g.bias) return -1;
    if (g.kv8 ? (!g.k8 || !g.v8 || !g.ks8 || !g.vs8) : (!g.k || !g.v)) return -1;
    if (g.d < 64 || g.d % 64 || g.H * 64 != g.d || g.L < 1 || g.M % g.L) return -1;
    if (g.epi == mwx::EPI_ENC_QKV) {
      // the 8-byte V^T stores hold 4 consecutive t of one clip
      if (!g.q || g.N != 3 * g.d || g.L % 4 || g.ldv < g.L || g.ldv % 4) return -1;
    } else {
      if (g.N % (2 * g.d) || !g.slot || g.lcap < g.L || g.lcap > 1536 || g.ncap < 1 ||
          g.ncap > 64)
        return -1;
      const int nb = g.M / g.L;
      uint64_t seen = 0;
      for (int b = 0; b < nb; ++b) {
        if (g.slot[b] < 0 || g.slot[b] >= g.ncap || (seen >> g.slot[b] & 1)) return -1;
        seen |= 1ull << g.slot[b];
      }
    }
  } else {
    return -1;
  }
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (g.bf16) return test_gemm_enc_impl<__bf16>(ctx, g);
    return test_gemm_enc_impl<_Float16>(ctx, g);
  } catch (...) {
    return -2;
  }
}

template <typename T>
static int test_layer_norm_impl(int dec, int M, int N, float* x, const float* w, const float* b,
                                const int* active, const float* P, int KS, const float* pbias,
                                const float* te, const float* pe, const int* tok, const int* pos,
                                int n_tok, int n_pos, float* y) {
  const bool bf = std::is_same<T, __bf16>::value;
  const size_t rb = (size_t)N * 4, xb = (size_t)M * rb;
  const size_t yrows = dec ? (size_t)(M + 63) / 64 * 64 : (size_t)M;
  DevScratch m;
  auto up = [&](const void* src, size_t bytes) -> void* {
    if (!src) return nullptr;
    void* d = m.get(bytes);
    HIPC(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    return d;
  };
  GuardedBuf xg, yg;
  float* dx = (float*)xg.make(m, xb, x);
  T* dy = (T*)yg.make(m, yrows * N * 2, nullptr);
  const float* dw = (const float*)up(w, rb);
  const float* db = (const float*)up(b, rb);
  const int* dact = (const int*)up(active, (size_t)M * 4);
  const float* dP = (const float*)up(P, P ? (size_t)KS * xb : 0);
  const float* dpb = (const float*)up(pbias, rb);
  if (!dec) {
    mwx::layer_norm<T>(dx, dw, db, dy, M, N, dact, nullptr, dP, KS, dpb);
  } else {
    mwx::EmbedIn<T> emb;
    if (te) {
      std::vector<uint16_t> th((size_t)n_tok * N);
      for (size_t i = 0; i < th.size(); ++i)
        th[i] = bf ? mwx::f32_to_bf16(te[i]) : mwx::f32_to_f16(te[i]);
      emb.te = (const T*)up(th.data(), th.size() * 2);
      emb.pe = (const float*)up(pe, (size_t)n_pos * rb);
      emb.tok = (const int*)up(tok, (size_t)M * 4);
      emb.pos = (const int*)up(pos, (size_t)M * 4);
      emb.n_tok = n_tok;
      emb.n_pos = n_pos;
    }
    mwx::layer_norm_dec<T>(dx, dw, db, dy, M, N, dact, nullptr, dP, KS, dpb, emb);
  }
  HIPC(hipGetLastError());
  HIPC(hipDeviceSynchronize());
  std::vector<uint16_t> yh(yrows * N);
  if (!yg.take(yh.data()) || !xg.take(x)) return -3;
  for (int r = 0; r < M; ++r)
    for (int c = 0; c < N; ++c) {
      const uint16_t v = yh[dec ? (size_t)mwx::pack_index(r, c, N) : (size_t)r * N + c];
      y[(size_t)r * N + c] = bf ? mwx::bf16_to_f32(v) : mwx::f16_to_f32(v);
    }
  return 0;
}

extern "C" int mwx_test_layer_norm(struct mwx_context* ctx, int bf16, int dec, int M, int N,
                                   float* x, const float* w, const float* b, const int* active,
                                   const float* P, int KS, const float* pbias, const float* te,
                                   const float* pe, const int* tok, const int* pos, int n_tok,
                                   int n_pos, float* y) {
  if (!ctx || !x || !w || !b || !y || M < 1 || M > 1024 || N < 1) return -1;
  if (P && (KS < 1 || KS > 8 || !pbias)) return -1;
  if (te && (!dec || !pe || !tok || !pos || n_tok < 1 || n_pos < 1 || n_tok > 4096 ||
             n_pos > 4096))
    return -1;
  // layer_norm launches nothing for N > 2048; the decode kernel owns 8
  // elements per thread and writes pack_index tiles (32 deep)
  if (N > 2048 || (dec && N % 32)) return -4;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (bf16)
      return test_layer_norm_impl<__bf16>(dec, M, N, x, w, b, active, P, KS, pbias, te, pe, tok,
                                          pos, n_tok, n_pos, y);
    return test_layer_norm_impl<_Float16>(dec, M, N, x, w, b, active, P, KS, pbias, te, pe, tok,
                                          pos, n_tok, n_pos, y);
  } catch (...) {
    return -2;
  }
}

extern "C" int mwx_test_gelu_table_size(void) { return mwx::GELU_TAB_N; }

extern "C" int mwx_test_gelu_table(struct mwx_context* ctx, uint16_t* out) {
  if (!ctx || !out || !ctx->c.gelu_tab) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    HIPC(hipMemcpy(out, ctx->c.gelu_tab, (size_t)mwx::GELU_TAB_N * 2, hipMemcpyDeviceToHost));
    return 0;
  } catch (...) {
    return -2;
  }
}

// ---------------------------------------------------------------------------
// Logits processing on given data (mwx_test_logits_process / _setup)
// ---------------------------------------------------------------------------
static int test_logits_process_impl(struct mwx_context* ctx, int R, int V, const float* logits,
                                    const float* smask, const struct mwx_test_logits_ctl* ctl,
                                    const struct mwx_test_logits_const* lc, float* flt,
                                    float* probs, float* logprobs,
                                    struct mwx_test_logits_out* out, const uint64_t* cmask,
                                    float cpenalty) {
  if (!ctx || !logits || !smask || !ctl || !lc || !flt || !probs || !logprobs || !out) return -1;
  if (R < 1 || R > 256 || V < 1 || lc->n_vocab != V) return -1;
  auto in_v = [&](int i) { return i >= 0 && i < V; };
  if (!in_v(lc->eot) || !in_v(lc->space_id) || !in_v(lc->nosp_id) || lc->beg < 0 || lc->beg > V)
    return -1;
  for (int r = 0; r < R; ++r)
    if (ctl[r].seek_delta < 0) return -1;
  if (V > mwx::LP_G * mwx::LP_CHUNK) return -4;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    mwx::LogitsConst C;
    C.n_vocab = V;
    C.eot = lc->eot;
    C.beg = lc->beg;
    C.space_id = lc->space_id;
    C.suppress_blank = lc->suppress_blank;
    C.max_initial_tid = lc->max_initial_tid;
    C.nosp_id = lc->nosp_id;
    std::vector<mwx::RowCtl> hc(R);
    for (int r = 0; r < R; ++r) {
      mwx::RowCtl& k = hc[r];
      memset(&k, 0, sizeof(k));
      k.active = ctl[r].active;
      k.sample = ctl[r].sample;
      k.is_initial = ctl[r].is_initial;
      k.last_ts = ctl[r].last_ts;
      k.penult_ts = ctl[r].penult_ts;
      k.has_ts = ctl[r].has_ts;
      k.seek_delta = ctl[r].seek_delta;
      k.want_probs = ctl[r].want_probs;
      k.temperature = ctl[r].temperature;
      k.want_nosp = ctl[r].want_nosp;
    }
    const size_t rv = (size_t)R * V * 4;
    DevScratch m;
    float* dl = (float*)m.get(rv);
    float* dm = (float*)m.get((size_t)V * 4);
    mwx::RowCtl* dc = (mwx::RowCtl*)m.get((size_t)R * sizeof(mwx::RowCtl));
    HIPC(hipMemcpy(dl, logits, rv, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dm, smask, (size_t)V * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dc, hc.data(), (size_t)R * sizeof(mwx::RowCtl), hipMemcpyHostToDevice));
    GuardedBuf gf, gp, gl, go, gparts, gres;
    mwx::LPScratch ws;
    ws.flt = (float*)gf.make(m, rv, nullptr);
    ws.parts = (mwx::LPPart*)gparts.make(m, (size_t)R * mwx::LP_G * sizeof(mwx::LPPart), nullptr);
    ws.res = (mwx::LPRes*)gres.make(m, (size_t)R * mwx::LP_G * sizeof(mwx::LPRes), nullptr);
    float* dp = (float*)gp.make(m, rv, nullptr);
    float* dlp = (float*)gl.make(m, rv, nullptr);
    mwx::TokOut* dout = (mwx::TokOut*)go.make(m, (size_t)R * sizeof(mwx::TokOut), nullptr);
    unsigned long long* dcm = nullptr;
    if (cmask) {  // (constrained decoding: the filter's mask and penalty arguments)
      const size_t mb = (size_t)R * ((V + 63) / 64) * 8;
      dcm = (unsigned long long*)m.get(mb);
      HIPC(hipMemcpy(dcm, cmask, mb, hipMemcpyHostToDevice));
    }
    mwx::logits_process(dl, dm, dc, dout, dp, dlp, C, R, ws, nullptr, true, dcm,
                        dcm ? cpenalty : 0.0f);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    std::vector<mwx::TokOut> ho(R);
    std::vector<uint8_t> hparts(gparts.bytes), hres(gres.bytes);
    bool ok = gf.take(flt);
    ok = gp.take(probs) && ok;
    ok = gl.take(logprobs) && ok;
    ok = go.take(ho.data()) && ok;
    ok = gparts.take(hparts.data()) && ok;
    ok = gres.take(hres.data()) && ok;
    if (!ok) return -3;
    for (int r = 0; r < R; ++r) {
      out[r].id = ho[r].id;
      out[r].tid = ho[r].tid;
      out[r].p = ho[r].p;
      out[r].plog = ho[r].plog;
      out[r].pt = ho[r].pt;
      out[r].ptsum = ho[r].ptsum;
      out[r].nosp = ho[r].nosp;
    }
    return 0;
  } catch (...) {
    return -2;
  }
}

extern "C" int mwx_test_logits_process(struct mwx_context* ctx, int R, int V, const float* logits,
                                       const float* smask,
                                       const struct mwx_test_logits_ctl* ctl,
                                       const struct mwx_test_logits_const* lc, float* flt,
                                       float* probs, float* logprobs,
                                       struct mwx_test_logits_out* out) {
  return test_logits_process_impl(ctx, R, V, logits, smask, ctl, lc, flt, probs, logprobs, out,
                                  nullptr, 0.0f);
}
extern "C" int mwx_test_logits_process_masked(struct mwx_context* ctx, int R, int V,
                                              const float* logits, const float* smask,
                                              const struct mwx_test_logits_ctl* ctl,
                                              const struct mwx_test_logits_const* lc,
                                              const uint64_t* cmask, float penalty, float* flt,
                                              float* probs, float* logprobs,
                                              struct mwx_test_logits_out* out) {
  if (!cmask || !std::isfinite(penalty) || !(penalty > 0.0f)) return -1;
  return test_logits_process_impl(ctx, R, V, logits, smask, ctl, lc, flt, probs, logprobs, out,
                                  cmask, penalty);
}

extern "C" int mwx_test_logits_setup(struct mwx_context* ctx, const struct mwx_full_params* params,
                                     struct mwx_test_logits_const* lc, float* smask) {
  if (!ctx || !params || !lc || !smask) return -1;
  const mwx::LogitsConst C = mwx::logits_const(ctx->c, *params);
  lc->n_vocab = C.n_vocab;
  lc->eot = C.eot;
  lc->beg = C.beg;
  lc->space_id = C.space_id;
  lc->suppress_blank = C.suppress_blank;
  lc->max_initial_tid = C.max_initial_tid;
  lc->nosp_id = C.nosp_id;
  const std::vector<float> m = mwx::static_mask(ctx->c, *params);
  memcpy(smask, m.data(), m.size() * sizeof(float));
  return 0;
}

// ---------------------------------------------------------------------------
// DTW token timestamps: the three kernels on given data, and a state's passes
// ---------------------------------------------------------------------------
extern "C" int mwx_test_align_probs(struct mwx_context* ctx, int mx, int R, int H, int KS,
                                    int n_keys, int slots, int n_heads, const int* heads, int A,
                                    int pos0, int n_rows_cap, const float* P, const float* bias,
                                    float qscale, float scale, const void* k,
                                    const uint8_t* kscale, const int* kv_index, const int* pos,
                                    const int* active, float* out) {
  if (!ctx || !heads || !P || !bias || !k || !kv_index || !pos || !active || !out) return -1;
  if (mx && !kscale) return -1;
  if (R < 1 || R > 1024 || H < 1 || H > 32 || KS < 1 || KS > 8 || n_keys < 1 ||
      n_keys > mwx::DTW_MAX_KEYS || slots < 1 || slots > 64 || n_heads < 1 || n_heads > 64 ||
      A < 1 || A > 64 || n_rows_cap < 1 || n_rows_cap > mwx::DTW_MAX_ROWS)
    return -1;
  for (int i = 0; i < n_heads; ++i)
    if (heads[2 * i] < 0 || heads[2 * i] >= H || heads[2 * i + 1] < 0 || heads[2 * i + 1] >= A)
      return -1;
  for (int r = 0; r < R; ++r)
    if (kv_index[r] < 0 || kv_index[r] >= slots) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    const int D = H * 64;
    const size_t pb = (size_t)KS * R * D * 4, kb = (size_t)slots * H * n_keys * 64 * (mx ? 1 : 2),
                 sb = (size_t)slots * H * n_keys * 2, ob = (size_t)slots * A * n_rows_cap * n_keys * 4;
    DevScratch m;
    void* dP = m.get(pb);
    void* dbias = m.get((size_t)D * 4);
    void* dk = m.get(kb);
    void* dks = mx ? m.get(sb) : nullptr;
    void* dkvi = m.get((size_t)R * 4);
    void* dpos = m.get((size_t)R * 4);
    void* dact = m.get((size_t)R * 4);
    void* dh = m.get((size_t)n_heads * 8);
    void* dout = m.get(ob);
    HIPC(hipMemcpy(dP, P, pb, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dbias, bias, (size_t)D * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dk, k, kb, hipMemcpyHostToDevice));
    if (dks) HIPC(hipMemcpy(dks, kscale, sb, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dkvi, kv_index, (size_t)R * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dpos, pos, (size_t)R * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dact, active, (size_t)R * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dh, heads, (size_t)n_heads * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dout, out, ob, hipMemcpyHostToDevice));
    const bool ok = mwx::align_probs((const float*)dP, KS, D, (const float*)dbias, qscale, scale, dk,
                                     (const uint8_t*)dks, (const int*)dkvi, (const int*)dpos,
                                     (const int*)dact, (const int2*)dh, n_heads, n_keys, n_keys, R,
                                     H, pos0, A, n_rows_cap, (float*)dout, nullptr);
    if (!ok) return -4;
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
    return 0;
  } catch (...) {
    return -2;
  }
}

static bool dtw_test_shapes(int B, const int* Ns, const int* Ts, int n_cap, int t_cap, int* n_max,
                            int* t_max) {
  if (B < 1 || B > 64 || !Ns || !Ts) return false;
  *n_max = *t_max = 0;
  for (int b = 0; b < B; ++b) {
    if (Ns[b] < 1 || Ns[b] > n_cap || Ts[b] < 1 || Ts[b] > t_cap) return false;
    *n_max = std::max(*n_max, Ns[b]);
    *t_max = std::max(*t_max, Ts[b]);
  }
  return true;
}

extern "C" int mwx_test_dtw_cost(struct mwx_context* ctx, int B, int A, int n_rows_cap, int n_keys,
                                 const int* Ns, const int* Ts, const float* w, float* cost) {
  int n_max = 0, t_max = 0;
  if (!ctx || !w || !cost || A < 1 || A > 1024 || n_rows_cap < 1 ||
      n_rows_cap > mwx::DTW_MAX_ROWS || n_keys < 1 || n_keys > mwx::DTW_MAX_KEYS ||
      !dtw_test_shapes(B, Ns, Ts, n_rows_cap, n_keys, &n_max, &t_max))
    return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    const size_t wb = (size_t)B * A * n_rows_cap * n_keys * 4;
    const long cstride = (long)n_rows_cap * t_max;
    DevScratch m;
    void* dw = m.get(wb);
    int* dmeta = (int*)m.get((size_t)3 * B * 4);
    void* dc = m.get((size_t)B * cstride * 4);
    std::vector<int> hm(3 * B);
    for (int b = 0; b < B; ++b) {
      hm[b] = b;
      hm[B + b] = Ns[b];
      hm[2 * B + b] = Ts[b];
    }
    HIPC(hipMemcpy(dw, w, wb, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dmeta, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
    HIPC(hipMemset(dc, 0xff, (size_t)B * cstride * 4));
    if (!mwx::dtw_cost((const float*)dw, dmeta, dmeta + B, dmeta + 2 * B, B, A, n_rows_cap, n_keys,
                       t_max, cstride, (float*)dc, nullptr))
      return -4;
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(cost, dc, (size_t)B * cstride * 4, hipMemcpyDeviceToHost));
    return 0;
  } catch (...) {
    return -2;
  }
}

extern "C" int mwx_test_dtw_path(struct mwx_context* ctx, int B, const int* Ns, const int* Ts,
                                 const float* cost, int* frames, int* path, int* path_len) {
  int n_max = 0, t_max = 0;
  if (!ctx || !cost || !frames || !path || !path_len ||
      !dtw_test_shapes(B, Ns, Ts, mwx::DTW_MAX_ROWS, mwx::DTW_MAX_KEYS, &n_max, &t_max))
    return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    const long cstride = (long)n_max * t_max;
    const int pcap = n_max + t_max;
    DevScratch m;
    void* dc = m.get((size_t)B * cstride * 4);
    int* dmeta = (int*)m.get((size_t)2 * B * 4);
    void* df = m.get((size_t)B * n_max * 4);
    void* dp = m.get((size_t)B * pcap * 8);
    void* dl = m.get((size_t)B * 4);
    std::vector<int> hm(2 * B);
    for (int b = 0; b < B; ++b) {
      hm[b] = Ns[b];
      hm[B + b] = Ts[b];
    }
    HIPC(hipMemcpy(dc, cost, (size_t)B * cstride * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dmeta, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
    HIPC(hipMemset(df, 0xff, (size_t)B * n_max * 4));
    HIPC(hipMemset(dp, 0xff, (size_t)B * pcap * 8));
    HIPC(hipMemset(dl, 0, (size_t)B * 4));
    if (!mwx::dtw_path((const float*)dc, dmeta, dmeta + B, B, n_max, t_max, cstride, n_max,
                       (int*)df, pcap, (int*)dp, (int*)dl, nullptr))
      return -4;
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(frames, df, (size_t)B * n_max * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(path, dp, (size_t)B * pcap * 8, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(path_len, dl, (size_t)B * 4, hipMemcpyDeviceToHost));
    return 0;
  } catch (...) {
    return -2;
  }
}

extern "C" int mwx_test_dtw_keep(struct mwx_state* state, int on) {
  if (!state) return -1;
  const int prev = state->s.dtw_keep ? 1 : 0;
  state->s.dtw_keep = on != 0;
  if (!on) state->s.dtw_dump.clear();
  return prev;
}

extern "C" int mwx_test_dtw_n_passes(struct mwx_state* state) {
  return state ? (int)state->s.dtw_dump.size() : -1;
}

extern "C" int mwx_test_dtw_last(struct mwx_state* state, int pass, int* dims, int64_t* seek,
                                 float* probs, long probs_cap, float* cost, long cost_cap,
                                 int* frames, long frames_cap) {
  if (!state || pass < 0 || pass >= (int)state->s.dtw_dump.size() || !dims) return -1;
  const mwx::State::DtwDump& d = state->s.dtw_dump[pass];
  dims[0] = d.N;
  dims[1] = d.T;
  dims[2] = d.A;
  dims[3] = d.n_keys;
  if (seek) *seek = d.seek;
  if (probs) {
    if (probs_cap < (long)d.probs.size()) return -1;
    memcpy(probs, d.probs.data(), d.probs.size() * 4);
  }
  if (cost) {
    if (cost_cap < (long)d.cost.size()) return -1;
    memcpy(cost, d.cost.data(), d.cost.size() * 4);
  }
  if (frames) {
    if (frames_cap < (long)d.frames.size()) return -1;
    memcpy(frames, d.frames.data(), d.frames.size() * 4);
  }
  return 0;
}

namespace mwx {
template <typename T>
static int test_dtw_align_impl(Context& C, State& S, const int* tokens, int n, int pos0,
                               int n_cols) {
  mwx_full_params P = mwx_full_default_params(MWX_SAMPLING_GREEDY);
  Driver<T> D(C, S, P);
  D.live_slots = {0};
  typename Driver<T>::DtwClip x;
  x.slot = 0;
  x.tokens.assign(tokens, tokens + n);
  x.pos0 = pos0;
  x.n_rows = n - pos0;
  x.n_cols = n_cols;
  std::vector<typename Driver<T>::DtwClip> dc{x};
  std::vector<State*> st{&S};
  int64_t seek = 0;
  const bool keep = S.dtw_keep;
  S.dtw_keep = true;
  S.dtw_dump.clear();
  try {
    D.dtw_pass(dc, st, &seek);
  } catch (...) {
    S.dtw_keep = keep;
    throw;
  }
  S.dtw_keep = keep;
  return 0;
}
}  // namespace mwx

extern "C" int mwx_test_dtw_align(struct mwx_context* ctx, struct mwx_state* state,
                                  const int* tokens, int n, int pos0, int n_cols) {
  if (!ctx || !state || !tokens || !ctx->c.dtw || state->s.cross_cap < 1) return -1;
  if (pos0 < 0 || n - pos0 < 2 || n - pos0 > mwx::DTW_MAX_ROWS || n > ctx->c.hp.n_text_ctx ||
      n_cols < 1 || n_cols > ctx->c.hp.n_audio_ctx)
    return -1;
  if (!mwx::tokens_valid(tokens, n, ctx->c.hp.n_vocab)) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    if (ctx->c.wtype == mwx::GGML_BF16)
      return mwx::test_dtw_align_impl<__bf16>(ctx->c, state->s, tokens, n, pos0, n_cols);
    return mwx::test_dtw_align_impl<_Float16>(ctx->c, state->s, tokens, n, pos0, n_cols);
  } catch (...) {
    return -2;
  }
}

// ---------------------------------------------------------------------------
// Transcript scoring on given data (k_score.hip), and the alignment pass's
// logits block size
// ---------------------------------------------------------------------------
extern "C" int mwx_test_score_rows(struct mwx_context* ctx, int R, int V, const float* logits,
                                   const int* target, const int* active, float* plog, float* p,
                                   int* top_id, float* top_plog) {
  if (!ctx || !logits || !target || !active || !plog || !p || !top_id || !top_plog) return -1;
  if (R < 1 || R > 4096 || V < 1 || V > mwx::SCORE_MAX_VOCAB) return -1;
  for (int r = 0; r < R; ++r)
    if (target[r] < 0 || target[r] >= V) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    const size_t rv = (size_t)R * V * 4;
    DevScratch m;
    float* dl = (float*)m.get(rv);
    int* dt = (int*)m.get((size_t)R * 4);
    int* da = (int*)m.get((size_t)R * 4);
    HIPC(hipMemcpy(dl, logits, rv, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dt, target, (size_t)R * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(da, active, (size_t)R * 4, hipMemcpyHostToDevice));
    GuardedBuf go;
    mwx::ScoreOut* dout = (mwx::ScoreOut*)go.make(m, (size_t)R * sizeof(mwx::ScoreOut), nullptr);
    if (!mwx::score_rows(dl, dt, da, R, V, dout, nullptr)) return -1;
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    std::vector<mwx::ScoreOut> ho(R);
    if (!go.take(ho.data())) return -3;
    for (int r = 0; r < R; ++r) {
      plog[r] = ho[r].plog;
      p[r] = ho[r].p;
      top_id[r] = ho[r].top_id;
      top_plog[r] = ho[r].top_plog;
    }
    return 0;
  } catch (...) {
    return -2;
  }
}

extern "C" int mwx_test_set_score_rows_cap(int rows) {
  return mwx::score_rows_cap_var().exchange(rows > 0 ? rows : mwx::kScoreRowsCap);
}

// ---------------------------------------------------------------------------
// Language identification on given data (k_lang.hip), and the detection
// pass's kept logit row
// ---------------------------------------------------------------------------
extern "C" int mwx_test_lang_probs(struct mwx_context* ctx, int R, int V, const float* logits,
                                   int t0, int n, float* probs, int* best) {
  if (!ctx || !logits || !probs || !best) return -1;
  if (R <= 0 || n < 1 || n > mwx::LANG_MAX_N || t0 < 0 || (long)t0 + n > V) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    const size_t rv = (size_t)R * V * 4;
    DevScratch m;
    float* dl = (float*)m.get(rv);
    HIPC(hipMemcpy(dl, logits, rv, hipMemcpyHostToDevice));
    GuardedBuf gp, gb;
    float* dp = (float*)gp.make(m, (size_t)R * n * 4, nullptr);
    int* db = (int*)gb.make(m, (size_t)R * 4, nullptr);
    if (!mwx::lang_probs(dl, R, V, t0, n, dp, db, nullptr)) return -1;
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    std::vector<float> hp((size_t)R * n);
    std::vector<int> hb((size_t)R);
    if (!gp.take(hp.data()) || !gb.take(hb.data())) return -3;
    memcpy(probs, hp.data(), hp.size() * 4);
    memcpy(best, hb.data(), hb.size() * 4);
    return 0;
  } catch (...) {
    return -2;
  }
}

extern "C" int mwx_test_lang_keep(struct mwx_state* state, int on) {
  if (!state) return -1;
  const int prev = state->s.lang_keep ? 1 : 0;
  state->s.lang_keep = on != 0;
  if (!on) state->s.lang_last.clear();
  return prev;
}

extern "C" int mwx_test_lang_last(struct mwx_state* state, float* logits_out, int n) {
  if (!state || !logits_out || n < mwx::lang_max_id() + 1) return -1;
  const std::vector<float>& ll = state->s.lang_last;
  if (!ll.empty()) memcpy(logits_out, ll.data(), ll.size() * 4);
  return (int)ll.size();
}

// ---------------------------------------------------------------------------
// Contextual biasing on given data (k_bias.hip; mwx_test_bias_match is in
// bias.cpp: it needs no device)
// ---------------------------------------------------------------------------
extern "C" int mwx_test_logits_bias(struct mwx_context* ctx, const struct mwx_bias_phrase* phrases,
                                    int n, int R, int V, const float* logits,
                                    const mwx_token* hist, int H, const int* hist_len,
                                    const int* active, const int* sample, float* logits_out,
                                    int* state_out) {
  if (!ctx || !logits || !hist_len || !active || !sample || !logits_out || !state_out) return -1;
  if (R < 1 || R > 256 || V < 1 || H < 0 || (H > 0 && !hist) || n < 1) return -1;
  for (int r = 0; r < R; ++r)
    if (hist_len[r] < 0 || hist_len[r] > H) return -1;
  if (mwx::bias_validate(phrases, n, V) != 0) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    const std::vector<int32_t> tab = mwx::bias_build(phrases, n);
    std::vector<mwx::RowCtl> hc(R);
    for (int r = 0; r < R; ++r) {
      memset(&hc[r], 0, sizeof(mwx::RowCtl));
      hc[r].active = active[r];
      hc[r].sample = sample[r];
    }
    DevScratch m;
    int* dt = (int*)m.get(tab.size() * 4);
    int* dh = (int*)m.get(std::max<size_t>(1, (size_t)R * H) * 4);
    int* dn = (int*)m.get((size_t)R * 4);
    mwx::RowCtl* dc = (mwx::RowCtl*)m.get((size_t)R * sizeof(mwx::RowCtl));
    HIPC(hipMemcpy(dt, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    if (H > 0) HIPC(hipMemcpy(dh, hist, (size_t)R * H * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dn, hist_len, (size_t)R * 4, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dc, hc.data(), (size_t)R * sizeof(mwx::RowCtl), hipMemcpyHostToDevice));
    GuardedBuf gl, gs;
    float* dl = (float*)gl.make(m, (size_t)R * V * 4, logits);
    int* ds = (int*)gs.make(m, (size_t)R * 4, nullptr);
    mwx::bias_walk_rows(dt, dh, dn, H, R, dc, ds, nullptr);
    if (!mwx::logits_bias(dl, dc, dt, R, V, nullptr)) return -1;
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    std::vector<float> hl((size_t)R * V);
    std::vector<int> hs((size_t)R);
    if (!gl.take(hl.data()) || !gs.take(hs.data())) return -3;
    memcpy(logits_out, hl.data(), hl.size() * 4);
    memcpy(state_out, hs.data(), hs.size() * 4);
    return 0;
  } catch (...) {
    return -2;
  }
}

// ---------------------------------------------------------------------------
// Constrained decoding on given data (k_constrain.hip; mwx_test_constraint_walk
// is in constraint.cpp: it needs no device)
// ---------------------------------------------------------------------------
extern "C" int mwx_test_constraint_mask(struct mwx_context* ctx, const struct mwx_constraint* c,
                                        int R, int V, int eot, const uint32_t* tok_off,
                                        const uint8_t* tok_bytes, const int* state,
                                        const int* active, const int* sample, uint64_t* mask_out) {
  if (!ctx || !c || !state || !active || !sample || !mask_out) return -1;
  if (R < 1 || R > 256 || V < 1 || V > mwx::LP_G * mwx::LP_CHUNK) return -1;
  if (tok_off) {
    if (eot < 0 || eot > V || (!tok_bytes && tok_off[eot] > 0) || tok_off[0] != 0) return -1;
    for (int t = 0; t < eot; ++t)
      if (tok_off[t + 1] < tok_off[t]) return -1;
  } else {
    if (V != ctx->c.hp.n_vocab) return -1;
    eot = ctx->c.vocab.token_eot;
  }
  for (int r = 0; r < R; ++r)
    if (state[r] < 0 || state[r] >= c->S) return -1;
  try {
    HIPC(hipSetDevice(ctx->c.device));
    const mwx::ConTokens tk = tok_off ? mwx::constraint_tokens_raw(tok_off, tok_bytes, eot)
                                      : mwx::constraint_tokens(ctx->c.vocab.id_to_token, eot);
    const mwx::ConBlock blk = mwx::constraint_block(*c);
    std::vector<mwx::RowCtl> hc(R);
    for (int r = 0; r < R; ++r) {
      memset(&hc[r], 0, sizeof(mwx::RowCtl));
      hc[r].active = active[r];
      hc[r].sample = sample[r];
      hc[r].pad[1] = state[r];
    }
    DevScratch m;
    uint8_t* db = (uint8_t*)m.get(blk.data.size());
    uint8_t* dt = (uint8_t*)m.get(tk.data.size());
    mwx::RowCtl* dc = (mwx::RowCtl*)m.get((size_t)R * sizeof(mwx::RowCtl));
    HIPC(hipMemcpy(db, blk.data.data(), blk.data.size(), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dt, tk.data.data(), tk.data.size(), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dc, hc.data(), (size_t)R * sizeof(mwx::RowCtl), hipMemcpyHostToDevice));
    const size_t mb = (size_t)R * ((V + 63) / 64) * 8;
    GuardedBuf gm;
    unsigned long long* dm = (unsigned long long*)gm.make(m, mb, nullptr);
    const mwx::ConView v = mwx::constraint_view_dev(*c, blk, db, tk, dt);
    if (!mwx::logits_constrain(dm, dc, v, R, V, nullptr)) return -1;
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    std::vector<uint8_t> hm(mb);
    if (!gm.take(hm.data())) return -3;
    memcpy(mask_out, hm.data(), mb);
    return 0;
  } catch (...) {
    return -2;
  }
}
