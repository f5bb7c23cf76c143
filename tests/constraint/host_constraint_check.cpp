// TEST INFRASTRUCTURE ONLY — the host SttEngine's constrained decoding
// (RequestOptions::choices / choice_flags / choice_penalty,
// Settings::choice_penalty) over the CPU stand-in constraint_stub.cpp and the
// real csrc/constraint.cpp (tests/constraint/Makefile; AddressSanitizer +
// UBSan), run by tests/test_constraint_host.py: the key rule (no choices: the
// old key), the penalty's default and resolution order, dropped choices, the
// per-key constraint cache, choice_match, the batch entry point and a
// streaming session; and constraint.cpp's own refusals and limit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "stt_engine.h"
#include "stt_stream.h"

using namespace mwx_host;

extern int g_con_calls, g_con_clips, g_con_states, g_con_yes;
extern const mwx_constraint* g_con_ptr;
extern float g_con_penalty;
extern bool g_con_no_ts;

namespace {

int failures = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

Settings base(const std::string& dir) {
  Settings s;
  s.model_dir = dir;
  s.model_filename = "ggml-micro.bin";
  s.parallel_requests = 1;
  s.request_queue_timeout_ms = 1000;
  s.language = "en";
  s.enable_vad = false;
  return s;
}

int walk(const mwx_constraint* c, const char* text) {
  return mwx_constraint_walk(c, mwx_constraint_start(c), (const uint8_t*)text,
                             (int)std::strlen(text));
}

void constraint_source_checks() {
  // choices, every flag
  const char* texts[] = {"yes", "no"};
  mwx_constraint* c = mwx_constraint_from_choices(
      texts, 2, MWX_CONSTRAINT_FOLD_CASE | MWX_CONSTRAINT_LEADING_SPACE |
                    MWX_CONSTRAINT_TRAILING_PUNCT);
  CHECK(c != nullptr);
  if (c) {
    CHECK(mwx_constraint_accepting(c, walk(c, "yes")) == 1);
    CHECK(mwx_constraint_accepting(c, walk(c, " YeS!")) == 1);
    CHECK(walk(c, "ye") != 0 && mwx_constraint_accepting(c, walk(c, "ye")) == 0);
    CHECK(walk(c, "yes!!") == 0 && walk(c, "  no") == 0 && walk(c, "maybe") == 0);
    CHECK(mwx_constraint_accepting(c, 0) == 0 && mwx_constraint_accepting(c, -1) == 0 &&
          mwx_constraint_accepting(c, mwx_constraint_n_states(c)) == 0);
    CHECK(mwx_constraint_walk(c, 0, (const uint8_t*)"y", 1) == 0);
    CHECK(mwx_constraint_walk(c, 1 << 20, (const uint8_t*)"y", 1) == 0);
    mwx_constraint_free(c);
  }
  mwx_constraint_free(nullptr);
  // refusals
  CHECK(mwx_constraint_from_choices(texts, 0, 0) == nullptr);
  CHECK(mwx_constraint_from_choices(nullptr, 2, 0) == nullptr);
  CHECK(mwx_constraint_from_choices(texts, 2, 8) == nullptr);
  const char* with_empty[] = {"yes", ""};
  CHECK(mwx_constraint_from_choices(with_empty, 2, 0) == nullptr);
  // the state limit: 4095 live states fit, one more does not
  const std::string fits(4094, 'a'), over(4095, 'a');
  const char* t1[] = {fits.c_str()};
  const char* t2[] = {over.c_str()};
  mwx_constraint* big = mwx_constraint_from_choices(t1, 1, 0);
  CHECK(big && mwx_constraint_n_states(big) == MWX_CONSTRAINT_MAX_STATES);
  if (big) CHECK(mwx_constraint_accepting(big, walk(big, fits.c_str())) == 1);
  mwx_constraint_free(big);
  CHECK(mwx_constraint_from_choices(t2, 1, 0) == nullptr);
  // a DFA: 1 -a-> 2 (accepting) -b-> 1; and its refusals
  std::vector<uint16_t> tr(3 * 256, 0);
  tr[1 * 256 + 'a'] = 2;
  tr[2 * 256 + 'b'] = 1;
  const uint8_t acc[3] = {0, 0, 1};
  mwx_constraint* d = mwx_constraint_from_dfa(3, 1, tr.data(), acc);
  CHECK(d && walk(d, "aba") == 2 && walk(d, "ab") == 1 && walk(d, "b") == 0);
  mwx_constraint_free(d);
  CHECK(mwx_constraint_from_dfa(1, 1, tr.data(), acc) == nullptr);
  CHECK(mwx_constraint_from_dfa(MWX_CONSTRAINT_MAX_STATES + 1, 1, tr.data(), acc) == nullptr);
  CHECK(mwx_constraint_from_dfa(3, 0, tr.data(), acc) == nullptr);
  CHECK(mwx_constraint_from_dfa(3, 3, tr.data(), acc) == nullptr);
  CHECK(mwx_constraint_from_dfa(3, 1, nullptr, acc) == nullptr);
  std::vector<uint16_t> bad = tr;
  bad[2 * 256 + 'c'] = 3;
  CHECK(mwx_constraint_from_dfa(3, 1, bad.data(), acc) == nullptr);
  bad = tr;
  bad[0 * 256 + 'c'] = 1;
  CHECK(mwx_constraint_from_dfa(3, 1, bad.data(), acc) == nullptr);
  const uint8_t acc0[3] = {1, 0, 1};
  CHECK(mwx_constraint_from_dfa(3, 1, tr.data(), acc0) == nullptr);
  const uint8_t none[3] = {0, 0, 0};
  CHECK(mwx_constraint_from_dfa(3, 1, tr.data(), none) == nullptr);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ofstream(dir + "/ggml-micro.bin") << "stub";
  std::vector<float> pcm(16000 * 4);
  for (size_t i = 0; i < pcm.size(); ++i) pcm[i] = 0.01f * (float)((i / 160) % 23);

  constraint_source_checks();

  // the environment: unset leaves 100; a number > 0 sets it; junk is ignored
  {
    unsetenv("STT_WHISPER_SERVICE_CHOICE_PENALTY");
    Settings s;
    CHECK(s.choice_penalty == 100.0f);
    settings_choices_from_env(s);
    CHECK(s.choice_penalty == 100.0f);
    setenv("STT_WHISPER_SERVICE_CHOICE_PENALTY", "42.5", 1);
    settings_choices_from_env(s);
    CHECK(s.choice_penalty == 42.5f);
    for (const char* junk : {"abc", "-1", "0", "nan", "inf", ""}) {
      setenv("STT_WHISPER_SERVICE_CHOICE_PENALTY", junk, 1);
      settings_choices_from_env(s);
      CHECK(s.choice_penalty == 42.5f);
    }
    unsetenv("STT_WHISPER_SERVICE_CHOICE_PENALTY");
  }

  for (int max_batch : {1, 4}) {
    Settings s = base(dir);
    s.max_batch = max_batch;
    SttEngine e(s);
    RequestOptions none;
    CHECK(none.choice_flags == 7 && none.choice_penalty < 0.0f && none.choices.empty());
    // no choices: nothing passed, the key as it always was, choice_match -1
    const int calls = g_con_calls;
    auto r0 = e.transcribe(pcm, 16000, none);
    CHECK(!r0.empty() && r0[0].choice_match == -1);
    CHECK(g_con_calls == calls + 1 && g_con_ptr == nullptr && !g_con_no_ts);
    CHECK(e.options_key(none) == "5|0|5|0|0|en|");
    RequestOptions pen_only = none;
    pen_only.choice_penalty = 9.0f;  // a penalty or flags without choices change nothing
    pen_only.choice_flags = 0;
    CHECK(e.options_key(pen_only) == e.options_key(none));
    CHECK(!e.transcribe(pcm, 16000, pen_only).empty() && g_con_ptr == nullptr);

    // choices: a constraint with the default penalty, every default flag
    RequestOptions ch;
    ch.choices = {"yes", "no", "repeat"};
    auto r1 = e.transcribe(pcm, 16000, ch);
    CHECK(!r1.empty() && r1[0].choice_match == 1);
    CHECK(g_con_ptr != nullptr && g_con_penalty == 100.0f && g_con_yes == 1);
    CHECK(g_con_no_ts);  // (a request with choices decodes without timestamps)
    const mwx_constraint* first = g_con_ptr;
    const int states_all = g_con_states;
    // the same choices again: the cached constraint
    CHECK(!e.transcribe(pcm, 16000, ch).empty() && g_con_ptr == first);
    // the request's penalty wins over the setting's; the same constraint serves
    RequestOptions ch2 = ch;
    ch2.choice_penalty = 7.5f;
    CHECK(!e.transcribe(pcm, 16000, ch2).empty());
    CHECK(g_con_ptr == first && g_con_penalty == 7.5f);
    // other flags: another constraint (fewer states without the optional parts)
    RequestOptions ch3 = ch;
    ch3.choice_flags = 0;
    CHECK(!e.transcribe(pcm, 16000, ch3).empty());
    CHECK(g_con_ptr != nullptr && g_con_states < states_all && g_con_yes == 1);
    // keys
    CHECK(e.options_key(ch) != e.options_key(none));
    CHECK(e.options_key(ch).compare(0, e.options_key(none).size(), e.options_key(none)) == 0);
    CHECK(e.options_key(ch) != e.options_key(ch2));
    CHECK(e.options_key(ch) != e.options_key(ch3));
    RequestOptions same = ch;
    same.choice_penalty = 100.0f;  // resolves to what the setting gives
    CHECK(e.options_key(same) == e.options_key(ch));
    RequestOptions ch4 = ch;
    ch4.choices = {"yes", "no|6:repeat"};  // (lengths in the key: no way to forge a separator)
    CHECK(e.options_key(ch4) != e.options_key(ch));
    RequestOptions both = ch;
    both.hotwords = {"word"};
    CHECK(e.options_key(both) != e.options_key(ch));
    // dropped: empty choices, and one with a NUL; the rest still constrain
    RequestOptions drop;
    drop.choices = {"", std::string("a\0b", 3), "no"};
    CHECK(!e.transcribe(pcm, 16000, drop).empty());
    CHECK(g_con_ptr != nullptr && g_con_yes == 0);
    RequestOptions all_dropped;
    all_dropped.choices = {"", ""};
    auto r2 = e.transcribe(pcm, 16000, all_dropped);
    CHECK(!r2.empty() && g_con_ptr == nullptr && r2[0].choice_match == -1);
    // a set the engine refuses (too many states): unconstrained
    RequestOptions huge;
    huge.choices = {std::string(5000, 'x')};
    CHECK(!e.transcribe(pcm, 16000, huge).empty() && g_con_ptr == nullptr);
    // the pcm16 entry point and the batch entry point
    std::vector<int16_t> p16(pcm.size(), 300);
    CHECK(!e.transcribe_pcm16(p16, 16000, ch2).empty());
    CHECK(g_con_ptr == first && g_con_penalty == 7.5f);
    if (max_batch == 1) {
      const auto rb = e.transcribe_batch({pcm, pcm}, ch);
      CHECK(rb.size() == 2 && g_con_clips == 2 && g_con_ptr == first);
    }
    // a streaming session passes its choices through
    {
      StreamSession ss(e);
      ss.set_choices({"yes", "no", "repeat"}, -1, 3.0f);
      std::vector<uint8_t> chunk(2 * 16000, 0);
      for (size_t i = 0; i < chunk.size(); i += 2) chunk[i + 1] = (uint8_t)((i / 320) % 9);
      const int c0 = g_con_calls;
      (void)ss.feed(chunk.data(), chunk.size());
      (void)ss.feed(nullptr, 0);
      CHECK(g_con_calls > c0 && g_con_ptr == first && g_con_penalty == 3.0f);
    }
  }
  // the setting's penalty
  {
    Settings s = base(dir);
    s.choice_penalty = 55.0f;
    SttEngine e(s);
    RequestOptions ch;
    ch.choices = {"yes"};
    CHECK(!e.transcribe(pcm, 16000, ch).empty());
    CHECK(g_con_ptr != nullptr && g_con_penalty == 55.0f);
  }
  std::printf("host_constraint_check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
