// Voice-activity detection: the model file (reader and seeded writer), the
// VAD context and the mwx_vad_* entry points of include/mwx.h, speech segments
// and silence trimming (mwx_vad_segments_*, mwx_vad_trim_batch) and the chunk
// plan of a long clip (mwx_vad_trim_batch_chunked) included, and
// the streams that are fed a piece at a time (mwx_vad_stream_*, D11). The
// kernels are in k_vad.hip; the network, the file layout and the segment rule
// are written down in INTEGRATION.md ("VAD model", "VAD speech segments").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "mwx_test.h"
#include "vad_trim.h"

#define HIPC(x)                                                                        \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      MWX_LOG_ERROR("mwx: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                         \
      throw std::runtime_error("hip");                                                 \
    }                                                                                  \
  } while (0)

namespace mwx {
namespace {

constexpr uint32_t kGgmlMagic = 0x67676d6c;  // "ggml"
const char* const kVadType = "silero-16k";
const int32_t kVadVersion[3] = {5, 0, 0};
constexpr int kLayers = 4;
const int32_t kEncIn[kLayers] = {129, 128, 64, 64};
const int32_t kEncOut[kLayers] = {128, 64, 64, 128};
const int32_t kEncKernel[kLayers] = {3, 3, 3, 3};

struct VadTensorSpec {
  std::string name;
  std::vector<int64_t> shape;  // outermost first
  int type;                    // the synthetic writer's type
  float gain;                  // uniform in +-gain / sqrt(fan_in); 0 = the STFT basis
  int fan_in;
};

// Every tensor of the file, in file order.
std::vector<VadTensorSpec> vad_tensor_specs() {
  std::vector<VadTensorSpec> v;
  v.push_back({"_model.stft.forward_basis_buffer", {2 * VAD_BINS, VAD_NFFT}, GGML_F16, 0.0f, 1});
  for (int l = 0; l < kLayers; ++l) {
    const std::string p = "_model.encoder." + std::to_string(l) + ".reparam_conv.";
    const int fan = kEncIn[l] * kEncKernel[l];
    v.push_back({p + "weight", {kEncOut[l], kEncIn[l], kEncKernel[l]}, GGML_F16, 2.0f, fan});
    v.push_back({p + "bias", {kEncOut[l]}, GGML_F32, 2.0f, fan});
  }
  const std::string r = "_model.decoder.rnn.";
  v.push_back({r + "weight_ih", {VAD_GATES, VAD_HID}, GGML_F32, 3.0f, VAD_HID});
  v.push_back({r + "weight_hh", {VAD_GATES, VAD_HID}, GGML_F32, 3.0f, VAD_HID});
  v.push_back({r + "bias_ih", {VAD_GATES}, GGML_F32, 3.0f, VAD_HID});
  v.push_back({r + "bias_hh", {VAD_GATES}, GGML_F32, 3.0f, VAD_HID});
  v.push_back({"_model.decoder.decoder.2.weight", {1, VAD_HID, 1}, GGML_F32, 16.0f, VAD_HID});
  v.push_back({"_model.decoder.decoder.2.bias", {1}, GGML_F32, 16.0f, VAD_HID});
  return v;
}

// ---- reader -----------------------------------------------------------------
struct Cursor {
  const std::vector<uint8_t>& b;
  size_t pos = 0;
  bool take(void* dst, size_t n) {
    if (n > b.size() - pos) return false;
    memcpy(dst, b.data() + pos, n);
    pos += n;
    return true;
  }
  bool i32(int32_t& v) { return take(&v, 4); }
};

// Reads the file into f32 tensors keyed by name. false (logged) on any error.
bool read_vad_file(const char* path, std::map<std::string, std::vector<float>>& out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    MWX_LOG_ERROR("mwx_vad: cannot open '%s'\n", path);
    return false;
  }
  const std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)),
                                   std::istreambuf_iterator<char>());
  Cursor c{bytes};
  auto truncated = [&](const char* what) {
    MWX_LOG_ERROR("mwx_vad: '%s' is truncated (%s)\n", path, what);
    return false;
  };
  uint32_t magic = 0;
  if (!c.take(&magic, 4)) return truncated("magic");
  if (magic != kGgmlMagic) {
    MWX_LOG_ERROR("mwx_vad: '%s' has a bad magic %08x\n", path, magic);
    return false;
  }
  int32_t len = 0;
  if (!c.i32(len)) return truncated("model type");
  if (len < 0 || (size_t)len > bytes.size() - c.pos) return truncated("model type");
  std::string type(len, '\0');
  c.take(&type[0], len);
  if (type != kVadType) {
    MWX_LOG_ERROR("mwx_vad: model type '%s' is not '%s'\n", type.c_str(), kVadType);
    return false;
  }
  int32_t version[3];
  if (!c.take(version, sizeof version)) return truncated("version");
  // hyper-parameters: only the shape of INTEGRATION.md is supported
  int32_t hp[1 + 3 * kLayers + 4];
  if (!c.take(hp, sizeof hp)) return truncated("hyper-parameters");
  bool ok = hp[0] == kLayers;
  for (int l = 0; ok && l < kLayers; ++l)
    ok = hp[1 + l] == kEncIn[l] && hp[1 + kLayers + l] == kEncOut[l] &&
         hp[1 + 2 * kLayers + l] == kEncKernel[l];
  const int32_t* tail = hp + 1 + 3 * kLayers;
  ok = ok && tail[0] == VAD_HID && tail[1] == VAD_HID && tail[2] == VAD_HID && tail[3] == 1;
  if (!ok) {
    MWX_LOG_ERROR("mwx_vad: '%s' has unsupported hyper-parameters (expected 4 encoder layers "
                  "129-128-64-64-128, kernel 3, LSTM 128/128, final conv 128 -> 1)\n", path);
    return false;
  }
  std::map<std::string, VadTensorSpec> want;
  for (auto& s : vad_tensor_specs()) want[s.name] = s;
  while (c.pos < bytes.size()) {
    int32_t nd = 0, nlen = 0, ttype = 0;
    if (!c.i32(nd) || !c.i32(nlen) || !c.i32(ttype)) return truncated("tensor header");
    if (nd < 1 || nd > 4 || nlen < 0 || nlen > 256) {
      MWX_LOG_ERROR("mwx_vad: '%s' has a malformed tensor header\n", path);
      return false;
    }
    std::vector<int64_t> shape(nd);
    for (int i = 0; i < nd; ++i) {
      int32_t d = 0;
      if (!c.i32(d)) return truncated("tensor dims");
      shape[nd - 1 - i] = d;  // file order is ggml's: innermost first
    }
    std::string name(nlen, '\0');
    if (!c.take(&name[0], nlen)) return truncated("tensor name");
    auto it = want.find(name);
    if (it == want.end()) {
      MWX_LOG_ERROR("mwx_vad: unknown tensor '%s'\n", name.c_str());
      return false;
    }
    if (shape != it->second.shape) {
      MWX_LOG_ERROR("mwx_vad: tensor '%s' has the wrong shape\n", name.c_str());
      return false;
    }
    if (ttype != GGML_F32 && ttype != GGML_F16) {
      MWX_LOG_ERROR("mwx_vad: tensor '%s' has type %d (f32 or f16 expected)\n", name.c_str(),
                    ttype);
      return false;
    }
    int64_t n = 1;
    for (auto d : shape) n *= d;
    const size_t esz = ttype == GGML_F32 ? 4 : 2;
    if ((size_t)n * esz > bytes.size() - c.pos) return truncated(name.c_str());
    std::vector<float> v((size_t)n);
    if (ttype == GGML_F32) {
      memcpy(v.data(), bytes.data() + c.pos, (size_t)n * 4);
    } else {
      for (int64_t i = 0; i < n; ++i) {
        uint16_t h;
        memcpy(&h, bytes.data() + c.pos + 2 * (size_t)i, 2);
        v[(size_t)i] = f16_to_f32(h);
      }
    }
    c.pos += (size_t)n * esz;
    out[name] = std::move(v);
  }
  for (auto& kv : want)
    if (!out.count(kv.first)) {
      MWX_LOG_ERROR("mwx_vad: '%s' lacks tensor '%s'\n", path, kv.first.c_str());
      return false;
    }
  return true;
}

// grow-only device buffer of the VAD context; a fresh allocation is zeroed on
// the context's stream (never the null stream, which that stream does not
// wait for). The stream is idle when a buffer grows: every call ends with a
// synchronization.
struct VBuf {
  void* p = nullptr;
  size_t n = 0;
  void* get(size_t bytes, hipStream_t st) {
    if (bytes > n) {
      std::lock_guard<std::recursive_mutex> lock(capture_mutex());
      if (p) (void)hipFree(p);
      p = nullptr;
      n = 0;
      HIPC(hipMalloc(&p, bytes));
      n = bytes;
      HIPC(hipMemsetAsync(p, 0, bytes, st));
    }
    return p;
  }
  void release() {
    std::lock_guard<std::recursive_mutex> lock(capture_mutex());
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};
struct PinBuf {  // grow-only pinned host buffer
  void* p = nullptr;
  size_t n = 0;
  void* get(size_t bytes) {
    if (bytes > n) {
      std::lock_guard<std::recursive_mutex> lock(capture_mutex());
      if (p) (void)hipHostFree(p);
      p = nullptr;
      n = 0;
      HIPC(hipHostMalloc(&p, bytes, hipHostMallocDefault));
      n = bytes;
    }
    return p;
  }
  void release() {
    std::lock_guard<std::recursive_mutex> lock(capture_mutex());
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
  }
};

// (as driver.inc: plain host memory is unknown to HIP and reports an error)
bool vad_is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}

}  // namespace
}  // namespace mwx

struct mwx_vad_context {
  int device = 0;
  hipStream_t stream = nullptr;
  // front end | recurrence | segments, around the compaction, around the chunk plan
  // ... and [8..11] around the three network kernels of a stream call
  hipEvent_t ev[12] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool timed = false, timed_trim = false, timed_chunks = false, timed_stream = false;
  float* d_weights = nullptr;
  mwx::VadWeights w{};
  mwx::VBuf d_pcm, d_pre, d_probs, d_meta, d_tab, d_ooff, d_ctab, d_caps;
  mwx::PinBuf h_meta, h_probs, h_tab, h_ooff, h_ctab, h_caps;
  std::vector<float> probs;  // mwx_vad_probs
  int probs_n_samples = 0;   // the clip length they belong to
  // streams: the slot table grows a block at a time, so a
  // stream's slot never moves; a freed slot is handed out again
  std::vector<mwx::VadStreamSlot*> slot_blocks;
  std::vector<mwx::VadStreamSlot*> free_slots;
  std::vector<mwx_vad_stream*> streams;  // live ones: orphaned when the context goes first
  mwx::VBuf d_stage, d_sout;
  mwx::PinBuf h_sout;
};

struct mwx_vad_stream {
  mwx_vad_context* ctx = nullptr;  // null once its context is freed
  mwx::VadStreamSlot* slot = nullptr;
  mwx::VadSegParams prm{};
  // host mirror of the slot: what splits a feed into chunks, and the scan's
  // registers as of the last call (mwx_vad_stream_finish needs trig and start)
  int64_t n_samples = 0, n_chunks = 0;
  int tail_n = 0, par = 0;
  bool finished = false, provisional = false;
  bool trig = false;
  int64_t start = 0, temp_end = 0, prev_end = 0, next_start = 0;
  std::vector<float> probs;  // all since reset; the last one provisional when `provisional`
  float max_whole = 0.0f;    // over the whole chunks' probabilities
  std::vector<int64_t> seg;  // raw segments closed since reset: (s0, s1, closed_at)
};

namespace mwx {
namespace {

void vad_destroy(mwx_vad_context* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  if (v->stream) (void)hipStreamSynchronize(v->stream);
  v->d_pcm.release();
  v->d_pre.release();
  v->d_probs.release();
  v->d_meta.release();
  v->d_tab.release();
  v->d_ooff.release();
  v->d_ctab.release();
  v->d_caps.release();
  v->h_ctab.release();
  v->h_caps.release();
  v->h_meta.release();
  v->h_probs.release();
  v->h_tab.release();
  v->h_ooff.release();
  v->d_stage.release();
  v->d_sout.release();
  v->h_sout.release();
  for (mwx_vad_stream* s : v->streams) s->ctx = nullptr;
  {
    std::lock_guard<std::recursive_mutex> lock(capture_mutex());
    if (v->d_weights) (void)hipFree(v->d_weights);
    for (VadStreamSlot* b : v->slot_blocks) (void)hipFree(b);
  }
  for (auto& e : v->ev)
    if (e) (void)hipEventDestroy(e);
  if (v->stream) (void)hipStreamDestroy(v->stream);
  delete v;
}

// Weights to the device, transposed so that the output row is contiguous.
void vad_upload(mwx_vad_context* v, std::map<std::string, std::vector<float>>& t) {
  std::vector<float> host;
  auto reserve = [&](size_t n) {
    const size_t at = host.size();
    host.resize(at + (n + 3) / 4 * 4, 0.0f);  // 16-byte aligned pieces
    return at;
  };
  const int rows = 2 * VAD_BINS;
  const auto& basis = t["_model.stft.forward_basis_buffer"];
  const size_t o_basis = reserve((size_t)rows * VAD_NFFT);
  for (int r = 0; r < rows; ++r)
    for (int k = 0; k < VAD_NFFT; ++k) host[o_basis + (size_t)k * rows + r] = basis[(size_t)r * VAD_NFFT + k];
  size_t o_conv[kLayers], o_bias[kLayers];
  for (int l = 0; l < kLayers; ++l) {
    const std::string p = "_model.encoder." + std::to_string(l) + ".reparam_conv.";
    const auto& wt = t[p + "weight"];  // [out][in][3]
    const int co = kEncOut[l], ci = kEncIn[l];
    o_conv[l] = reserve((size_t)co * ci * 3);
    for (int o = 0; o < co; ++o)
      for (int i = 0; i < ci * 3; ++i) host[o_conv[l] + (size_t)i * co + o] = wt[(size_t)o * ci * 3 + i];
    o_bias[l] = reserve(co);
    memcpy(&host[o_bias[l]], t[p + "bias"].data(), (size_t)co * 4);
  }
  auto transposed_gates = [&](const std::vector<float>& wt) {  // [512][128] -> [128][512]
    const size_t at = reserve((size_t)VAD_GATES * VAD_HID);
    for (int j = 0; j < VAD_GATES; ++j)
      for (int k = 0; k < VAD_HID; ++k) host[at + (size_t)k * VAD_GATES + j] = wt[(size_t)j * VAD_HID + k];
    return at;
  };
  const size_t o_ih = transposed_gates(t["_model.decoder.rnn.weight_ih"]);
  const size_t o_hh = transposed_gates(t["_model.decoder.rnn.weight_hh"]);
  auto plain = [&](const std::vector<float>& x) {
    const size_t at = reserve(x.size());
    memcpy(&host[at], x.data(), x.size() * 4);
    return at;
  };
  const size_t o_bih = plain(t["_model.decoder.rnn.bias_ih"]);
  const size_t o_bhh = plain(t["_model.decoder.rnn.bias_hh"]);
  const size_t o_wf = plain(t["_model.decoder.decoder.2.weight"]);
  {
    std::lock_guard<std::recursive_mutex> lock(capture_mutex());
    HIPC(hipMalloc((void**)&v->d_weights, host.size() * 4));
  }
  HIPC(hipMemcpyAsync(v->d_weights, host.data(), host.size() * 4, hipMemcpyHostToDevice, v->stream));
  HIPC(hipStreamSynchronize(v->stream));
  const float* d = v->d_weights;
  v->w.basis_t = d + o_basis;
  for (int l = 0; l < kLayers; ++l) {
    v->w.conv_t[l] = d + o_conv[l];
    v->w.conv_b[l] = d + o_bias[l];
  }
  v->w.wih_t = d + o_ih;
  v->w.whh_t = d + o_hh;
  v->w.b_ih = d + o_bih;
  v->w.b_hh = d + o_bhh;
  v->w.w_f = d + o_wf;
  v->w.b_f = t["_model.decoder.decoder.2.bias"][0];
}

// mwx_vad_params -> the integers of the rule; false (logged)
// for values outside it.
bool vad_derive_params(const mwx_vad_params& p, VadSegParams& d) {
  auto bad = [](const char* what) {
    MWX_LOG_ERROR("mwx_vad: invalid parameters (%s)\n", what);
    return false;
  };
  if (std::isnan(p.threshold) || std::isnan(p.max_speech_duration_s) ||
      std::isnan(p.samples_overlap))
    return bad("NaN");
  if (!(p.threshold > 0.0f && p.threshold < 1.0f)) return bad("threshold outside (0, 1)");
  if (p.min_speech_duration_ms < 0 || p.min_silence_duration_ms < 0 || p.speech_pad_ms < 0)
    return bad("negative duration");
  if (!(p.max_speech_duration_s > 0.0f)) return bad("max_speech_duration_s <= 0");
  if (p.samples_overlap < 0.0f) return bad("samples_overlap < 0");
  if (p.samples_overlap > 100000.0f) return bad("samples_overlap too large");
  d.thr = p.threshold;
  d.neg = std::max(p.threshold - 0.15f, 0.01f);
  d.min_speech = 16LL * p.min_speech_duration_ms;
  d.min_sil = 16LL * p.min_silence_duration_ms;
  d.pad = 16LL * p.speech_pad_ms;
  const double ms = (double)p.max_speech_duration_s * 16000.0 - 512.0 - 2.0 * (double)d.pad;
  d.max_speech = (long long)std::min(ms, 4611686018427387904.0 /* 2^62 */);
  d.ov = (int)(p.samples_overlap * 16000.0f);
  return true;
}

// One call's inputs as the kernels see them.
struct VadPass {
  std::vector<int> off;  // chunk prefix sums
  int total = 0, max_chunks = 0;
  const float* const* d_ptrs = nullptr;
  const int* d_ns = nullptr;
  const int* d_off = nullptr;
  const VadSegParams* d_prm = nullptr;
};

// Chunk prefix sums of the clips; < 0 on bad arguments.
int vad_chunk_offsets(const int* n_samples, int n_clips, VadPass& ps) {
  ps.off.assign((size_t)n_clips + 1, 0);
  ps.max_chunks = 0;
  for (int b = 0; b < n_clips; ++b) {
    if (n_samples[b] < 0) return -2;
    const int nc = mwx_vad_n_chunks(n_samples[b]);
    if ((long)ps.off[b] + nc > 0x7fffffffL) return -3;
    ps.off[b + 1] = ps.off[b] + nc;
    ps.max_chunks = std::max(ps.max_chunks, nc);
  }
  ps.total = ps.off[n_clips];
  return 0;
}

// meta: [clip pointers][n_samples][chunk_off][segment parameters], one upload
void vad_upload_meta(mwx_vad_context* v, const std::vector<const float*>& ptrs,
                     const int* n_samples, int n_clips, const VadSegParams* prm, int n_prm,
                     VadPass& ps) {
  hipStream_t st = v->stream;
  const size_t m_ptr = 0, m_ns = m_ptr + (size_t)n_clips * 8, m_off = m_ns + (size_t)n_clips * 4;
  const size_t m_prm = (m_off + ((size_t)n_clips + 1) * 4 + 7) / 8 * 8;
  const size_t m_bytes = m_prm + (size_t)n_prm * sizeof(VadSegParams);
  char* hm = (char*)v->h_meta.get(m_bytes);
  char* dm = (char*)v->d_meta.get(m_bytes, st);
  memcpy(hm + m_ptr, ptrs.data(), (size_t)n_clips * 8);
  memcpy(hm + m_ns, n_samples, (size_t)n_clips * 4);
  memcpy(hm + m_off, ps.off.data(), ((size_t)n_clips + 1) * 4);
  if (n_prm > 0) memcpy(hm + m_prm, prm, (size_t)n_prm * sizeof(VadSegParams));
  HIPC(hipMemcpyAsync(dm, hm, m_bytes, hipMemcpyHostToDevice, st));
  ps.d_ptrs = (const float* const*)(dm + m_ptr);
  ps.d_ns = (const int*)(dm + m_ns);
  ps.d_off = (const int*)(dm + m_off);
  ps.d_prm = n_prm > 0 ? (const VadSegParams*)(dm + m_prm) : nullptr;
}

// Stages the host clips back to back in d_pcm, uploads the meta block and runs
// the two network kernels; the probabilities are in d_probs when the stream
// gets there. ps.total == 0: nothing was launched.
int vad_forward(mwx_vad_context* v, const float* const* samples, const int* n_samples, int n_clips,
                const VadSegParams* prm, int n_prm, VadPass& ps) {
  HIPC(hipSetDevice(v->device));
  v->timed = v->timed_trim = v->timed_chunks = v->timed_stream = false;
  std::vector<size_t> stage((size_t)n_clips, 0);
  std::vector<char> on_device((size_t)n_clips, 0);
  size_t stage_floats = 0;
  for (int b = 0; b < n_clips; ++b)
    if (n_samples[b] > 0 && !samples[b]) return -2;
  const int rc = vad_chunk_offsets(n_samples, n_clips, ps);
  if (rc != 0) return rc;
  for (int b = 0; b < n_clips; ++b)
    if (n_samples[b] > 0 && !(on_device[b] = vad_is_device_ptr(samples[b]))) {
      stage[b] = stage_floats;
      stage_floats += ((size_t)n_samples[b] + 3) / 4 * 4;
    }
  if (ps.total == 0) return 0;
  const long tiles = (ps.max_chunks + VAD_TILE - 1) / VAD_TILE;  // front-end grid = clips x tiles
  if (tiles * n_clips > 0x7fffffffL) return -3;
  hipStream_t st = v->stream;
  float* d_pcm = stage_floats ? (float*)v->d_pcm.get(stage_floats * 4, st) : nullptr;
  std::vector<const float*> ptrs((size_t)n_clips);
  for (int b = 0; b < n_clips; ++b) {
    ptrs[b] = samples[b];
    if (n_samples[b] > 0 && !on_device[b]) {
      HIPC(hipMemcpyAsync(d_pcm + stage[b], samples[b], (size_t)n_samples[b] * 4,
                          hipMemcpyHostToDevice, st));
      ptrs[b] = d_pcm + stage[b];
    }
  }
  vad_upload_meta(v, ptrs, n_samples, n_clips, prm, n_prm, ps);
  float* d_pre = (float*)v->d_pre.get((size_t)ps.total * VAD_GATES * 4, st);
  float* d_probs = (float*)v->d_probs.get((size_t)ps.total * 4, st);
  HIPC(hipEventRecord(v->ev[0], st));
  vad_frontend_launch(v->w, ps.d_ptrs, ps.d_ns, ps.d_off, n_clips, ps.max_chunks, d_pre, st);
  HIPC(hipEventRecord(v->ev[1], st));
  vad_lstm_launch(v->w, d_pre, ps.d_off, n_clips, d_probs, st);
  HIPC(hipEventRecord(v->ev[2], st));
  HIPC(hipGetLastError());
  return 0;
}

int vad_run(mwx_vad_context* v, const float* const* samples, const int* n_samples, int n_clips,
            float* probs_out, const int* probs_offset) {
  VadPass ps;
  const int rc = vad_forward(v, samples, n_samples, n_clips, nullptr, 0, ps);
  if (rc != 0 || ps.total == 0) return rc;
  hipStream_t st = v->stream;
  float* h_probs = (float*)v->h_probs.get((size_t)ps.total * 4);
  HIPC(hipMemcpyAsync(h_probs, v->d_probs.p, (size_t)ps.total * 4, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  v->timed = true;
  for (int b = 0; b < n_clips; ++b)
    if (ps.off[b + 1] > ps.off[b])
      memcpy(probs_out + probs_offset[b], h_probs + ps.off[b],
             (size_t)(ps.off[b + 1] - ps.off[b]) * 4);
  return 0;
}

// vad_segments_kernel over the probabilities in d_probs, then the one copy
// back: the tables of every clip (kernels.h, vad_table_off) in pinned memory,
// valid until the context's next call. Synchronizes. With caps (one cap in
// samples for all clips, n_caps = 1, or one per clip), vad_chunks_kernel runs
// behind it and the chunk tables (kernels.h, vad_chunk_table_off) come back in
// v->h_ctab with the same synchronize.
const int64_t* vad_segment_tables(mwx_vad_context* v, int n_clips, int prm_stride,
                                  const VadPass& ps, const int64_t* caps = nullptr,
                                  int n_caps = 0) {
  static_assert(sizeof(long long) == sizeof(int64_t), "table entries");
  hipStream_t st = v->stream;
  const size_t n_tab = (size_t)vad_table_off(ps.total, n_clips);
  long long* d_tab = (long long*)v->d_tab.get(n_tab * 8, st);
  int64_t* h_tab = (int64_t*)v->h_tab.get(n_tab * 8);
  vad_segments_launch((const float*)v->d_probs.p, ps.d_ns, ps.d_off, n_clips, ps.d_prm,
                      prm_stride, d_tab, st);
  HIPC(hipEventRecord(v->ev[3], st));
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h_tab, d_tab, n_tab * 8, hipMemcpyDeviceToHost, st));
  if (n_caps > 0) {
    const size_t n_ctab = (size_t)vad_chunk_table_off(ps.total, n_clips);
    long long* d_ctab = (long long*)v->d_ctab.get(n_ctab * 8, st);
    int64_t* h_ctab = (int64_t*)v->h_ctab.get(n_ctab * 8);
    long long* d_caps = (long long*)v->d_caps.get((size_t)n_caps * 8, st);
    int64_t* h_caps = (int64_t*)v->h_caps.get((size_t)n_caps * 8);
    memcpy(h_caps, caps, (size_t)n_caps * 8);
    HIPC(hipMemcpyAsync(d_caps, h_caps, (size_t)n_caps * 8, hipMemcpyHostToDevice, st));
    HIPC(hipEventRecord(v->ev[6], st));
    vad_chunks_launch(ps.d_off, n_clips, d_tab, d_caps, n_caps > 1 ? 1 : 0, d_ctab, st);
    HIPC(hipEventRecord(v->ev[7], st));
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(h_ctab, d_ctab, n_ctab * 8, hipMemcpyDeviceToHost, st));
  }
  HIPC(hipStreamSynchronize(st));
  v->timed_chunks = n_caps > 0;
  return h_tab;
}

// Clip b's chunk table -> (first piece, n pieces) pairs; false when the table
// is not a partition of the clip's m pieces in order.
bool vad_read_chunk_table(const int64_t* h_ctab, const VadPass& ps, int b, int64_t m,
                          std::vector<int64_t>& chunk) {
  const int64_t* X = h_ctab + vad_chunk_table_off(ps.off[b], b);
  const int64_t cap = ps.off[b + 1] - ps.off[b] + 1;
  const int64_t nc = X[0];
  if (nc < 0 || nc > cap) return false;
  int64_t next = 0;
  for (int64_t j = 0; j < nc; ++j) {
    if (X[1 + 2 * j] != next || X[2 + 2 * j] < 1) return false;
    next += X[2 + 2 * j];
  }
  if (next != m) return false;
  chunk.assign(X + 1, X + 1 + 2 * nc);
  return true;
}

// Clip b's table -> segments and pieces; false when the table is not one the
// kernel can have written.
bool vad_read_table(const int64_t* h_tab, const VadPass& ps, int b, std::vector<int64_t>& seg,
                    std::vector<int64_t>& piece, int64_t& n_compact) {
  const int64_t* T = h_tab + vad_table_off(ps.off[b], b);
  const int64_t cap = ps.off[b + 1] - ps.off[b] + 1;
  const int64_t m = T[0];
  if (m < 0 || m > cap || T[1] < 0) return false;
  seg.assign(T + 2, T + 2 + 2 * m);
  piece.assign(T + 2 + 2 * cap, T + 2 + 2 * cap + 3 * m);
  n_compact = T[1];
  return true;
}

// The segment kernel over caller-supplied probabilities (clip b's at
// probs + probs_offset[b]): mwx_vad_segments_from_probs and the test hook.
// prm: one entry per clip.
int vad_segments_of_probs(mwx_vad_context* v, const VadSegParams* prm, const float* probs,
                          const int* probs_offset, const int* n_samples, int n_clips,
                          std::vector<mwx_vad_trimmed::Clip>& out,
                          const int64_t* caps = nullptr) {
  HIPC(hipSetDevice(v->device));
  v->timed = v->timed_trim = v->timed_chunks = v->timed_stream = false;
  VadPass ps;
  const int rc = vad_chunk_offsets(n_samples, n_clips, ps);
  if (rc != 0) return rc;
  out.assign((size_t)n_clips, mwx_vad_trimmed::Clip());
  hipStream_t st = v->stream;
  float* h_probs = (float*)v->h_probs.get((size_t)std::max(ps.total, 1) * 4);
  float* d_probs = (float*)v->d_probs.get((size_t)std::max(ps.total, 1) * 4, st);
  for (int b = 0; b < n_clips; ++b)
    if (ps.off[b + 1] > ps.off[b])
      memcpy(h_probs + ps.off[b], probs + probs_offset[b],
             (size_t)(ps.off[b + 1] - ps.off[b]) * 4);
  if (ps.total > 0)
    HIPC(hipMemcpyAsync(d_probs, h_probs, (size_t)ps.total * 4, hipMemcpyHostToDevice, st));
  vad_upload_meta(v, std::vector<const float*>((size_t)n_clips, nullptr), n_samples, n_clips, prm,
                  n_clips, ps);
  const int64_t* h_tab = vad_segment_tables(v, n_clips, 1, ps, caps, caps ? n_clips : 0);
  for (int b = 0; b < n_clips; ++b) {
    if (!vad_read_table(h_tab, ps, b, out[b].seg, out[b].piece, out[b].n_compact)) return -5;
    if (caps && !vad_read_chunk_table((const int64_t*)v->h_ctab.p, ps, b,
                                      (int64_t)out[b].piece.size() / 3, out[b].chunk))
      return -5;
  }
  return 0;
}

// VAD, segments and compaction of all clips; fills t (whose d_pcm the caller
// frees, also after an exception). chunk_cap > 0: the chunk plan with that cap
// in samples; 0: no plan, every clip that has segments is one chunk.
int vad_trim_run(mwx_vad_context* v, const VadSegParams& prm, const float* const* samples,
                 const int* n_samples, int n_clips, mwx_vad_trimmed& t, int64_t chunk_cap) {
  t.device = v->device;
  t.clips.assign((size_t)n_clips, mwx_vad_trimmed::Clip());
  VadPass ps;
  const int rc = vad_forward(v, samples, n_samples, n_clips, &prm, 1, ps);
  if (rc != 0 || ps.total == 0) return rc;
  hipStream_t st = v->stream;
  const int64_t* h_tab = vad_segment_tables(v, n_clips, 0, ps, &chunk_cap, chunk_cap > 0 ? 1 : 0);
  size_t total = 0;
  int64_t max_len = 0;
  int64_t* h_ooff = (int64_t*)v->h_ooff.get((size_t)n_clips * 8);
  for (int b = 0; b < n_clips; ++b) {
    mwx_vad_trimmed::Clip& c = t.clips[b];
    if (!vad_read_table(h_tab, ps, b, c.seg, c.piece, c.n_compact)) return -5;
    const int64_t m = (int64_t)c.piece.size() / 3;
    if (chunk_cap > 0) {
      if (!vad_read_chunk_table((const int64_t*)v->h_ctab.p, ps, b, m, c.chunk)) return -5;
    } else if (m > 0) {
      c.chunk = {0, m};
    }
    c.off = total;
    h_ooff[b] = (int64_t)total;
    total += ((size_t)c.n_compact + 3) / 4 * 4;  // 16-byte aligned clip starts
    max_len = std::max(max_len, c.n_compact);
  }
  v->timed = true;
  if (total == 0) return 0;
  const int64_t tiles = (max_len + VAD_CP_TILE - 1) / VAD_CP_TILE;  // compaction grid = clips x tiles
  if (tiles * n_clips > 0x7fffffffL) return -3;
  {
    std::lock_guard<std::recursive_mutex> lock(capture_mutex());
    HIPC(hipMalloc((void**)&t.d_pcm, total * 4));
  }
  long long* d_ooff = (long long*)v->d_ooff.get((size_t)n_clips * 8, st);
  HIPC(hipMemcpyAsync(d_ooff, h_ooff, (size_t)n_clips * 8, hipMemcpyHostToDevice, st));
  HIPC(hipEventRecord(v->ev[4], st));
  vad_compact_launch(ps.d_ptrs, ps.d_ns, ps.d_off, n_clips, (const long long*)v->d_tab.p, d_ooff,
                     max_len, t.d_pcm, st);
  HIPC(hipEventRecord(v->ev[5], st));
  HIPC(hipGetLastError());
  // the object is complete, and independent of this context's buffers, when
  // the call returns
  HIPC(hipStreamSynchronize(st));
  v->timed_trim = true;
  return 0;
}

void vad_trimmed_destroy(mwx_vad_trimmed* t) {
  if (!t) return;
  if (t->d_pcm) {
    (void)hipSetDevice(t->device);
    std::lock_guard<std::recursive_mutex> lock(capture_mutex());
    (void)hipFree(t->d_pcm);
  }
  delete t;
}

// ---- streams --------------------------------------------------
constexpr int kSlotBlock = 32;           // slots per allocation of the table
constexpr int kStreamMaxFeed = 480000;   // samples per stream per call (30 s)

VadStreamSlot* vad_slot_take(mwx_vad_context* v) {
  if (v->free_slots.empty()) {
    VadStreamSlot* block = nullptr;
    {
      std::lock_guard<std::recursive_mutex> lock(capture_mutex());
      HIPC(hipMalloc((void**)&block, sizeof(VadStreamSlot) * kSlotBlock));
    }
    v->slot_blocks.push_back(block);
    for (int i = kSlotBlock - 1; i >= 0; --i) v->free_slots.push_back(block + i);
  }
  VadStreamSlot* s = v->free_slots.back();
  v->free_slots.pop_back();
  return s;
}

void vad_stream_clear(mwx_vad_stream* s) {
  s->n_samples = s->n_chunks = 0;
  s->tail_n = s->par = 0;
  s->finished = s->provisional = s->trig = false;
  s->start = s->temp_end = s->prev_end = s->next_start = 0;
  s->probs.clear();
  s->max_whole = 0.0f;
  s->seg.clear();
}

// One call over n streams. given == nullptr: counts[i] new samples at src[i]
// go through the staging kernel, the front end, the stream recurrence and the
// scan. given != nullptr (the test hook): counts[i] probabilities at given[i]
// stand in for as many whole chunks and only the scan runs. The arguments have
// been checked. The streams change only when everything has succeeded.
int vad_stream_call(mwx_vad_context* v, mwx_vad_stream* const* streams, const float* const* src,
                    const int* counts, int n, const float* const* given) {
  HIPC(hipSetDevice(v->device));
  v->timed = v->timed_trim = v->timed_chunks = v->timed_stream = false;
  hipStream_t st = v->stream;
  std::vector<VadStreamFeed> feeds((size_t)n);
  std::vector<int> off((size_t)n + 1, 0), ns((size_t)n, 0);
  std::vector<size_t> up((size_t)n, 0);  // host samples: where they go in d_pcm
  std::vector<char> on_device((size_t)n, 0);
  size_t up_floats = 0;
  int max_chunks = 0;
  for (int i = 0; i < n; ++i) {
    const mwx_vad_stream* s = streams[i];
    VadStreamFeed& f = feeds[i];
    f.slot = s->slot;
    f.src = nullptr;
    f.par = s->par;
    f.fresh = s->n_chunks == 0;
    f.prm = s->prm;
    if (given) {
      f.n_new = f.tail_n = f.rem = 0;
      f.n_full = counts[i];
    } else {
      f.n_new = counts[i];
      f.tail_n = s->tail_n;
      const int total = f.tail_n + f.n_new;  // < 512 + 480000
      f.n_full = total / VAD_CHUNK;
      f.rem = total % VAD_CHUNK;
      ns[i] = total;
      if (f.n_new > 0 && !(on_device[i] = vad_is_device_ptr(src[i]))) {
        up[i] = up_floats;
        up_floats += ((size_t)f.n_new + 3) / 4 * 4;
      }
    }
    const int staged = f.n_full + (f.rem > 0 ? 1 : 0);
    if ((long)off[i] + staged > 0x7fffffffL / VAD_CHUNK) return -3;
    off[i + 1] = off[i] + staged;
    max_chunks = std::max(max_chunks, staged);
  }
  const int total = off[n];
  if (total == 0) return 0;  // nothing fed and no tail anywhere: nothing changes
  float* d_pcm = up_floats ? (float*)v->d_pcm.get(up_floats * 4, st) : nullptr;
  float* d_stage = given ? nullptr : (float*)v->d_stage.get((size_t)total * VAD_CHUNK * 4, st);
  std::vector<const float*> ptrs((size_t)n, nullptr);
  for (int i = 0; i < n && !given; ++i) {
    if (feeds[i].n_new > 0) {
      feeds[i].src = src[i];
      if (!on_device[i]) {
        HIPC(hipMemcpyAsync(d_pcm + up[i], src[i], (size_t)feeds[i].n_new * 4,
                            hipMemcpyHostToDevice, st));
        feeds[i].src = d_pcm + up[i];
      }
    }
    ptrs[i] = d_stage + (size_t)off[i] * VAD_CHUNK;
  }
  // meta: [feeds][stage pointers][sample counts][chunk_off], one upload
  const size_t m_feed = 0, m_ptr = m_feed + (size_t)n * sizeof(VadStreamFeed);
  const size_t m_ns = m_ptr + (size_t)n * 8, m_off = m_ns + (size_t)n * 4;
  const size_t m_bytes = m_off + ((size_t)n + 1) * 4;
  static_assert(sizeof(VadStreamFeed) % 8 == 0, "meta alignment");
  char* hm = (char*)v->h_meta.get(m_bytes);
  char* dm = (char*)v->d_meta.get(m_bytes, st);
  memcpy(hm + m_feed, feeds.data(), (size_t)n * sizeof(VadStreamFeed));
  memcpy(hm + m_ptr, ptrs.data(), (size_t)n * 8);
  memcpy(hm + m_ns, ns.data(), (size_t)n * 4);
  memcpy(hm + m_off, off.data(), ((size_t)n + 1) * 4);
  HIPC(hipMemcpyAsync(dm, hm, m_bytes, hipMemcpyHostToDevice, st));
  const VadStreamFeed* d_feeds = (const VadStreamFeed*)(dm + m_feed);
  const int* d_off = (const int*)(dm + m_off);
  // out: [header and events, int64][probabilities, f32], one copy back
  const size_t o_words = (size_t)VAD_STREAM_HDR * n + 3 * (size_t)total;
  const size_t o_bytes = o_words * 8 + (size_t)total * 4;
  char* d_out = (char*)v->d_sout.get(o_bytes, st);
  char* h_out = (char*)v->h_sout.get(o_bytes);
  float* d_probs = (float*)(d_out + o_words * 8);
  if (given) {
    float* h_in = (float*)(h_out + o_words * 8);  // (overwritten by the copy back)
    for (int i = 0; i < n; ++i)
      if (counts[i] > 0) memcpy(h_in + off[i], given[i], (size_t)counts[i] * 4);
    HIPC(hipMemcpyAsync(d_probs, h_in, (size_t)total * 4, hipMemcpyHostToDevice, st));
  } else {
    float* d_pre = (float*)v->d_pre.get((size_t)total * VAD_GATES * 4, st);
    HIPC(hipEventRecord(v->ev[8], st));
    vad_stream_stage_launch(d_feeds, d_off, n, max_chunks, d_stage, st);
    HIPC(hipEventRecord(v->ev[9], st));
    vad_frontend_launch(v->w, (const float* const*)(dm + m_ptr), (const int*)(dm + m_ns), d_off, n,
                        max_chunks, d_pre, st);
    HIPC(hipEventRecord(v->ev[10], st));
    vad_lstm_stream_launch(v->w, d_pre, d_feeds, d_off, n, d_probs, st);
    HIPC(hipEventRecord(v->ev[11], st));
  }
  vad_stream_scan_launch(d_probs, d_feeds, d_off, n, (long long*)d_out, st);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h_out, d_out, o_bytes, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  const int64_t* words = (const int64_t*)h_out;
  const float* probs = (const float*)(h_out + o_words * 8);
  for (int i = 0; i < n; ++i) {  // what the scan kernel can have written
    const int64_t* hdr = words + (size_t)VAD_STREAM_HDR * i;
    if (hdr[0] < 0 || hdr[0] > feeds[i].n_full || hdr[6] != streams[i]->n_chunks + feeds[i].n_full)
      return -5;
  }
  v->timed_stream = !given;
  for (int i = 0; i < n; ++i) {
    mwx_vad_stream* s = streams[i];
    const VadStreamFeed& f = feeds[i];
    const int64_t* hdr = words + (size_t)VAD_STREAM_HDR * i;
    const int staged = off[i + 1] - off[i];
    if (staged > 0) {
      if (s->provisional) s->probs.pop_back();
      s->probs.insert(s->probs.end(), probs + off[i], probs + off[i] + staged);
      for (int k = 0; k < f.n_full; ++k) s->max_whole = std::max(s->max_whole, probs[off[i] + k]);
      s->provisional = f.rem > 0;
    }
    s->n_samples += given ? (int64_t)VAD_CHUNK * f.n_full : (int64_t)f.n_new;
    s->n_chunks = hdr[6];
    if (!given) {
      s->tail_n = f.rem;
      s->par ^= 1;
    }
    const int64_t* ev = words + (size_t)VAD_STREAM_HDR * n + 3 * (size_t)off[i];
    s->seg.insert(s->seg.end(), ev, ev + 3 * hdr[0]);
    s->trig = hdr[1] != 0;
    s->start = hdr[2];
    s->temp_end = hdr[3];
    s->prev_end = hdr[4];
    s->next_start = hdr[5];
  }
  return 0;
}

}  // namespace
}  // namespace mwx

extern "C" {

struct mwx_vad_context_params mwx_vad_default_context_params(void) {
  mwx_vad_context_params p;
  p.n_threads = 4;
  p.use_gpu = true;
  p.gpu_device = 0;
  return p;
}

struct mwx_vad_context* mwx_vad_init_from_file_with_params(const char* path_model,
                                                           struct mwx_vad_context_params params) {
  if (!path_model) return nullptr;
  if (!params.use_gpu) {
    MWX_LOG_ERROR("mwx_vad: use_gpu = false is not supported (there is no CPU path)\n");
    return nullptr;
  }
  std::map<std::string, std::vector<float>> tensors;
  if (!mwx::read_vad_file(path_model, tensors)) return nullptr;
  mwx_vad_context* v = new mwx_vad_context();
  v->device = params.gpu_device;
  try {
    HIPC(hipSetDevice(v->device));
    HIPC(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
    for (auto& e : v->ev) HIPC(hipEventCreate(&e));
    mwx::vad_upload(v, tensors);
  } catch (const std::exception&) {
    mwx::vad_destroy(v);
    return nullptr;
  }
  return v;
}

void mwx_vad_free(struct mwx_vad_context* vctx) { mwx::vad_destroy(vctx); }

int mwx_vad_n_chunks(int n_samples) {
  return n_samples <= 0 ? 0 : (int)(((long)n_samples + mwx::VAD_CHUNK - 1) / mwx::VAD_CHUNK);
}

int mwx_vad_detect_speech_batch(struct mwx_vad_context* vctx, const float* const* samples,
                                const int* n_samples, int n_clips, float* probs_out,
                                const int* probs_offset) {
  if (!vctx || n_clips < 0) return -1;
  if (n_clips == 0) return 0;
  if (!samples || !n_samples || !probs_out || !probs_offset) return -1;
  try {
    return mwx::vad_run(vctx, samples, n_samples, n_clips, probs_out, probs_offset);
  } catch (const std::exception&) {
    return -4;
  }
}

bool mwx_vad_detect_speech(struct mwx_vad_context* vctx, const float* samples, int n_samples) {
  if (!vctx || n_samples < 0 || (n_samples > 0 && !samples)) return false;
  std::vector<float> out((size_t)mwx_vad_n_chunks(n_samples));
  float dummy = 0.0f;
  const int zero = 0;
  const int rc = mwx_vad_detect_speech_batch(vctx, &samples, &n_samples, 1,
                                             out.empty() ? &dummy : out.data(), &zero);
  if (rc != 0) return false;
  vctx->probs = std::move(out);
  vctx->probs_n_samples = n_samples;
  return true;
}

int mwx_vad_n_probs(struct mwx_vad_context* vctx) { return vctx ? (int)vctx->probs.size() : 0; }

const float* mwx_vad_probs(struct mwx_vad_context* vctx) {
  return vctx && !vctx->probs.empty() ? vctx->probs.data() : nullptr;
}

int mwx_vad_last_kernel_ms(struct mwx_vad_context* vctx, float* frontend_ms, float* lstm_ms) {
  if (!vctx || !vctx->timed) return -1;
  float a = 0.0f, b = 0.0f;
  if (hipEventElapsedTime(&a, vctx->ev[0], vctx->ev[1]) != hipSuccess ||
      hipEventElapsedTime(&b, vctx->ev[1], vctx->ev[2]) != hipSuccess)
    return -1;
  if (frontend_ms) *frontend_ms = a;
  if (lstm_ms) *lstm_ms = b;
  return 0;
}

// ---- speech segments and trimming ---------------------------------------------
struct mwx_vad_params mwx_vad_default_params(void) {
  mwx_vad_params p;
  p.threshold = 0.5f;
  p.min_speech_duration_ms = 250;
  p.min_silence_duration_ms = 100;
  p.max_speech_duration_s = 3.402823466e+38f;  // FLT_MAX
  p.speech_pad_ms = 30;
  p.samples_overlap = 0.1f;
  return p;
}

struct mwx_vad_segments* mwx_vad_segments_from_probs(struct mwx_vad_context* vctx,
                                                     struct mwx_vad_params params) {
  if (!vctx) return nullptr;
  mwx::VadSegParams prm;
  if (!mwx::vad_derive_params(params, prm)) return nullptr;
  const int n = vctx->probs_n_samples, zero = 0;
  if (mwx_vad_n_chunks(n) != (int)vctx->probs.size()) return nullptr;
  try {
    const std::vector<float>& probs = vctx->probs;
    const float dummy = 0.0f;
    std::vector<mwx_vad_trimmed::Clip> out;
    if (mwx::vad_segments_of_probs(vctx, &prm, probs.empty() ? &dummy : probs.data(), &zero, &n,
                                   1, out) != 0)
      return nullptr;
    mwx_vad_segments* s = new mwx_vad_segments();
    s->seg = std::move(out[0].seg);
    return s;
  } catch (const std::exception&) {
    return nullptr;
  }
}

struct mwx_vad_segments* mwx_vad_segments_from_samples(struct mwx_vad_context* vctx,
                                                       struct mwx_vad_params params,
                                                       const float* samples, int n_samples) {
  mwx::VadSegParams prm;
  if (!vctx || !mwx::vad_derive_params(params, prm)) return nullptr;
  if (!mwx_vad_detect_speech(vctx, samples, n_samples)) return nullptr;
  return mwx_vad_segments_from_probs(vctx, params);
}

int mwx_vad_segments_n_segments(struct mwx_vad_segments* s) {
  return s ? (int)(s->seg.size() / 2) : 0;
}
float mwx_vad_segments_get_segment_t0(struct mwx_vad_segments* s, int i) {
  return (float)s->seg.at(2 * (size_t)i) / 160.0f;
}
float mwx_vad_segments_get_segment_t1(struct mwx_vad_segments* s, int i) {
  return (float)s->seg.at(2 * (size_t)i + 1) / 160.0f;
}
void mwx_vad_free_segments(struct mwx_vad_segments* s) { delete s; }

static mwx_vad_trimmed* vad_trim_batch_any(struct mwx_vad_context* vctx,
                                           struct mwx_vad_params params, int64_t chunk_cap,
                                           const float* const* samples, const int* n_samples,
                                           int n_clips) {
  if (!vctx || n_clips < 0 || (n_clips > 0 && (!samples || !n_samples))) return nullptr;
  mwx::VadSegParams prm;
  if (!mwx::vad_derive_params(params, prm)) return nullptr;
  mwx_vad_trimmed* t = new mwx_vad_trimmed();
  t->device = vctx->device;
  if (n_clips == 0) return t;
  int rc = -4;
  try {
    rc = mwx::vad_trim_run(vctx, prm, samples, n_samples, n_clips, *t, chunk_cap);
  } catch (const std::exception&) {
  }
  if (rc != 0) {
    MWX_LOG_ERROR("mwx_vad_trim_batch failed (%d)\n", rc);
    mwx::vad_trimmed_destroy(t);
    return nullptr;
  }
  return t;
}

struct mwx_vad_trimmed* mwx_vad_trim_batch(struct mwx_vad_context* vctx,
                                           struct mwx_vad_params params,
                                           const float* const* samples, const int* n_samples,
                                           int n_clips) {
  return vad_trim_batch_any(vctx, params, 0, samples, n_samples, n_clips);
}

struct mwx_vad_trimmed* mwx_vad_trim_batch_chunked(struct mwx_vad_context* vctx,
                                                   struct mwx_vad_params params, float chunk_s,
                                                   const float* const* samples,
                                                   const int* n_samples, int n_clips) {
  if (std::isnan(chunk_s) || !(chunk_s >= 1.0f && chunk_s <= 30.0f)) {
    MWX_LOG_ERROR("mwx_vad_trim_batch_chunked: chunk_s outside [1, 30]\n");
    return nullptr;
  }
  const int64_t cap = (int64_t)((double)chunk_s * 16000.0);
  return vad_trim_batch_any(vctx, params, cap, samples, n_samples, n_clips);
}

int mwx_vad_trimmed_n_clips(const struct mwx_vad_trimmed* t) { return t ? (int)t->clips.size() : 0; }

#define MWX_TRIM_CLIP(t, clip, fail) \
  if (!(t) || (clip) < 0 || (size_t)(clip) >= (t)->clips.size()) return fail

int mwx_vad_trimmed_n_segments(const struct mwx_vad_trimmed* t, int clip) {
  MWX_TRIM_CLIP(t, clip, -1);
  return (int)(t->clips[clip].seg.size() / 2);
}
int mwx_vad_trimmed_segment(const struct mwx_vad_trimmed* t, int clip, int i, int64_t* s0,
                            int64_t* s1) {
  MWX_TRIM_CLIP(t, clip, -1);
  const std::vector<int64_t>& seg = t->clips[clip].seg;
  if (i < 0 || 2 * (size_t)i + 1 >= seg.size()) return -1;
  if (s0) *s0 = seg[2 * (size_t)i];
  if (s1) *s1 = seg[2 * (size_t)i + 1];
  return 0;
}
int64_t mwx_vad_trimmed_n_samples(const struct mwx_vad_trimmed* t, int clip) {
  MWX_TRIM_CLIP(t, clip, -1);
  return t->clips[clip].n_compact;
}
const float* mwx_vad_trimmed_pcm(const struct mwx_vad_trimmed* t, int clip) {
  MWX_TRIM_CLIP(t, clip, nullptr);
  return t->clips[clip].n_compact > 0 ? t->d_pcm + t->clips[clip].off : nullptr;
}
int64_t mwx_vad_trimmed_map_time(const struct mwx_vad_trimmed* t, int clip, int64_t t_cs,
                                 bool is_end) {
  MWX_TRIM_CLIP(t, clip, t_cs);
  return mwx::vad_map_time(t->clips[clip], t_cs, is_end);
}
void mwx_vad_trimmed_free(struct mwx_vad_trimmed* t) { mwx::vad_trimmed_destroy(t); }

int mwx_vad_trimmed_n_chunks(const struct mwx_vad_trimmed* t, int clip) {
  MWX_TRIM_CLIP(t, clip, -1);
  return (int)(t->clips[clip].chunk.size() / 2);
}
int mwx_vad_trimmed_chunk(const struct mwx_vad_trimmed* t, int clip, int j, int* first_segment,
                          int* n_segments, int64_t* start, int64_t* len) {
  MWX_TRIM_CLIP(t, clip, -1);
  int64_t first, n, s, l;
  if (!mwx::vad_chunk_span(t->clips[clip], j, first, n, s, l)) return -1;
  if (first_segment) *first_segment = (int)first;
  if (n_segments) *n_segments = (int)n;
  if (start) *start = s;
  if (len) *len = l;
  return 0;
}
int64_t mwx_vad_trimmed_chunk_map_time(const struct mwx_vad_trimmed* t, int clip, int j,
                                       int64_t t_cs, bool is_end) {
  MWX_TRIM_CLIP(t, clip, t_cs);
  return mwx::vad_chunk_map_time(t->clips[clip], j, t_cs, is_end);
}

int mwx_vad_last_chunk_kernel_ms(struct mwx_vad_context* vctx, float* chunks_ms) {
  if (!vctx || !vctx->timed_chunks) return -1;
  float a = 0.0f;
  if (hipEventElapsedTime(&a, vctx->ev[6], vctx->ev[7]) != hipSuccess) return -1;
  if (chunks_ms) *chunks_ms = a;
  return 0;
}

int mwx_vad_last_trim_kernel_ms(struct mwx_vad_context* vctx, float* segments_ms,
                                float* compact_ms) {
  if (!vctx || !vctx->timed_trim) return -1;
  float a = 0.0f, b = 0.0f;
  if (hipEventElapsedTime(&a, vctx->ev[2], vctx->ev[3]) != hipSuccess ||
      hipEventElapsedTime(&b, vctx->ev[4], vctx->ev[5]) != hipSuccess)
    return -1;
  if (segments_ms) *segments_ms = a;
  if (compact_ms) *compact_ms = b;
  return 0;
}

int mwx_test_vad_segments(struct mwx_vad_context* vctx, const struct mwx_vad_params* params,
                          const float* probs, const int* probs_offset, const int* n_samples,
                          int n_clips, int* n_segments, int64_t* compact_len, int64_t* segments,
                          int64_t* pieces, const int* out_offset) {
  if (!vctx || n_clips <= 0 || !params || !probs || !probs_offset || !n_samples || !n_segments ||
      !compact_len || !segments || !pieces || !out_offset)
    return -1;
  std::vector<mwx::VadSegParams> prm((size_t)n_clips);
  for (int b = 0; b < n_clips; ++b)
    if (!mwx::vad_derive_params(params[b], prm[b])) return -2;
  try {
    std::vector<mwx_vad_trimmed::Clip> out;
    const int rc = mwx::vad_segments_of_probs(vctx, prm.data(), probs, probs_offset, n_samples,
                                              n_clips, out);
    if (rc != 0) return rc;
    for (int b = 0; b < n_clips; ++b) {
      const mwx_vad_trimmed::Clip& c = out[b];
      n_segments[b] = (int)(c.seg.size() / 2);
      compact_len[b] = c.n_compact;
      if (c.seg.size() / 2 > (size_t)mwx_vad_n_chunks(n_samples[b])) return -5;
      std::copy(c.seg.begin(), c.seg.end(), segments + 2 * (size_t)out_offset[b]);
      std::copy(c.piece.begin(), c.piece.end(), pieces + 3 * (size_t)out_offset[b]);
    }
    return 0;
  } catch (const std::exception&) {
    return -4;
  }
}

int mwx_test_vad_chunks(struct mwx_vad_context* vctx, const struct mwx_vad_params* params,
                        const int64_t* caps, const float* probs, const int* probs_offset,
                        const int* n_samples, int n_clips, int* n_chunks, int64_t* chunks,
                        const int* out_offset) {
  if (!vctx || n_clips <= 0 || !params || !caps || !probs || !probs_offset || !n_samples ||
      !n_chunks || !chunks || !out_offset)
    return -1;
  std::vector<mwx::VadSegParams> prm((size_t)n_clips);
  for (int b = 0; b < n_clips; ++b)
    if (caps[b] < 1 || !mwx::vad_derive_params(params[b], prm[b])) return -2;
  try {
    std::vector<mwx_vad_trimmed::Clip> out;
    const int rc = mwx::vad_segments_of_probs(vctx, prm.data(), probs, probs_offset, n_samples,
                                              n_clips, out, caps);
    if (rc != 0) return rc;
    for (int b = 0; b < n_clips; ++b) {
      const mwx_vad_trimmed::Clip& c = out[b];
      const int64_t nc = (int64_t)c.chunk.size() / 2;
      if (nc > mwx_vad_n_chunks(n_samples[b])) return -5;
      n_chunks[b] = (int)nc;
      for (int64_t j = 0; j < nc; ++j) {
        int64_t* o = chunks + 4 * ((size_t)out_offset[b] + (size_t)j);
        if (!mwx::vad_chunk_span(c, j, o[0], o[1], o[2], o[3])) return -5;
      }
    }
    return 0;
  } catch (const std::exception&) {
    return -4;
  }
}

int64_t mwx_test_vad_trimmed_pcm(const struct mwx_vad_trimmed* t, int clip, float* out,
                                 int64_t cap) {
  MWX_TRIM_CLIP(t, clip, -1);
  const mwx_vad_trimmed::Clip& c = t->clips[clip];
  if (c.n_compact > cap || (c.n_compact > 0 && !out)) return -2;
  if (c.n_compact == 0) return 0;
  if (hipSetDevice(t->device) != hipSuccess) return -4;
  std::lock_guard<std::recursive_mutex> lock(mwx::capture_mutex());  // (legacy-stream copy)
  if (hipMemcpy(out, t->d_pcm + c.off, (size_t)c.n_compact * 4, hipMemcpyDeviceToHost) !=
      hipSuccess)
    return -4;
  return c.n_compact;
}

// ---- streams --------------------------------------------------------------------
struct mwx_vad_stream* mwx_vad_stream_init(struct mwx_vad_context* vctx,
                                           struct mwx_vad_params params) {
  if (!vctx) return nullptr;
  mwx::VadSegParams prm;
  if (!mwx::vad_derive_params(params, prm)) return nullptr;
  mwx_vad_stream* s = new mwx_vad_stream();
  try {
    HIPC(hipSetDevice(vctx->device));
    s->slot = mwx::vad_slot_take(vctx);
  } catch (const std::exception&) {
    delete s;
    return nullptr;
  }
  s->ctx = vctx;
  s->prm = prm;
  vctx->streams.push_back(s);
  return s;
}

void mwx_vad_stream_free(struct mwx_vad_stream* s) {
  if (!s) return;
  if (mwx_vad_context* v = s->ctx) {  // every call has ended with a synchronization
    v->free_slots.push_back(s->slot);
    v->streams.erase(std::find(v->streams.begin(), v->streams.end(), s));
  }
  delete s;
}

int mwx_vad_stream_reset(struct mwx_vad_stream* s) {
  if (!s || !s->ctx) return -1;
  mwx::vad_stream_clear(s);  // the slot is read as new while the chunk count is 0
  return 0;
}

int mwx_vad_stream_feed_batch(struct mwx_vad_context* vctx, struct mwx_vad_stream* const* streams,
                              const float* const* samples, const int* n_samples, int n_streams) {
  if (!vctx || n_streams < 0) return -1;
  if (n_streams == 0) return 0;
  if (!streams || !samples || !n_samples) return -1;
  for (int i = 0; i < n_streams; ++i) {
    const mwx_vad_stream* s = streams[i];
    if (!s || s->ctx != vctx || s->finished) return -2;
    if (n_samples[i] < 0 || n_samples[i] > mwx::kStreamMaxFeed) return -2;
    if (n_samples[i] > 0 && !samples[i]) return -2;
  }
  std::vector<const mwx_vad_stream*> sorted(streams, streams + n_streams);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return -2;
  try {
    return mwx::vad_stream_call(vctx, streams, samples, n_samples, n_streams, nullptr);
  } catch (const std::exception&) {
    return -4;
  }
}

int mwx_vad_stream_finish(struct mwx_vad_stream* s) {
  if (!s || !s->ctx || s->finished) return -1;
  s->finished = true;
  if (s->trig && s->n_samples - s->start > s->prm.min_speech) {
    const int64_t e[3] = {s->start, s->n_samples, s->n_samples};
    s->seg.insert(s->seg.end(), e, e + 3);
  }
  s->trig = false;
  return 0;
}

int64_t mwx_vad_stream_n_samples(const struct mwx_vad_stream* s) { return s ? s->n_samples : 0; }
int mwx_vad_stream_n_probs(const struct mwx_vad_stream* s) { return s ? (int)s->probs.size() : 0; }
const float* mwx_vad_stream_probs(const struct mwx_vad_stream* s) {
  return s && !s->probs.empty() ? s->probs.data() : nullptr;
}
float mwx_vad_stream_max_prob(const struct mwx_vad_stream* s) {
  if (!s || s->probs.empty()) return 0.0f;
  return s->provisional ? std::max(s->max_whole, s->probs.back()) : s->max_whole;
}
int mwx_vad_stream_n_segments(const struct mwx_vad_stream* s) {
  return s ? (int)(s->seg.size() / 3) : 0;
}
int mwx_vad_stream_segment(const struct mwx_vad_stream* s, int i, int64_t* s0, int64_t* s1,
                           int64_t* closed_at) {
  if (!s || i < 0 || 3 * (size_t)i + 2 >= s->seg.size()) return -1;
  if (s0) *s0 = s->seg[3 * (size_t)i];
  if (s1) *s1 = s->seg[3 * (size_t)i + 1];
  if (closed_at) *closed_at = s->seg[3 * (size_t)i + 2];
  return 0;
}
bool mwx_vad_stream_in_speech(const struct mwx_vad_stream* s) { return s && s->trig; }

int mwx_vad_stream_last_kernel_ms(struct mwx_vad_context* vctx, float* stage_ms,
                                  float* frontend_ms, float* lstm_ms) {
  if (!vctx || !vctx->timed_stream) return -1;
  float a = 0.0f, b = 0.0f, c = 0.0f;
  if (hipEventElapsedTime(&a, vctx->ev[8], vctx->ev[9]) != hipSuccess ||
      hipEventElapsedTime(&b, vctx->ev[9], vctx->ev[10]) != hipSuccess ||
      hipEventElapsedTime(&c, vctx->ev[10], vctx->ev[11]) != hipSuccess)
    return -1;
  if (stage_ms) *stage_ms = a;
  if (frontend_ms) *frontend_ms = b;
  if (lstm_ms) *lstm_ms = c;
  return 0;
}

int mwx_test_vad_stream_scan(struct mwx_vad_context* vctx, const struct mwx_vad_params* params,
                             const float* probs, int n_probs, const int* splits, int n_splits,
                             int* n_events, int64_t* events, int64_t* state) {
  if (!vctx || !params || n_probs < 0 || (n_probs > 0 && !probs) || n_splits < 0 ||
      (n_splits > 0 && !splits) || !n_events || !events || !state)
    return -1;
  long sum = 0;
  for (int k = 0; k < n_splits; ++k) {
    if (splits[k] < 0 || splits[k] > 0x7fffffff / mwx::VAD_CHUNK) return -2;
    sum += splits[k];
  }
  if (sum != n_probs) return -2;
  mwx_vad_stream* s = mwx_vad_stream_init(vctx, *params);
  if (!s) return -2;
  int rc = 0;
  try {
    const float* p = probs;
    for (int k = 0; k < n_splits && rc == 0; ++k) {
      rc = mwx::vad_stream_call(vctx, &s, nullptr, &splits[k], 1, &p);
      p += splits[k];
    }
  } catch (const std::exception&) {
    rc = -4;
  }
  if (rc == 0 && s->seg.size() / 3 > (size_t)n_probs) rc = -5;
  if (rc == 0) {
    *n_events = (int)(s->seg.size() / 3);
    std::copy(s->seg.begin(), s->seg.end(), events);
    const int64_t st[6] = {s->trig ? 1 : 0, s->start, s->temp_end, s->prev_end, s->next_start,
                           s->n_chunks};
    std::copy(st, st + 6, state);
  }
  mwx_vad_stream_free(s);
  return rc;
}

// ---- synthetic writer -------------------------------------------------------
int mwx_write_synthetic_vad_model(const char* path, uint64_t seed) {
  using namespace mwx;
  if (!path) return -1;
  std::ofstream f(path, std::ios::binary);
  if (!f) {
    MWX_LOG_ERROR("mwx_write_synthetic_vad_model: cannot open '%s'\n", path);
    return -1;
  }
  auto put = [&](const void* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)n); };
  auto put32 = [&](int32_t v) { put(&v, 4); };
  put(&kGgmlMagic, 4);
  put32((int32_t)strlen(kVadType));
  put(kVadType, strlen(kVadType));
  put(kVadVersion, sizeof kVadVersion);
  put32(kLayers);
  put(kEncIn, sizeof kEncIn);
  put(kEncOut, sizeof kEncOut);
  put(kEncKernel, sizeof kEncKernel);
  put32(VAD_HID);  // lstm_input
  put32(VAD_HID);  // lstm_hidden
  put32(VAD_HID);  // final_conv_in
  put32(1);        // final_conv_out
  const double two_pi = 6.283185307179586476925286766559;
  for (const auto& s : vad_tensor_specs()) {
    put32((int32_t)s.shape.size());
    put32((int32_t)s.name.size());
    put32(s.type);
    for (int i = (int)s.shape.size() - 1; i >= 0; --i) put32((int32_t)s.shape[i]);
    put(s.name.data(), s.name.size());
    int64_t n = 1;
    for (auto d : s.shape) n *= d;
    const uint64_t key = fnv1a64(s.name) ^ seed;
    const float bound = s.gain / std::sqrt((float)s.fan_in);
    for (int64_t i = 0; i < n; ++i) {
      float v;
      if (s.gain == 0.0f) {
        // Hann-windowed DFT: rows k < 129 cos, the rest -sin; periodic window
        const int row = (int)(i / VAD_NFFT), t = (int)(i % VAD_NFFT);
        const int k = row % VAD_BINS;
        const double win = 0.5 - 0.5 * std::cos(two_pi * t / VAD_NFFT);
        const double ang = two_pi * (double)((k * t) % VAD_NFFT) / VAD_NFFT;
        v = (float)((row < VAD_BINS ? std::cos(ang) : -std::sin(ang)) * win);
      } else {
        const uint64_t r = splitmix64(key + (uint64_t)i * 0xD1B54A32D192ED03ull);
        const float u = (float)((double)(r >> 40) * (1.0 / 8388608.0) - 1.0);
        v = bound * u;
      }
      if (s.type == GGML_F32) {
        put(&v, 4);
      } else {
        const uint16_t h = f32_to_f16(v);
        put(&h, 2);
      }
    }
  }
  f.close();
  return f ? 0 : -1;
}

}  // extern "C"
