// Voice-activity detection on gfx950: a Silero-v5-shaped network (INTEGRATION.md,
// "VAD model") over 512-sample chunks of 16 kHz PCM, one speech probability per
// chunk. Replaces the whisper_vad_* calls behind SttEngine::is_speech_detected
// (src/stt_engine.cpp:108-115), which the reference runs on the CPU one clip
// at a time.
//
// Two kernels compute the probabilities:
//   vad_frontend_kernel — everything that does not depend on the LSTM state,
//     for every chunk of every clip of the call at once: reflect padding, the
//     STFT magnitude, four kernel-3 convolutions with ReLU and the LSTM input
//     projection W_ih x + b_ih + b_hh. A workgroup takes VAD_TILE consecutive
//     chunks of one clip so that each weight it loads is used for all of them;
//     the activations of the tile live in LDS.
//   vad_lstm_kernel — the 128-wide recurrence and the head, one workgroup per
//     clip: 512 threads, thread j keeps row j of W_hh in registers for the
//     whole clip, h is broadcast through LDS.
//
// Two more turn them into trimmed audio without leaving the device
// (DESIGN.md D7): vad_segments_kernel (one wave per clip: the segment rule over
// the probabilities, padding, the piece layout of the compacted clip) and
// vad_compact_kernel (gathers the pieces of every clip into one dense buffer).
//
// Three serve streams that are fed a piece at a time:
// vad_stream_stage_kernel, vad_lstm_stream_kernel (the same step with h and c
// carried in the stream's slot) and vad_stream_scan_kernel (the segment rule's
// scan, one chunk per step, with its registers carried too).
//
// All arithmetic is f32. Every output is one fixed chain of fmaf over its
// inputs in index order, so a chunk's result does not depend on its slot in a
// tile or on which other clips are in the launch: a batch gives the bits of
// the single calls.
#include "kcommon.h"
#include "kernels.h"

namespace mwx {

namespace {

constexpr int VAD_FE_THREADS = 256;
constexpr int VAD_XP = VAD_CHUNK + 2 * VAD_PAD;  // 640 padded samples
constexpr int VAD_ROWS = 2 * VAD_BINS;           // 258 basis rows
constexpr int VAD_FRAMES = 4;
// per-chunk LDS: A holds the raw STFT [258][4] (then conv1 / conv3 outputs),
// B the padded samples [640] (then magnitude [129][4], conv2 / conv4 outputs)
constexpr int VAD_LA = VAD_ROWS * VAD_FRAMES;  // 1032 floats
constexpr int VAD_LB = VAD_XP;                 // 640 floats

__device__ __forceinline__ float sigmoidf_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

// Kernel-3, zero-pad-1 convolution + bias + ReLU over the tile: in
// [chunk][CIN][FIN] (chunk stride in_cs) -> out [chunk][COUT][FOUT] (chunk
// stride out_cs), weights wt [(ci * 3 + k)][COUT]. Thread = one output channel
// of VAD_TILE / (256 / COUT) chunks; taps that fall into the padding are
// skipped at compile time.
template <int CIN, int COUT, int FIN, int FOUT, int STRIDE>
__device__ __forceinline__ void vad_conv(const float* __restrict__ wt, const float* __restrict__ bias,
                                         const float* in, int in_cs, float* out, int out_cs) {
  constexpr int G = VAD_FE_THREADS / COUT;  // chunk groups
  constexpr int CPG = VAD_TILE / G;         // chunks per thread
  static_assert(G * COUT == VAD_FE_THREADS && CPG * G == VAD_TILE, "tile split");
  const int o = threadIdx.x % COUT, c0 = (threadIdx.x / COUT) * CPG;
  float acc[CPG][FOUT];
#pragma unroll
  for (int c = 0; c < CPG; ++c)
#pragma unroll
    for (int f = 0; f < FOUT; ++f) acc[c][f] = 0.0f;
  for (int ci = 0; ci < CIN; ++ci) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float w = wt[(ci * 3 + k) * COUT + o];
#pragma unroll
      for (int c = 0; c < CPG; ++c)
#pragma unroll
        for (int f = 0; f < FOUT; ++f) {
          const int pos = f * STRIDE + k - 1;
          if (pos >= 0 && pos < FIN)
            acc[c][f] = fmaf(w, in[(c0 + c) * in_cs + ci * FIN + pos], acc[c][f]);
        }
    }
  }
  const float b = bias[o];
#pragma unroll
  for (int c = 0; c < CPG; ++c)
#pragma unroll
    for (int f = 0; f < FOUT; ++f)
      out[(c0 + c) * out_cs + o * FOUT + f] = fmaxf(acc[c][f] + b, 0.0f);
}

}  // namespace

// grid.x = n_clips * tiles (tiles = ceil(max_chunks / VAD_TILE)); workgroup
// (clip b, tile x) handles chunks [x * VAD_TILE, ...) of clip b and leaves at
// once when the clip has fewer. Chunks of the tile past the clip's last are
// computed on zeros and not stored.
__global__ __launch_bounds__(VAD_FE_THREADS) void vad_frontend_kernel(
    VadWeights W, const float* const* __restrict__ pcm, const int* __restrict__ n_samples,
    const int* __restrict__ chunk_off, int n_clips, int tiles, float* __restrict__ pre) {
  __shared__ __attribute__((aligned(16))) float sA[VAD_TILE * VAD_LA];
  __shared__ __attribute__((aligned(16))) float sB[VAD_TILE * VAD_LB];
  const int b = blockIdx.x / tiles;
  const int n0 = (blockIdx.x % tiles) * VAD_TILE;
  if (b >= n_clips) return;
  const int off = chunk_off[b];
  const int nch = chunk_off[b + 1] - off;  // chunks of this clip
  if (n0 >= nch) return;
  const int t = threadIdx.x;

  // padded samples: chunk-local index s in [-64, 576) reflects about 0 and 511
  // (edge not repeated); samples past the clip's end are zero
  {
    const float* __restrict__ x = pcm[b];
    const long ns = n_samples[b];
    for (int idx = t; idx < VAD_TILE * VAD_XP; idx += VAD_FE_THREADS) {
      const int c = idx / VAD_XP, p = idx % VAD_XP;
      int s = p - VAD_PAD;
      if (s < 0) s = -s;
      if (s >= VAD_CHUNK) s = 2 * (VAD_CHUNK - 1) - s;
      const long gi = (long)(n0 + c) * VAD_CHUNK + s;
      sB[c * VAD_LB + p] = (n0 + c < nch && gi < ns) ? x[gi] : 0.0f;
    }
  }
  __syncthreads();

  // STFT: raw[c][row][f] = sum_tap basis[row][tap] * x[c][128 f + tap].
  // Thread t takes row t for the whole tile; rows 256, 257 are split by
  // (row, chunk, frame) over 64 threads afterwards (the same chain per output).
  {
    float acc[VAD_TILE][VAD_FRAMES];
#pragma unroll
    for (int c = 0; c < VAD_TILE; ++c)
#pragma unroll
      for (int f = 0; f < VAD_FRAMES; ++f) acc[c][f] = 0.0f;
    for (int tap = 0; tap < VAD_NFFT; tap += 4) {
      float w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) w[u] = W.basis_t[(tap + u) * VAD_ROWS + t];
#pragma unroll
      for (int c = 0; c < VAD_TILE; ++c)
#pragma unroll
        for (int f = 0; f < VAD_FRAMES; ++f) {
          const float4 xv = *reinterpret_cast<const float4*>(&sB[c * VAD_LB + 128 * f + tap]);
          float a = acc[c][f];
          a = fmaf(w[0], xv.x, a);
          a = fmaf(w[1], xv.y, a);
          a = fmaf(w[2], xv.z, a);
          a = fmaf(w[3], xv.w, a);
          acc[c][f] = a;
        }
    }
#pragma unroll
    for (int c = 0; c < VAD_TILE; ++c)
      *reinterpret_cast<float4*>(&sA[c * VAD_LA + t * VAD_FRAMES]) =
          make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
    if (t < (VAD_ROWS - VAD_FE_THREADS) * VAD_TILE * VAD_FRAMES) {
      const int row = VAD_FE_THREADS + t / (VAD_TILE * VAD_FRAMES);
      const int c = (t / VAD_FRAMES) % VAD_TILE, f = t % VAD_FRAMES;
      float a = 0.0f;
      for (int tap = 0; tap < VAD_NFFT; ++tap)
        a = fmaf(W.basis_t[tap * VAD_ROWS + row], sB[c * VAD_LB + 128 * f + tap], a);
      sA[c * VAD_LA + row * VAD_FRAMES + f] = a;
    }
  }
  __syncthreads();

  // magnitude [c][bin][f] -> B
  for (int idx = t; idx < VAD_TILE * VAD_BINS * VAD_FRAMES; idx += VAD_FE_THREADS) {
    const int c = idx / (VAD_BINS * VAD_FRAMES), r = idx % (VAD_BINS * VAD_FRAMES);
    const float re = sA[c * VAD_LA + r], im = sA[c * VAD_LA + VAD_BINS * VAD_FRAMES + r];
    sB[c * VAD_LB + r] = sqrtf(re * re + im * im);
  }
  __syncthreads();

  // encoder: 129 -> 128 (s1), 128 -> 64 (s2), 64 -> 64 (s2), 64 -> 128 (s1);
  // frames 4 -> 4 -> 2 -> 1 -> 1
  vad_conv<129, 128, 4, 4, 1>(W.conv_t[0], W.conv_b[0], sB, VAD_LB, sA, VAD_LA);
  __syncthreads();
  vad_conv<128, 64, 4, 2, 2>(W.conv_t[1], W.conv_b[1], sA, VAD_LA, sB, VAD_LB);
  __syncthreads();
  vad_conv<64, 64, 2, 1, 2>(W.conv_t[2], W.conv_b[2], sB, VAD_LB, sA, VAD_LA);
  __syncthreads();
  vad_conv<64, 128, 1, 1, 1>(W.conv_t[3], W.conv_b[3], sA, VAD_LA, sB, VAD_LB);
  __syncthreads();

  // LSTM input projection: pre[chunk][j] = W_ih[j] . x + b_ih[j] + b_hh[j]
  for (int j = t; j < VAD_GATES; j += VAD_FE_THREADS) {
    float acc[VAD_TILE];
#pragma unroll
    for (int c = 0; c < VAD_TILE; ++c) acc[c] = 0.0f;
    for (int i = 0; i < VAD_HID; ++i) {
      const float w = W.wih_t[i * VAD_GATES + j];
#pragma unroll
      for (int c = 0; c < VAD_TILE; ++c) acc[c] = fmaf(w, sB[c * VAD_LB + i], acc[c]);
    }
    const float bi = W.b_ih[j], bh = W.b_hh[j];
#pragma unroll
    for (int c = 0; c < VAD_TILE; ++c)
      if (n0 + c < nch) pre[(size_t)(off + n0 + c) * VAD_GATES + j] = (acc[c] + bi) + bh;
  }
}

// One step of the recurrence, shared by vad_lstm_kernel and
// vad_lstm_stream_kernel: every thread adds its W_hh row . h to its
// pre-activation `cur` and posts the gate in LDS; after the barrier threads
// 0..127 (waves 0, 1) update c and h for their unit, publish h and reduce
// w_f . relu(h) into sp; the second barrier ends the step. The probability is
// sigmoid((sp[0] + sp[1]) + b_f).
__device__ __forceinline__ void vad_lstm_step(const float (&w)[VAD_HID], float cur, float wf, int j,
                                              float& c, float& h, float* sh, float* sg,
                                              float* sp) {
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
  for (int q = 0; q < VAD_HID / 4; ++q) {
    const float4 hv = *reinterpret_cast<const float4*>(&sh[4 * q]);
    a0 = fmaf(w[4 * q + 0], hv.x, a0);
    a1 = fmaf(w[4 * q + 1], hv.y, a1);
    a2 = fmaf(w[4 * q + 2], hv.z, a2);
    a3 = fmaf(w[4 * q + 3], hv.w, a3);
  }
  sg[j] = cur + ((a0 + a1) + (a2 + a3));
  __syncthreads();  // gates posted; every read of h for this step is done
  if (j < VAD_HID) {
    const float gi = sigmoidf_acc(sg[j]);
    const float gf = sigmoidf_acc(sg[VAD_HID + j]);
    const float gg = tanhf(sg[2 * VAD_HID + j]);
    const float go = sigmoidf_acc(sg[3 * VAD_HID + j]);
    c = gf * c + gi * gg;
    h = go * tanhf(c);
    sh[j] = h;
    const float part = wave_sum(wf * fmaxf(h, 0.0f));
    if ((j & 63) == 0) sp[j >> 6] = part;
  }
  __syncthreads();  // h and the head's two partial sums posted
}

// One workgroup per clip: 512 threads, thread j keeps row j of W_hh in
// registers for the whole clip; thread 0 writes each step's probability.
__global__ __launch_bounds__(VAD_GATES) void vad_lstm_kernel(
    const float* __restrict__ whh_t, const float* __restrict__ w_f, float b_f,
    const float* __restrict__ pre, const int* __restrict__ chunk_off, int n_clips,
    float* __restrict__ probs) {
  __shared__ __attribute__((aligned(16))) float sh[VAD_HID];
  __shared__ float sg[VAD_GATES];
  __shared__ float sp[2];
  const int b = blockIdx.x;
  if (b >= n_clips) return;
  const int off = chunk_off[b];
  const int nch = chunk_off[b + 1] - off;
  if (nch <= 0) return;
  const int j = threadIdx.x;
  float w[VAD_HID];
#pragma unroll
  for (int k = 0; k < VAD_HID; ++k) w[k] = whh_t[k * VAD_GATES + j];
  const float wf = j < VAD_HID ? w_f[j] : 0.0f;
  float c = 0.0f, h = 0.0f;
  if (j < VAD_HID) sh[j] = 0.0f;
  __syncthreads();
  const float* __restrict__ pj = pre + (size_t)off * VAD_GATES + j;
  float nxt = pj[0];
  for (int s = 0; s < nch; ++s) {
    const float cur = nxt;
    if (s + 1 < nch) nxt = pj[(size_t)(s + 1) * VAD_GATES];
    vad_lstm_step(w, cur, wf, j, c, h, sh, sg, sp);
    if (j == 0) probs[(size_t)off + s] = sigmoidf_acc((sp[0] + sp[1]) + b_f);
  }
}

// ---- streaming ------------------------------------------------------------------
// A stream is fed a piece at a time and keeps what crosses a chunk boundary in
// its VadStreamSlot: h and c of the recurrence, the samples that do not fill a
// chunk yet, the chunk count and the registers of the segment scan. One call
// (VadStreamFeed per stream) runs three kernels of this section around the
// unchanged vad_frontend_kernel.

// Lays [tail | new samples] of every stream out as whole 512-sample chunks in
// `stage` (stream b's at stage + 512 chunk_off[b]); a remainder makes one more,
// provisional chunk that is zero-filled past the last sample. The samples of
// the remainder become the new tail, written to the other of the slot's two
// tail buffers: other workgroups of this launch still read the old one.
// grid.x = n_streams * tiles, tiles = ceil(512 max_chunks / VAD_ST_TILE).
constexpr int VAD_ST_THREADS = 256;
constexpr int VAD_ST_TILE = 2048;

__global__ __launch_bounds__(VAD_ST_THREADS) void vad_stream_stage_kernel(
    const VadStreamFeed* __restrict__ feeds, const int* __restrict__ chunk_off, int n_streams,
    int tiles, float* __restrict__ stage) {
  const int b = blockIdx.x / tiles;
  if (b >= n_streams) return;
  const int off = chunk_off[b];
  const int len = (chunk_off[b + 1] - off) * VAD_CHUNK;  // staged samples, zeros included
  const int x0 = (blockIdx.x % tiles) * VAD_ST_TILE;
  if (x0 >= len) return;
  const VadStreamFeed F = feeds[b];
  const int total = F.tail_n + F.n_new;
  const int keep0 = F.n_full * VAD_CHUNK;  // first sample of the new tail
  const float* __restrict__ old_tail = F.slot->tail[F.par];
  float* __restrict__ new_tail = F.slot->tail[F.par ^ 1];
  const float* __restrict__ src = F.src;
  float* __restrict__ out = stage + (size_t)off * VAD_CHUNK;
  const int x1 = min(len, x0 + VAD_ST_TILE);
  for (int p = x0 + (int)threadIdx.x; p < x1; p += VAD_ST_THREADS) {
    float v = 0.0f;
    if (p < F.tail_n)
      v = old_tail[p];
    else if (p < total)
      v = src[p - F.tail_n];
    out[p] = v;
    if (p >= keep0 && p < total) new_tail[p - keep0] = v;
  }
}

// vad_lstm_kernel's step over the staged chunks of every stream, one workgroup
// per stream: h and c come from the slot (zeros for a stream that has no
// committed chunk yet) and go back to it after the last whole chunk; the step
// of a provisional chunk runs from there and leaves only its probability.
__global__ __launch_bounds__(VAD_GATES) void vad_lstm_stream_kernel(
    const float* __restrict__ whh_t, const float* __restrict__ w_f, float b_f,
    const float* __restrict__ pre, const VadStreamFeed* __restrict__ feeds,
    const int* __restrict__ chunk_off, int n_streams, float* __restrict__ probs) {
  __shared__ __attribute__((aligned(16))) float sh[VAD_HID];
  __shared__ float sg[VAD_GATES];
  __shared__ float sp[2];
  const int b = blockIdx.x;
  if (b >= n_streams) return;
  const int off = chunk_off[b];
  const int nch = chunk_off[b + 1] - off;
  if (nch <= 0) return;
  VadStreamSlot* __restrict__ slot = feeds[b].slot;
  const bool fresh = feeds[b].fresh != 0;
  const int n_full = feeds[b].n_full;
  const int j = threadIdx.x;
  float w[VAD_HID];
#pragma unroll
  for (int k = 0; k < VAD_HID; ++k) w[k] = whh_t[k * VAD_GATES + j];
  const float wf = j < VAD_HID ? w_f[j] : 0.0f;
  float c = 0.0f, h = 0.0f;
  if (j < VAD_HID) {
    sh[j] = fresh ? 0.0f : slot->h[j];
    c = fresh ? 0.0f : slot->c[j];
  }
  __syncthreads();
  const float* __restrict__ pj = pre + (size_t)off * VAD_GATES + j;
  float nxt = pj[0];
  for (int s = 0; s < nch; ++s) {
    const float cur = nxt;
    if (s + 1 < nch) nxt = pj[(size_t)(s + 1) * VAD_GATES];
    vad_lstm_step(w, cur, wf, j, c, h, sh, sg, sp);
    if (j == 0) probs[(size_t)off + s] = sigmoidf_acc((sp[0] + sp[1]) + b_f);
    if (s == n_full - 1 && j < VAD_HID) {
      slot->h[j] = h;
      slot->c[j] = c;
    }
  }
}

// The loop body of vad_segments_kernel's scan (rule D7), one chunk per step,
// over the whole chunks a call added, with the scan's registers kept in the
// slot between calls: one wave per stream, masks and walk as in that kernel.
// A segment the scan closes is appended raw (no padding: that looks ahead) as
// (start, end, closed_at), closed_at = the end of the chunk whose step closed
// it; a step closes at most one. Lane 0 stores. out: per stream a header of
// VAD_STREAM_HDR int64 (event count, trig, start, temp_end, prev_end,
// next_start, chunk count), then stream b's events at
// out + VAD_STREAM_HDR n_streams + 3 chunk_off[b].
__global__ __launch_bounds__(64) void vad_stream_scan_kernel(
    const float* __restrict__ probs, const VadStreamFeed* __restrict__ feeds,
    const int* __restrict__ chunk_off, int n_streams, long long* __restrict__ out) {
  const int b = blockIdx.x;
  if (b >= n_streams) return;
  const int lane = threadIdx.x;
  const int off = chunk_off[b];
  const VadStreamFeed F = feeds[b];
  const int nch = min(F.n_full, chunk_off[b + 1] - off);  // the provisional chunk is not scanned
  const VadSegParams P = F.prm;
  VadStreamSlot* __restrict__ slot = F.slot;
  long long* __restrict__ hdr = out + (size_t)VAD_STREAM_HDR * b;
  long long* __restrict__ ev = out + (size_t)VAD_STREAM_HDR * n_streams + 3 * (size_t)off;

  bool trig = false;
  long long start = 0, temp_end = 0, prev_end = 0, next_start = 0, chunk0 = 0;
  if (!F.fresh) {
    trig = slot->trig != 0;
    start = slot->start;
    temp_end = slot->temp_end;
    prev_end = slot->prev_end;
    next_start = slot->next_start;
    chunk0 = slot->n_chunks;
  }
  int m = 0;
  long long closed_at = 0;
  auto emit = [&](long long s, long long e) {
    if (lane == 0 && m < nch) {
      ev[3 * m] = s;
      ev[3 * m + 1] = e;
      ev[3 * m + 2] = closed_at;
    }
    ++m;
  };
  const float* __restrict__ p = probs + off;
  float nxt = lane < nch ? p[lane] : 0.0f;
  for (int base = 0; base < nch; base += 64) {
    const float v = nxt;
    const bool valid = base + lane < nch;
    if (base + 64 + lane < nch) nxt = p[base + 64 + lane];
    const unsigned long long ms = __ballot(valid && v >= P.thr);
    const unsigned long long ml = __ballot(valid && v < P.neg);
    const int cnt = min(64, nch - base);
    for (int j = 0; j < cnt; ++j) {
      const bool sp = (ms >> j) & 1, sl = (ml >> j) & 1;
      const long long cur = (long long)VAD_CHUNK * (chunk0 + base + j);
      closed_at = cur + VAD_CHUNK;
      if (sp && temp_end != 0) {
        temp_end = 0;
        if (next_start < prev_end) next_start = cur;
      }
      if (sp && !trig) {
        trig = true;
        start = cur;
        continue;
      }
      if (trig && cur - start > P.max_speech) {
        if (prev_end > 0) {
          emit(start, prev_end);
          if (next_start < prev_end)
            trig = false;
          else
            start = next_start;
          prev_end = next_start = temp_end = 0;
        } else {
          emit(start, cur);
          prev_end = next_start = temp_end = 0;
          trig = false;
          continue;
        }
      }
      if (sl && trig) {
        if (temp_end == 0) temp_end = cur;
        if (cur - temp_end > VAD_SIL_AT_MAX) prev_end = temp_end;
        if (cur - temp_end < P.min_sil) continue;
        if (temp_end - start > P.min_speech) emit(start, temp_end);
        prev_end = next_start = temp_end = 0;
        trig = false;
      }
    }
  }
  if (lane == 0) {
    const long long n_chunks = chunk0 + nch;
    slot->trig = trig ? 1 : 0;
    slot->start = start;
    slot->temp_end = temp_end;
    slot->prev_end = prev_end;
    slot->next_start = next_start;
    slot->n_chunks = n_chunks;
    hdr[0] = min(m, nch);
    hdr[1] = trig ? 1 : 0;
    hdr[2] = start;
    hdr[3] = temp_end;
    hdr[4] = prev_end;
    hdr[5] = next_start;
    hdr[6] = n_chunks;
    hdr[7] = 0;
  }
}

// ---- speech segments ----------------------------------------------------------
// One wave per clip. The scan is a serial state machine, so it runs in
// wave-uniform code: each step loads 64 probabilities (one per lane), turns
// them into two ballot masks (speech: p >= thr, silence: p < neg; a lane past
// the clip's end sets neither) and walks the masks bit by bit with the state
// in scalar registers. A segment is final once its successor is known (the
// padding rule moves only e_k and s_{k+1}), so padding and the piece layout
// are done on the fly with one pending segment; lane 0 stores the results.
__global__ __launch_bounds__(64) void vad_segments_kernel(
    const float* __restrict__ probs, const int* __restrict__ n_samples,
    const int* __restrict__ chunk_off, int n_clips, const VadSegParams* __restrict__ prm,
    int prm_stride, long long* __restrict__ tables) {
  const int b = blockIdx.x;
  if (b >= n_clips) return;
  const int lane = threadIdx.x;
  const int off = chunk_off[b];
  const int nch = chunk_off[b + 1] - off;
  const long long N = n_samples[b];
  const VadSegParams P = prm[(size_t)b * prm_stride];
  const int cap = nch + 1;
  long long* __restrict__ T = tables + vad_table_off(off, b);
  long long* __restrict__ seg = T + 2;
  long long* __restrict__ pc = T + 2 + 2LL * cap;

  int m = 0;            // final segments written
  bool have = false;    // one emitted segment whose end is not final yet
  long long ps = 0, pe = 0;
  long long c = 0;      // compacted position of the pending segment's piece
  auto put = [&](long long s, long long e, long long len) {
    if (lane == 0 && m < cap) {
      seg[2 * m] = s;
      seg[2 * m + 1] = e;
      pc[3 * m] = s;
      pc[3 * m + 1] = len;
      pc[3 * m + 2] = c;
    }
    ++m;
  };
  auto emit = [&](long long s, long long e) {
    if (have) {
      const long long gap = s - pe;
      if (gap < 2 * P.pad) {
        pe += gap >> 1;
        s = max(0LL, s - (gap >> 1));
      } else {
        pe = min(N, pe + P.pad);
        s = max(0LL, s - P.pad);
      }
      const long long end = min(pe + P.ov, s);
      put(ps, pe, end - ps);
      c += (end - ps) + (end == s ? 0 : VAD_GAP);
    } else {
      s = max(0LL, s - P.pad);
    }
    have = true;
    ps = s;
    pe = e;
  };

  bool trig = false;
  long long start = 0, temp_end = 0, prev_end = 0, next_start = 0;
  const float* __restrict__ p = probs + off;
  float nxt = lane < nch ? p[lane] : 0.0f;
  for (int base = 0; base < nch; base += 64) {
    const float v = nxt;
    const bool valid = base + lane < nch;
    if (base + 64 + lane < nch) nxt = p[base + 64 + lane];
    const unsigned long long ms = __ballot(valid && v >= P.thr);
    const unsigned long long ml = __ballot(valid && v < P.neg);
    const int cnt = min(64, nch - base);
    for (int j = 0; j < cnt; ++j) {
      const bool sp = (ms >> j) & 1, sl = (ml >> j) & 1;
      const long long cur = (long long)VAD_CHUNK * (base + j);
      if (sp && temp_end != 0) {
        temp_end = 0;
        if (next_start < prev_end) next_start = cur;
      }
      if (sp && !trig) {
        trig = true;
        start = cur;
        continue;
      }
      if (trig && cur - start > P.max_speech) {
        if (prev_end > 0) {
          emit(start, prev_end);
          if (next_start < prev_end)
            trig = false;
          else
            start = next_start;
          prev_end = next_start = temp_end = 0;
        } else {
          emit(start, cur);
          prev_end = next_start = temp_end = 0;
          trig = false;
          continue;
        }
      }
      if (sl && trig) {
        if (temp_end == 0) temp_end = cur;
        if (cur - temp_end > VAD_SIL_AT_MAX) prev_end = temp_end;
        if (cur - temp_end < P.min_sil) continue;
        if (temp_end - start > P.min_speech) emit(start, temp_end);
        prev_end = next_start = temp_end = 0;
        trig = false;
      }
    }
  }
  if (trig && N - start > P.min_speech) emit(start, N);
  if (have) {
    pe = min(N, pe + P.pad);
    put(ps, pe, pe - ps);
    c += pe - ps;
  }
  if (lane == 0) {
    T[0] = min(m, cap);
    T[1] = c;
  }
}

// ---- chunk plan ---------------------------------------------------------------
// One wave per clip, over the piece table vad_segments_kernel left (DESIGN.md
// D10). The walk over chunk starts is serial and wave-uniform; the search for
// the first piece that does not fit is one piece per lane, 64 pieces a round:
// piece k > a fits chunk a while dst_k + len_k - dst_a <= L. Lane 0 stores.
__global__ __launch_bounds__(64) void vad_chunks_kernel(
    const int* __restrict__ chunk_off, int n_clips, const long long* __restrict__ tables,
    const long long* __restrict__ caps, int cap_stride, long long* __restrict__ ctabs) {
  const int b = blockIdx.x;
  if (b >= n_clips) return;
  const int lane = threadIdx.x;
  const int off = chunk_off[b];
  const int cap = chunk_off[b + 1] - off + 1;
  const long long* __restrict__ T = tables + vad_table_off(off, b);
  const int m = (int)max(0LL, min(T[0], (long long)cap));
  const long long* __restrict__ pc = T + 2 + 2LL * cap;
  const long long L = caps[(size_t)b * cap_stride];
  long long* __restrict__ X = ctabs + vad_chunk_table_off(off, b);
  int nc = 0;
  int a = 0;
  while (a < m) {
    const long long c0 = pc[3 * a + 2];
    int nxt = m;
    for (int base = a + 1; base < m; base += 64) {
      const int k = base + lane;
      const bool over = k < m && pc[3 * k + 2] + pc[3 * k + 1] - c0 > L;
      const unsigned long long mo = __ballot(over);
      if (mo != 0) {
        // the pieces of this round that still fit: those below the first that does not
        nxt = base + __popcll((mo & (0ULL - mo)) - 1);
        break;
      }
    }
    if (lane == 0 && nc < cap) {
      X[1 + 2 * nc] = a;
      X[2 + 2 * nc] = nxt - a;
    }
    ++nc;
    a = nxt;
  }
  if (lane == 0) X[0] = min(nc, cap);
}

// ---- compaction ---------------------------------------------------------------
// grid.x = n_clips * tiles (tiles = ceil(max_len / VAD_CP_TILE)); workgroup
// (clip b, tile x) writes compacted samples [x * VAD_CP_TILE, ...) of clip b
// and leaves at once when the clip is shorter. It finds the piece of its first
// sample by binary search over dst and moves on piece by piece from there;
// a position past its piece's len lies in the gap and gets a zero. Loads and
// stores are one dword per lane, consecutive lanes consecutive samples: the
// sources have any 4-byte alignment.
constexpr int VAD_CP_THREADS = 256;

__global__ __launch_bounds__(VAD_CP_THREADS) void vad_compact_kernel(
    const float* const* __restrict__ pcm, const int* __restrict__ n_samples,
    const int* __restrict__ chunk_off, int n_clips, int tiles,
    const long long* __restrict__ tables, const long long* __restrict__ out_off,
    float* __restrict__ out) {
  const int b = blockIdx.x / tiles;
  if (b >= n_clips) return;
  const int off = chunk_off[b];
  const int cap = chunk_off[b + 1] - off + 1;
  const long long* __restrict__ T = tables + vad_table_off(off, b);
  const int m = (int)T[0];
  const long long clen = T[1];
  const long long o0 = (long long)(blockIdx.x % tiles) * VAD_CP_TILE;
  if (m <= 0 || o0 >= clen) return;
  const long long o1 = min(clen, o0 + VAD_CP_TILE);
  const long long* __restrict__ pc = T + 2 + 2LL * cap;
  int lo = 0, hi = m - 1;  // the last piece with dst <= o0 (dst_0 = 0)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pc[3 * mid + 2] <= o0)
      lo = mid;
    else
      hi = mid - 1;
  }
  int k = lo;
  const float* __restrict__ src = pcm[b];
  const long long N = n_samples[b];
  float* __restrict__ dst = out + out_off[b];
  long long ks = pc[3 * k], kl = pc[3 * k + 1], kd = pc[3 * k + 2];
  long long nd = k + 1 < m ? pc[3 * (k + 1) + 2] : clen;
  for (long long x = o0 + threadIdx.x; x < o1; x += VAD_CP_THREADS) {
    while (x >= nd && k + 1 < m) {
      ++k;
      ks = pc[3 * k];
      kl = pc[3 * k + 1];
      kd = pc[3 * k + 2];
      nd = k + 1 < m ? pc[3 * (k + 1) + 2] : clen;
    }
    const long long r = x - kd;
    dst[x] = (r < kl && ks + r < N) ? src[ks + r] : 0.0f;
  }
}

void vad_frontend_launch(const VadWeights& w, const float* const* pcm, const int* n_samples,
                         const int* chunk_off, int n_clips, int max_chunks, float* pre,
                         hipStream_t st) {
  if (n_clips <= 0 || max_chunks <= 0) return;
  const int tiles = (max_chunks + VAD_TILE - 1) / VAD_TILE;
  vad_frontend_kernel<<<(unsigned)((long)n_clips * tiles), VAD_FE_THREADS, 0, st>>>(
      w, pcm, n_samples, chunk_off, n_clips, tiles, pre);
}

void vad_lstm_launch(const VadWeights& w, const float* pre, const int* chunk_off, int n_clips,
                     float* probs, hipStream_t st) {
  if (n_clips <= 0) return;
  vad_lstm_kernel<<<n_clips, VAD_GATES, 0, st>>>(w.whh_t, w.w_f, w.b_f, pre, chunk_off, n_clips,
                                                 probs);
}

void vad_stream_stage_launch(const VadStreamFeed* feeds, const int* chunk_off, int n_streams,
                             int max_chunks, float* stage, hipStream_t st) {
  if (n_streams <= 0 || max_chunks <= 0) return;
  const long tiles = ((long)max_chunks * VAD_CHUNK + VAD_ST_TILE - 1) / VAD_ST_TILE;
  vad_stream_stage_kernel<<<(unsigned)(tiles * n_streams), VAD_ST_THREADS, 0, st>>>(
      feeds, chunk_off, n_streams, (int)tiles, stage);
}

void vad_lstm_stream_launch(const VadWeights& w, const float* pre, const VadStreamFeed* feeds,
                            const int* chunk_off, int n_streams, float* probs, hipStream_t st) {
  if (n_streams <= 0) return;
  vad_lstm_stream_kernel<<<n_streams, VAD_GATES, 0, st>>>(w.whh_t, w.w_f, w.b_f, pre, feeds,
                                                          chunk_off, n_streams, probs);
}

void vad_stream_scan_launch(const float* probs, const VadStreamFeed* feeds, const int* chunk_off,
                            int n_streams, long long* out, hipStream_t st) {
  if (n_streams <= 0) return;
  vad_stream_scan_kernel<<<n_streams, 64, 0, st>>>(probs, feeds, chunk_off, n_streams, out);
}

void vad_segments_launch(const float* probs, const int* n_samples, const int* chunk_off,
                         int n_clips, const VadSegParams* prm, int prm_stride, long long* tables,
                         hipStream_t st) {
  if (n_clips <= 0) return;
  vad_segments_kernel<<<n_clips, 64, 0, st>>>(probs, n_samples, chunk_off, n_clips, prm,
                                              prm_stride, tables);
}

void vad_chunks_launch(const int* chunk_off, int n_clips, const long long* tables,
                       const long long* caps, int cap_stride, long long* ctabs, hipStream_t st) {
  if (n_clips <= 0) return;
  vad_chunks_kernel<<<n_clips, 64, 0, st>>>(chunk_off, n_clips, tables, caps, cap_stride, ctabs);
}

void vad_compact_launch(const float* const* pcm, const int* n_samples, const int* chunk_off,
                        int n_clips, const long long* tables, const long long* out_off,
                        long long max_len, float* out, hipStream_t st) {
  if (n_clips <= 0 || max_len <= 0) return;
  const long long tiles = (max_len + VAD_CP_TILE - 1) / VAD_CP_TILE;
  vad_compact_kernel<<<(unsigned)(tiles * n_clips), VAD_CP_THREADS, 0, st>>>(
      pcm, n_samples, chunk_off, n_clips, (int)tiles, tables, out_off, out);
}

}  // namespace mwx
