// Contextual biasing for gfx950: x'[t] = x[t] + bias[t] on the
// raw logits of the rows that sample this step, between the logits GEMM and
// logits_process.
//
// One 256-thread workgroup per row. The row's matcher state (RowCtl.pad[0],
// bias.h) names a trie node; its matches are the nodes on the node's failure
// chain (at most 17, the root last), and a node's edges are its (token, boost)
// entries, sorted by token. Thread 0 walks the chain into LDS; then the
// workgroup strides over every chain node's edges. The thread that holds edge
// (node i, token t) looks t up (binary search) in the other chain nodes: if a
// deeper node (j < i) also lists t, that node's thread owns t and this one
// does nothing; otherwise it takes the maximum boost over the shallower nodes
// that list t and does the one float add. So each (row, token) is written by
// exactly one thread, with no atomics and no pass over the vocabulary: the work
// is the tens of entries of the row's state plus the root's list. Rows with
// active == 0 or sample == 0, and every entry no match points at, keep their
// bits. A row's result involves no other row and no launch dimension.
//
// Latency-bound (a few dependent table reads, tables L2-resident): the launch
// is R small workgroups and adds one graph node to a biased call's step.
#include "bias.h"
#include "kcommon.h"
#include "kernels.h"

namespace mwx {

constexpr int LB_T = 256;

__global__ __launch_bounds__(LB_T) void logits_bias_kernel(float* __restrict__ logits,
                                                           const RowCtl* __restrict__ ctl,
                                                           const int* __restrict__ tables, int V) {
  __shared__ int s_chain[kBiasMaxChain];
  __shared__ int s_n;
  const int row = blockIdx.x;
  const RowCtl c = ctl[row];
  if (!c.active || !c.sample) return;  // (workgroup-uniform)
  const BiasView v = bias_view(tables);
  if (threadIdx.x == 0) {
    int s = c.pad[0];
    if (s < 0 || s >= v.S) s = 0;
    int n = 0;
    for (;;) {
      s_chain[n++] = s;
      if (s == 0 || n == kBiasMaxChain) break;
      s = v.fail[s];
    }
    s_n = n;
  }
  __syncthreads();
  const int n = s_n;
  float* x = logits + (long)row * V;
  for (int i = 0; i < n; ++i) {
    const int u = s_chain[i];
    const int e1 = v.off[u + 1];
    for (int e = v.off[u] + (int)threadIdx.x; e < e1; e += LB_T) {
      const int t = v.etok[e];
      if (t < 0 || t >= V) continue;
      bool owner = true;
      for (int j = 0; j < i && owner; ++j) owner = bias_find(v, s_chain[j], t) < 0;
      if (!owner) continue;
      float b = v.eboost[e];
      for (int j = i + 1; j < n; ++j) {
        const int f = bias_find(v, s_chain[j], t);
        if (f >= 0) b = fmaxf(b, v.eboost[f]);
      }
      x[t] = x[t] + b;
    }
  }
}

bool logits_bias(float* logits, const RowCtl* ctl, const int* tables, int R, int V,
                 hipStream_t st) {
  if (!logits || !ctl || !tables || R < 1 || V < 1) return false;
  logits_bias_kernel<<<R, LB_T, 0, st>>>(logits, ctl, tables, V);
  return true;
}

// (test hook) every row's state after its history, from the root, with the
// transition the advance kernels use; written to state[r] and ctl[r].pad[0]
__global__ __launch_bounds__(64) void bias_walk_kernel(const int* __restrict__ tables,
                                                       const int* __restrict__ hist,
                                                       const int* __restrict__ hist_len, int H,
                                                       int R, RowCtl* __restrict__ ctl,
                                                       int* __restrict__ state) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  int s = 0;
  const int n = min(max(hist_len[r], 0), H);
  for (int i = 0; i < n; ++i) s = bias_next_state(tables, s, hist[(long)r * H + i]);
  ctl[r].pad[0] = s;
  state[r] = s;
}
void bias_walk_rows(const int* tables, const int* hist, const int* hist_len, int H, int R,
                    RowCtl* ctl, int* state, hipStream_t st) {
  bias_walk_kernel<<<(R + 63) / 64, 64, 0, st>>>(tables, hist, hist_len, H, R, ctl, state);
}

}  // namespace mwx
