// Transcript scoring for gfx950 ("Transcript alignment and
// scoring"): per row of raw f32 logits x[V] and a target id t,
//   plog = x[t] - logsumexp(x), p = expf(plog),
//   top_id = argmax x (the lowest index among bit-equal values),
//   top_plog = x[top_id] - logsumexp(x).
// No mask, no temperature, no timestamp rule, and nothing written per
// vocabulary entry: 16 bytes per row leave the kernel.
//
// One 1024-thread workgroup per row. Thread t owns the entries t + 1024 k
// (k < SC_NPT = 52: every vocabulary the loader admits, LP_G * LP_CHUNK),
// loaded once, coalesced, and kept in registers for both passes over them
// (the maximum, then sum exp(x - max)): one pass over the row in memory. A
// row's arithmetic involves no other row, so its bits do not depend on R or on
// the rows that share the launch. Fixed order of every combine:
//   maximum / argmax: per thread in ascending k (strict >, so the lowest
//     index wins), the wave's xor butterfly with better(), the 16 wave
//     results in wave order;
//   sum: per thread the <= 52 terms in ascending k, the wave's xor butterfly
//     (wave_sum: 6 levels), the 16 wave sums pairwise in wave order (4 levels):
//     summation depth D = 52 + 6 + 4 = 62.
// -inf entries contribute exactly 0; a target at -inf gives plog = -inf,
// p = 0. Rows with no finite entry, and NaN, are outside the contract.
#include <type_traits>

#include "kcommon.h"
#include "kernels.h"

namespace mwx {

constexpr int SC_T = 1024;
constexpr int SC_W = SC_T / 64;
constexpr int SC_NPT = (SCORE_MAX_VOCAB + SC_T - 1) / SC_T;
static_assert(SC_NPT * SC_T >= LP_G * LP_CHUNK, "a row of any admitted vocabulary fits the registers");

// argmax with lowest-index tie break (k_misc.hip: better)
__device__ __forceinline__ void sc_better(float& v, int& idx, float ov, int oi) {
  if (ov > v || (ov == v && oi < idx)) {
    v = ov;
    idx = oi;
  }
}

template <int I, int N, typename F>
__device__ __forceinline__ void sc_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    sc_for<I + 1, N>(f);
  }
}

__global__ __launch_bounds__(SC_T) void score_rows_kernel(const float* __restrict__ logits,
                                                          const int* __restrict__ target,
                                                          const int* __restrict__ active, int V,
                                                          ScoreOut* __restrict__ out) {
  __shared__ float redm[SC_W];
  __shared__ int redi[SC_W];
  __shared__ float reds[SC_W];
  const int row = blockIdx.x;
  if (active && !active[row]) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* L = logits + (long)row * V;
  float x[SC_NPT];
  float m = -INFINITY;
  int mi = 0x7fffffff;
  sc_for<0, SC_NPT>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const int i = tid + k * SC_T;
    x[k] = i < V ? L[i] : -INFINITY;
    if (x[k] > m) {
      m = x[k];
      mi = i;
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sc_better(m, mi, __shfl_xor(m, o, 64), __shfl_xor(mi, o, 64));
  if (lane == 0) {
    redm[wid] = m;
    redi[wid] = mi;
  }
  __syncthreads();
  m = redm[0];
  mi = redi[0];
#pragma unroll
  for (int k = 1; k < SC_W; ++k) sc_better(m, mi, redm[k], redi[k]);
  float s = 0.0f;
  sc_for<0, SC_NPT>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if (x[k] > -INFINITY) s += expf(x[k] - m);
  });
  s = wave_sum(s);
  if (lane == 0) reds[wid] = s;
  __syncthreads();
  if (tid != 0) return;
  float w[SC_W];
#pragma unroll
  for (int k = 0; k < SC_W; ++k) w[k] = reds[k];
#pragma unroll
  for (int n = SC_W / 2; n > 0; n >>= 1)
#pragma unroll
    for (int k = 0; k < n; ++k) w[k] = w[2 * k] + w[2 * k + 1];
  const float lse = logf(w[0]) + m;
  const float xt = L[target[row]];
  ScoreOut r;
  r.plog = xt == -INFINITY ? -INFINITY : xt - lse;
  r.p = xt == -INFINITY ? 0.0f : expf(r.plog);
  r.top_plog = m - lse;
  r.top_id = mi;
  out[row] = r;
}

bool score_rows(const float* logits, const int* target, const int* active, int R, int V,
                ScoreOut* out, hipStream_t st) {
  if (R < 1 || V < 1 || V > SCORE_MAX_VOCAB) return false;
  score_rows_kernel<<<R, SC_T, 0, st>>>(logits, target, active, V, out);
  return true;
}

}  // namespace mwx
