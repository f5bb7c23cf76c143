// Language identification for gfx950 (DESIGN.md "Language identification"):
// per row of raw f32 logits x[V], over the n language entries x[t0 .. t0 + n)
// only (upstream's softmax over the language logits),
//   M = max x_i, p_i = expf(x_i - M) / sum_j expf(x_j - M),
//   best = the lowest index i with x_i == M (taken from the logits, never from
//          the rounded probabilities).
// A -inf entry gives exactly 0. Rows with no finite entry, and NaN, are outside
// the contract (nothing is read or written out of bounds for them).
//
// One wave per row, four rows per 256-thread workgroup. Lane l owns entries l
// and l + 64 (n <= LANG_MAX_N = 128), loaded once and kept in registers.
// Nothing goes through LDS memory and no wave waits for another. A row's
// arithmetic involves no other row and no launch dimension, so its bits do not
// depend on R or on its position in the launch. Fixed order of every combine:
//   maximum: per lane fmaxf of its two entries, then the wave's xor butterfly;
//   best: per lane the lower of its entries equal to M, then the butterfly's
//     integer minimum;
//   sum: per lane e_l + e_(l+64) (one addition), then the wave's xor butterfly
//     (wave_sum: 6 levels): summation depth ceil(n / 64) - 1 + 6.
#include "kcommon.h"
#include "kernels.h"

namespace mwx {

constexpr int LG_ROWS = 4;
constexpr int LG_T = 64 * LG_ROWS;
static_assert(LANG_MAX_N == 128, "a lane owns entries lane and lane + 64");

__global__ __launch_bounds__(LG_T) void lang_probs_kernel(const float* __restrict__ logits, int R,
                                                          int V, int t0, int n,
                                                          float* __restrict__ probs,
                                                          int* __restrict__ best) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * LG_ROWS + wid;
  if (row >= R) return;  // (wave-uniform)
  const float* x = logits + row * V + t0;
  const int i0 = lane, i1 = lane + 64;
  const float x0 = i0 < n ? x[i0] : -INFINITY;
  const float x1 = i1 < n ? x[i1] : -INFINITY;
  const float m = wave_max(fmaxf(x0, x1));
  int bi = 0x7fffffff;
  if (i1 < n && x1 == m) bi = i1;
  if (i0 < n && x0 == m) bi = i0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bi = min(bi, __shfl_xor(bi, o, 64));
  const float e0 = x0 > -INFINITY ? expf(x0 - m) : 0.0f;
  const float e1 = x1 > -INFINITY ? expf(x1 - m) : 0.0f;
  const float s = wave_sum(e0 + e1);
  float* p = probs + row * n;
  if (i0 < n) p[i0] = e0 / s;
  if (i1 < n) p[i1] = e1 / s;
  if (lane == 0) best[row] = bi;
}

bool lang_probs(const float* logits, int R, int V, int t0, int n, float* probs, int* best,
                hipStream_t st) {
  if (R <= 0 || n < 1 || n > LANG_MAX_N || t0 < 0 || (long)t0 + n > V) return false;
  lang_probs_kernel<<<(R + LG_ROWS - 1) / LG_ROWS, LG_T, 0, st>>>(logits, R, V, t0, n, probs, best);
  return true;
}

}  // namespace mwx
