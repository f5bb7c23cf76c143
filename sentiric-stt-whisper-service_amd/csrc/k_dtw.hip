// DTW token timestamps from cross-attention alignment heads:
// the alignment heads' softmax probabilities of a teacher-forced pass
// (align_qk_kernel), their normalised, median-filtered head mean as a cost
// matrix (dtw_cost_kernel) and the dynamic-time-warping path through it
// (dtw_path_kernel). The rule restates HF transformers'
// _extract_token_timestamps / _median_filter / _dynamic_time_warping.
#include "kcommon.h"

namespace mwx {

// ---------------------------------------------------------------------------
// alignment-head probabilities
// ---------------------------------------------------------------------------
// One workgroup per (virtual row, alignment head of this layer). The query is
// the one the cross-attention kernels form, q = f16((sum of the split-K slabs
// + bias) * qscale); the scores are q.k over the slot's f16 key rows (MX-fp8
// cache: the codes widened with dequant_h8, as dec_xattn_kernel widens them),
// eight lanes per 128-B key row, times `scale`; the softmax is the decoder's
// (f32 max, expf, double sum in block_sum_256d's order) but its f32
// probabilities are kept (the decoder rounds them to f16 for P.V). A row below
// pos0 (the sot sequence) or inactive (padding) writes nothing.
// VL: slot's key count xkeys[slot] <= n_max; the output row stride stays n_max.
template <bool KV8, bool VL = false>
__global__ __launch_bounds__(256) void align_qk_kernel(
    const float* __restrict__ P, int KS, int pcols, const float* __restrict__ bias, float qscale,
    float scale, const void* __restrict__ kbase, const uint8_t* __restrict__ kscale8,
    const int* __restrict__ kv_index, const int* __restrict__ pos, const int* __restrict__ active,
    const int2* __restrict__ heads, int n_max, int cap, int R, int H, int pos0, int A,
    int n_rows_cap, float* __restrict__ out, const int* __restrict__ xkeys = nullptr) {
  __shared__ float sc[DTW_MAX_KEYS];
  __shared__ float redf[4];
  __shared__ double redd[4];
  __shared__ float sq[64];
  const int row = blockIdx.y;
  const int act_r = active[row];
  const int p_row = pos[row];
  const int slot = kv_index[row];
  const int2 ha = heads[blockIdx.x];
  const int orow = p_row - pos0;
  if (!act_r || orow < 0 || orow >= n_rows_cap) return;
  int n = n_max;
  if constexpr (VL) n = max(1, min(xkeys[slot], n_max));
  const int h = ha.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kg = lane >> 3, c = lane & 7;
  if (tid < 64) {
    const long pstride = (long)R * pcols;
    const float* pp = P + (long)row * pcols + h * 64 + tid;
    float acc = pp[0];
    for (int k = 1; k < KS; ++k) acc += pp[k * pstride];
    sq[tid] = (float)f16r((acc + bias[h * 64 + tid]) * qscale);
  }
  __syncthreads();
  h2 qh[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    qh[e] = h2{(_Float16)sq[c * 8 + 2 * e], (_Float16)sq[c * 8 + 2 * e + 1]};
  const long rbase = ((long)slot * H + h) * cap;
  const _Float16* K = reinterpret_cast<const _Float16*>(kbase) + rbase * 64;
  const uint8_t* K8 = reinterpret_cast<const uint8_t*>(kbase) + rbase * 64;
  const uint8_t* KS8 = KV8 ? kscale8 + rbase * 2 : nullptr;
  // 32 key rows per trip (8 per wave); rows past the end are clamped, so every
  // lane takes part in the 8-lane sums
  for (int j0 = wid * 8 + kg; j0 < ((n + 31) & ~31); j0 += 32) {
    const int j = min(j0, n - 1);
    f16x8 kk;
    if constexpr (KV8) {
      const u32x2 raw = *reinterpret_cast<const u32x2*>(K8 + (long)j * 64 + c * 8);
      kk = dequant_h8(uint2{raw[0], raw[1]}, KS8[(long)j * 2 + (c >> 2)]);
    } else {
      kk = *reinterpret_cast<const f16x8*>(K + (long)j * 64 + c * 8);
    }
    const float d = dpp_sum8(dot8(qh, kk));
    if (c == 0 && j0 < n) sc[j0] = d * scale;
  }
  __syncthreads();
  constexpr int NI = DTW_MAX_KEYS / 256;
  float sv[NI];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int j = tid + 256 * i;
    sv[i] = j < n ? sc[j] : -INFINITY;
    mx = fmaxf(mx, sv[i]);
  }
  mx = block_max_256(mx, redf);
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (tid + 256 * i < n) {
      const float e = expf(sv[i] - mx);
      sv[i] = e;
      sum += (double)e;
    }
  }
  sum = block_sum_256d(sum, redd);
  const float inv = (float)(1.0 / sum);
  float* o = out + (((long)slot * A + ha.y) * n_rows_cap + orow) * n_max;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int j = tid + 256 * i;
    if (j < n) o[j] = sv[i] * inv;
  }
}

bool align_probs(const float* P, int KS, int pcols, const float* bias, float qscale, float scale,
                 const void* kbase, const uint8_t* kscale8, const int* kv_index, const int* pos,
                 const int* active, const int2* heads, int n_heads, int n_keys, int cap, int R, int H,
                 int pos0, int A, int n_rows_cap, float* out, hipStream_t st, const int* xkeys) {
  if (n_keys < 1 || n_keys > DTW_MAX_KEYS || n_keys > cap || KS < 1 || R < 1 || n_heads < 1)
    return false;
  const dim3 grid(n_heads, R);
  if (xkeys && kscale8)
    align_qk_kernel<true, true><<<grid, 256, 0, st>>>(P, KS, pcols, bias, qscale, scale, kbase,
                                                      kscale8, kv_index, pos, active, heads, n_keys,
                                                      cap, R, H, pos0, A, n_rows_cap, out, xkeys);
  else if (xkeys)
    align_qk_kernel<false, true><<<grid, 256, 0, st>>>(P, KS, pcols, bias, qscale, scale, kbase,
                                                       nullptr, kv_index, pos, active, heads, n_keys,
                                                       cap, R, H, pos0, A, n_rows_cap, out, xkeys);
  else if (kscale8)
    align_qk_kernel<true><<<grid, 256, 0, st>>>(P, KS, pcols, bias, qscale, scale, kbase, kscale8,
                                                kv_index, pos, active, heads, n_keys, cap, R, H,
                                                pos0, A, n_rows_cap, out);
  else
    align_qk_kernel<false><<<grid, 256, 0, st>>>(P, KS, pcols, bias, qscale, scale, kbase, nullptr,
                                                 kv_index, pos, active, heads, n_keys, cap, R, H,
                                                 pos0, A, n_rows_cap, out);
  return true;
}

// ---------------------------------------------------------------------------
// cost matrix
// ---------------------------------------------------------------------------
// median of 7 by a selection network: every step is a min / max of two inputs,
// so the result is one of the inputs (no smoothing error)
__device__ __forceinline__ void cswap(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}
__device__ __forceinline__ float median7(float v0, float v1, float v2, float v3, float v4, float v5,
                                         float v6) {
  cswap(v0, v5); cswap(v0, v3); cswap(v1, v6); cswap(v2, v4); cswap(v0, v1); cswap(v3, v5);
  cswap(v2, v6); cswap(v2, v3); cswap(v3, v6); cswap(v4, v5); cswap(v1, v4); cswap(v1, v3);
  cswap(v3, v4);
  return v3;
}

// Workgroup (64 columns, 4 row groups) of clip blockIdx.y. Per head a, in
// order: threads 0..69 take one column of the tile and its halo of 3 each
// (reflected at the clip's ends) and loop over the rows n = 0 .. N-1 for the
// column's mean and population variance (two passes, fixed order); then every
// thread forms, for its column and its rows, the 7 normalised neighbours
// z = (w - mean) / sqrt(var) (0 where var == 0), takes their median (T <= 3:
// z itself, as HF skips the filter) and adds it to cost[n][t], which only this
// thread touches; after the last head cost = -sum / A.
// w: [slot][A][n_rows_cap][n_keys] (align_qk_kernel's output); cost: clip b at
// b * cost_stride, rows compact ([N][T]).
__global__ __launch_bounds__(256) void dtw_cost_kernel(const float* __restrict__ w,
                                                       const int* __restrict__ slot_of,
                                                       const int* __restrict__ Ns,
                                                       const int* __restrict__ Ts, int A,
                                                       int n_rows_cap, int n_keys,
                                                       long cost_stride, float* __restrict__ cost) {
  __shared__ float smean[70], sstd[70];
  const int b = blockIdx.y;
  const int N = Ns[b], T = Ts[b];
  const int t0 = blockIdx.x * 64;
  if (t0 >= T) return;  // (uniform per workgroup)
  const int tx = threadIdx.x & 63, ny = threadIdx.x >> 6;
  const int t = t0 + tx;
  const bool filt = T > 3;
  auto reflect = [&](int tt) {
    if (tt < 0) tt = -tt;
    if (tt >= T) tt = 2 * (T - 1) - tt;
    return max(0, min(T - 1, tt));
  };
  int col[7];
#pragma unroll
  for (int o = 0; o < 7; ++o) col[o] = reflect(t + o - 3);
  float* cb = cost + (long)b * cost_stride;
  const float* wb = w + (long)slot_of[b] * A * n_rows_cap * n_keys;
  for (int a = 0; a < A; ++a) {
    const float* wa = wb + (long)a * n_rows_cap * n_keys;
    if (threadIdx.x < 70) {
      const int cc = reflect(t0 + (int)threadIdx.x - 3);
      float s = 0.0f;
      for (int n = 0; n < N; ++n) s += wa[(long)n * n_keys + cc];
      const float mean = s / (float)N;
      float v = 0.0f;
      for (int n = 0; n < N; ++n) {
        const float dlt = wa[(long)n * n_keys + cc] - mean;
        v += dlt * dlt;
      }
      smean[threadIdx.x] = mean;
      sstd[threadIdx.x] = sqrtf(v / (float)N);
    }
    __syncthreads();
    if (t < T) {
      for (int n = ny; n < N; n += 4) {
        const float* wr = wa + (long)n * n_keys;
        float z[7];
#pragma unroll
        for (int o = 0; o < 7; ++o) {
          const float sd = sstd[tx + o];
          z[o] = sd > 0.0f ? (wr[col[o]] - smean[tx + o]) / sd : 0.0f;
        }
        const float m = filt ? median7(z[0], z[1], z[2], z[3], z[4], z[5], z[6]) : z[3];
        float* cp = cb + (long)n * T + t;
        const float acc = (a == 0 ? 0.0f : *cp) + m;
        *cp = a == A - 1 ? -(acc / (float)A) : acc;
      }
    }
    __syncthreads();
  }
}

bool dtw_cost(const float* w, const int* slot_of, const int* Ns, const int* Ts, int n_clips, int A,
              int n_rows_cap, int n_keys, int t_max, long cost_stride, float* cost,
              hipStream_t st) {
  if (n_clips < 1 || A < 1 || t_max < 1 || t_max > n_keys) return false;
  dtw_cost_kernel<<<dim3((t_max + 63) / 64, n_clips), 256, 0, st>>>(w, slot_of, Ns, Ts, A, n_rows_cap,
                                                                    n_keys, cost_stride, cost);
  return true;
}

// ---------------------------------------------------------------------------
// DTW path
// ---------------------------------------------------------------------------
// One workgroup per clip; thread i - 1 owns row i of HF's (N + 1) x (T + 1)
// cost table and walks it along the anti-diagonals k = i + j: step k needs
// D[i][j-1] (its own last value, a register), D[i-1][j] (row i - 1's value of
// diagonal k - 1, read from LDS) and D[i-1][j-1] (what it read there one step
// earlier, a register). The diagonals are double-buffered in LDS, one barrier
// per step. A row's cost entries are fetched 16 steps ahead of their use. The
// trace is packed at 2 bits per cell in LDS (row stride W words, odd): 0 =
// diagonal, 1 = up (i - 1), 2 = left (j - 1), chosen as HF chooses (strict <
// for the diagonal, then strict < for up, otherwise left). Thread 0 then walks
// back from (N, T): frame[n] = the smallest j of the path in row n. path
// (nullable): the (row, column) pairs in path order, right-aligned in
// [N + T] pairs, and their count.
__global__ __launch_bounds__(256) void dtw_path_kernel(const float* __restrict__ cost,
                                                       const int* __restrict__ Ns,
                                                       const int* __restrict__ Ts, long cost_stride,
                                                       int n_rows_cap, int W,
                                                       int* __restrict__ frames, int path_cap,
                                                       int* __restrict__ path,
                                                       int* __restrict__ path_len) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* diag = reinterpret_cast<float*>(smem);                 // [2][DTW_MAX_ROWS + 1]
  uint32_t* tr = reinterpret_cast<uint32_t*>(smem + 2 * (DTW_MAX_ROWS + 16) * 4);  // [N][W]
  const int b = blockIdx.x;
  const int N = Ns[b], T = Ts[b];
  const int i = threadIdx.x + 1;  // row of the cost table
  const bool mine = i <= N;
  const float* crow = cost + (long)b * cost_stride + (long)(i - 1) * T;
  diag[i] = INFINITY;
  diag[(DTW_MAX_ROWS + 16) + i] = INFINITY;
  if (threadIdx.x == 0) {
    diag[0] = INFINITY;  // D[0][j >= 1] (and D[0][0] is row 1's c_diag start)
    diag[DTW_MAX_ROWS + 16] = INFINITY;
  }
  float c_diag = i == 1 ? 0.0f : INFINITY;  // D[i-1][0]
  float c_left = INFINITY;                  // D[i][0]
  uint32_t word = 0;
  float cur[16], nxt[16];
  auto fetch = [&](float* buf, int kc) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int j = kc + u - i;
      buf[u] = (mine && j >= 1 && j <= T) ? crow[j - 1] : 0.0f;
    }
  };
  const int k_end = N + T;
  fetch(nxt, 2);
  __syncthreads();
  for (int kc = 2; kc <= k_end; kc += 16) {
#pragma unroll
    for (int u = 0; u < 16; ++u) cur[u] = nxt[u];
    fetch(nxt, kc + 16);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int k = kc + u;
      const int j = k - i;
      const float* dprev = diag + ((k - 1) & 1) * (DTW_MAX_ROWS + 16);
      float* dcur = diag + (k & 1) * (DTW_MAX_ROWS + 16);
      if (mine && j >= 1 && j <= T) {
        const float c0 = c_diag, c1 = dprev[i - 1], c2 = c_left;
        float cm;
        uint32_t tv;
        if (c0 < c1 && c0 < c2) {
          cm = c0;
          tv = 0;
        } else if (c1 < c0 && c1 < c2) {
          cm = c1;
          tv = 1;
        } else {
          cm = c2;
          tv = 2;
        }
        const float nv = cur[u] + cm;
        dcur[i] = nv;
        c_left = nv;
        c_diag = c1;
        const int bit = (j - 1) & 15;
        word |= tv << (2 * bit);
        if (bit == 15 || j == T) {
          tr[(long)(i - 1) * W + ((j - 1) >> 4)] = word;
          word = 0;
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    int* fr = frames + (long)b * n_rows_cap;
    int* pp = path ? path + (long)b * path_cap * 2 : nullptr;
    int ii = N, jj = T, cnt = 0;
    while (ii > 0 || jj > 0) {
      if (ii > 0) fr[ii - 1] = jj - 1;
      if (pp && cnt < path_cap) {
        pp[(path_cap - 1 - cnt) * 2] = ii - 1;
        pp[(path_cap - 1 - cnt) * 2 + 1] = jj - 1;
      }
      ++cnt;
      uint32_t tv;
      if (ii == 0)
        tv = 2;
      else if (jj == 0)
        tv = 1;
      else
        tv = (tr[(long)(ii - 1) * W + ((jj - 1) >> 4)] >> (2 * ((jj - 1) & 15))) & 3u;
      if (tv == 0) {
        --ii;
        --jj;
      } else if (tv == 1) {
        --ii;
      } else {
        --jj;
      }
    }
    if (path_len) path_len[b] = cnt;
  }
}

bool dtw_path(const float* cost, const int* Ns, const int* Ts, int n_clips, int n_max, int t_max,
              long cost_stride, int n_rows_cap, int* frames, int path_cap, int* path, int* path_len,
              hipStream_t st) {
  if (n_clips < 1 || n_max < 1 || n_max > DTW_MAX_ROWS || n_max > n_rows_cap || t_max < 1 ||
      t_max > DTW_MAX_KEYS || (path && path_cap < n_max + t_max))
    return false;
  const int W = ((t_max + 15) / 16) | 1;
  const size_t lds = 2 * (DTW_MAX_ROWS + 16) * 4 + (size_t)n_max * W * 4;
  // (226 x 1500 cells: 2.1 + 85.9 KB of the CU's 160 KB)
  // the kernel's dynamic-LDS ceiling: always the size of the largest shape
  // served (256 rows x 1536 columns: 99.1 KB of the CU's 160 KB), so that
  // concurrent callers never lower it under each other's launches
  constexpr int lds_max =
      2 * (DTW_MAX_ROWS + 16) * 4 + DTW_MAX_ROWS * (((DTW_MAX_KEYS + 15) / 16) | 1) * 4;
  if (lds > (size_t)lds_max) return false;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(dtw_path_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess)
    return false;
  dtw_path_kernel<<<n_clips, 256, lds, st>>>(cost, Ns, Ts, cost_stride, n_rows_cap, W, frames,
                                             path_cap, path, path_len);
  return true;
}

}  // namespace mwx
