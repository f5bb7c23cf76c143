// Constrained decoding for gfx950: the step's rejection mask.
// mask[r][w] bit b set <=> token 64 w + b is rejected for row r in its state
// RowCtl.pad[1]. logits_process's filter phase subtracts the penalty where a
// bit is set; this kernel changes no logit.
//
// One lane per (row, token): lane t walks the token's bytes through the
// class-compressed table from the row's state. A wave holds 64 consecutive
// tokens and writes their word from one ballot: one 8-byte store per 64 tokens,
// no atomics, each (row, token) decided by exactly one lane, and the bits above
// V in the tail word are zero because those lanes vote false. Rows with
// active == 0 or sample == 0 are not written; a row in state 0 writes zeros. A
// row's words depend on its own state only, not on R or on the grid.
//
// Grid: (ceil(V / 256), R) workgroups of 4 waves. The kernel is latency-bound:
// per lane two coalesced loads (off, head) and then a chain of dependent
// 2-byte table reads, one per byte until the state dies, which for most tokens
// is the first byte. The table (S x classes x 2 bytes: a few KB for a menu, at
// most 2 MB) and the 256-byte class map are read through the vector L1 / L2,
// not staged in LDS: a workgroup touches only the rows of the states its 256
// tokens pass through (for most of them one row, the row state's), so a copy
// of the whole table per workgroup would cost more than the walk it serves, and
// the largest tables do not fit the LDS at all.
#define MWX_CON_NO_HOST
#include "constraint.h"
#include "kcommon.h"
#include "kernels.h"

namespace mwx {

constexpr int LC_T = 256;

__global__ __launch_bounds__(LC_T) void logits_constrain_kernel(
    unsigned long long* __restrict__ mask, const RowCtl* __restrict__ ctl, ConView v, int V,
    int W) {
  const int row = blockIdx.y;
  const RowCtl c = ctl[row];
  if (!c.active || !c.sample) return;  // (workgroup-uniform)
  const int t = blockIdx.x * LC_T + (int)threadIdx.x;
  const int word = t >> 6;  // (wave-uniform: LC_T and the wave are multiples of 64)
  int s = c.pad[1];
  if (s < 0 || s >= v.S) s = 0;
  const bool rej = (s != 0 && t < V) ? con_rejects(v, s, t) : false;
  const unsigned long long bits = __ballot(rej);
  if ((threadIdx.x & 63) == 0 && word < W) mask[(long)row * W + word] = bits;
}

bool logits_constrain(unsigned long long* mask, const RowCtl* ctl, const ConView& v, int R, int V,
                      hipStream_t st) {
  if (!mask || !ctl || !v.tab || !v.cls || !v.acc || !v.off || !v.head || !v.bytes) return false;
  if (R < 1 || V < 1 || v.S < 2 || v.C < 1 || v.C > 256 || v.eot < 0 || v.eot > V) return false;
  const int W = (V + 63) / 64;
  logits_constrain_kernel<<<dim3((V + LC_T - 1) / LC_T, R), LC_T, 0, st>>>(mask, ctl, v, V, W);
  return true;
}

}  // namespace mwx
