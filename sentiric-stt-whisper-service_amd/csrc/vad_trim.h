// The objects behind mwx_vad_segments_* and mwx_vad_trim_batch (vad.cpp), shared
// with mwx_full_batch_trimmed (driver.inc). Host data only, plus the one device
// buffer a trimmed batch owns.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

struct mwx_vad_segments {
  std::vector<int64_t> seg;  // (start, end) in samples
};

struct mwx_vad_trimmed {
  struct Clip {
    std::vector<int64_t> seg;    // (start, end) in samples, the caller's timeline
    std::vector<int64_t> piece;  // (src, len, dst) in samples
    int64_t n_compact = 0;       // compacted length
    size_t off = 0;              // of the compacted clip in d_pcm, in floats
  };
  int device = 0;
  float* d_pcm = nullptr;  // owned; every clip starts 16-byte aligned
  std::vector<Clip> clips;
};

namespace mwx {

// Compacted centiseconds -> the caller's centiseconds (time map).
inline int64_t vad_map_time(const mwx_vad_trimmed::Clip& c, int64_t t_cs, bool is_end) {
  const int64_t m = (int64_t)c.piece.size() / 3;
  if (t_cs < 0 || m == 0) return t_cs;
  const int64_t x = 160 * t_cs;
  int64_t lo = 0, hi = m - 1;  // the last piece with dst <= x (dst_0 = 0)
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (c.piece[3 * mid + 2] <= x)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int64_t src = c.piece[3 * lo], len = c.piece[3 * lo + 1], dst = c.piece[3 * lo + 2];
  int64_t orig;
  if (x - dst < len)
    orig = src + (x - dst);
  else if (is_end || lo == m - 1)
    orig = src + len;
  else
    orig = c.piece[3 * (lo + 1)];
  return orig / 160;
}

}  // namespace mwx
