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
    std::vector<int64_t> chunk;  // (first piece, n pieces): the chunk plan
    int64_t n_compact = 0;       // compacted length
    size_t off = 0;              // of the compacted clip in d_pcm, in floats
  };
  int device = 0;
  float* d_pcm = nullptr;  // owned; every clip starts 16-byte aligned
  std::vector<Clip> clips;
};

namespace mwx {

// Centiseconds of the audio laid out by the m pieces at `piece`, counted from
// compacted position `base` (the first piece's dst) -> the caller's
// centiseconds (time map).
inline int64_t vad_map_time_pieces(const int64_t* piece, int64_t m, int64_t base, int64_t t_cs,
                                   bool is_end) {
  if (t_cs < 0 || m <= 0) return t_cs;
  const int64_t x = 160 * t_cs + base;
  int64_t lo = 0, hi = m - 1;  // the last piece with dst <= x (dst_0 = base)
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (piece[3 * mid + 2] <= x)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int64_t src = piece[3 * lo], len = piece[3 * lo + 1], dst = piece[3 * lo + 2];
  int64_t orig;
  if (x - dst < len)
    orig = src + (x - dst);
  else if (is_end || lo == m - 1)
    orig = src + len;
  else
    orig = piece[3 * (lo + 1)];
  return orig / 160;
}

// Compacted centiseconds of the whole clip -> the caller's centiseconds.
inline int64_t vad_map_time(const mwx_vad_trimmed::Clip& c, int64_t t_cs, bool is_end) {
  return vad_map_time_pieces(c.piece.data(), (int64_t)c.piece.size() / 3, 0, t_cs, is_end);
}

// Chunk j of the clip: its start and length in the compacted
// clip; false when j is out of range.
inline bool vad_chunk_span(const mwx_vad_trimmed::Clip& c, int64_t j, int64_t& first, int64_t& n,
                           int64_t& start, int64_t& len) {
  if (j < 0 || 2 * j + 1 >= (int64_t)c.chunk.size()) return false;
  first = c.chunk[2 * j];
  n = c.chunk[2 * j + 1];
  const int64_t last = first + n - 1;
  start = c.piece[3 * first + 2];
  len = c.piece[3 * last + 2] + c.piece[3 * last + 1] - start;
  return true;
}

// Chunk-local centiseconds -> the caller's centiseconds: the time map over the
// chunk's pieces with dst counted from the chunk's start.
inline int64_t vad_chunk_map_time(const mwx_vad_trimmed::Clip& c, int64_t j, int64_t t_cs,
                                  bool is_end) {
  int64_t first, n, start, len;
  if (!vad_chunk_span(c, j, first, n, start, len)) return t_cs;
  return vad_map_time_pieces(c.piece.data() + 3 * first, n, start, t_cs, is_end);
}

}  // namespace mwx
