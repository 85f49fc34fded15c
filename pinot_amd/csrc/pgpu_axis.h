// What the kernels over the value axis of a group table share (pgpu_fold.hip, pgpu_select.hip, pgpu_mode.hip): the
// 64-bit wave shuffles, the cut of the cid axis into chunks with the strides of a per-chunk buffer that go with it, and
// the grid of a grid-stride launch.  Everything here is static and inlined: no translation unit depends on another.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#define PGPU_AXIS_THREADS 256  // workgroup size of every kernel over the axis
#define PGPU_AXIS_WAVES (PGPU_AXIS_THREADS / 64)
#define PGPU_AXIS_MAX_CHUNKS 1024
#define PGPU_AXIS_MIN_WAVE_CHUNK 256  // cid per (g, chunk) wave at least: four steps of 64 lanes

// Cell (chunk, g) of a per-chunk buffer is at chunk * sc + g * sg: [chunk][g] (sc = inner, sg = 1) or [g][chunk]
// (sc = 1, sg = nchunks).
struct PartialAt {
  uint64_t sc, sg;
};

// ---- 64-bit values through the wave's 32-bit shuffles ----
#define PGPU_AXIS_FI static __device__ __forceinline__
PGPU_AXIS_FI int axis_lo32(int64_t v) { return (int)(uint32_t)v; }
PGPU_AXIS_FI int axis_hi32(int64_t v) { return (int)(uint32_t)((uint64_t)v >> 32); }
PGPU_AXIS_FI int64_t axis_join64(int lo, int hi) { return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo); }
PGPU_AXIS_FI int64_t shfl_xor64(int64_t v, int d) {  // from lane ^ d
  return axis_join64(__shfl_xor(axis_lo32(v), d, 64), __shfl_xor(axis_hi32(v), d, 64));
}
PGPU_AXIS_FI int64_t shfl_up64(int64_t v, int d) {  // from lane - d
  return axis_join64(__shfl_up(axis_lo32(v), d, 64), __shfl_up(axis_hi32(v), d, 64));
}
PGPU_AXIS_FI int64_t shfl64(int64_t v, int lane) {  // from `lane`
  return axis_join64(__shfl(axis_lo32(v), lane, 64), __shfl(axis_hi32(v), lane, 64));
}
#undef PGPU_AXIS_FI

// Workgroups of a grid-stride kernel over n items.
static inline unsigned grid_of(uint64_t n) {
  return (unsigned)std::min<uint64_t>(4096, std::max<uint64_t>(1, (n + PGPU_AXIS_THREADS - 1) / PGPU_AXIS_THREADS));
}

// Chunks of cid for dense input: (chunk, nchunks).  inner < 64 gives a wave a (g, chunk), inner >= 64 a thread.
static inline void chunks_of(uint64_t inner, uint64_t card, int num_cus, uint64_t* chunk, uint32_t* nchunks) {
  const bool wave = inner < 64;
  // a few waves per SIMD: what the keys do not give comes from splitting cid
  const uint64_t have = wave ? inner : (inner + PGPU_AXIS_THREADS - 1) / PGPU_AXIS_THREADS;
  const uint64_t want = (wave ? 32ull : 8ull) * (uint64_t)std::max(num_cus, 1);
  const uint64_t fill = (want + have - 1) / have;
  const uint64_t most = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(card, PGPU_AXIS_MAX_CHUNKS), fill));
  uint64_t c = (card + most - 1) / most;
  if (wave) c = std::max<uint64_t>(PGPU_AXIS_MIN_WAVE_CHUNK, (c + 63) & ~63ull);
  *chunk = c;
  *nchunks = (uint32_t)((card + c - 1) / c);
}
