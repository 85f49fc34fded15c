// HyperLogLog sketches of a group table (pgpu_table_hll, include/pinot_gpu.h): DISTINCTCOUNTHLL / DISTINCTCOUNTRAWHLL.
// The reference keeps a bitmap of the column's dictionary ids per group and offers dictionary.get(id) to the sketch
// only at extract time (DistinctCountHLLAggregationFunction.java:104-110,176-184,438-447), so the sketch of group g is
// a function of the occupancy of section 0 of the table GROUP BY g, c -- cell key = g + inner * cid -- along cid:
// register j of g is the largest r over the occupied cid whose value hashes into j.  The host hashes the dictionary
// once (pinot_amd/hll.py: lut[cid] = j | r << 16); this stage reads, per occupied cell, one LUT entry and raises one
// 5-bit register.  Output: regs uint32[inner * W], group g's W packed words at g * W in RegisterSet's layout (register
// p in word p / 6 at bit 5 * (p mod 6)) -- a byte swap away from the wire form.  A cell is occupied when its count is
// > 0, the fold's test; a key without an occupied cell keeps W zero words.
//
// Accumulation: a compare-and-swap loop on the owning packed word (RegisterSet.updateIfGreater restated), entered only
// when a plain read of the word shows a smaller register.  Registers only grow, so a stale read can only be too small:
// it costs one failed exchange, which returns the current word.  After the first few values of a group nearly every
// cell ends at the read, which is why this shape was chosen over OR-ing one-hot masks (an atomic per cell whatever
// the register holds, six times the memory and a second kernel to pack).  The maximum is commutative and associative:
// the result depends neither on scheduling nor on how chunks_of cuts cid.
//
// Where inner * W * 4 B fits PGPU_HLL_LDS_BYTES (the fold's own switch) a workgroup accumulates in an LDS copy of the
// rows it can meet and merges the words it touched (non-zero) into HBM once; beyond that the loop runs on HBM directly.
// Dense input in pgpu_axis.h's two orientations (inner < 64: a wave owns a (g, chunk) with its lanes along cid;
// inner >= 64: a thread owns it and adjacent lanes read adjacent cells); hash input grid-strides over the slots with
// g = key % inner, cid = key / inner.  A cid >= num_values reads no LUT entry and offers nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pinot_gpu.h"
#include "pgpu_axis.h"

#define PGPU_HLL_LDS_BYTES (64 * 1024)
#define PGPU_HLL_THREADS PGPU_AXIS_THREADS
#define PGPU_HLL_WAVES PGPU_AXIS_WAVES
#define PGPU_HLL_UNROLL 4  // cells per thread (steps of 64 cid per wave) whose counts are loaded before any is used

namespace {

#define FI __device__ __forceinline__

// Raise register j of the row `words` (LDS or HBM) to r when it is smaller.  An entry that names no register of the
// sketch (j >= m) or no 5-bit rank is no output of the host's LUT: it is skipped, so that no LUT writes out of a row.
FI void hll_offer(uint32_t* words, uint32_t entry, uint32_t m) {
  const uint32_t j = entry & 0xFFFFu, r = entry >> 16;
  if (j >= m || r > 31u) return;
  uint32_t* p = words + j / 6;
  const uint32_t sh = 5 * (j % 6);
  uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (((old >> sh) & 31u) < r) {
    const uint32_t seen = atomicCAS(p, old, (old & ~(31u << sh)) | (r << sh));
    if (seen == old) break;
    old = seen;
  }
}

// Register-wise maximum of two packed words.
FI uint32_t hll_max_word(uint32_t a, uint32_t b) {
  uint32_t o = 0;
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    const uint32_t x = (a >> (5 * f)) & 31u, y = (b >> (5 * f)) & 31u;
    o |= (x > y ? x : y) << (5 * f);
  }
  return o;
}

// Merge the word w into *p (HBM).
FI void hll_merge_word(uint32_t* p, uint32_t w) {
  uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  for (;;) {
    const uint32_t nw = hll_max_word(old, w);
    if (nw == old) break;
    const uint32_t seen = atomicCAS(p, old, nw);
    if (seen == old) break;
    old = seen;
  }
}

// The workgroup's LDS rows [g_lo, g_lo + rows) zeroed (before) and merged into HBM where touched (after).
FI void hll_lds_clear(uint32_t* tab, uint32_t n) {
  for (uint32_t i = threadIdx.x; i < n; i += PGPU_HLL_THREADS) tab[i] = 0;
  __syncthreads();
}
FI void hll_lds_flush(const uint32_t* tab, uint32_t n, uint32_t* regs_at) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += PGPU_HLL_THREADS) {
    const uint32_t w = tab[i];
    if (w) hll_merge_word(regs_at + i, w);
  }
}

// Dense input [.][card * inner].  WAVE: wave w of the launch owns (g, chunk) = (w % inner, w / inner), lanes along cid;
// else thread g of blockIdx.x owns (g, blockIdx.y).  LDS: rows [g_lo, g_lo + rows) of the sketches in dynamic LDS --
// every key when WAVE (inner < 64), the workgroup's own keys otherwise.  No thread leaves before the flush.
template <bool WAVE, bool LDS>
__global__ __launch_bounds__(PGPU_HLL_THREADS) void hll_dense_kernel(const int64_t* __restrict__ in, uint64_t inner,
                                                                     uint64_t card, uint64_t chunk, uint32_t nchunks,
                                                                     const uint32_t* __restrict__ lut,
                                                                     uint64_t num_values, uint32_t m, uint32_t W,
                                                                     uint32_t* __restrict__ regs) {
  extern __shared__ uint32_t ltab[];
  const uint64_t g_lo = WAVE ? 0 : blockIdx.x * (uint64_t)PGPU_HLL_THREADS;
  const uint32_t rows = (uint32_t)(WAVE || inner - g_lo < PGPU_HLL_THREADS ? inner - g_lo : PGPU_HLL_THREADS);
  if (LDS) hll_lds_clear(ltab, rows * W);
  const int lane = threadIdx.x & 63;
  uint64_t g;
  uint32_t ck;
  bool work;
  if (WAVE) {
    const uint64_t w = blockIdx.x * (uint64_t)PGPU_HLL_WAVES + (threadIdx.x >> 6);
    work = w < inner * nchunks;
    ck = work ? (uint32_t)(w / inner) : 0;
    g = work ? w - (uint64_t)ck * inner : 0;
  } else {
    g = g_lo + threadIdx.x;
    ck = blockIdx.y;
    work = g < inner;
  }
  if (work) {
    uint32_t* row = LDS ? ltab + (uint32_t)(g - g_lo) * W : regs + g * W;
    const uint64_t c0 = ck * chunk;
    uint64_t c1 = c0 + chunk < card ? c0 + chunk : card;
    if (c1 > num_values) c1 = num_values;  // (a cid without a value offers nothing and reads no LUT entry)
    const uint64_t step = WAVE ? 64 : 1;
    for (uint64_t c = c0 + (WAVE ? lane : 0); c < c1; c += step * PGPU_HLL_UNROLL) {
      int64_t cnt[PGPU_HLL_UNROLL];
#pragma unroll
      for (int u = 0; u < PGPU_HLL_UNROLL; ++u) cnt[u] = c + u * step < c1 ? in[(c + u * step) * inner + g] : 0;
#pragma unroll
      for (int u = 0; u < PGPU_HLL_UNROLL; ++u)
        if (cnt[u] > 0) hll_offer(row, lut[c + u * step], m);
    }
  }
  if (LDS) hll_lds_flush(ltab, rows * W, regs + g_lo * W);
}

// Hash input: slot i of N holds its count at in[i] and its key word at in[nsec * N + i].  LDS: every key's row.
template <bool LDS>
__global__ __launch_bounds__(PGPU_HLL_THREADS) void hll_hash_kernel(const int64_t* __restrict__ in, uint64_t N,
                                                                    int32_t nsec, uint64_t inner,
                                                                    const uint32_t* __restrict__ lut,
                                                                    uint64_t num_values, uint32_t m, uint32_t W,
                                                                    uint32_t* __restrict__ regs) {
  extern __shared__ uint32_t ltab[];
  if (LDS) hll_lds_clear(ltab, (uint32_t)inner * W);
  const uint64_t stride = (uint64_t)gridDim.x * PGPU_HLL_THREADS;
  for (uint64_t e = blockIdx.x * (uint64_t)PGPU_HLL_THREADS + threadIdx.x; e < N; e += stride * PGPU_HLL_UNROLL) {
    int64_t cnt[PGPU_HLL_UNROLL];
#pragma unroll
    for (int u = 0; u < PGPU_HLL_UNROLL; ++u) cnt[u] = e + u * stride < N ? in[e + u * stride] : 0;
#pragma unroll
    for (int u = 0; u < PGPU_HLL_UNROLL; ++u) {
      if (cnt[u] <= 0) continue;
      const uint64_t key = (uint64_t)in[(uint64_t)nsec * N + e + u * stride];
      const uint64_t cid = key / inner, g = key - cid * inner;
      if (cid >= num_values) continue;
      hll_offer(LDS ? ltab + (uint32_t)g * W : regs + g * W, lut[cid], m);
    }
  }
  if (LDS) hll_lds_flush(ltab, (uint32_t)inner * W, regs);
}

}  // namespace

// RegisterSet's words for 2^log2m registers; 0 outside 4..16.
uint32_t pgpu_hll_words_of(int32_t log2m) {
  if (log2m < PGPU_HLL_MIN_LOG2M || log2m > PGPU_HLL_MAX_LOG2M) return 0;
  const uint32_t b = (1u << log2m) / 6;
  if (b == 0) return 1;
  return b % 32 == 0 ? b : b + 1;
}

// Enqueue the sketches of `in` ([nsec (+ key word when hash)][N] int64) on `st`: regs[inner * W], zeroed here first.
// lut[num_values] is in device memory.  The caller has checked N % inner == 0 for dense input and the byte cap.
hipError_t pgpu_launch_hll(const int64_t* in, uint64_t N, int32_t nsec, bool hash, uint64_t inner, const uint32_t* lut,
                           uint64_t num_values, int32_t log2m, uint32_t* regs, int num_cus, hipStream_t st) {
  const uint32_t W = pgpu_hll_words_of(log2m);
  if (W == 0 || inner == 0 || N == 0 || !lut || !regs) return hipErrorInvalidValue;
  const uint64_t bytes = inner * (uint64_t)W * 4;
  hipError_t e = hipMemsetAsync(regs, 0, bytes, st);
  if (e != hipSuccess) return e;
  if (num_values == 0) return hipSuccess;
  const bool lds = bytes <= PGPU_HLL_LDS_BYTES;
  const unsigned T = PGPU_HLL_THREADS;
  const uint32_t m = 1u << log2m;
  if (hash) {
    const uint64_t per_cu = lds ? std::max<uint64_t>(1, std::min<uint64_t>(8, (160 * 1024) / bytes)) : 8;
    const uint64_t rounds = (N + (uint64_t)T * PGPU_HLL_UNROLL - 1) / ((uint64_t)T * PGPU_HLL_UNROLL);
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(rounds, per_cu * (uint64_t)std::max(num_cus, 1)));
    if (lds)
      hipLaunchKernelGGL((hll_hash_kernel<true>), dim3(grid), dim3(T), (size_t)bytes, st, in, N, nsec, inner, lut,
                         num_values, m, W, regs);
    else
      hipLaunchKernelGGL((hll_hash_kernel<false>), dim3(grid), dim3(T), 0, st, in, N, nsec, inner, lut, num_values, m, W,
                         regs);
    return hipGetLastError();
  }
  const uint64_t card = N / inner;
  uint64_t chunk;
  uint32_t nchunks;
  chunks_of(inner, card, num_cus, &chunk, &nchunks);
  if (inner < 64) {
    const unsigned waves = (unsigned)((inner * nchunks + PGPU_HLL_WAVES - 1) / PGPU_HLL_WAVES);
    if (lds)
      hipLaunchKernelGGL((hll_dense_kernel<true, true>), dim3(waves), dim3(T), (size_t)bytes, st, in, inner, card, chunk,
                         nchunks, lut, num_values, m, W, regs);
    else
      hipLaunchKernelGGL((hll_dense_kernel<true, false>), dim3(waves), dim3(T), 0, st, in, inner, card, chunk, nchunks,
                         lut, num_values, m, W, regs);
  } else {
    const unsigned bx = (unsigned)((inner + T - 1) / T);
    const size_t lb = (size_t)std::min<uint64_t>(T, inner) * W * 4;
    if (lds)
      hipLaunchKernelGGL((hll_dense_kernel<false, true>), dim3(bx, nchunks), dim3(T), lb, st, in, inner, card, chunk,
                         nchunks, lut, num_values, m, W, regs);
    else
      hipLaunchKernelGGL((hll_dense_kernel<false, false>), dim3(bx, nchunks), dim3(T), 0, st, in, inner, card, chunk,
                         nchunks, lut, num_values, m, W, regs);
  }
  return hipGetLastError();
}

// Gather kernel of pgpu_query_collect_hll: row i of out = the W words of key keys[i].
namespace {
__global__ __launch_bounds__(PGPU_HLL_THREADS) void hll_gather_kernel(const uint32_t* __restrict__ regs,
                                                                      const int64_t* __restrict__ keys, uint64_t n,
                                                                      uint64_t inner, uint32_t W,
                                                                      uint32_t* __restrict__ out) {
  const uint64_t total = n * W;
  for (uint64_t i = blockIdx.x * (uint64_t)PGPU_HLL_THREADS + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * PGPU_HLL_THREADS) {
    const uint64_t row = i / W;
    const uint64_t k = (uint64_t)keys[row];
    out[i] = k < inner ? regs[k * W + (i - row * W)] : 0;
  }
}
}  // namespace

hipError_t pgpu_launch_hll_gather(const uint32_t* regs, const int64_t* keys, uint64_t n, uint64_t inner, int32_t log2m,
                                  uint32_t* out, hipStream_t st) {
  const uint32_t W = pgpu_hll_words_of(log2m);
  if (W == 0 || !regs || !keys || !out) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(hll_gather_kernel, dim3(grid_of(n * W)), dim3(PGPU_HLL_THREADS), 0, st, regs, keys, n, inner, W, out);
  return hipGetLastError();
}
