// Value runs of a group table (pgpu_table_runs, include/pinot_gpu.h): the broker-mergeable intermediates of
// DISTINCTCOUNT, PERCENTILE and MODE.  Section 0 of the table GROUP BY g, c -- count(g, cid), cell key = g + inner * cid
// -- is the value set (DistinctCountAggregationFunction.java:252-310), the value list (PercentileAggregationFunction
// .java:82-100) and the value -> count map (ModeAggregationFunction.java:416-456) of every group at once.  This stage
// hands it back as a CSR over the `inner` keys g:
//   offsets  uint64[inner + 1]  offsets[g] = the occupied cells (g', cid) with g' < g; offsets[inner] = the total
//   cids     uint32[total]      elements offsets[g] .. offsets[g + 1]: the occupied cid of g, strictly ascending
//   counts   int64[total]       their section-0 counts
// A cell is occupied when its count is > 0, the test of the fold and the selection, so offsets[g + 1] - offsets[g] is
// the fold's distinct-count section, cell for cell.  Every element has exactly one writer and a plain store; nothing
// is accumulated with atomics, so the output does not depend on scheduling.  No element with an index >= the
// caller's run_capacity is written.
//
// Two phases, so that a caller that synchronises anyway (pgpu_query_collect_runs) reads the total between them:
// count (offsets, complete whatever the capacity) and emit (cids, counts).  Dense input, over chunks of cid in
// pgpu_select.hip's two orientations (inner < 64: a wave owns a (g, chunk) with its lanes along cid; inner >= 64: a
// thread owns it and adjacent lanes read adjacent cells):
//   runs_partial_kernel  partial[chunk][g] = occupied cells of the chunk
//   runs_scan_kernel     partial[.][g] becomes its exclusive prefix over chunks, in place, and totals[g] the key's sum;
//                        rocPRIM's exclusive scan of totals[0 .. inner] (a 0 behind the last key) is `offsets`
//   runs_emit_kernel     per (g, chunk), from offsets[g] + partial[chunk][g] on: a lane's position is the popcount of
//                        the occupancy ballot below it plus a running base; a thread walks its chunk with a counter.
//                        The thread's stores (4 + 8 B to its own region) are uncoalesced across lanes.
// Hash input: every slot becomes (g << 32 | cid, count) -- an empty slot the largest key -- sorted by key (rocPRIM
// radix sort); offsets[g] is the position of the first key not below g << 32 (a binary search per g: the count of the
// keys below), and cids / counts are the sorted prefix.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/pinot_gpu.h"
#include "pgpu_axis.h"

#define PGPU_RUNS_THREADS PGPU_AXIS_THREADS
#define PGPU_RUNS_WAVES PGPU_AXIS_WAVES
#define PGPU_RUNS_UNROLL 8          // cells per thread whose counts are loaded before any is used
#define PGPU_RUNS_WAVE_UNROLL 4     // steps of 64 cid a wave loads before it places any
#define PGPU_RUNS_SCAN_BY_WAVE 4096  // inner below this: the chunk prefix of a key is taken by a wave, not a thread

namespace {

#define FI __device__ __forceinline__

// Inclusive prefix sum over the wave's 64 lanes.
FI int64_t wave_inclusive(int64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t t = shfl_up64(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// WAVE: the (g, chunk) of this wave, false when there is none (whole waves leave together).
FI bool wave_job(uint64_t inner, uint32_t nchunks, uint64_t* g, uint32_t* ck) {
  const uint64_t w = blockIdx.x * (uint64_t)PGPU_RUNS_WAVES + (threadIdx.x >> 6);
  if (w >= inner * nchunks) return false;
  *ck = (uint32_t)(w / inner);
  *g = w - (uint64_t)*ck * inner;
  return true;
}

template <bool WAVE>
__global__ __launch_bounds__(PGPU_RUNS_THREADS) void runs_partial_kernel(const int64_t* __restrict__ in, uint64_t inner,
                                                                         uint64_t card, uint64_t chunk, uint32_t nchunks,
                                                                         PartialAt at, int64_t* __restrict__ partial) {
  uint64_t g;
  uint32_t ck;
  const int lane = threadIdx.x & 63;
  if (WAVE) {
    if (!wave_job(inner, nchunks, &g, &ck)) return;
  } else {
    g = blockIdx.x * (uint64_t)PGPU_RUNS_THREADS + threadIdx.x;
    ck = blockIdx.y;
    if (g >= inner) return;
  }
  const uint64_t c0 = ck * chunk;
  const uint64_t c1 = c0 + chunk < card ? c0 + chunk : card;
  const uint64_t step = WAVE ? 64 : 1;
  int64_t sum = 0;
  for (uint64_t c = c0 + (WAVE ? lane : 0); c < c1; c += step * PGPU_RUNS_UNROLL) {
    int64_t cnt[PGPU_RUNS_UNROLL];
#pragma unroll
    for (int u = 0; u < PGPU_RUNS_UNROLL; ++u) cnt[u] = c + u * step < c1 ? in[(c + u * step) * inner + g] : 0;
#pragma unroll
    for (int u = 0; u < PGPU_RUNS_UNROLL; ++u) sum += cnt[u] > 0;
  }
  if (WAVE) {
    sum = shfl64(wave_inclusive(sum, lane), 63);
    if (lane != 0) return;
  }
  partial[ck * at.sc + g * at.sg] = sum;
}

// partial(., g) -> its exclusive prefix over chunks, totals[g] = its sum, totals[inner] = 0.  !WAVE: one thread per g;
// WAVE: one wave per g, lanes along chunks.
template <bool WAVE>
__global__ __launch_bounds__(PGPU_RUNS_THREADS) void runs_scan_kernel(int64_t* __restrict__ partial, uint64_t inner,
                                                                      uint32_t nchunks, PartialAt at,
                                                                      uint64_t* __restrict__ totals) {
  const int lane = threadIdx.x & 63;
  const uint64_t g = WAVE ? blockIdx.x * (uint64_t)PGPU_RUNS_WAVES + (threadIdx.x >> 6)
                          : blockIdx.x * (uint64_t)PGPU_RUNS_THREADS + threadIdx.x;
  if (g >= inner) return;
  int64_t run = 0;
  if (WAVE) {
    for (uint32_t base = 0; base < nchunks; base += 64) {
      const uint32_t ck = base + lane;
      const int64_t v = ck < nchunks ? partial[ck * at.sc + g * at.sg] : 0;
      const int64_t inc = wave_inclusive(v, lane);
      if (ck < nchunks) partial[ck * at.sc + g * at.sg] = run + inc - v;
      run += shfl64(inc, 63);
    }
    if (lane != 0) return;
  } else {
    for (uint32_t base = 0; base < nchunks; base += PGPU_RUNS_UNROLL) {
      int64_t v[PGPU_RUNS_UNROLL];
#pragma unroll
      for (int u = 0; u < PGPU_RUNS_UNROLL; ++u) v[u] = base + u < nchunks ? partial[(base + u) * at.sc + g * at.sg] : 0;
#pragma unroll
      for (int u = 0; u < PGPU_RUNS_UNROLL; ++u) {
        if (base + u < nchunks) partial[(base + u) * at.sc + g * at.sg] = run;
        run += v[u];
      }
    }
  }
  totals[g] = (uint64_t)run;
  if (g == 0) totals[inner] = 0;
}

// The runs of (g, chunk) at offsets[g] + partial(chunk, g) on; nothing at or beyond `cap`.
template <bool WAVE>
__global__ __launch_bounds__(PGPU_RUNS_THREADS) void runs_emit_kernel(const int64_t* __restrict__ in, uint64_t inner,
                                                                      uint64_t card, uint64_t chunk, uint32_t nchunks,
                                                                      PartialAt at, const int64_t* __restrict__ partial,
                                                                      const uint64_t* __restrict__ offsets,
                                                                      uint32_t* __restrict__ cids,
                                                                      int64_t* __restrict__ counts, uint64_t cap) {
  uint64_t g;
  uint32_t ck;
  const int lane = threadIdx.x & 63;
  if (WAVE) {
    if (!wave_job(inner, nchunks, &g, &ck)) return;
  } else {
    g = blockIdx.x * (uint64_t)PGPU_RUNS_THREADS + threadIdx.x;
    ck = blockIdx.y;
    if (g >= inner) return;
  }
  uint64_t pos = offsets[g] + (uint64_t)partial[ck * at.sc + g * at.sg];
  const uint64_t c0 = ck * chunk;
  const uint64_t c1 = c0 + chunk < card ? c0 + chunk : card;
  if (WAVE) {
    // (pos is the same in every lane: the loop is wave-uniform)
    const uint64_t below = (1ull << lane) - 1;
    for (uint64_t base = c0; base < c1 && pos < cap; base += 64 * PGPU_RUNS_WAVE_UNROLL) {
      int64_t cnt[PGPU_RUNS_WAVE_UNROLL];
#pragma unroll
      for (int u = 0; u < PGPU_RUNS_WAVE_UNROLL; ++u) {
        const uint64_t c = base + 64 * u + lane;
        cnt[u] = c < c1 ? in[c * inner + g] : 0;
      }
#pragma unroll
      for (int u = 0; u < PGPU_RUNS_WAVE_UNROLL; ++u) {
        const bool occ = cnt[u] > 0;
        const uint64_t mask = __ballot(occ);
        const uint64_t at_ = pos + (uint64_t)__popcll(mask & below);
        if (occ && at_ < cap) {
          cids[at_] = (uint32_t)(base + 64 * u + lane);
          counts[at_] = cnt[u];
        }
        pos += (uint64_t)__popcll(mask);
      }
    }
  } else {
    for (uint64_t c = c0; c < c1 && pos < cap; c += PGPU_RUNS_UNROLL) {
      int64_t cnt[PGPU_RUNS_UNROLL];
#pragma unroll
      for (int u = 0; u < PGPU_RUNS_UNROLL; ++u) cnt[u] = c + u < c1 ? in[(c + u) * inner + g] : 0;
#pragma unroll
      for (int u = 0; u < PGPU_RUNS_UNROLL; ++u) {
        if (cnt[u] <= 0) continue;
        if (pos < cap) {
          cids[pos] = (uint32_t)(c + u);
          counts[pos] = cnt[u];
        }
        ++pos;
      }
    }
  }
}

// ---- hash input ----
// (g, cid) of every slot as one sortable key; empty slots sort last and name no key (g = 2^32 - 1 >= inner).
__global__ __launch_bounds__(PGPU_RUNS_THREADS) void runs_hash_keys_kernel(const int64_t* __restrict__ in, uint64_t N,
                                                                           int32_t nsec, uint64_t inner,
                                                                           uint64_t* __restrict__ keys,
                                                                           int64_t* __restrict__ counts) {
  for (uint64_t i = blockIdx.x * (uint64_t)PGPU_RUNS_THREADS + threadIdx.x; i < N;
       i += (uint64_t)gridDim.x * PGPU_RUNS_THREADS) {
    const int64_t cnt = in[i];
    uint64_t k = ~0ull;
    if (cnt > 0) {
      const uint64_t key = (uint64_t)in[(uint64_t)nsec * N + i];
      const uint64_t cid = key / inner;
      // cid is an id of a global dictionary, an int32, on every table the runtime builds.  A key beyond that cannot be
      // packed: its slot is dropped here though the fold counted it -- a hand-made table with such keys is outside
      // this call's contract, as it is outside the selection's.
      if (cid < (1ull << 32)) k = ((key - cid * inner) << 32) | cid;
    }
    keys[i] = k;
    counts[i] = k == ~0ull ? 0 : cnt;
  }
}
// offsets[g] = the sorted keys below g << 32, g in [0, inner]: the first position whose key is not below it.
__global__ __launch_bounds__(PGPU_RUNS_THREADS) void runs_hash_offsets_kernel(const uint64_t* __restrict__ skeys,
                                                                              uint64_t N, uint64_t inner,
                                                                              uint64_t* __restrict__ offsets) {
  for (uint64_t g = blockIdx.x * (uint64_t)PGPU_RUNS_THREADS + threadIdx.x; g <= inner;
       g += (uint64_t)gridDim.x * PGPU_RUNS_THREADS) {
    const uint64_t want = g << 32;
    uint64_t lo = 0, hi = N;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (skeys[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    offsets[g] = lo;
  }
}
__global__ __launch_bounds__(PGPU_RUNS_THREADS) void runs_hash_emit_kernel(const uint64_t* __restrict__ skeys,
                                                                           const int64_t* __restrict__ scounts,
                                                                           uint64_t N, uint32_t* __restrict__ cids,
                                                                           int64_t* __restrict__ counts, uint64_t cap) {
  const uint64_t n = N < cap ? N : cap;
  for (uint64_t i = blockIdx.x * (uint64_t)PGPU_RUNS_THREADS + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * PGPU_RUNS_THREADS) {
    const uint64_t k = skeys[i];
    if (k == ~0ull) continue;  // (the empty slots are the sorted tail)
    cids[i] = (uint32_t)k;
    counts[i] = scounts[i];
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// rocPRIM's temporary bytes: the sort of n pairs (hash) or the scan of n totals (dense).  A host-side query, asked
// anew every time: the answer belongs to the current device.
size_t prim_temp(uint64_t n, bool sort) {
  size_t b = 0;
  if (sort)
    (void)rocprim::radix_sort_pairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (int64_t*)nullptr,
                                    (int64_t*)nullptr, (size_t)n);
  else
    (void)rocprim::exclusive_scan(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)n,
                                  rocprim::plus<uint64_t>());
  return std::max<size_t>(b, 1);
}

// Where the two phases keep their state in the temporary buffer.
struct RunsTemp {
  // dense
  uint64_t chunk = 0;
  uint32_t nchunks = 0;
  int64_t* partial = nullptr;
  uint64_t* totals = nullptr;
  // hash
  uint64_t *keys = nullptr, *skeys = nullptr;
  int64_t *counts = nullptr, *scounts = nullptr;
  void* prim = nullptr;
  size_t prim_bytes = 0, bytes = 0;
};
RunsTemp runs_temp(void* temp, uint64_t N, bool hash, uint64_t inner, int num_cus) {
  RunsTemp r;
  char* t = (char*)temp;
  if (hash) {
    const size_t a = align256(8 * N);
    r.keys = (uint64_t*)t;
    r.counts = (int64_t*)(t + a);
    r.skeys = (uint64_t*)(t + 2 * a);
    r.scounts = (int64_t*)(t + 3 * a);
    r.prim = t + 4 * a;
    r.prim_bytes = align256(prim_temp(N, true));
    r.bytes = 4 * a + r.prim_bytes;
    return r;
  }
  chunks_of(inner, N / inner, num_cus, &r.chunk, &r.nchunks);
  const size_t a = align256(8ull * r.nchunks * inner), b = align256(8 * (inner + 1));
  r.partial = (int64_t*)t;
  r.totals = (uint64_t*)(t + a);
  r.prim = t + a + b;
  r.prim_bytes = align256(prim_temp(inner + 1, false));
  r.bytes = a + b + r.prim_bytes;
  return r;
}

}  // namespace

// Temporary bytes the two phases share (the emit reads what the count left there).
size_t pgpu_runs_temp_bytes(uint64_t N, bool hash, uint64_t inner, int num_cus) {
  if (inner == 0 || N == 0) return 0;
  return runs_temp(nullptr, N, hash, inner, num_cus).bytes;
}

// Phase 1: enqueue the count of the runs of `in` ([nsec (+ key word when hash)][N] int64) on `st`: offsets[inner + 1],
// complete.  temp holds pgpu_runs_temp_bytes(...) bytes and is handed to pgpu_launch_runs_emit as it is left here.  The
// caller has checked N % inner == 0 for dense input.
hipError_t pgpu_launch_runs_count(const int64_t* in, uint64_t N, int32_t nsec, bool hash, uint64_t inner,
                                  uint64_t* offsets, void* temp, size_t temp_bytes, int num_cus, hipStream_t st) {
  if (inner == 0 || N == 0 || !temp) return hipErrorInvalidValue;
  const RunsTemp r = runs_temp(temp, N, hash, inner, num_cus);
  if (temp_bytes < r.bytes) return hipErrorInvalidValue;
  const unsigned T = PGPU_RUNS_THREADS;
  size_t tb = r.prim_bytes;
  if (hash) {
    hipLaunchKernelGGL(runs_hash_keys_kernel, dim3(grid_of(N)), dim3(T), 0, st, in, N, nsec, inner, r.keys, r.counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(r.prim, tb, r.keys, r.skeys, r.counts, r.scounts, (size_t)N, 0, 64, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(runs_hash_offsets_kernel, dim3(grid_of(inner + 1)), dim3(T), 0, st, r.skeys, N, inner, offsets);
    return hipGetLastError();
  }
  const uint64_t card = N / inner;
  const bool scan_by_wave = inner < PGPU_RUNS_SCAN_BY_WAVE;
  const PartialAt at = scan_by_wave ? PartialAt{1, r.nchunks} : PartialAt{inner, 1};
  const unsigned bx = (unsigned)((inner + T - 1) / T);
  const unsigned waves = (unsigned)((inner * r.nchunks + PGPU_RUNS_WAVES - 1) / PGPU_RUNS_WAVES);
  if (inner < 64)
    hipLaunchKernelGGL((runs_partial_kernel<true>), dim3(waves), dim3(T), 0, st, in, inner, card, r.chunk, r.nchunks, at,
                       r.partial);
  else
    hipLaunchKernelGGL((runs_partial_kernel<false>), dim3(bx, r.nchunks), dim3(T), 0, st, in, inner, card, r.chunk,
                       r.nchunks, at, r.partial);
  if (scan_by_wave)
    hipLaunchKernelGGL((runs_scan_kernel<true>), dim3((unsigned)((inner + PGPU_RUNS_WAVES - 1) / PGPU_RUNS_WAVES)),
                       dim3(T), 0, st, r.partial, inner, r.nchunks, at, r.totals);
  else
    hipLaunchKernelGGL((runs_scan_kernel<false>), dim3(bx), dim3(T), 0, st, r.partial, inner, r.nchunks, at, r.totals);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return rocprim::exclusive_scan(r.prim, tb, r.totals, offsets, (uint64_t)0, (size_t)(inner + 1),
                                 rocprim::plus<uint64_t>(), st);
}

// Phase 2, behind phase 1 on `st` with the same arguments and the temporary buffer as it left it: cids and counts, the
// elements with an index below `cap` only.
hipError_t pgpu_launch_runs_emit(const int64_t* in, uint64_t N, int32_t nsec, bool hash, uint64_t inner,
                                 const uint64_t* offsets, uint32_t* cids, int64_t* counts, uint64_t cap, void* temp,
                                 size_t temp_bytes, int num_cus, hipStream_t st) {
  if (inner == 0 || N == 0 || !temp) return hipErrorInvalidValue;
  if (cap == 0) return hipSuccess;
  const RunsTemp r = runs_temp(temp, N, hash, inner, num_cus);
  if (temp_bytes < r.bytes) return hipErrorInvalidValue;
  const unsigned T = PGPU_RUNS_THREADS;
  if (hash) {
    hipLaunchKernelGGL(runs_hash_emit_kernel, dim3(grid_of(std::min(N, cap))), dim3(T), 0, st, r.skeys, r.scounts, N,
                       cids, counts, cap);
    return hipGetLastError();
  }
  const uint64_t card = N / inner;
  const PartialAt at = inner < PGPU_RUNS_SCAN_BY_WAVE ? PartialAt{1, r.nchunks} : PartialAt{inner, 1};
  if (inner < 64)
    hipLaunchKernelGGL((runs_emit_kernel<true>),
                       dim3((unsigned)((inner * r.nchunks + PGPU_RUNS_WAVES - 1) / PGPU_RUNS_WAVES)), dim3(T), 0, st, in,
                       inner, card, r.chunk, r.nchunks, at, r.partial, offsets, cids, counts, cap);
  else
    hipLaunchKernelGGL((runs_emit_kernel<false>), dim3((unsigned)((inner + T - 1) / T), r.nchunks), dim3(T), 0, st, in,
                       inner, card, r.chunk, r.nchunks, at, r.partial, offsets, cids, counts, cap);
  return hipGetLastError();
}
