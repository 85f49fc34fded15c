// Rank selection over the value axis of a group table (pgpu_table_select, include/pinot_gpu.h): PERCENTILE(c, p) with
// group columns g runs as GROUP BY g, c like DISTINCTCOUNT (pgpu_fold.hip).  Global dictionaries are sorted, so
// section 0 of that table -- count(g, cid), cell key = g + inner * cid -- is the sorted multiset of c per group, and
// PercentileAggregationFunction.java:152-165's values[(int) ((long) size * percentile / 100)] is the smallest cid whose
// running count along cid passes that rank.  The selection runs behind the fold, on the same stream: it reads the
// folded count N_g from the folded table and writes one int64 section per percentile behind it.
//
// Every output cell has exactly one writer and a plain store; nothing is accumulated with atomics, so the result does
// not depend on scheduling.  Dense input, three kernels over chunks of cid:
//   select_partial_kernel  partial[chunk][g] = sum of count(g, cid) over the chunk's cid
//   select_scan_kernel     partial[.][g] becomes its exclusive prefix over chunks, in place: one wave per g with its
//                          lanes along the chunks (partial laid out [g][chunk]) while inner < 4,096, where there are
//                          many chunks and few keys; one thread per g (partial [chunk][g]) from there on
//   select_pick_kernel     per (chunk, g): the ranks r_j with partial[chunk][g] <= r_j < partial[chunk + 1][g] fall in
//                          this chunk, which is walked once to the exact cid of each; chunk 0 writes the 0 of an empty
//                          key.  Exactly one chunk holds each rank, since r_j < N_g = the sum over all chunks.
// in two orientations: inner >= 64 puts lanes along g (adjacent lanes read adjacent cells, a thread walks its chunk);
// inner < 64 (aggregation only is inner = 1) gives a wave a (g, chunk) with its lanes along cid and a wave-level prefix
// by shuffles, so that no thread walks card cells alone.  One chunk (card small against inner) skips the first two.
// Hash input: every slot becomes (g << 32 | cid, count) -- an empty slot the largest key -- the pairs are sorted by key
// (rocPRIM radix sort), the counts scanned inclusively within each g (rocPRIM scan by key), and the element whose
// [exclusive, inclusive) interval holds r_j writes its cid; a kernel over g writes the 0 of the empty keys.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan_by_key.hpp>

#include "../../include/pinot_gpu.h"
#include "pgpu_axis.h"

#define PGPU_SEL_THREADS PGPU_AXIS_THREADS
#define PGPU_SEL_WAVES PGPU_AXIS_WAVES
#define PGPU_SEL_UNROLL 8       // cells per thread whose counts are loaded before any is used
#define PGPU_SEL_SCAN_BY_WAVE 4096  // inner below this: the chunk prefix of a key is taken by a wave, not a thread

// The percentiles, by value.
struct SelectRanks {
  double p[PGPU_SELECT_MAX];
  int32_t k;
};

namespace {

#define FI __device__ __forceinline__

// PercentileAggregationFunction.java:152-165 in IEEE double, this operation order, no contraction.  (A percentile
// within an ulp of 100 could round the quotient up to n, where the reference indexes past its list: the last value.)
FI int64_t select_rank(int64_t n, double p) {
#pragma clang fp contract(off)
  if (p == 100.0) return n - 1;
  const double x = (double)n * p;
  const int64_t r = (int64_t)(x / 100.0);
  return r < n ? r : n - 1;
}

// Inclusive prefix sum over the wave's 64 lanes.
FI int64_t wave_inclusive(int64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t t = shfl_up64(v, d);
    if (lane >= d) v += t;
  }
  return v;
}
FI int64_t occupied(int64_t cnt) { return cnt > 0 ? cnt : 0; }  // (the fold skips cells of count <= 0 too)

// WAVE: the (g, chunk) of this wave, false when there is none (whole waves leave together).
FI bool wave_job(uint64_t inner, uint32_t nchunks, uint64_t* g, uint32_t* ck) {
  const uint64_t w = blockIdx.x * (uint64_t)PGPU_SEL_WAVES + (threadIdx.x >> 6);
  if (w >= inner * nchunks) return false;
  *ck = (uint32_t)(w / inner);
  *g = w - (uint64_t)*ck * inner;
  return true;
}

template <bool WAVE>
__global__ __launch_bounds__(PGPU_SEL_THREADS) void select_partial_kernel(const int64_t* __restrict__ in, uint64_t inner,
                                                                          uint64_t card, uint64_t chunk, uint32_t nchunks,
                                                                          PartialAt at, int64_t* __restrict__ partial) {
  uint64_t g;
  uint32_t ck;
  const int lane = threadIdx.x & 63;
  if (WAVE) {
    if (!wave_job(inner, nchunks, &g, &ck)) return;
  } else {
    g = blockIdx.x * (uint64_t)PGPU_SEL_THREADS + threadIdx.x;
    ck = blockIdx.y;
    if (g >= inner) return;
  }
  const uint64_t c0 = ck * chunk;
  const uint64_t c1 = c0 + chunk < card ? c0 + chunk : card;
  const uint64_t step = WAVE ? 64 : 1;
  int64_t sum = 0;
  for (uint64_t c = c0 + (WAVE ? lane : 0); c < c1; c += step * PGPU_SEL_UNROLL) {
    int64_t cnt[PGPU_SEL_UNROLL];
#pragma unroll
    for (int u = 0; u < PGPU_SEL_UNROLL; ++u) cnt[u] = c + u * step < c1 ? in[(c + u * step) * inner + g] : 0;
#pragma unroll
    for (int u = 0; u < PGPU_SEL_UNROLL; ++u) sum += occupied(cnt[u]);
  }
  if (WAVE) {
    sum = shfl64(wave_inclusive(sum, lane), 63);
    if (lane != 0) return;
  }
  partial[ck * at.sc + g * at.sg] = sum;
}

// partial(., g) -> its exclusive prefix over chunks.  !WAVE: one thread per g; WAVE: one wave per g, lanes along chunks.
template <bool WAVE>
__global__ __launch_bounds__(PGPU_SEL_THREADS) void select_scan_kernel(int64_t* __restrict__ partial, uint64_t inner,
                                                                       uint32_t nchunks, PartialAt at) {
  const int lane = threadIdx.x & 63;
  const uint64_t g = WAVE ? blockIdx.x * (uint64_t)PGPU_SEL_WAVES + (threadIdx.x >> 6)
                          : blockIdx.x * (uint64_t)PGPU_SEL_THREADS + threadIdx.x;
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
  } else {
    for (uint32_t base = 0; base < nchunks; base += PGPU_SEL_UNROLL) {
      int64_t v[PGPU_SEL_UNROLL];
#pragma unroll
      for (int u = 0; u < PGPU_SEL_UNROLL; ++u) v[u] = base + u < nchunks ? partial[(base + u) * at.sc + g * at.sg] : 0;
#pragma unroll
      for (int u = 0; u < PGPU_SEL_UNROLL; ++u) {
        if (base + u < nchunks) partial[(base + u) * at.sc + g * at.sg] = run;
        run += v[u];
      }
    }
  }
}

// partial = nullptr: one chunk, which holds every rank.  folded = section 0 of the folded table (N_g), sel = the K
// sections behind it ([K][inner]).
template <bool WAVE>
__global__ __launch_bounds__(PGPU_SEL_THREADS) void select_pick_kernel(const int64_t* __restrict__ in, uint64_t inner,
                                                                       uint64_t card, uint64_t chunk, uint32_t nchunks,
                                                                       PartialAt at, const int64_t* __restrict__ partial,
                                                                       const int64_t* __restrict__ folded,
                                                                       SelectRanks ranks, int64_t* __restrict__ sel) {
  uint64_t g;
  uint32_t ck;
  const int lane = threadIdx.x & 63;
  if (WAVE) {
    if (!wave_job(inner, nchunks, &g, &ck)) return;
  } else {
    g = blockIdx.x * (uint64_t)PGPU_SEL_THREADS + threadIdx.x;
    ck = blockIdx.y;
    if (g >= inner) return;
  }
  const int64_t n = folded[g];
  const bool writer = !WAVE || lane == 0;
  if (n <= 0) {
    if (ck == 0 && writer)
      for (int j = 0; j < ranks.k; ++j) sel[(uint64_t)j * inner + g] = 0;
    return;
  }
  const int64_t lo = partial ? partial[ck * at.sc + g * at.sg] : 0;
  const int64_t hi = partial && ck + 1 < nchunks ? partial[(ck + 1) * at.sc + g * at.sg] : n;
  int64_t r[PGPU_SELECT_MAX];
  uint32_t need = 0;  // the ranks that fall in this chunk and are not placed yet
#pragma unroll
  for (int j = 0; j < PGPU_SELECT_MAX; ++j) {
    r[j] = j < ranks.k ? select_rank(n, ranks.p[j]) : 0;
    if (j < ranks.k && lo <= r[j] && r[j] < hi) need |= 1u << j;
  }
  if (!need) return;
  const uint64_t c0 = ck * chunk;
  const uint64_t c1 = c0 + chunk < card ? c0 + chunk : card;
  int64_t run = lo;
  if (WAVE) {
    // (need and run are the same in every lane: the loop is wave-uniform)
    for (uint64_t base = c0; base < c1 && need; base += 64) {
      const uint64_t c = base + lane;
      const int64_t inc = run + wave_inclusive(c < c1 ? occupied(in[c * inner + g]) : 0, lane);
#pragma unroll
      for (int j = 0; j < PGPU_SELECT_MAX; ++j) {
        if (!(need >> j & 1)) continue;
        const uint64_t past = __ballot(inc > r[j]);
        if (!past) continue;
        if (lane == 0) sel[(uint64_t)j * inner + g] = (int64_t)(base + (uint64_t)__builtin_ctzll(past));
        need &= ~(1u << j);
      }
      run = shfl64(inc, 63);
    }
  } else {
    for (uint64_t c = c0; c < c1 && need; c += PGPU_SEL_UNROLL) {
      int64_t cnt[PGPU_SEL_UNROLL];
#pragma unroll
      for (int u = 0; u < PGPU_SEL_UNROLL; ++u) cnt[u] = c + u < c1 ? in[(c + u) * inner + g] : 0;
#pragma unroll
      for (int u = 0; u < PGPU_SEL_UNROLL; ++u) {
        if (cnt[u] <= 0) continue;
        run += cnt[u];
#pragma unroll
        for (int j = 0; j < PGPU_SELECT_MAX; ++j) {
          if ((need >> j & 1) && run > r[j]) {
            sel[(uint64_t)j * inner + g] = (int64_t)(c + u);
            need &= ~(1u << j);
          }
        }
      }
    }
  }
}

// ---- hash input ----
// (g, cid) of every slot as one sortable key; empty slots sort last and name no key (g = 2^32 - 1 >= inner).
__global__ __launch_bounds__(PGPU_SEL_THREADS) void select_hash_keys_kernel(const int64_t* __restrict__ in, uint64_t N,
                                                                            int32_t nsec, uint64_t inner,
                                                                            uint64_t* __restrict__ keys,
                                                                            int64_t* __restrict__ counts) {
  for (uint64_t i = blockIdx.x * (uint64_t)PGPU_SEL_THREADS + threadIdx.x; i < N;
       i += (uint64_t)gridDim.x * PGPU_SEL_THREADS) {
    const int64_t cnt = in[i];
    uint64_t k = ~0ull;
    if (cnt > 0) {
      const uint64_t key = (uint64_t)in[(uint64_t)nsec * N + i];
      const uint64_t cid = key / inner;
      // cid is an id of a global dictionary, an int32, on every table the runtime builds.  A key beyond that cannot be
      // packed: its slot is dropped here though the fold counted it, so a rank of its g may then find no element and
      // that cell stays unwritten -- a hand-made table with such keys is outside this call's contract.
      if (cid < (1ull << 32)) k = ((key - cid * inner) << 32) | cid;
    }
    keys[i] = k;
    counts[i] = k == ~0ull ? 0 : cnt;
  }
}
struct SameGroup {
  __host__ __device__ bool operator()(uint64_t a, uint64_t b) const { return (a >> 32) == (b >> 32); }
};
// Sorted pairs with the counts' inclusive prefix within each g: element i covers the ranks [inc - count, inc).
__global__ __launch_bounds__(PGPU_SEL_THREADS) void select_hash_pick_kernel(const uint64_t* __restrict__ keys,
                                                                            const int64_t* __restrict__ counts,
                                                                            const int64_t* __restrict__ inc, uint64_t N,
                                                                            uint64_t inner,
                                                                            const int64_t* __restrict__ folded,
                                                                            SelectRanks ranks, int64_t* __restrict__ sel) {
  for (uint64_t i = blockIdx.x * (uint64_t)PGPU_SEL_THREADS + threadIdx.x; i < N;
       i += (uint64_t)gridDim.x * PGPU_SEL_THREADS) {
    const uint64_t k = keys[i];
    const uint64_t g = k >> 32;
    if (g >= inner) continue;
    const int64_t hi = inc[i], lo = hi - counts[i], n = folded[g];
    for (int j = 0; j < ranks.k; ++j) {
      const int64_t r = select_rank(n, ranks.p[j]);
      if (lo <= r && r < hi) sel[(uint64_t)j * inner + g] = (int64_t)(k & 0xFFFFFFFFull);
    }
  }
}
__global__ __launch_bounds__(PGPU_SEL_THREADS) void select_empty_kernel(const int64_t* __restrict__ folded, uint64_t inner,
                                                                        int32_t k, int64_t* __restrict__ sel) {
  for (uint64_t g = blockIdx.x * (uint64_t)PGPU_SEL_THREADS + threadIdx.x; g < inner;
       g += (uint64_t)gridDim.x * PGPU_SEL_THREADS)
    if (folded[g] <= 0)
      for (int j = 0; j < k; ++j) sel[(uint64_t)j * inner + g] = 0;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// rocPRIM's temporary bytes for the sort and the scan of N pairs.  Asked twice per selection (by the caller sizing its
// buffer, then by the launch checking it) and with the same N query after query: the last answer is kept per thread.
size_t hash_sort_temp(uint64_t N) {
  thread_local uint64_t last_n = 0;
  thread_local size_t last_bytes = 0;
  if (N == last_n && last_bytes) return last_bytes;
  size_t a = 0, b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (int64_t*)nullptr,
                                  (int64_t*)nullptr, (size_t)N);
  (void)rocprim::inclusive_scan_by_key(nullptr, b, (uint64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr, (size_t)N,
                                       rocprim::plus<int64_t>(), SameGroup());
  last_n = N;
  last_bytes = std::max<size_t>(std::max(a, b), 1);
  return last_bytes;
}

}  // namespace

// Temporary bytes pgpu_launch_select needs for this input (0: none).
size_t pgpu_select_temp_bytes(uint64_t N, bool hash, uint64_t inner, int num_cus) {
  if (inner == 0 || N == 0) return 0;
  if (hash) return 5 * align256(8 * N) + align256(hash_sort_temp(N));
  uint64_t chunk;
  uint32_t nchunks;
  chunks_of(inner, N / inner, num_cus, &chunk, &nchunks);
  return nchunks > 1 ? 8ull * nchunks * inner : 0;
}

// Enqueue the selection of `k` percentiles over `in` ([nsec (+ key word when hash)][N] int64) on `st`, behind the fold
// of the same input into `folded` ([nsec + 1][inner], already enqueued on `st`): sel = [k][inner].  temp holds
// pgpu_select_temp_bytes(...) bytes.  The caller has checked N % inner == 0 for dense input and the percentiles.
hipError_t pgpu_launch_select(const int64_t* in, uint64_t N, int32_t nsec, bool hash, uint64_t inner,
                              const double* percentiles, int32_t k, const int64_t* folded, int64_t* sel, void* temp,
                              size_t temp_bytes, int num_cus, hipStream_t st) {
  if (k < 1 || k > PGPU_SELECT_MAX || inner == 0 || N == 0) return hipErrorInvalidValue;
  if (temp_bytes < pgpu_select_temp_bytes(N, hash, inner, num_cus)) return hipErrorInvalidValue;
  SelectRanks ranks{};
  ranks.k = k;
  for (int j = 0; j < k; ++j) ranks.p[j] = percentiles[j];
  const unsigned T = PGPU_SEL_THREADS;
  if (hash) {
    char* t = (char*)temp;
    const size_t a = align256(8 * N);
    uint64_t* keys = (uint64_t*)t;
    int64_t* counts = (int64_t*)(t + a);
    uint64_t* skeys = (uint64_t*)(t + 2 * a);
    int64_t* scounts = (int64_t*)(t + 3 * a);
    int64_t* inc = (int64_t*)(t + 4 * a);
    void* rtemp = t + 5 * a;
    const size_t rbytes = temp_bytes - 5 * a;
    hipLaunchKernelGGL(select_hash_keys_kernel, dim3(grid_of(N)), dim3(T), 0, st, in, N, nsec, inner, keys, counts);
    hipLaunchKernelGGL(select_empty_kernel, dim3(grid_of(inner)), dim3(T), 0, st, folded, inner, k, sel);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = rbytes;
    e = rocprim::radix_sort_pairs(rtemp, tb, keys, skeys, counts, scounts, (size_t)N, 0, 64, st);
    if (e != hipSuccess) return e;
    tb = rbytes;
    e = rocprim::inclusive_scan_by_key(rtemp, tb, skeys, scounts, inc, (size_t)N, rocprim::plus<int64_t>(), SameGroup(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(select_hash_pick_kernel, dim3(grid_of(N)), dim3(T), 0, st, skeys, scounts, inc, N, inner, folded,
                       ranks, sel);
    return hipGetLastError();
  }
  const uint64_t card = N / inner;
  uint64_t chunk;
  uint32_t nchunks;
  chunks_of(inner, card, num_cus, &chunk, &nchunks);
  int64_t* partial = nchunks > 1 ? (int64_t*)temp : nullptr;
  const bool scan_by_wave = inner < PGPU_SEL_SCAN_BY_WAVE;
  const PartialAt at = scan_by_wave ? PartialAt{1, nchunks} : PartialAt{inner, 1};
  const unsigned bx = (unsigned)((inner + T - 1) / T);
  const unsigned waves = (unsigned)((inner * nchunks + PGPU_SEL_WAVES - 1) / PGPU_SEL_WAVES);
  const bool wave = inner < 64;
  if (partial) {
    if (wave)
      hipLaunchKernelGGL((select_partial_kernel<true>), dim3(waves), dim3(T), 0, st, in, inner, card, chunk, nchunks, at,
                         partial);
    else
      hipLaunchKernelGGL((select_partial_kernel<false>), dim3(bx, nchunks), dim3(T), 0, st, in, inner, card, chunk,
                         nchunks, at, partial);
    if (scan_by_wave)
      hipLaunchKernelGGL((select_scan_kernel<true>), dim3((unsigned)((inner + PGPU_SEL_WAVES - 1) / PGPU_SEL_WAVES)),
                         dim3(T), 0, st, partial, inner, nchunks, at);
    else
      hipLaunchKernelGGL((select_scan_kernel<false>), dim3(bx), dim3(T), 0, st, partial, inner, nchunks, at);
  }
  if (wave)
    hipLaunchKernelGGL((select_pick_kernel<true>), dim3(waves), dim3(T), 0, st, in, inner, card, chunk, nchunks, at,
                       partial, folded, ranks, sel);
  else
    hipLaunchKernelGGL((select_pick_kernel<false>), dim3(bx, nchunks), dim3(T), 0, st, in, inner, card, chunk, nchunks,
                       at, partial, folded, ranks, sel);
  return hipGetLastError();
}
