// Most frequent value over the value axis of a group table (pgpu_table_mode, include/pinot_gpu.h): MODE(c) with group
// columns g runs as GROUP BY g, c like DISTINCTCOUNT (pgpu_fold.hip) and PERCENTILE (pgpu_select.hip).  Section 0 of
// that table -- count(g, cid), cell key = g + inner * cid -- is ModeAggregationFunction.java:463-672's value -> count
// map per group with the values as ids of the sorted global dictionary, and the mode is an argmax over cid.  The
// reduction runs behind the fold (and the selection), on the same stream, and writes per key g the tuple
//   M  largest count            T  number of ids with that count (the tied ids)
//   LO smallest tied id         HI largest tied id          S  sum of values[cid] over the tied ids (AVG reducer only)
// -- all 0 for a key with no cell of count > 0 -- from which MIN / MAX / AVG of the tied values follow on the host
// (ids are ordered as their values).  The tuple of a range of cid is a monoid: of two ranges the larger M wins whole,
// equal M > 0 merge (T and S add, LO min, HI max).  Counts are compared as int64.
//
// Dense input, chunks of cid cut as for the selection (chunks_of, pgpu_axis.h) and in its two orientations:
//   mode_partial_kernel  one tuple per (chunk, g).  inner >= 64 puts lanes along g: a thread walks its chunk in
//                        ascending cid, eight counts loaded before the first is used.  inner < 64 gives a wave a
//                        (g, chunk) with its lanes along cid: a lane walks every 64th cid in ascending order, then the
//                        lanes' tuples are combined by a butterfly of shuffles.  One chunk: the tuple is the output.
//   mode_combine_kernel  merges the chunk tuples of a key in ascending chunk order: one thread per g, or while
//                        inner < 4,096 (many chunks, few keys) one wave per g that takes 64 chunks per step.
// Every output cell has one writer and a plain store, and every add of S happens in an order the geometry fixes, so
// the dense result -- S included -- does not depend on scheduling.
// One-word hash input (g = key % inner, cid = key / inner) is not sorted: the output is initialised, pass one takes
// the int64 atomic max of the counts into M[g], pass two visits the slots with count = M[g] > 0 and adds to T,
// takes the atomic min / max of cid into LO / HI and adds values[cid] to S with a float64 atomic, and a kernel over g
// writes the 0 of LO for the empty keys.  M, T, LO and HI are scheduling-independent; S is exact up to the order of
// its adds.  With inner = 1 every slot is of the one key: both passes merge a wave's slots by shuffles first and
// issue one atomic per wave and section, not one per slot on the same address.
// values[] is indexed by min(cid, num_values - 1): no launch reads outside it, whatever the table holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pinot_gpu.h"
#include "pgpu_axis.h"

#define PGPU_MODE_THREADS PGPU_AXIS_THREADS
#define PGPU_MODE_WAVES PGPU_AXIS_WAVES
#define PGPU_MODE_UNROLL 8              // cells per thread whose counts are loaded before any is used
#define PGPU_MODE_COMBINE_BY_WAVE 4096  // inner below this: the chunks of a key are merged by a wave, not a thread

// The tuple sections of `count` keys each: the output ([inner]) or the chunk tuples, laid out by `at`.
struct ModeAt {
  int64_t *m, *t, *lo, *hi;
  double* s;
  PartialAt at;
};

namespace {

#define FI __device__ __forceinline__

struct ModeTuple {
  int64_t m, t, lo, hi;
  double s;
};

// The monoid.  (Commutative, bit for bit: IEEE addition is.)
template <bool AVG>
FI ModeTuple mode_merge(const ModeTuple& a, const ModeTuple& b) {
  if (b.m > a.m) return b;
  if (b.m < a.m || a.m <= 0) return a;
  ModeTuple r;
  r.m = a.m;
  r.t = a.t + b.t;
  r.lo = b.lo < a.lo ? b.lo : a.lo;
  r.hi = b.hi > a.hi ? b.hi : a.hi;
  r.s = AVG ? a.s + b.s : 0.0;
  return r;
}

// One more cell, of a larger cid than every cell the tuple holds.
template <bool AVG>
FI void mode_cell(ModeTuple& a, int64_t cnt, uint64_t cid, const double* __restrict__ values, uint64_t last_value) {
  if (cnt <= 0 || cnt < a.m) return;
  const double v = AVG ? values[cid < last_value ? cid : last_value] : 0.0;
  if (cnt > a.m) {
    a.m = cnt;
    a.t = 1;
    a.lo = (int64_t)cid;
    a.s = v;
  } else {
    a.t += 1;
    a.s += v;
  }
  a.hi = (int64_t)cid;
}

// Butterfly over the wave's 64 lanes: every lane ends with the merge of all, in the same fixed tree.
template <bool AVG>
FI ModeTuple mode_wave(ModeTuple a) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    ModeTuple b;
    b.m = shfl_xor64(a.m, d);
    b.t = shfl_xor64(a.t, d);
    b.lo = shfl_xor64(a.lo, d);
    b.hi = shfl_xor64(a.hi, d);
    b.s = AVG ? __longlong_as_double(shfl_xor64(__double_as_longlong(a.s), d)) : 0.0;
    a = mode_merge<AVG>(a, b);
  }
  return a;
}

template <bool AVG>
FI ModeTuple mode_load(const ModeAt& at, uint64_t i) {
  ModeTuple a;
  a.m = at.m[i];
  a.t = at.t[i];
  a.lo = at.lo[i];
  a.hi = at.hi[i];
  a.s = AVG ? at.s[i] : 0.0;
  return a;
}
template <bool AVG>
FI void mode_store(const ModeAt& at, uint64_t i, const ModeTuple& a) {
  at.m[i] = a.m;
  at.t[i] = a.t;
  at.lo[i] = a.lo;
  at.hi[i] = a.hi;
  if (AVG) at.s[i] = a.s;
}

// dst = the chunk tuples, or with one chunk the output itself (at = {0, 1}).
template <bool WAVE, bool AVG>
__global__ __launch_bounds__(PGPU_MODE_THREADS) void mode_partial_kernel(const int64_t* __restrict__ in, uint64_t inner,
                                                                         uint64_t card, uint64_t chunk, uint32_t nchunks,
                                                                         const double* __restrict__ values,
                                                                         uint64_t last_value, ModeAt dst) {
  uint64_t g;
  uint32_t ck;
  const int lane = threadIdx.x & 63;
  if (WAVE) {
    // the (g, chunk) of this wave (whole waves leave together)
    const uint64_t w = blockIdx.x * (uint64_t)PGPU_MODE_WAVES + (threadIdx.x >> 6);
    if (w >= inner * nchunks) return;
    ck = (uint32_t)(w / inner);
    g = w - (uint64_t)ck * inner;
  } else {
    g = blockIdx.x * (uint64_t)PGPU_MODE_THREADS + threadIdx.x;
    ck = blockIdx.y;
    if (g >= inner) return;
  }
  const uint64_t c0 = ck * chunk;
  const uint64_t c1 = c0 + chunk < card ? c0 + chunk : card;
  const uint64_t step = WAVE ? 64 : 1;
  ModeTuple a{0, 0, 0, 0, 0.0};
  for (uint64_t c = c0 + (WAVE ? lane : 0); c < c1; c += step * PGPU_MODE_UNROLL) {
    int64_t cnt[PGPU_MODE_UNROLL];
#pragma unroll
    for (int u = 0; u < PGPU_MODE_UNROLL; ++u) cnt[u] = c + u * step < c1 ? in[(c + u * step) * inner + g] : 0;
#pragma unroll
    for (int u = 0; u < PGPU_MODE_UNROLL; ++u) mode_cell<AVG>(a, cnt[u], c + u * step, values, last_value);
  }
  if (WAVE) {
    a = mode_wave<AVG>(a);
    if (lane != 0) return;
  }
  mode_store<AVG>(dst, ck * dst.at.sc + g * dst.at.sg, a);
}

// The chunk tuples of a key merged in ascending chunk order into the output.
template <bool WAVE, bool AVG>
__global__ __launch_bounds__(PGPU_MODE_THREADS) void mode_combine_kernel(ModeAt part, uint64_t inner, uint32_t nchunks,
                                                                         ModeAt out) {
  const int lane = threadIdx.x & 63;
  const uint64_t g = WAVE ? blockIdx.x * (uint64_t)PGPU_MODE_WAVES + (threadIdx.x >> 6)
                          : blockIdx.x * (uint64_t)PGPU_MODE_THREADS + threadIdx.x;
  if (g >= inner) return;
  ModeTuple a{0, 0, 0, 0, 0.0};
  if (WAVE) {
    for (uint32_t base = 0; base < nchunks; base += 64) {
      const uint32_t ck = base + lane;
      ModeTuple b{0, 0, 0, 0, 0.0};
      if (ck < nchunks) b = mode_load<AVG>(part, ck * part.at.sc + g * part.at.sg);
      a = mode_merge<AVG>(a, mode_wave<AVG>(b));
    }
    if (lane != 0) return;
  } else {
    for (uint32_t ck = 0; ck < nchunks; ++ck)
      a = mode_merge<AVG>(a, mode_load<AVG>(part, ck * part.at.sc + g * part.at.sg));
  }
  mode_store<AVG>(out, g, a);
}

// ---- hash input ----
// LO starts at the identity of its atomic min; mode_hash_finish_kernel makes it the 0 of an empty key.
template <bool AVG>
__global__ __launch_bounds__(PGPU_MODE_THREADS) void mode_hash_init_kernel(ModeAt out, uint64_t inner) {
  for (uint64_t g = blockIdx.x * (uint64_t)PGPU_MODE_THREADS + threadIdx.x; g < inner;
       g += (uint64_t)gridDim.x * PGPU_MODE_THREADS) {
    out.m[g] = 0;
    out.t[g] = 0;
    out.lo[g] = INT64_MAX;
    out.hi[g] = 0;
    if (AVG) out.s[g] = 0.0;
  }
}
__global__ __launch_bounds__(PGPU_MODE_THREADS) void mode_hash_finish_kernel(ModeAt out, uint64_t inner) {
  for (uint64_t g = blockIdx.x * (uint64_t)PGPU_MODE_THREADS + threadIdx.x; g < inner;
       g += (uint64_t)gridDim.x * PGPU_MODE_THREADS)
    if (out.m[g] <= 0) out.lo[g] = 0;
}
// PASS 1: M[g] = max count.  PASS 2: the slots whose count is M[g] are the tied ids.  ONE (inner = 1, aggregation
// only): every slot is of the one key, whose cell every atomic would meet -- a thread keeps the tuple of its slots, the
// wave merges its lanes' by shuffles and one lane updates the cell.
template <int PASS, bool AVG, bool ONE>
__global__ __launch_bounds__(PGPU_MODE_THREADS) void mode_hash_kernel(const int64_t* __restrict__ in, uint64_t N,
                                                                      int32_t nsec, uint64_t inner,
                                                                      const double* __restrict__ values,
                                                                      uint64_t last_value, ModeAt out) {
  ModeTuple a{0, 0, 0, 0, 0.0};
  const int64_t m0 = ONE && PASS == 2 ? out.m[0] : 0;
  for (uint64_t i = blockIdx.x * (uint64_t)PGPU_MODE_THREADS + threadIdx.x; i < N;
       i += (uint64_t)gridDim.x * PGPU_MODE_THREADS) {
    const int64_t cnt = in[i];
    if (cnt <= 0) continue;
    const uint64_t key = (uint64_t)in[(uint64_t)nsec * N + i];
    if (ONE) {
      if (PASS == 1) {
        if (cnt > a.m) a.m = cnt;
      } else if (cnt == m0) {
        const ModeTuple b{cnt, 1, (int64_t)key, (int64_t)key, AVG ? values[key < last_value ? key : last_value] : 0.0};
        a = mode_merge<AVG>(a, b);
      }
      continue;
    }
    const uint64_t cid = ((key | inner) >> 32) ? key / inner : (uint64_t)((uint32_t)key / (uint32_t)inner);
    const uint64_t g = key - cid * inner;
    if (PASS == 1) {
      // (M[g] only grows: a count that an earlier value of it already covers needs no atomic)
      if (cnt > __hip_atomic_load(&out.m[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax((long long*)&out.m[g], (long long)cnt);
    } else if (cnt == out.m[g]) {
      atomicAdd((unsigned long long*)&out.t[g], 1ull);
      atomicMin((long long*)&out.lo[g], (long long)cid);
      atomicMax((long long*)&out.hi[g], (long long)cid);
      if (AVG) atomicAdd(&out.s[g], values[cid < last_value ? cid : last_value]);
    }
  }
  if (!ONE) return;
  // (whole waves reach here: no lane left the loop by a return)
  if (PASS == 1) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t o = shfl_xor64(a.m, d);
      if (o > a.m) a.m = o;
    }
    if ((threadIdx.x & 63) == 0 && a.m > 0) atomicMax((long long*)&out.m[0], (long long)a.m);
  } else {
    a = mode_wave<AVG>(a);
    if ((threadIdx.x & 63) != 0 || a.t == 0) return;
    atomicAdd((unsigned long long*)&out.t[0], (unsigned long long)a.t);
    atomicMin((long long*)&out.lo[0], (long long)a.lo);
    atomicMax((long long*)&out.hi[0], (long long)a.hi);
    if (AVG) atomicAdd(&out.s[0], a.s);
  }
}

template <bool AVG>
hipError_t launch_mode(const int64_t* in, uint64_t N, int32_t nsec, bool hash, uint64_t inner, const double* values,
                       uint64_t num_values, int64_t* mode, void* temp, int num_cus, hipStream_t st) {
  const unsigned T = PGPU_MODE_THREADS;
  const uint64_t last_value = num_values ? num_values - 1 : 0;
  const ModeAt out{mode, mode + inner, mode + 2 * inner, mode + 3 * inner, (double*)(mode + 4 * inner), {0, 1}};
  if (hash) {
    hipLaunchKernelGGL((mode_hash_init_kernel<AVG>), dim3(grid_of(inner)), dim3(T), 0, st, out, inner);
    if (inner == 1) {
      hipLaunchKernelGGL((mode_hash_kernel<1, AVG, true>), dim3(grid_of(N)), dim3(T), 0, st, in, N, nsec, inner, values,
                         last_value, out);
      hipLaunchKernelGGL((mode_hash_kernel<2, AVG, true>), dim3(grid_of(N)), dim3(T), 0, st, in, N, nsec, inner, values,
                         last_value, out);
    } else {
      hipLaunchKernelGGL((mode_hash_kernel<1, AVG, false>), dim3(grid_of(N)), dim3(T), 0, st, in, N, nsec, inner, values,
                         last_value, out);
      hipLaunchKernelGGL((mode_hash_kernel<2, AVG, false>), dim3(grid_of(N)), dim3(T), 0, st, in, N, nsec, inner, values,
                         last_value, out);
    }
    hipLaunchKernelGGL(mode_hash_finish_kernel, dim3(grid_of(inner)), dim3(T), 0, st, out, inner);
    return hipGetLastError();
  }
  const uint64_t card = N / inner;
  uint64_t chunk;
  uint32_t nchunks;
  chunks_of(inner, card, num_cus, &chunk, &nchunks);
  ModeAt dst = out;
  const bool by_wave = inner < PGPU_MODE_COMBINE_BY_WAVE;
  if (nchunks > 1) {
    int64_t* t = (int64_t*)temp;
    const uint64_t n = (uint64_t)nchunks * inner;
    dst = ModeAt{t, t + n, t + 2 * n, t + 3 * n, (double*)(t + 4 * n),
                by_wave ? PartialAt{1, nchunks} : PartialAt{inner, 1}};
  }
  const unsigned bx = (unsigned)((inner + T - 1) / T);
  if (inner < 64)
    hipLaunchKernelGGL((mode_partial_kernel<true, AVG>),
                       dim3((unsigned)((inner * nchunks + PGPU_MODE_WAVES - 1) / PGPU_MODE_WAVES)), dim3(T), 0, st, in,
                       inner, card, chunk, nchunks, values, last_value, dst);
  else
    hipLaunchKernelGGL((mode_partial_kernel<false, AVG>), dim3(bx, nchunks), dim3(T), 0, st, in, inner, card, chunk,
                       nchunks, values, last_value, dst);
  if (nchunks > 1) {
    if (by_wave)
      hipLaunchKernelGGL((mode_combine_kernel<true, AVG>),
                         dim3((unsigned)((inner + PGPU_MODE_WAVES - 1) / PGPU_MODE_WAVES)), dim3(T), 0, st, dst, inner,
                         nchunks, out);
    else
      hipLaunchKernelGGL((mode_combine_kernel<false, AVG>), dim3(bx), dim3(T), 0, st, dst, inner, nchunks, out);
  }
  return hipGetLastError();
}

}  // namespace

// Temporary bytes pgpu_launch_mode needs for this input (0: none -- hash input, or dense input of one chunk).
size_t pgpu_mode_temp_bytes(uint64_t N, bool hash, uint64_t inner, bool avg, int num_cus) {
  if (hash || inner == 0 || N == 0) return 0;
  uint64_t chunk;
  uint32_t nchunks;
  chunks_of(inner, N / inner, num_cus, &chunk, &nchunks);
  return nchunks > 1 ? 8ull * (avg ? 5 : 4) * nchunks * inner : 0;
}

// Enqueue the mode reduction of `in` ([nsec (+ key word when hash)][N] int64) on `st`: mode = [4 (+ 1 when avg)][inner],
// the sections M, T, LO, HI (, S).  values = `num_values` doubles in device memory, read only when avg.  temp holds
// pgpu_mode_temp_bytes(...) bytes.  The caller has checked N % inner == 0 for dense input.
hipError_t pgpu_launch_mode(const int64_t* in, uint64_t N, int32_t nsec, bool hash, uint64_t inner, const double* values,
                            uint64_t num_values, bool avg, int64_t* mode, void* temp, size_t temp_bytes, int num_cus,
                            hipStream_t st) {
  if (nsec < 1 || inner == 0 || N == 0 || (avg && (!values || num_values == 0))) return hipErrorInvalidValue;
  if (temp_bytes < pgpu_mode_temp_bytes(N, hash, inner, avg, num_cus)) return hipErrorInvalidValue;
  return avg ? launch_mode<true>(in, N, nsec, hash, inner, values, num_values, mode, temp, num_cus, st)
             : launch_mode<false>(in, N, nsec, hash, inner, nullptr, 0, mode, temp, num_cus, st);
}
