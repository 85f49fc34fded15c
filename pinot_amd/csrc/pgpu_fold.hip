// Fold of a group table over its last group column (pgpu_table_fold, include/pinot_gpu.h): DISTINCTCOUNT(c) with
// group columns g runs as GROUP BY g, c, whose table cell key = g + inner * cid is occupied exactly when group g met
// the value cid of c -- the reference's per-group bitmap of dictionary ids (DistinctCountAggregationFunction.java
// :66-250).  The fold reduces that table over cid into a dense table over the `inner` keys g: every input section by
// its own op over the cells of count > 0, plus one int64 section counting those cells, the distinct count.
//
// A pure bandwidth operation: section 0 (the counts) is read whole, the other sections only where count > 0, and
// 8 * (nsec + 1) * inner bytes are written.  Three shapes:
//   fold_columns_kernel  dense input, inner too large for an LDS table: one thread per g walks cid, so adjacent lanes
//                        read adjacent cells of every section; cid is split over blockIdx.y when inner alone does
//                        not fill the GPU, each thread ending with one atomic per section
//   fold_cells_kernel    one thread per input cell (dense: contiguous along cid, g = cell % inner; hash: one slot,
//                        g = key % inner), accumulated per workgroup in an LDS table of inner x (nsec + 1) cells
//                        and flushed once with global atomics; inner = 1 keeps the sums in registers and reduces
//                        them per wave.  Hash input whose output does not fit the LDS table updates HBM directly.
// The output is set to the sections' identities first (fold_init_kernel); every kernel then only adds to it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pinot_gpu.h"
#include "pgpu_axis.h"

// LDS table of fold_cells_kernel: 64 KiB is what a workgroup gets without opting in to more, and two such
// workgroups still share a CU's 160 KiB, so one's flush overlaps the other's reads.  inner x (nsec + 1) x 8 B
// beyond it takes fold_columns_kernel (dense) or HBM atomics (hash).
#define PGPU_FOLD_LDS_BYTES (64 * 1024)
#define PGPU_FOLD_THREADS 256
#define PGPU_FOLD_UNROLL 4  // cells per thread whose counts are loaded before any is used

// Section ops of the folded table, by value: op[nsec] is the appended distinct-count section.
struct FoldOps {
  int32_t op[PGPU_MAX_SECTIONS + 1];
};

namespace {

#define FI __device__ __forceinline__

FI int64_t fold_identity(int32_t op) {
  return op == PGPU_RED_MIN_I64 ? INT64_MAX : (op == PGPU_RED_MAX_I64 ? INT64_MIN : 0);
}
FI int64_t fold_combine(int32_t op, int64_t a, int64_t b) {
  if (op == PGPU_RED_SUM_I64) return a + b;
  if (op == PGPU_RED_SUM_F64) return __double_as_longlong(__longlong_as_double(a) + __longlong_as_double(b));
  if (op == PGPU_RED_MIN_I64) return b < a ? b : a;
  return b > a ? b : a;
}
// Atomic update of an LDS or HBM cell: a float64 SUM section adds doubles, MIN / MAX are 64-bit integer atomics.
FI void fold_atomic(int64_t* cell, int32_t op, int64_t v) {
  if (op == PGPU_RED_SUM_I64) atomicAdd((unsigned long long*)cell, (unsigned long long)v);
  else if (op == PGPU_RED_SUM_F64) atomicAdd((double*)cell, __longlong_as_double(v));
  else if (op == PGPU_RED_MIN_I64) atomicMin((long long*)cell, (long long)v);
  else atomicMax((long long*)cell, (long long)v);
}
// Butterfly over the wave's 64 lanes: every lane ends with the combination of all.
FI int64_t fold_wave(int32_t op, int64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fold_combine(op, v, shfl_xor64(v, d));
  return v;
}

__global__ __launch_bounds__(PGPU_FOLD_THREADS) void fold_init_kernel(int64_t* out, uint64_t inner, int32_t nsec,
                                                                      FoldOps ops) {
  const uint64_t n = inner * (uint64_t)(nsec + 1);
  for (uint64_t i = blockIdx.x * (uint64_t)PGPU_FOLD_THREADS + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * PGPU_FOLD_THREADS)
    out[i] = fold_identity(ops.op[i / inner]);
}

// Dense input [nsec][card * inner]: thread g of blockIdx.x walks the cids [blockIdx.y * chunk, + chunk) with the
// sections' partial results in registers (the section loop is unrolled over PGPU_MAX_SECTIONS, so acc[] never
// leaves them), then adds them to the pre-initialised output -- nothing when it met no occupied cell.
__global__ __launch_bounds__(PGPU_FOLD_THREADS) void fold_columns_kernel(const int64_t* __restrict__ in, uint64_t N,
                                                                         int32_t nsec, uint64_t inner, uint64_t card,
                                                                         uint64_t chunk, FoldOps ops,
                                                                         int64_t* __restrict__ out) {
  const uint64_t g = blockIdx.x * (uint64_t)PGPU_FOLD_THREADS + threadIdx.x;
  if (g >= inner) return;
  const uint64_t c0 = blockIdx.y * chunk;
  const uint64_t c1 = c0 + chunk < card ? c0 + chunk : card;
  int64_t acc[PGPU_MAX_SECTIONS];
#pragma unroll
  for (int s = 0; s < PGPU_MAX_SECTIONS; ++s) acc[s] = s < nsec ? fold_identity(ops.op[s]) : 0;
  int64_t distinct = 0;
  for (uint64_t c = c0; c < c1; c += PGPU_FOLD_UNROLL) {
    int64_t cnt[PGPU_FOLD_UNROLL];
#pragma unroll
    for (int u = 0; u < PGPU_FOLD_UNROLL; ++u) cnt[u] = c + u < c1 ? in[(c + u) * inner + g] : 0;
#pragma unroll
    for (int u = 0; u < PGPU_FOLD_UNROLL; ++u) {
      if (cnt[u] <= 0) continue;
      const uint64_t cell = (c + u) * inner + g;
      acc[0] += cnt[u];
      ++distinct;
#pragma unroll
      for (int s = 1; s < PGPU_MAX_SECTIONS; ++s)
        if (s < nsec) acc[s] = fold_combine(ops.op[s], acc[s], in[(uint64_t)s * N + cell]);
    }
  }
  if (distinct == 0) return;
#pragma unroll
  for (int s = 0; s < PGPU_MAX_SECTIONS; ++s)
    if (s < nsec) fold_atomic(&out[(uint64_t)s * inner + g], ops.op[s], acc[s]);
  fold_atomic(&out[(uint64_t)nsec * inner + g], PGPU_RED_SUM_I64, distinct);
}

// One thread per input cell, grid-stride.  HASH: cell = hash slot, key word 0 at in[nsec * N + slot]; dense: the
// cell index is the key.  LDS: the workgroup's partial table [nsec + 1][inner] in dynamic LDS (inner = 1: registers
// and a wave reduction in front of it); otherwise every occupied cell updates the output in HBM.
template <bool HASH, bool LDS>
__global__ __launch_bounds__(PGPU_FOLD_THREADS) void fold_cells_kernel(const int64_t* __restrict__ in, uint64_t N,
                                                                       int32_t nsec, uint64_t inner, FoldOps ops,
                                                                       int64_t* __restrict__ out) {
  extern __shared__ int64_t ltab[];  // LDS: [nsec + 1][inner]
  const int nout = nsec + 1;
  const uint32_t ncell = LDS ? (uint32_t)inner * (uint32_t)nout : 0;
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < ncell; i += PGPU_FOLD_THREADS) ltab[i] = fold_identity(ops.op[i / (uint32_t)inner]);
    __syncthreads();
  }
  const bool regs = LDS && inner == 1;  // every cell folds into the one key: keep the sums in registers
  int64_t acc[PGPU_MAX_SECTIONS];
#pragma unroll
  for (int s = 0; s < PGPU_MAX_SECTIONS; ++s) acc[s] = s < nsec ? fold_identity(ops.op[s]) : 0;
  int64_t distinct = 0;
  int64_t* tab = LDS ? ltab : out;
  const uint64_t stride = (uint64_t)gridDim.x * PGPU_FOLD_THREADS;
  uint64_t e = blockIdx.x * (uint64_t)PGPU_FOLD_THREADS + threadIdx.x;
  // dense: g = e % inner follows e by conditional subtraction (one division per thread, none per cell)
  const uint64_t gstep = HASH ? 0 : stride % inner;
  uint64_t g = HASH ? 0 : e % inner;
  for (; e < N; e += stride * PGPU_FOLD_UNROLL) {
    int64_t cnt[PGPU_FOLD_UNROLL];
#pragma unroll
    for (int u = 0; u < PGPU_FOLD_UNROLL; ++u) cnt[u] = e + u * stride < N ? in[e + u * stride] : 0;
#pragma unroll
    for (int u = 0; u < PGPU_FOLD_UNROLL; ++u) {
      const uint64_t cell = e + u * stride;
      uint64_t gk = g;
      if (!HASH) {
        g += gstep;
        if (g >= inner) g -= inner;
      }
      if (cnt[u] <= 0) continue;
      if (HASH) {
        const uint64_t key = (uint64_t)in[(uint64_t)nsec * N + cell];
        gk = ((key | inner) >> 32) ? key % inner : (uint64_t)((uint32_t)key % (uint32_t)inner);
      }
      if (regs) {
        acc[0] += cnt[u];
        ++distinct;
#pragma unroll
        for (int s = 1; s < PGPU_MAX_SECTIONS; ++s)
          if (s < nsec) acc[s] = fold_combine(ops.op[s], acc[s], in[(uint64_t)s * N + cell]);
      } else {
        fold_atomic(&tab[gk], PGPU_RED_SUM_I64, cnt[u]);
        for (int s = 1; s < nsec; ++s) fold_atomic(&tab[(uint64_t)s * inner + gk], ops.op[s], in[(uint64_t)s * N + cell]);
        fold_atomic(&tab[(uint64_t)nsec * inner + gk], PGPU_RED_SUM_I64, 1);
      }
    }
  }
  if (!LDS) return;
  if (regs) {
    // (whole waves reach here: no lane left the loop by a return)
    distinct = fold_wave(PGPU_RED_SUM_I64, distinct);
#pragma unroll
    for (int s = 0; s < PGPU_MAX_SECTIONS; ++s)
      if (s < nsec) acc[s] = fold_wave(ops.op[s], acc[s]);
    if ((threadIdx.x & 63) == 0 && distinct > 0) {
#pragma unroll
      for (int s = 0; s < PGPU_MAX_SECTIONS; ++s)
        if (s < nsec) fold_atomic(&ltab[s], ops.op[s], acc[s]);
      fold_atomic(&ltab[nsec], PGPU_RED_SUM_I64, distinct);
    }
  }
  __syncthreads();
  // flush: the keys this workgroup met (count > 0), one global atomic per cell
  for (uint32_t i = threadIdx.x; i < ncell; i += PGPU_FOLD_THREADS) {
    const uint32_t s = i / (uint32_t)inner, gk = i - s * (uint32_t)inner;
    if (ltab[gk] > 0) fold_atomic(&out[i], ops.op[s], ltab[i]);
  }
}

}  // namespace

// Enqueue the fold of `in` ([nsec (+ key word when hash)][N] int64) into `out` ([nsec + 1][inner]) on `st`.
// ops[0..nsec) = the input's section ops.  The caller has checked N % inner == 0 for dense input.
hipError_t pgpu_launch_fold(const int64_t* in, uint64_t N, int32_t nsec, const int32_t* ops, bool hash, uint64_t inner,
                            int64_t* out, int num_cus, hipStream_t st) {
  if (nsec < 1 || nsec > PGPU_MAX_SECTIONS || inner == 0 || N == 0) return hipErrorInvalidValue;
  FoldOps fo{};
  for (int s = 0; s < nsec; ++s) fo.op[s] = ops[s];
  fo.op[nsec] = PGPU_RED_SUM_I64;
  const uint64_t ncell = inner * (uint64_t)(nsec + 1);
  const unsigned T = PGPU_FOLD_THREADS;
  hipLaunchKernelGGL(fold_init_kernel, dim3((unsigned)std::min<uint64_t>(4096, (ncell + T - 1) / T)), dim3(T), 0, st,
                     out, inner, nsec, fo);
  const uint64_t lds_bytes = 8 * ncell;
  const bool lds = lds_bytes <= PGPU_FOLD_LDS_BYTES;
  if (!hash && !lds) {
    // enough workgroups for a few waves per SIMD: what inner does not give comes from splitting cid
    const uint64_t card = N / inner;
    const uint64_t bx = (inner + T - 1) / T;
    const uint64_t want = 8ull * (uint64_t)num_cus;
    uint64_t by = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(card, 65535), (want + bx - 1) / bx));
    const uint64_t chunk = (card + by - 1) / by;
    by = (card + chunk - 1) / chunk;
    hipLaunchKernelGGL(fold_columns_kernel, dim3((unsigned)bx, (unsigned)by), dim3(T), 0, st, in, N, nsec, inner, card,
                       chunk, fo, out);
    return hipGetLastError();
  }
  // as many workgroups as stay resident with this LDS table (at most 8 per CU), each with at least one round of cells
  const uint64_t per_cu = lds ? std::max<uint64_t>(1, std::min<uint64_t>(8, (160 * 1024) / std::max<uint64_t>(lds_bytes, 1))) : 8;
  const uint64_t rounds = (N + (uint64_t)T * PGPU_FOLD_UNROLL - 1) / ((uint64_t)T * PGPU_FOLD_UNROLL);
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(rounds, per_cu * (uint64_t)num_cus));
  if (hash && lds)
    hipLaunchKernelGGL((fold_cells_kernel<true, true>), dim3(grid), dim3(T), (size_t)lds_bytes, st, in, N, nsec, inner, fo, out);
  else if (hash)
    hipLaunchKernelGGL((fold_cells_kernel<true, false>), dim3(grid), dim3(T), 0, st, in, N, nsec, inner, fo, out);
  else
    hipLaunchKernelGGL((fold_cells_kernel<false, true>), dim3(grid), dim3(T), (size_t)lds_bytes, st, in, N, nsec, inner, fo, out);
  return hipGetLastError();
}
