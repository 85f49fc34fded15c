// Tile presence rows of a bit-sliced fixed-bit column (layout and hash: pgpu_internal.h).  A point predicate on a
// high-cardinality column is true in one tile out of hundreds, and the register-direct kernel learns that only by
// streaming the tile's planes; the rows answer "can tile t hold id x" from PGPU_PRESENCE_PROBES words per 32 tiles,
// with no false negatives, so the kernel streams only the tiles they keep (rdirect_consumer, DevParams::rd_skip).
//
// presence_build_kernel: a workgroup takes 32 consecutive tiles = one word of every row at a time.  The 32 tiles'
// signatures (2 KB each) are held in LDS already transposed -- word r of the 64-KB table is the workgroup's word of
// row r, a tile sets its own bit of it with an LDS atomic OR -- and are written out once, one 4-B store per row.  No
// global atomics; every word of every row is written, so the rows need no memset.  The ids come from the bit-sliced
// copy: a thread takes one lane word of every plane of a tile and rebuilds that lane's 32 ids in registers.
// A build on use runs beside queries, so its grid can be bounded (max_wgs): the workgroups then walk the words, and
// the query kernels keep most of the CUs to themselves for the few milliseconds it takes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pinot_gpu.h"
#include "pgpu_internal.h"

#define PGPU_PRESENCE_THREADS 256

namespace {

__global__ __launch_bounds__(PGPU_PRESENCE_THREADS) void presence_build_kernel(const uint32_t* sliced, int bits,
                                                                               int32_t num_docs, int32_t ntiles,
                                                                               int32_t wpr, uint32_t* rows) {
  extern __shared__ uint32_t sig[];  // [PGPU_PRESENCE_ROWS]: bit t = tile 32 * w + t
  for (int w = blockIdx.x; w < wpr; w += gridDim.x) {
    for (int r = threadIdx.x; r < PGPU_PRESENCE_ROWS; r += PGPU_PRESENCE_THREADS) sig[r] = 0u;
    __syncthreads();
    // 32 tiles x 64 lane records, PGPU_PRESENCE_THREADS at a time: a wave takes one tile's 64 records (coalesced)
    for (int u = threadIdx.x; u < 32 * 64; u += PGPU_PRESENCE_THREADS) {
      const int tt = u >> 6, l = u & 63;
      const int64_t tile = (int64_t)w * 32 + tt;
      if (tile >= ntiles) break;  // (wave-uniform: u >> 6 is)
      const int64_t doc0 = tile * PGPU_WT + 32 * l;
      const int64_t left = (int64_t)num_docs - doc0;
      if (left <= 0) continue;
      const uint32_t valid = left >= 32 ? 0xFFFFFFFFu : ((1u << (int)left) - 1u);
      const uint32_t* src = sliced + ((size_t)tile * bits) * 64 + l;
      uint32_t x[32];
#pragma unroll
      for (int k = 0; k < 32; ++k) x[k] = k < bits ? src[64 * k] : 0u;
      const uint32_t tbit = 1u << tt;
      for (int i = 0; i < 32; ++i) {
        if (!((valid >> i) & 1u)) break;
        uint32_t id = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) id |= ((x[k] >> i) & 1u) << k;
#pragma unroll
        for (int j = 0; j < PGPU_PRESENCE_PROBES; ++j) {
          uint32_t* cell = &sig[pgpu_presence_row_of(id, j)];
          if (!(*(volatile uint32_t*)cell & tbit)) atomicOr(cell, tbit);
        }
      }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < PGPU_PRESENCE_ROWS; r += PGPU_PRESENCE_THREADS) rows[(size_t)r * wpr + w] = sig[r];
    __syncthreads();  // (the table is cleared for the next word)
  }
}

// One variant, listed once.  Its LDS table is exactly the 64 KiB a kernel may have without asking; the launch sets the
// attribute all the same, so that the size can grow with PGPU_PRESENCE_ROWS.
constexpr size_t kPresenceLds = (size_t)PGPU_PRESENCE_ROWS * 4;

}  // namespace

// Enqueue the build of a column's presence rows on `st`: `sliced` is its bit-sliced copy (`bits` planes per tile, at
// least ceil(num_docs / PGPU_WT) tiles), `rows` holds PGPU_PRESENCE_ROWS x wpr words, wpr = ceil(ntiles / 32).
// max_wgs > 0 bounds the grid.
hipError_t pgpu_launch_presence_build(const uint32_t* sliced, int bits, int32_t num_docs, uint32_t* rows, int max_wgs,
                                      hipStream_t st) {
  if (!sliced || !rows || bits < 1 || bits > 31 || num_docs < 1) return hipErrorInvalidValue;
  const int32_t ntiles = (int32_t)(((int64_t)num_docs + PGPU_WT - 1) / PGPU_WT);
  const int32_t wpr = (ntiles + 31) / 32;
  // (per launch: the attribute belongs to the current device, and a build is rare)
  const hipError_t attr = hipFuncSetAttribute((const void*)presence_build_kernel,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPresenceLds);
  if (attr != hipSuccess) return attr;
  const int grid = max_wgs > 0 && max_wgs < wpr ? max_wgs : wpr;
  hipLaunchKernelGGL(presence_build_kernel, dim3((unsigned)grid), dim3(PGPU_PRESENCE_THREADS), kPresenceLds, st, sliced,
                     bits, num_docs, ntiles, wpr, rows);
  return hipGetLastError();
}
