// kernels_agg2.hip — two-phase hash aggregation for high-cardinality GROUP BY
// (SURVEY.md §7 hard part (b)): radix-partition rows by key-hash into buckets
// whose groups fit in LDS, then aggregate each bucket entirely in LDS and
// merge the (bounded, counted) per-bucket group lists into the global slot
// table. Replaces the single-phase kernel's per-row random slot-line round
// trips (~183 B/row measured, profiles/r01_agg_pmc.md) with sequential
// streams; group-table traffic becomes per-GROUP, not per-row.
// This file holds the ends of the pipeline — the per-block histogram, the
// counts scan, and the merges into the slot table (staged groups, leftover
// rows, special keys); the scatter and the bucket aggregation between them
// live in kernels_agg3.hip.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "dev_agg.h"
#include "kernels.h"
#include "launch_check.h"

namespace auron {

namespace {
constexpr int BLOCK = 256;
constexpr int64_t MAX_BLOCKS = 256 * 8;
inline int grid2(int64_t n) {
  int64_t b = (n + BLOCK - 1) / BLOCK;
  if (b > MAX_BLOCKS) b = MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

// bucket id = HIGH bits of the mix (the LDS probe uses the LOW bits, so the
// two are independent)
__device__ __forceinline__ uint32_t bucket_of(int64_t key, int nbuck_log2) {
  return (uint32_t)(mix64((uint64_t)key) >> (64 - nbuck_log2));
}

}  // namespace

// ---- phase P1: per-BLOCK per-bucket histogram (reads keys only) ------------
// counts_matrix is bucket-major: counts[(b << GRID_LOG2) | blockIdx]. An
// exclusive scan over the flat matrix then gives every block a private,
// contiguous output range per bucket — the scatter needs NO global atomics.
// Launched at 1024 threads: 16 waves per block, and the scatter
// (kernels_agg3.hip) walks rows with the SAME grid and block geometry.

// MINMAX: also track the order-mapped (sign bit flipped) min/max of the
// NORMAL keys and publish them with one atomicMin/atomicMax per wave into
// kminmax[0..1]. The engine reads the pair after the first chunk's histogram
// to pick the packed-16B record layout, so the decision costs no pass over
// the keys of its own.
template <bool MINMAX>
__global__ __launch_bounds__(1024) void k_agg2_hist(
    const int64_t* __restrict__ keys,
                            const uint8_t* __restrict__ key_valid, int64_t n,
                            int nbuck_log2, int grid_log2,
                            uint32_t* __restrict__ counts_matrix,
                            uint32_t* __restrict__ special_rows,
                            unsigned long long* __restrict__ kminmax) {
  extern __shared__ uint32_t lds_hist[];
  const uint32_t nbuck = 1u << nbuck_log2;
  for (uint32_t b = threadIdx.x; b < nbuck; b += blockDim.x) lds_hist[b] = 0;
  __syncthreads();
  uint32_t special = 0;
  unsigned long long kmin = ~0ull, kmax = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    bool knull = key_valid && !bit_get_dev(key_valid, i);
    int64_t k = keys[i];
    if (knull || k == KEY_EMPTY) {
      special++;
      continue;
    }
    if (MINMAX) {
      unsigned long long m = (unsigned long long)k ^ 0x8000000000000000ull;
      kmin = m < kmin ? m : kmin;
      kmax = m > kmax ? m : kmax;
    }
    atomicAdd(&lds_hist[bucket_of(k, nbuck_log2)], 1u);
  }
  if (MINMAX) {
    // every lane takes part in the shuffles; lanes without a normal key
    // carry the identities
    for (int off = 32; off > 0; off >>= 1) {
      unsigned long long omin = __shfl_xor(kmin, off);
      unsigned long long omax = __shfl_xor(kmax, off);
      kmin = omin < kmin ? omin : kmin;
      kmax = omax > kmax ? omax : kmax;
    }
    if ((threadIdx.x & 63) == 0 && kmin != ~0ull) {
      atomicMin(&kminmax[0], kmin);
      atomicMax(&kminmax[1], kmax);
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbuck; b += blockDim.x)
    counts_matrix[((size_t)b << grid_log2) | blockIdx.x] = lds_hist[b];
  if (special) atomicAdd(special_rows, special);
}

// specials (null key / i64::MIN key): straight to the global special slots
__global__ void k_agg2_specials(const AggTable t,
                                const int64_t* __restrict__ keys,
                                const uint8_t* __restrict__ key_valid,
                                const double* __restrict__ vals,
                                const uint8_t* __restrict__ val_valid,
                                int64_t n, uint64_t row_offset) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    bool knull = key_valid && !bit_get_dev(key_valid, i);
    int64_t k = keys[i];
    if (!(knull || k == KEY_EMPTY)) continue;
    int which = knull ? 1 : 0;
    if (atomicCAS(&t.special_used[which], 0u, 1u) == 0u)
      atomicAdd(t.num_groups, 1ull);
    AggSlot* sl = &t.slots[t.cap + which];
    uint64_t row = row_offset + (uint64_t)i;
    if (sl->first_row > row) atomicMin(&sl->first_row, row);
    bool vvalid = !val_valid || bit_get_dev(val_valid, i);
    if (vvalid) {
      sum_accum(&sl->sum, vals[i], t.sum_int);
      atomicAdd(&sl->cnt, 1ull);
    }
  }
}

// merge staged groups into the global slot table (per-GROUP work). Staged and
// leftover keys are never null or i64::MIN (the scatter filters specials), so
// both merges probe with key_null = false.
__global__ void k_agg2_merge_groups(const AggTable t,
                                    const StagedGroup* __restrict__ staged,
                                    int64_t n, uint64_t row_offset) {
  uint32_t new_groups = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = agg_upsert_slot_counted(t, staged[i].key, false, &new_groups);
    if (a < 0) continue;  // probe exhausted: error bit 1 raised
    AggSlot* sl = &t.slots[a];
    unsigned long long cf = staged[i].cnt_first;
    uint64_t row = row_offset + (uint32_t)cf;
    if (sl->first_row > row) atomicMin(&sl->first_row, row);
    uint32_t cnt = (uint32_t)(cf >> 32);
    if (cnt) {  // cnt==0: group seen only via null values — key+order only
      sum_accum(&sl->sum, staged[i].sum, t.sum_int);
      atomicAdd(&sl->cnt, (unsigned long long)cnt);
    }
  }
  agg_publish_new_groups(t, new_groups);
}

// leftover raw rows (LDS window overflow — rare): single-phase accumulate
__global__ void k_agg2_leftovers(const AggTable t,
                                 const PartRow* __restrict__ rows, int64_t n,
                                 uint64_t row_offset) {
  uint32_t new_groups = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = agg_upsert_slot_counted(t, rows[i].key, false, &new_groups);
    if (a < 0) continue;  // probe exhausted: error bit 1 raised
    AggSlot* sl = &t.slots[a];
    uint32_t rv = rows[i].rowv;
    uint64_t row = row_offset + (rv & 0x7FFFFFFFu);
    if (sl->first_row > row) atomicMin(&sl->first_row, row);
    if (rv & 0x80000000u) {
      sum_accum(&sl->sum, rows[i].val, t.sum_int);
      atomicAdd(&sl->cnt, 1ull);
    }
  }
  agg_publish_new_groups(t, new_groups);
}

void launch_agg2_leftovers(const AggTable& t, const PartRow* rows, int64_t n,
                           uint64_t row_offset, hipStream_t s) {
  hipLaunchKernelGGL(k_agg2_leftovers, dim3(grid2(n)), dim3(BLOCK), 0, s, t,
                     rows, n, row_offset);
  check_launch("k_agg2_leftovers");
}

void launch_agg2_hist(const int64_t* keys, const uint8_t* key_valid, int64_t n,
                      int nbuck_log2, int grid_log2, uint32_t* counts_matrix,
                      uint32_t* special_rows, unsigned long long* kminmax,
                      hipStream_t s) {
  size_t lds = (size_t)(1u << nbuck_log2) * 4;
  if (kminmax)
    hipLaunchKernelGGL(k_agg2_hist<true>, dim3(1 << grid_log2), dim3(1024),
                       lds, s, keys, key_valid, n, nbuck_log2, grid_log2,
                       counts_matrix, special_rows, kminmax);
  else
    hipLaunchKernelGGL(k_agg2_hist<false>, dim3(1 << grid_log2), dim3(1024),
                       lds, s, keys, key_valid, n, nbuck_log2, grid_log2,
                       counts_matrix, special_rows, kminmax);
  check_launch("k_agg2_hist");
}

void scan_counts_matrix(const uint32_t* counts, uint32_t* scanned, int64_t n,
                        void* temp, size_t* temp_bytes, hipStream_t s) {
  hipError_t e = rocprim::exclusive_scan(temp, *temp_bytes, counts, scanned,
                                         0u, (size_t)n,
                                         rocprim::plus<uint32_t>(), s);
  if (e != hipSuccess) abort();
}

void launch_agg2_specials(const AggTable& t, const int64_t* keys,
                          const uint8_t* key_valid, const double* vals,
                          const uint8_t* val_valid, int64_t n,
                          uint64_t row_offset, hipStream_t s) {
  hipLaunchKernelGGL(k_agg2_specials, dim3(grid2(n)), dim3(BLOCK), 0, s, t,
                     keys, key_valid, vals, val_valid, n, row_offset);
  check_launch("k_agg2_specials");
}

void launch_agg2_merge_groups(const AggTable& t, const StagedGroup* staged,
                              int64_t n, uint64_t row_offset, hipStream_t s) {
  hipLaunchKernelGGL(k_agg2_merge_groups, dim3(grid2(n)), dim3(BLOCK), 0, s, t,
                     staged, n, row_offset);
  check_launch("k_agg2_merge_groups");
}

}  // namespace auron
