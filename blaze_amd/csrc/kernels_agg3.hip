// kernels_agg3.hip — v3 partition scatter for the two-phase aggregation:
// LDS-staged packet flushes into 64B-aligned per-(block,bucket) ranges.
//
// Round-1/2 PMC evidence (profiles/r01_final_pmc.md, r2chain stats): the
// per-record scatter wrote partial cache lines across ~512K open regions and
// paid ~2x write-back amplification — 30 ms of the 41 ms step at 1.35 TB/s
// effective. Here every (block,bucket) range starts 64B-aligned (the hist
// scan pads sizes to whole lines) and records are staged in LDS until a full
// 8-record packet (8 x 24 B = 192 B = 3 exact lines) can be written, so the
// L2 never holds a partially written line between flushes. Layout per block:
//   staging[512 buckets][12 records][24 B]  = 147 KB LDS
//   cnt/fl counters                          = 4 KB
// (one 1024-thread workgroup per CU; the scatter is bandwidth-bound, not
// latency-bound, so 16 waves suffice — measured round 2.)
//
// The bucket aggregation kernel widens its LDS hash window to 4096 slots
// (512 buckets x ~2000 distinct keys/bucket at the 1M-group north star needs
// >2048) at 24 B/slot SoA = 96 KB -> one 1024-thread workgroup per CU.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "dev_agg.h"
#include "kernels.h"
#include "launch_check.h"

namespace auron {

// ---- byte-line offsets: pad each (block,bucket) range to whole 64B lines --
// line_sizes[i] = ceil(counts[i] * 24 / 64): the exclusive scan of THIS
// matrix (in 64-byte line units, so 6 GB chunks still fit u32) gives every
// range a line-aligned start.
__global__ void k_agg3_line_sizes(const uint32_t* __restrict__ counts,
                                  int64_t n, uint32_t rec,
                                  uint32_t* __restrict__ sizes) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    sizes[i] = (counts[i] * rec + 63u) >> 6;
}

void launch_agg3_line_sizes(const uint32_t* counts, int64_t n,
                            uint32_t* sizes, int rec, hipStream_t s) {
  hipLaunchKernelGGL(k_agg3_line_sizes, dim3(256), dim3(256), 0, s, counts, n,
                     (uint32_t)rec, sizes);
  check_launch("k_agg3_line_sizes");
}

// ---- v3 scatter ------------------------------------------------------------
static constexpr int A3_CAP = 12;      // staged records per bucket (24B)
static constexpr int A3_CAP16 = 15;    // 16B records: more slots in less
                                       // LDS (512*15*16 = 123KB). HARD CAP:
                                       // pos must stay < 16 so a bucket
                                       // crosses the 8-record packet
                                       // boundary at most ONCE per tile —
                                       // two queue entries for one bucket
                                       // would race two flush subgroups
                                       // (observed as corrupted group keys
                                       // at CAP 18)
static constexpr int A3_QUANT = 8;     // records per flushed packet (192 B)
// staging slot stride: 24 B packed (a 28 B bank-spread pad was measured
// SLOWER — 7.71 vs 6.58 ms/chunk — the kernel is flush-latency-bound, not
// LDS-bank-bound)
static constexpr int A3_SLOT = 24;
// a thread that cannot stage its row after a few tiles (hot bucket under
// key skew: drain is bounded by CAP per tile) bypasses to the leftover
// list; the single-phase leftover kernel handles it — correct and bounded
// for ANY distribution, perf-relevant only under adversarial skew
static constexpr int A3_RETRY_BYPASS = 4;

// A3_RPT rows per thread per tile; a dirty QUEUE records buckets that
// crossed a packet boundary so the flush phase touches only those (the v3.0
// per-tile scan of every bucket made the kernel instruction-bound: PMC
// showed 20x the dynamic instructions of v2 and 77% parked waves while HBM
// writes ran at 1.0x algorithmic — gpurun_out/r2_pmc_scatter.json).
static constexpr int A3_RPT = 2;  // default; AURON_AGG2_RPT=4 selects the
                                  // wider tile instantiation

// REC = 24: [i64 key][f64 val][u32 rowv] (pad to 24). REC = 16: the key is
// stored as a u32 OFFSET from key_base packed with rowv into one u64 —
// [u64 koff|rowv<<32][f64 val] — 33% less scatter/bucket HBM traffic. Rows
// whose key falls outside [key_base, key_base+2^32) take the leftover
// bypass (counted in the correction matrix), so the packed path is exact
// for ANY input; the engine only selects it after observing chunk-1's key
// range (hist min/max).
template <int A3_RPT, int REC>
__global__ void __launch_bounds__(1024) k_agg3_scatter(
    const int64_t* __restrict__ keys, const uint8_t* __restrict__ key_valid,
    const double* __restrict__ vals, const uint8_t* __restrict__ val_valid,
    int64_t n, int nbuck_log2, int grid_log2, int64_t key_base,
    const uint32_t* __restrict__ line_scan, uint8_t* __restrict__ out,
    PartRow* __restrict__ leftover, unsigned long long* __restrict__ lo_n,
    uint32_t* __restrict__ bypass_matrix, uint32_t* __restrict__ err_flag) {
  const uint32_t nbuck = 1u << nbuck_log2;
  extern __shared__ uint8_t lds[];
  // layout: records [nbuck][A3_CAP][24] | cnt[nbuck] | fl[nbuck] |
  //         base_line[nbuck] | dirty queue [nbuck] u16-as-u32 | qn
  uint8_t* stage = lds;
  constexpr int CAP = REC == 16 ? A3_CAP16 : A3_CAP;
  uint32_t* cnt = (uint32_t*)(lds + (size_t)nbuck * CAP * REC);
  uint32_t* fl = cnt + nbuck;
  uint32_t* base_line = fl + nbuck;
  uint16_t* queue = (uint16_t*)(base_line + nbuck);
  uint32_t* qn = (uint32_t*)(queue + nbuck + 64);
  uint32_t* byp = qn + 1;  // rows bypassed to the leftover list, per bucket

  for (uint32_t b = threadIdx.x; b < nbuck; b += blockDim.x) {
    cnt[b] = 0;
    fl[b] = 0;
    byp[b] = 0;
    base_line[b] = line_scan[((size_t)b << grid_log2) | blockIdx.x];
  }
  if (threadIdx.x == 0) *qn = 0;
  __syncthreads();

  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int nwave = (int)(blockDim.x >> 6);
  const int wave = (int)(threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63);
  int64_t my[A3_RPT];
  int tries[A3_RPT] = {};
  int64_t k_cur[A3_RPT];
  double v_cur[A3_RPT];
#pragma unroll
  for (int r = 0; r < A3_RPT; r++) {
    my[r] = (int64_t)blockIdx.x * blockDim.x + threadIdx.x +
            (int64_t)r * stride;
    if (my[r] < n) {  // preload; refreshed right after each advance so the
      k_cur[r] = keys[my[r]];     // next tile's loads hide behind the flush
      v_cur[r] = vals[my[r]];
    }
  }
  const int64_t step = (int64_t)A3_RPT * stride;
  // hard tile bound: rows/thread plus a generous retry allowance — a full
  // staging bucket retries a row for a few tiles at most; exceeding this
  // means a logic bug, and the kernel must FAIL, never hang the box
  const int64_t max_tiles = 8 * ((n + step - 1) / step) + 256;
  int64_t tile = 0;

  for (;;) {
    if (++tile > max_tiles) {
      atomicOr(err_flag, 32u);
      break;
    }
    int mine = 0;
#pragma unroll
    for (int r = 0; r < A3_RPT; r++) {
      if (my[r] >= n) continue;
      mine = 1;
      int64_t k = k_cur[r];
      bool advanced = false;
      bool knull = key_valid && !bit_get_dev(key_valid, my[r]);
      if (knull || k == KEY_EMPTY) {
        my[r] += step;  // specials handled by k_agg2_specials
        mine |= (my[r] < n);
        advanced = true;
      } else {
        uint32_t b = (uint32_t)(mix64((uint64_t)k) >> (64 - nbuck_log2));
        bool range_ok = true;
        uint64_t koff = 0;
        if (REC == 16) {
          koff = (uint64_t)(k - key_base);
          range_ok = koff <= 0xFFFFFFFFull;
        }
        if (!range_ok) {
          // outside the packed key window: leftover bypass (exactness for
          // any input; the hist counted this row, so correct the matrix)
          bool vvalid = !val_valid || bit_get_dev(val_valid, my[r]);
          unsigned long long p = atomicAdd(lo_n, 1ull);
          leftover[p] = PartRow{
              k, v_cur[r], (uint32_t)my[r] | (vvalid ? 0x80000000u : 0u), 0};
          atomicAdd(&byp[b], 1u);
          my[r] += step;
          tries[r] = 0;
          advanced = true;
          if (advanced && my[r] < n) {
            k_cur[r] = keys[my[r]];
            v_cur[r] = vals[my[r]];
          }
          continue;
        }
        uint32_t pos = atomicAdd(&cnt[b], 1u);
        if (pos < CAP) {
          bool vvalid = !val_valid || bit_get_dev(val_valid, my[r]);
          uint8_t* rec = stage + ((size_t)b * CAP + pos) * REC;
          uint32_t rowv = (uint32_t)my[r] | (vvalid ? 0x80000000u : 0u);
          if (REC == 16) {
            *(uint64_t*)rec = koff | ((uint64_t)rowv << 32);
            *(double*)(rec + 8) = v_cur[r];
          } else {
            *(int64_t*)rec = k;
            *(double*)(rec + 8) = v_cur[r];
            *(uint32_t*)(rec + 16) = rowv;
          }
          if ((pos & (A3_QUANT - 1)) == A3_QUANT - 1) {  // crossed a packet
            uint32_t qi = atomicAdd(qn, 1u);
            if (qi < nbuck + 64) queue[qi] = (uint16_t)b;  // <=1 push per
          }                                                // bucket per tile
          my[r] += step;
          tries[r] = 0;
          advanced = true;
        } else {
          atomicSub(&cnt[b], 1u);
          if (++tries[r] >= A3_RETRY_BYPASS) {
            // hot bucket (skew): route the row to the leftover list; the
            // histogram already counted it, so record the correction the
            // bucket kernel must subtract from this (block,bucket) range
            bool vvalid = !val_valid || bit_get_dev(val_valid, my[r]);
            unsigned long long p = atomicAdd(lo_n, 1ull);
            leftover[p] = PartRow{
                k, v_cur[r],
                (uint32_t)my[r] | (vvalid ? 0x80000000u : 0u), 0};
            atomicAdd(&byp[b], 1u);
            my[r] += step;
            tries[r] = 0;
            advanced = true;
          }  // else: retry next tile (k_cur/v_cur stay valid)
        }
      }
      if (advanced && my[r] < n) {
        k_cur[r] = keys[my[r]];
        v_cur[r] = vals[my[r]];
      }
    }
    // block-wide termination check doubles as the pre-flush barrier
    int live = __syncthreads_count(mine);
    uint32_t nq = *qn;
    if (nq > nbuck + 64) nq = nbuck + 64;
    if (live == 0) {
      // drain: flush every bucket's remainder as (possibly partial) packets
      for (uint32_t b = wave; b < nbuck; b += nwave) {
        uint32_t c = cnt[b];
        if (!c) continue;
        uint8_t* dst = out + ((size_t)base_line[b] << 6) + (size_t)fl[b] * REC;
        const uint8_t* src = stage + (size_t)b * CAP * REC;
        for (uint32_t d = lane; d < c * (REC / 4); d += 64)
          ((uint32_t*)dst)[d] = ((const uint32_t*)src)[d];
      }
      __syncthreads();
      break;
    }
    // flush only queued (full-packet) buckets. Each entry is handled by an
    // 8-LANE subgroup (8 independent entries in flight per wave) — a
    // whole-wave-per-entry loop was a serial ~10-LDS-op latency chain per
    // entry and dominated the kernel.
    {
      const int sg = lane >> 3;        // subgroup 0..7 within the wave
      const int sl = lane & 7;         // lane within subgroup
      for (uint32_t i = wave * 8 + sg; i < nq; i += nwave * 8) {
        uint32_t b = queue[i];
        uint32_t c = cnt[b];
        uint32_t nfl = c & ~(uint32_t)(A3_QUANT - 1);
        if (!nfl) continue;
        uint8_t* dst = out + ((size_t)base_line[b] << 6) + (size_t)fl[b] * REC;
        uint8_t* src = stage + (size_t)b * CAP * REC;
        for (uint32_t d = sl; d < nfl * (REC / 4); d += 8)
          ((uint32_t*)dst)[d] = ((const uint32_t*)src)[d];
        uint32_t rem = c - nfl;
        for (uint32_t d = sl; d < rem * (REC / 4); d += 8)
          ((uint32_t*)src)[d] =
              ((const uint32_t*)(src + (size_t)nfl * REC))[d];
        if (sl == 0) {
          fl[b] += nfl;
          cnt[b] = rem;
        }
      }
    }
    // queue ENTRIES below nq are no longer needed; resetting the counter
    // concurrently with other waves' reads of those entries is benign
    if (threadIdx.x == 0) *qn = 0;
    __syncthreads();
  }
  // every (bucket, block) entry is written by its own block — on EVERY exit
  // path (incl. the tile-bound failure), so the bucket kernel never reads a
  // stale matrix
  for (uint32_t b = threadIdx.x; b < nbuck; b += blockDim.x)
    bypass_matrix[((size_t)b << grid_log2) | blockIdx.x] = byp[b];
}

void launch_agg3_scatter(const int64_t* keys, const uint8_t* key_valid,
                         const double* vals, const uint8_t* val_valid,
                         int64_t n, int nbuck_log2, int grid_log2,
                         const uint32_t* line_scan, uint8_t* out,
                         PartRow* leftover, unsigned long long* lo_n,
                         uint32_t* bypass_matrix, uint32_t* err_flag,
                         int rec, int64_t key_base, hipStream_t s) {
  const uint32_t nbuck = 1u << nbuck_log2;
  const int cap = rec == 16 ? A3_CAP16 : A3_CAP;
  size_t lds = (size_t)nbuck * cap * (size_t)rec + (size_t)nbuck * 16 +
               ((size_t)nbuck + 64) * 2 + 8;  // + queue + counters + bypass
  if (lds > 160 * 1024)
    throw std::runtime_error("agg3 scatter LDS over 160KB");
  static int rpt = [] {
    const char* e = getenv("AURON_AGG2_RPT");
    int v = e ? atoi(e) : 2;
    return (v >= 2 && v <= 4) ? v : 2;
  }();
  const void* fn;
  if (rec == 16)
    fn = rpt == 4   ? (const void*)k_agg3_scatter<4, 16>
         : rpt == 3 ? (const void*)k_agg3_scatter<3, 16>
                    : (const void*)k_agg3_scatter<2, 16>;
  else
    fn = rpt == 4   ? (const void*)k_agg3_scatter<4, 24>
         : rpt == 3 ? (const void*)k_agg3_scatter<3, 24>
                    : (const void*)k_agg3_scatter<2, 24>;
  hipError_t e = hipFuncSetAttribute(
      fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess)
    throw std::runtime_error("agg3 scatter LDS attribute failed");
#define A3_LAUNCH(R, P)                                                     \
  hipLaunchKernelGGL((k_agg3_scatter<R, P>), dim3(1 << grid_log2),          \
                     dim3(1024), lds, s, keys, key_valid, vals, val_valid,  \
                     n, nbuck_log2, grid_log2, key_base, line_scan, out,    \
                     leftover, lo_n, bypass_matrix, err_flag)
  if (rec == 16) {
    if (rpt == 4) A3_LAUNCH(4, 16);
    else if (rpt == 3) A3_LAUNCH(3, 16);
    else A3_LAUNCH(2, 16);
  } else {
    if (rpt == 4) A3_LAUNCH(4, 24);
    else if (rpt == 3) A3_LAUNCH(3, 24);
    else A3_LAUNCH(2, 24);
  }
#undef A3_LAUNCH
  check_launch("k_agg3_scatter");
}

// ---- v3 bucket aggregation (4096-slot LDS window, 1024 threads) ------------
static constexpr int L3SLOTS = 4096;
static constexpr int L3PROBE = 128;

template <int REC>
__global__ void __launch_bounds__(1024) k_agg3_bucket(
    const uint8_t* __restrict__ part, const uint32_t* __restrict__ counts,
    const uint32_t* __restrict__ bypass,
    const uint32_t* __restrict__ line_scan, int grid_log2, int is_int,
    int nbuckets, int64_t key_base, StagedGroup* __restrict__ staged,
    unsigned long long* __restrict__ staged_n, int64_t staged_cap,
    PartRow* __restrict__ leftover, unsigned long long* __restrict__ lo_n,
    uint32_t* __restrict__ error_flag) {
  __shared__ int64_t ls_key[L3SLOTS];
  __shared__ double ls_sum[L3SLOTS];
  __shared__ uint32_t ls_cnt[L3SLOTS];
  __shared__ uint32_t ls_first[L3SLOTS];
  // per-range cumulative record counts for this bucket (grid of ranges)
  __shared__ uint32_t cum[1 << AGG2_GRID_LOG2_MAX];
  const int nrange = 1 << grid_log2;

  for (int b = blockIdx.x; b < nbuckets; b += gridDim.x) {
    for (int s = threadIdx.x; s < L3SLOTS; s += blockDim.x) {
      ls_key[s] = KEY_EMPTY;
      ls_sum[s] = 0.0;
      ls_cnt[s] = 0;
      ls_first[s] = 0xFFFFFFFFu;
    }
    // serial scan of <=1024 range counts (one thread; ~us)
    if (threadIdx.x == 0) {
      uint32_t acc = 0;
      for (int k = 0; k < nrange; k++) {
        size_t e = ((size_t)b << grid_log2) | k;
        acc += counts[e] - bypass[e];  // bypassed rows were never written
        cum[k] = acc;
      }
    }
    __syncthreads();
    uint32_t total = cum[nrange - 1];
    // 2-way ILP: both record loads (random-ish global) and both first LDS
    // probe reads go out before either resolution — halves exposed latency
    // at the 16-wave occupancy this 100KB-LDS kernel gets
    auto locate = [&](uint32_t j) -> const uint8_t* {
      int lo = 0, hi = nrange - 1;
      while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (j < cum[mid]) hi = mid; else lo = mid + 1;
      }
      uint32_t before = lo ? cum[lo - 1] : 0;
      return part + ((size_t)line_scan[((size_t)b << grid_log2) | lo] << 6) +
             (size_t)(j - before) * REC;
    };
    // typed record parse: REC 16 packs (key - key_base) u32 with rowv
    auto load_rec = [&](const uint8_t* r, int64_t* k, double* v,
                        uint32_t* rv) {
      if (REC == 16) {
        uint64_t w = *(const uint64_t*)r;
        *k = key_base + (int64_t)(uint32_t)w;
        *rv = (uint32_t)(w >> 32);
      } else {
        *k = *(const int64_t*)r;
        *rv = *(const uint32_t*)(r + 16);
      }
      *v = *(const double*)(r + 8);
    };
    auto resolve = [&](int64_t k, double v, uint32_t rowv, uint32_t h) {
      uint32_t row = rowv & 0x7FFFFFFFu;
      bool vvalid = (rowv & 0x80000000u) != 0;
      int found = -1;
      for (int p = 0; p < L3PROBE; p++) {
        int64_t cur = ls_key[h];
        if (cur == k) {
          found = (int)h;
          break;
        }
        if (cur == KEY_EMPTY) {
          long long prev = atomicCAS((unsigned long long*)&ls_key[h],
                                     (unsigned long long)KEY_EMPTY,
                                     (unsigned long long)k);
          if (prev == (long long)KEY_EMPTY || prev == (long long)k) {
            found = (int)h;
            break;
          }
        }
        h = (h + 1) & (L3SLOTS - 1);
      }
      if (found >= 0) {
        atomicMin(&ls_first[found], row);
        if (vvalid) {
          sum_accum(&ls_sum[found], v, is_int);
          atomicAdd(&ls_cnt[found], 1u);
        }
      } else {
        unsigned long long p = atomicAdd(lo_n, 1ull);
        leftover[p] = PartRow{k, v, rowv, 0};
      }
    };
    uint32_t j = threadIdx.x;
    for (; j + 3 * blockDim.x < total; j += 4 * blockDim.x) {
      const uint8_t* r0 = locate(j);
      const uint8_t* r1 = locate(j + blockDim.x);
      const uint8_t* r2 = locate(j + 2 * blockDim.x);
      const uint8_t* r3 = locate(j + 3 * blockDim.x);
      int64_t k0, k1, k2, k3;       // all four record loads in flight
      double v0, v1, v2, v3;
      uint32_t rv0, rv1, rv2, rv3;
      load_rec(r0, &k0, &v0, &rv0);
      load_rec(r1, &k1, &v1, &rv1);
      load_rec(r2, &k2, &v2, &rv2);
      load_rec(r3, &k3, &v3, &rv3);
      uint32_t h0 = (uint32_t)mix64((uint64_t)k0) & (L3SLOTS - 1);
      uint32_t h1 = (uint32_t)mix64((uint64_t)k1) & (L3SLOTS - 1);
      uint32_t h2 = (uint32_t)mix64((uint64_t)k2) & (L3SLOTS - 1);
      uint32_t h3 = (uint32_t)mix64((uint64_t)k3) & (L3SLOTS - 1);
      resolve(k0, v0, rv0, h0);
      resolve(k1, v1, rv1, h1);
      resolve(k2, v2, rv2, h2);
      resolve(k3, v3, rv3, h3);
    }
    for (; j < total; j += blockDim.x) {
      const uint8_t* r = locate(j);
      int64_t k;
      double v;
      uint32_t rv;
      load_rec(r, &k, &v, &rv);
      resolve(k, v, rv, (uint32_t)mix64((uint64_t)k) & (L3SLOTS - 1));
    }
    __syncthreads();
    for (int s = threadIdx.x; s < L3SLOTS; s += blockDim.x) {
      if (ls_key[s] == KEY_EMPTY) continue;
      unsigned long long p = atomicAdd(staged_n, 1ull);
      if ((int64_t)p >= staged_cap) {
        atomicOr(error_flag, 2u);
        continue;
      }
      staged[p].key = ls_key[s];
      staged[p].sum = ls_sum[s];
      staged[p].cnt_first =
          ((unsigned long long)ls_cnt[s] << 32) | ls_first[s];
    }
    __syncthreads();
  }
}

void launch_agg3_bucket(const uint8_t* part, const uint32_t* counts,
                        const uint32_t* bypass,
                        const uint32_t* line_scan, int grid_log2, int is_int,
                        int nbuckets, StagedGroup* staged,
                        unsigned long long* staged_n, int64_t staged_cap,
                        PartRow* leftover, unsigned long long* lo_n,
                        uint32_t* error_flag, int rec, int64_t key_base,
                        hipStream_t s) {
  if (rec == 16)
    hipLaunchKernelGGL((k_agg3_bucket<16>), dim3(nbuckets), dim3(1024), 0, s,
                       part, counts, bypass, line_scan, grid_log2, is_int,
                       nbuckets, key_base, staged, staged_n, staged_cap,
                       leftover, lo_n, error_flag);
  else
    hipLaunchKernelGGL((k_agg3_bucket<24>), dim3(nbuckets), dim3(1024), 0, s,
                       part, counts, bypass, line_scan, grid_log2, is_int,
                       nbuckets, key_base, staged, staged_n, staged_cap,
                       leftover, lo_n, error_flag);
  check_launch("k_agg3_bucket");
}

}  // namespace auron
