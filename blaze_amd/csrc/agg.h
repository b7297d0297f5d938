// agg.h — AggOp, the GPU AggExec operator (agg_exec.rs:141-278 semantics);
// method bodies in agg.cpp. HashAgg in one of four modes:
//   legacy shared-argument table — one numeric key, all aggs over one column;
//   multi-argument bank (ma_mode_) — per-agg argument columns and pools;
//   generalized keys (gkey_) — Utf8 / multi-column grouping tuples;
//   two-phase fast path — partition-then-merge for large numeric-key chunks.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "emit.h"
#include "kernels.h"

namespace auron {

class AggOp {
 public:
  // what the Runtime reports as task metrics
  struct Metrics {
    int64_t update_ns, update_rows, spill_count;
    int64_t emit_d2h_bytes, emit_host_copy_bytes;
  };

  AggOp(const AggNode& node, const Conf& conf, hipStream_t stream);
  ~AggOp();

  void consume(DevBatch&& b);
  // drain: produce all output batches (host-staged)
  std::vector<HostOutBatch> finish();
  // device-resident variant of finish(): partial (key + a8 Binary) batches
  // stay in HBM. Spill / partial-skipping fall outside this mode (the bench
  // and exchange paths that use it never enter them) and FAIL loudly.
  std::vector<DevOutBatch> finish_dev();
  std::vector<OutField> output_fields() const;
  uint64_t num_groups_host();
  bool device_out() const { return device_out_; }
  Metrics metrics() const {
    return {update_ns_, update_rows_, spill_count_, emit_.d2h_bytes,
            emit_.host_copy_bytes};
  }

 private:
  struct SpillBucket {
    std::vector<int64_t> keys;
    std::vector<unsigned long long> first_rows;
    std::vector<int32_t> lens;
    std::vector<uint8_t> data;
  };

  static constexpr int64_t AGG2_MIN_CHUNK = 4 << 20;   // below: single-phase
  static constexpr int AGG3_NBUCK_LOG2 = 9;   // 512 buckets
  static constexpr int AGG3_NBUCK = 1 << AGG3_NBUCK_LOG2;
  static constexpr int AGG3_GRID_LOG2 = 8;    // hist/scatter grid: 256 blocks
                                              // x 1024 threads
  // staged-group capacity: every bucket's full 4096-slot LDS window
  static constexpr int64_t AGG3_STAGED_CAP = (int64_t)AGG3_NBUCK * 4096;

  // launch() between a pair of stream events that drain_timing() reads
  template <class F>
  void timed(F launch);

  bool maybe_enter_skipping(const DevBatch& b, int64_t done);
  std::vector<OutField> key_fields() const;
  DType ma_out_dt(size_t i) const;  // per-agg declared type (ma mode)
  DType key_out_dt() const;

  // table
  void init_table(int64_t slots);
  void ensure_capacity(int64_t need);
  void grow(int64_t new_cap);
  void refresh_ng();
  void drain_timing();
  int64_t table_order(DevBuf* slots_sorted, DevBuf* first_sorted);
  void spill_table();
  void reset_main();

  // per-mode chunk updates
  void ma_chunk(const DevBatch& b, int64_t done, int64_t chunk);
  void init_gkey();
  void gk_ensure_pool(int64_t need_more);
  GKeyCols gk_cols(const DevBatch& b, int64_t done) const;
  void gkey_chunk(const DevBatch& b, int64_t done, int64_t chunk);
  void init_agg2_conf();
  template <class Launch>
  void merge_counted(int64_t n, Launch launch);
  void two_phase_chunk(const DevBatch& b, int64_t done, int64_t chunk);

  // COLLECT pools
  std::pair<int64_t, int64_t> sort_collect_pool(
      const long long* key, const unsigned long long* prio,
      const unsigned long long* val, int64_t cap, int64_t n0, int64_t n1,
      bool dedup, DevBuf& skey, DevBuf& sval);
  void upload_pool_counts(unsigned long long* d_n, int64_t n0, int64_t n1);
  void prepare_collect();
  void prepare_ma_pools();
  void reset_collect_pool();

  // emit
  void emit_table(std::vector<HostOutBatch>* out, bool exclude_specials);
  template <class LensFn, class BytesFn>
  HostOutCol freeze_binary_col(int64_t n, LensFn write_lens,
                               BytesFn write_bytes);
  HostOutCol freeze_agg_buf(const uint32_t* order_slots, int64_t n);
  HostOutCol coll_list_col(const AggTable& tv, const uint32_t* order_slots,
                           int64_t n, DType item_dt);
  void narrow_keys(DevBuf& keys, DevBuf& wide, int64_t n);
  std::vector<HostOutCol> emit_gkey_cols(const uint32_t* order_slots,
                                         int64_t n);
  void emit_ma_aggs(const uint32_t* order_slots, int64_t n,
                    std::vector<HostOutCol>* cols);
  HostOutBatch emit_groups(const uint32_t* order_slots, int64_t n);
  DevOutBatch emit_groups_dev(const uint32_t* order_slots, int64_t n);
  HostOutBatch emit_skipped(const DevBatch& b);

  hipStream_t stream_;
  AggMode mode_ = AggMode::Partial;
  bool merge_mode_ = false, final_output_ = false;
  uint32_t key_col_ = 0, val_col_ = 0;
  DType key_dt_ = DType::Unsupported;
  uint32_t layout_ = 0;
  bool has_mm_ = false;  // agg list contains MIN/MAX: side mm array active
  bool has_coll_ = false, coll_sorted_ = false;  // COLLECT pool active
  bool coll_set_ = false;  // COLLECT_SET: dedup at prepare
  int64_t coll_cap_ = 0, conf_coll_cap_ = 16 << 20;
  int64_t coll_n0_ = 0, coll_n1_ = 0;
  bool val_is_int_ = false, val_typed_seen_ = false;  // i64 accumulator mode
  bool has_first_ = false;  // FIRST family: f_row/f_val/f_st arrays active
  std::vector<uint32_t> agg_kinds_;
  std::vector<std::string> agg_names_;
  std::string key_name_;
  int64_t batch_size_ = 10000;
  bool skip_enabled_ = false, skipping_ = false;
  bool device_out_ = false;
  // generalized grouping keys (Utf8 / multi-column; kernels_gkey.hip)
  bool key_mode_set_ = false, gkey_ = false;
  // multi-argument aggregation (kernels_maarg.hip)
  bool ma_mode_ = false, ma_args_checked_ = false;
  MaDesc ma_desc_;
  std::vector<int> ma_arg_cols_;   // per agg: input column or -1 (NULL lit)
  MaAcc ma_;
  MaPools mp_;
  DevBuf d_ma_acc_, d_ma_meta_, d_ma_st_, d_ma_slots_, d_mp_n_;
  DevBuf d_mp_key_[MA_MAX_POOLS], d_mp_prio_[MA_MAX_POOLS],
      d_mp_val_[MA_MAX_POOLS], d_mp_skey_[MA_MAX_POOLS],
      d_mp_sval_[MA_MAX_POOLS];
  bool ma_pools_sorted_ = false;
  int64_t mp_counts_[MA_MAX_POOLS][2] = {};
  std::vector<uint32_t> key_cols_;
  std::vector<std::string> key_names_;
  std::vector<DType> key_dts_;
  GKeyTable g_;
  int64_t gk_pool_cap_ = 0, gk_used_bound_ = 0;
  DevBuf d_gkpool_, d_gkpn_, d_gkoff_, d_gkdts_, d_enclens_, d_encoffs_,
      d_encbytes_, d_gkslots_, d_gkscan_tmp_;
  double skip_ratio_ = 0.999;
  int64_t skip_min_rows_ = 20000;
  uint64_t row_cursor_ = 0;
  uint64_t first_row_bound_ = 0;  // end of the two-phase chunk in flight
  uint64_t ng_bound_ = 0, ng_true_ = 0;  // conservative bound / last readback
  int64_t mem_budget_ = 8LL << 30, max_cap_ = 1 << 23;
  int num_spill_buckets_ = 16;
  int64_t specials_count_ = 0, spill_count_ = 0;
  std::vector<SpillBucket> spill_;
  int64_t update_ns_ = 0, update_rows_ = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pairs_;
  hipEvent_t ev_start_ = nullptr, ev_stop_ = nullptr;
  AggTable t_;
  DevBuf d_slots_, d_special_, d_ng_, d_err_, d_mm_, d_frow_, d_fval_, d_fst_;
  DevBuf d_ckey_, d_cprio_, d_cval_, d_cn_, d_cskey_, d_csval_;
  PinnedBuf pinned_meta_;
  HostEmit emit_;
  // two-phase scratch (allocated on first large chunk)
  // partition-buffer rows per two-phase chunk: bigger chunks amortize launch
  // tails and per-chunk syncs (24 B/row + 24 B/row leftover scratch; 256M
  // rows = 12 GB of the 288 GB HBM). Runtime-tunable for A/B sweeps.
  int64_t agg2_chunk_max_ = 256 << 20;
  bool agg2_p16_en_ = true;   // AURON_AGG2_P16=0 disables the adaptive path
  bool p16_decided_ = false;  // one key-range probe (chunk 1)
  bool packed16_ = false;     // chunks use 16B partition records
  int64_t key_base16_ = 0;
  DevBuf d_kminmax_;
  bool agg2_conf_read_ = false;
  DevBuf d_partkv_, d_leftover_, d_counts_, d_scanned_, d_scan_tmp_,
      d_staged_, d_counters_, d_linesz_;
  PinnedBuf pinned_agg2_;
  std::vector<DevBatch> held_, skipped_;
};

}  // namespace auron
