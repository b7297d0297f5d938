// agg.cpp — AggOp (agg.h): the hash table and its growth and spill, the
// per-mode chunk updates, the COLLECT pools and the host / device emit.
#include <algorithm>
#include <cstring>
#include <tuple>

#include "agg.h"
#include "ipc_scalar.h"

namespace auron {

namespace {
uint64_t host_mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
}  // namespace

AggOp::AggOp(const AggNode& node, const Conf& conf, hipStream_t stream)
    : stream_(stream) {
  emit_.stream = stream;
  if (node.exec_mode != 0) FAIL("SORT_AGG unsupported (hot path is HASH_AGG)");
  if (node.grouping_exprs.empty() ||
      node.grouping_exprs.size() > (size_t)GKEY_MAX_COLS)
    FAIL("AggExec: 1..4 Column grouping exprs supported");
  for (size_t gi = 0; gi < node.grouping_exprs.size(); gi++) {
    const Expr& ge = node.grouping_exprs[gi];
    if (ge.kind != Expr::Column)
      FAIL("AggExec: grouping exprs must be Columns");
    key_cols_.push_back(ge.col_index);
    key_names_.push_back(gi < node.grouping_names.size()
                             ? node.grouping_names[gi]
                             : "key" + std::to_string(gi));
  }
  key_col_ = key_cols_[0];
  key_name_ = key_names_[0];
  // agg set: any list of SUM/COUNT/AVG/MIN/MAX over ONE shared argument
  // column — {sum, cnt} accumulators (sum.rs, count.rs, avg.rs; AVG freeze
  // = sum ++ count, avg.rs:208-217) plus the optional side {min, max} pair
  // (maxmin.rs:104-119; single-phase path only). Anything else fails
  // loudly at plan build.
  if (node.agg_exprs.empty() ||
      node.agg_exprs.size() > (size_t)MA_MAX_AGGS)
    FAIL("AggExec: 1..12 aggregates supported");
  if (node.modes.size() != node.agg_exprs.size())
    FAIL("AggExec: modes/aggs length mismatch");
  for (const AggMode m : node.modes)
    if (m != node.modes[0]) FAIL("AggExec: mixed agg modes unsupported");
  mode_ = node.modes[0];
  merge_mode_ = (mode_ != AggMode::Partial);
  final_output_ = (mode_ == AggMode::Final);
  layout_ = 0;
  bool have_col = false, have_distinct_cols = false, have_null_lit = false;
  int fam_sum = 0, fam_cnt = 0, fam_min = 0, fam_max = 0, fam_first = 0,
      fam_firstin = 0, npools = 0;
  bool any_i32 = false, mixed_acc = false;
  for (size_t i = 0; i < node.agg_exprs.size(); i++) {
    const Expr& a = node.agg_exprs[i];
    uint32_t k;
    switch (a.agg_function) {
      case AGG_SUM: k = AGGL_SUM; fam_sum++; break;
      case AGG_COUNT: k = AGGL_CNT; fam_cnt++; break;
      case AGG_AVG: k = AGGL_AVG; fam_sum++; fam_cnt++; break;
      case AGG_MIN: k = AGGL_MIN; fam_min++; has_mm_ = true; break;
      case AGG_MAX: k = AGGL_MAX; fam_max++; has_mm_ = true; break;
      case AGG_FIRST: k = AGGL_FIRST; fam_first++; has_first_ = true; break;
      case AGG_FIRST_IGNORES_NULL:
        k = AGGL_FIRSTIN;
        fam_firstin++;
        has_first_ = true;
        break;
      case AGG_COLLECT_LIST:
        k = AGGL_CLIST;
        npools++;
        has_coll_ = true;
        break;
      case AGG_COLLECT_SET:
        k = AGGL_CSET;
        npools++;
        has_coll_ = true;
        coll_set_ = true;
        break;
      default:
        FAIL("AggExec: only SUM/COUNT/AVG/MIN/MAX/FIRST[_IGNORES_NULL]/"
             "COLLECT_LIST aggregates on this path");
    }
    if (i < 8) layout_ |= k << (4 * i);
    // accumulator arithmetic type follows the agg's declared data type
    // (sum.rs:78-88 casts inputs to it; maxmin.rs:81-83 preserves it)
    MaAgg ma;
    ma.kind = (uint8_t)k;
    if (k != AGGL_CNT) {
      bool is_int = (a.return_type == DType::Int64);
      bool is_i32 = (a.return_type == DType::Int32);
      ma.acc_t = is_i32 ? 2 : (is_int ? 1 : 0);
      any_i32 |= is_i32;
      if (!val_typed_seen_) {
        val_is_int_ = is_int;
        val_typed_seen_ = true;
      } else if (val_is_int_ != (is_int || is_i32)) {
        mixed_acc = true;
      }
      if (k == AGGL_AVG && (is_int || is_i32))
        FAIL("AggExec: AVG with integer output unsupported (avg.rs "
             "declares a floating result)");
    }
    ma_desc_.a[ma_desc_.n++] = ma;
    agg_kinds_.push_back(k);
    agg_names_.push_back(i < node.agg_names.size() ? node.agg_names[i]
                                                   : "agg" + std::to_string(i));
    ma_arg_cols_.push_back(-1);
    if (!merge_mode_) {
      const Expr& child = a.children.at(0);
      if (child.kind == Expr::Literal) {
        ScalarLit sl;
        std::string e2;
        if (!decode_ipc_scalar(child.literal_ipc.data(),
                               child.literal_ipc.size(), &sl, &e2) ||
            !sl.is_null)
          FAIL("aggregate Literal arg must be NULL on this path");
        have_null_lit = true;  // collect.rs-style empty behavior
      } else if (child.kind == Expr::Column) {
        ma_arg_cols_.back() = (int)child.col_index;
        if (!have_col) {
          val_col_ = child.col_index;
          have_col = true;
        } else if (child.col_index != val_col_) {
          have_distinct_cols = true;
        }
      } else {
        FAIL("aggregate arg must be a Column or NULL literal");
      }
    }
  }
  // Multi-argument mode (agg.rs:73-169: independent arg expressions per
  // agg; per-agg accumulator columns at the declared types). The trigger
  // rule is computable from the PLAN alone, so a Partial task and its
  // Final consumer always agree on the a8 wire layout: family duplicates
  // make the legacy shared-accumulator wire ambiguous; Int32/mixed
  // accumulator types and multiple collect pools are not representable in
  // it at all. Distinct arg columns / NULL-literal args additionally
  // trigger ma on the PARTIAL side (the wire stays legacy-parseable when
  // families do not repeat, so the Final side may run either mode).
  ma_mode_ = fam_sum > 1 || fam_cnt > 1 || fam_min > 1 || fam_max > 1 ||
             fam_first > 1 || fam_firstin > 1 || npools > 1 || any_i32 ||
             mixed_acc ||
             (!merge_mode_ && (have_distinct_cols || have_null_lit));
  if (!ma_mode_ && node.agg_exprs.size() > 8)
    FAIL("AggExec: >8 aggregates require the multi-arg layout");
  if (ma_mode_) {
    if (npools > MA_MAX_POOLS)
      FAIL("AggExec: at most 4 COLLECT aggregates");
    int pool = 0;
    for (int j = 0; j < ma_desc_.n; j++)
      if (ma_desc_.a[j].kind == AGGL_CLIST ||
          ma_desc_.a[j].kind == AGGL_CSET)
        ma_desc_.a[j].pool = (uint8_t)pool++;
    // the legacy side-array machinery is replaced by the bank
    has_mm_ = has_first_ = has_coll_ = false;
    skip_enabled_ = false;
  } else {
    bool has_l = false, has_s = false;
    for (uint32_t kk : agg_kinds_) {
      has_l |= (kk == AGGL_CLIST);
      has_s |= (kk == AGGL_CSET);
    }
    if (has_l && has_s)
      FAIL("COLLECT_LIST and COLLECT_SET together share one argument pool "
           "— unsupported on this path (single-pool legacy layout)");
    if (!merge_mode_ && !have_col && !node.agg_exprs.empty()) {
      bool only_counts = true;
      for (uint32_t kk : agg_kinds_) only_counts &= (kk == AGGL_CNT);
      if (!only_counts) FAIL("aggregate arg must be a Column");
    }
  }
  batch_size_ = conf.get_i("BATCH_SIZE", 10000);
  if (batch_size_ <= 0) FAIL("invalid BATCH_SIZE conf");
  skip_enabled_ =
      node.supports_partial_skipping && !merge_mode_ && !ma_mode_;
  skip_ratio_ = conf.get_d("PARTIAL_AGG_SKIPPING_RATIO", 0.999);
  skip_min_rows_ = conf.get_i("PARTIAL_AGG_SKIPPING_MIN_ROWS", 20000);
  // device output: partial freeze output stays in HBM (ArrowDeviceArray
  // export) so the bench/exchange chain never round-trips through host
  device_out_ = conf.get_i("AURON_HIP_DEVICE_OUTPUT", 0) != 0 &&
                !final_output_;
  int64_t slots = conf.get_i("AURON_HIP_AGG_TABLE_SLOTS", 1 << 23);
  conf_coll_cap_ =
      std::max<int64_t>(1024, conf.get_i("AURON_HIP_COLLECT_POOL", 16 << 20));
  // VRAM budget for the slot table (a9 analog of MemManager's budget,
  // memmgr/mod.rs:36-105): exceeding it spills frozen records to host
  // buckets instead of growing (agg_table.rs:540-588 semantics).
  mem_budget_ = conf.get_i("AURON_HIP_MEM_BUDGET", 8LL << 30);
  num_spill_buckets_ =
      (int)std::max<int64_t>(16, conf.get_i("AURON_HIP_SPILL_BUCKETS", 16));
  max_cap_ = 1;
  while (max_cap_ * 2 * (int64_t)sizeof(AggSlot) <= mem_budget_)
    max_cap_ *= 2;
  if (slots > max_cap_) slots = max_cap_;
  init_table(slots);
  t_.sum_int = val_is_int_ ? 1u : 0u;
  AURON_HIP(hipEventCreate(&ev_start_));
  AURON_HIP(hipEventCreate(&ev_stop_));
}

AggOp::~AggOp() {
  for (auto& [e0, e1] : ev_pairs_) {
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  (void)hipEventDestroy(ev_start_);
  (void)hipEventDestroy(ev_stop_);
}

// HIP-event timing on the launch stream (roofline evidence for the update
// kernels; pairs are drained once at finish() so the hot loop never
// synchronizes for timing)
template <class F>
void AggOp::timed(F launch) {
  hipEvent_t e0, e1;
  AURON_HIP(hipEventCreate(&e0));
  AURON_HIP(hipEventCreate(&e1));
  AURON_HIP(hipEventRecord(e0, stream_));
  launch();
  AURON_HIP(hipEventRecord(e1, stream_));
  ev_pairs_.push_back({e0, e1});
}

void AggOp::consume(DevBatch&& b) {
  if (b.num_rows == 0) return;
  DevColumn& key = b.cols.at(key_col_);
  if (!key_mode_set_) {
    // key mode: single numeric column keeps the i64 slot fast path
    // (incl. the two-phase pipeline); anything else — Utf8, Float64, or
    // 2..4-column tuples — runs the generalized-key path (a4 closure,
    // agg_ctx.rs:219-231 substitution per SURVEY.md 8c(i))
    key_mode_set_ = true;
    gkey_ = !(key_cols_.size() == 1 &&
              (key.dt == DType::Int64 || key.dt == DType::Int32));
    if (gkey_) {
      if (has_first_ || has_coll_)
        FAIL("FIRST/COLLECT with Utf8/multi-column grouping keys "
             "unsupported on this path");
      skip_enabled_ = false;  // emit_skipped is single-key-column shaped
      for (uint32_t ci : key_cols_) {
        DType dt = b.cols.at(ci).dt;
        if (dt != DType::Int64 && dt != DType::Int32 &&
            dt != DType::Float64 && dt != DType::Utf8 &&
            dt != DType::Binary)
          FAIL("unsupported grouping key dtype");
        key_dts_.push_back(dt);
      }
      init_gkey();
    }
  }
  if (gkey_) {
    for (size_t k = 0; k < key_cols_.size(); k++)
      if (b.cols.at(key_cols_[k]).dt != key_dts_[k])
        FAIL("grouping key dtype changed mid-stream");
  } else {
  if (key.dt != DType::Int64 && key.dt != DType::Int32)
    FAIL("grouping key must be Int64/Int32");
  if (key_dt_ == DType::Unsupported) key_dt_ = key.dt;
  if (key.dt != key_dt_) FAIL("grouping key dtype changed mid-stream");
  if (key.dt == DType::Int32) {
    // widen to the i64 slot table; the narrow Int32 view is restored at
    // output (values round-trip exactly)
    DevBuf wide(b.num_rows * 8);
    launch_widen_i32_i64((const int32_t*)key.values, b.num_rows,
                         wide.get<int64_t>(), stream_);
    key.own_values = std::move(wide);
    key.values = key.own_values.get();
    key.dt = DType::Int64;
  }
  }
  if (ma_mode_ && gkey_)
    FAIL("multi-argument aggregates with Utf8/multi-column grouping keys "
         "unsupported on this path");
  if (ma_mode_ && !merge_mode_ && !ma_args_checked_) {
    ma_args_checked_ = true;
    for (int j = 0; j < ma_desc_.n; j++) {
      if (ma_arg_cols_[j] < 0) {
        ma_desc_.a[j].arg_dt = 3;  // NULL literal
        continue;
      }
      DType dt = b.cols.at(ma_arg_cols_[j]).dt;
      uint8_t code;
      if (dt == DType::Float64) code = 0;
      else if (dt == DType::Int64) code = 1;
      else if (dt == DType::Int32) code = 2;
      else FAIL("unsupported aggregate argument dtype");
      if (ma_desc_.a[j].acc_t != 0 && code == 0)
        FAIL("float argument with integer accumulator unsupported");
      ma_desc_.a[j].arg_dt = code;
    }
  }
  if (!merge_mode_ && !ma_mode_) {
    // sum.rs:78-88 prepare_partial_args: the argument is CAST to the
    // accumulator type before update. Narrower numeric args widen on
    // device; anything else fails loudly.
    DevColumn& val = b.cols.at(val_col_);
    const DType want = val_is_int_ ? DType::Int64 : DType::Float64;
    if (val.dt != want) {
      DevBuf wide(b.num_rows * 8);
      if (val.dt == DType::Int32 && want == DType::Int64)
        launch_widen_i32_i64((const int32_t*)val.values, b.num_rows,
                             wide.get<int64_t>(), stream_);
      else if (val.dt == DType::Int32 && want == DType::Float64)
        launch_cast_i32_f64((const int32_t*)val.values, b.num_rows,
                            wide.get<double>(), stream_);
      else if (val.dt == DType::Int64 && want == DType::Float64)
        launch_cast_i64_f64((const int64_t*)val.values, b.num_rows,
                            wide.get<double>(), stream_);
      else
        FAIL("unsupported agg argument cast");
      val.own_values = std::move(wide);
      val.values = val.own_values.get();
      val.dt = want;
    }
  }
  if (skipping_) {
    skipped_.push_back(std::move(b));
    return;
  }
  // Process in chunks with a HARD no-overflow guarantee: before each chunk,
  // capacity is ensured for the conservative bound ng_bound_ (last readback
  // + every row since being a new key), so a probe can never exhaust the
  // table mid-launch. Readbacks (stream syncs) happen only when the bound
  // nears the 3/4 load threshold — rare once cardinality saturates.
  auto slice_valid = [](const uint8_t* v, int64_t done) {
    return v ? v + done / 8 : nullptr;  // done is a multiple of 8
  };
  int64_t done = 0;
  DBG("agg.consume n=%lld merge=%d", (long long)b.num_rows, (int)merge_mode_);

  while (done < b.num_rows) {
    // two-phase path (update mode, large chunks): its table inserts are
    // bounded by counted staged/leftover lists, not by chunk rows, so it
    // chunks on partition-buffer size instead of table free slots.
    init_agg2_conf();  // chunk bound must be read BEFORE sizing the chunk
    // MIN/MAX agg sets stay single-phase: the LDS bucket kernel's slot
    // holds {key,cnt,sum,first} only (perf note in DESIGN.md)
    if (!gkey_ && !ma_mode_ && !merge_mode_ && !has_mm_ && !has_first_ &&
        !has_coll_ && b.num_rows - done >= AGG2_MIN_CHUNK) {
      int64_t chunk2 = std::min(b.num_rows - done, agg2_chunk_max_);
      if (done + chunk2 < b.num_rows) chunk2 &= ~(int64_t)7;
      two_phase_chunk(b, done, chunk2);
      done += chunk2;
      row_cursor_ += (uint64_t)chunk2;
      if (maybe_enter_skipping(b, done)) break;
      continue;
    }
    int64_t free_slots = t_.cap * 3 / 4 - (int64_t)ng_bound_;
    if (free_slots < (1 << 16)) {
      // the conservative bound is exhausted: read the true cardinality
      // first; grow only if the table is genuinely near 3/4 load
      refresh_ng();
      free_slots = t_.cap * 3 / 4 - (int64_t)ng_true_;
      if (free_slots < (1 << 16)) {
        ensure_capacity((int64_t)ng_true_ + (1 << 20));
        free_slots = t_.cap * 3 / 4 - (int64_t)ng_bound_;
      }
    }
    int64_t chunk = std::min(b.num_rows - done, free_slots);
    if (done + chunk < b.num_rows) chunk &= ~(int64_t)7;  // bitmap-sliceable
    if (ma_mode_) {
      ma_chunk(b, done, chunk);
    } else if (gkey_) {
      gkey_chunk(b, done, chunk);
    } else if (merge_mode_) {
      const DevColumn& buf = b.cols.at(1);
      if (buf.dt != DType::Binary) FAIL("agg-buf column must be Binary");
      // acc_offsets are absolute into buf.values, so only the index shifts
      launch_agg_merge_frozen(t_, (const int64_t*)key.values + done,
                              slice_valid(key.validity, done),
                              (const uint8_t*)buf.values, buf.offsets + done,
                              chunk, row_cursor_, layout_, stream_);
      if (has_first_)  // pass B: capture the winning records' values
        launch_first_capture_frozen(t_, (const int64_t*)key.values + done,
                                    slice_valid(key.validity, done),
                                    (const uint8_t*)buf.values,
                                    buf.offsets + done, nullptr, chunk,
                                    row_cursor_, layout_, stream_);
    } else {
      const DevColumn& val = b.cols.at(val_col_);
      const DType want = val_is_int_ ? DType::Int64 : DType::Float64;
      if (val.dt != want)
        FAIL("agg arg dtype must match the declared accumulator type "
             "(narrower args are widened at batch import)");
      timed([&] {
        launch_agg_update(t_, (const int64_t*)key.values + done,
                          slice_valid(key.validity, done),
                          (const double*)val.values + done,
                          slice_valid(val.validity, done), chunk, row_cursor_,
                          stream_);
        if (has_first_)  // pass B: same stream, so it runs after pass A
          launch_first_capture_update(t_, (const int64_t*)key.values + done,
                                      slice_valid(key.validity, done),
                                      (const double*)val.values + done,
                                      slice_valid(val.validity, done), chunk,
                                      row_cursor_, stream_);
      });
      update_rows_ += chunk;
    }
    done += chunk;
    row_cursor_ += (uint64_t)chunk;
    ng_bound_ += (uint64_t)chunk;
    DBG("agg.chunk done=%lld/%lld cap=%lld ng_bound=%llu", (long long)done,
        (long long)b.num_rows, (long long)t_.cap,
        (unsigned long long)ng_bound_);
    if (maybe_enter_skipping(b, done)) break;
  }
  held_.push_back(std::move(b));  // keep borrowed buffers alive
}

// partial skipping (agg_table.rs:109-120): needs the true cardinality.
// Returns true (and slices this batch's unprocessed tail into skipped_)
// when the policy flips to pass-through.
bool AggOp::maybe_enter_skipping(const DevBatch& b, int64_t done) {
  if (!skip_enabled_ || skipping_ || row_cursor_ < (uint64_t)skip_min_rows_)
    return false;
  refresh_ng();
  if ((double)ng_true_ / (double)row_cursor_ < skip_ratio_) return false;
  skipping_ = true;
  if (done < b.num_rows) {
    // the un-aggregated tail of this batch passes through, like the
    // reference flipping between batches
    DevBatch tail;
    tail.num_rows = b.num_rows - done;
    for (const DevColumn& src : b.cols) {
      DevColumn sc;
      sc.dt = src.dt;
      sc.len = tail.num_rows;
      if (src.dt == DType::Binary || src.dt == DType::Utf8)
        FAIL("binary columns unsupported in skip-tail slice");
      sc.values = (const uint8_t*)src.values + done * dtype_width(src.dt);
      sc.validity = src.validity ? src.validity + done / 8 : nullptr;
      tail.cols.push_back(std::move(sc));
    }
    skipped_.push_back(std::move(tail));
  }
  return true;
}

std::vector<OutField> AggOp::key_fields() const {
  std::vector<OutField> f;
  for (size_t k = 0; k < key_cols_.size(); k++) {
    DType kd = k < key_dts_.size() ? key_dts_[k] : key_out_dt();
    f.push_back({key_names_[k], kd, true});
  }
  return f;
}

DType AggOp::ma_out_dt(size_t i) const {
  switch (ma_desc_.a[i].acc_t) {
    case 1: return DType::Int64;
    case 2: return DType::Int32;
    default: return DType::Float64;
  }
}

std::vector<OutField> AggOp::output_fields() const {
  if (final_output_) {
    std::vector<OutField> f = key_fields();
    const DType svdt = val_is_int_ ? DType::Int64 : DType::Float64;
    for (size_t i = 0; i < agg_kinds_.size(); i++) {
      DType vdt = ma_mode_ ? ma_out_dt(i) : svdt;
      if (agg_kinds_[i] == AGGL_CNT)
        f.push_back({agg_names_[i], DType::Int64, false});
      else if (agg_kinds_[i] == AGGL_AVG)
        f.push_back({agg_names_[i], DType::Float64, true});
      else if (agg_kinds_[i] == AGGL_CLIST || agg_kinds_[i] == AGGL_CSET)
        // collect.rs:110-112: nullable() = false (empty lists, not nulls)
        f.push_back({agg_names_[i], vdt, false, /*is_list=*/true});
      else
        f.push_back({agg_names_[i], vdt, true});
    }
    return f;
  }
  // partial/partial-merge: grouping + AGG_BUF (agg/mod.rs:37)
  std::vector<OutField> f = key_fields();
  f.push_back({"#9223372036854775807", DType::Binary, false});
  return f;
}

// Sort one raw COLLECT pool — keyed items at [0, n0), null-key items at
// [cap-n1, cap) — into the views the freeze/emit kernels binary-search:
// {key ascending (signed), prio ascending within key} at [0, n0) of
// skey/sval, then the null-key items in prio order at [n0, n0+n1) of sval.
// dedup (COLLECT_SET) keeps the first occurrence of each (key, value).
// Returns the post-dedup (n0, n1); the raw pool is left untouched.
std::pair<int64_t, int64_t> AggOp::sort_collect_pool(
    const long long* key, const unsigned long long* prio,
    const unsigned long long* val, int64_t cap, int64_t n0, int64_t n1,
    bool dedup, DevBuf& skey, DevBuf& sval) {
  using u64 = unsigned long long;
  if (!pinned_meta_.get()) pinned_meta_.alloc(16);
  int64_t nmax = std::max<int64_t>(std::max(n0, n1), 1);
  // tmp / stmp: sort and scan scratch, grown on first use and shared by
  // every pass of both segments
  DevBuf tmp, stmp, idx(nmax * 4), idxo(nmax * 4), scr(nmax * 8);
  skey.alloc(std::max<int64_t>(n0 + n1, 1) * 8);
  sval.alloc(std::max<int64_t>(n0 + n1, 1) * 8);

  // one stable radix pass over `by`, gathering key/prio/val (null = not
  // carried) into the given destinations
  auto sort_pass = [&](const u64* by, int64_t n, const u64* k, const u64* p,
                       const u64* v, u64* k_out, u64* p_out, u64* v_out) {
    launch_iota_u32(idx.get<uint32_t>(), n, stream_);
    sort_pairs(by, idx.get<uint32_t>(), scr.get<u64>(), idxo.get<uint32_t>(),
               n, 64, &tmp, stream_);
    if (k) launch_gather_u64_idx(k, idxo.get<uint32_t>(), n, k_out, stream_);
    if (p) launch_gather_u64_idx(p, idxo.get<uint32_t>(), n, p_out, stream_);
    launch_gather_u64_idx(v, idxo.get<uint32_t>(), n, v_out, stream_);
  };

  // one segment of n items into [at, at+n') of the views; seg_key is null
  // for the null-key segment, whose key arrays stay empty throughout
  auto sort_segment = [&](const long long* seg_key, const u64* seg_prio,
                          const u64* seg_val, int64_t n,
                          int64_t at) -> int64_t {
    if (n == 0) return 0;
    size_t kbytes = seg_key ? n * 8 : 0;
    // working copies (ping-pong pairs)
    DevBuf ka(kbytes), kb(kbytes), biased(kbytes), pa(n * 8), pb(n * 8),
        va(n * 8), vb(n * 8);
    if (seg_key)
      AURON_HIP(hipMemcpyAsync(ka.get(), seg_key, n * 8,
                               hipMemcpyDeviceToDevice, stream_));
    AURON_HIP(hipMemcpyAsync(pa.get(), seg_prio, n * 8,
                             hipMemcpyDeviceToDevice, stream_));
    AURON_HIP(hipMemcpyAsync(va.get(), seg_val, n * 8,
                             hipMemcpyDeviceToDevice, stream_));
    auto K = [](DevBuf& b) { return b.get<u64>(); };
    auto pass = [&](DevBuf& by) {
      sort_pass(K(by), n, K(ka), K(pa), K(va), K(kb), K(pb), K(vb));
      std::swap(ka, kb); std::swap(pa, pb); std::swap(va, vb);
    };
    pass(pa);  // arrival (prio) order
    if (dedup) {
      // AccSet dedup (collect.rs AccSet.append: only novel values): sort
      // by value then key (stable keeps prio asc inside runs), keep each
      // (key, value) run head = first occurrence
      pass(va);
      if (seg_key) {
        launch_bias_i64(K(ka), n, K(biased), stream_);
        pass(biased);
      }
      DevBuf mark(n), pos((n + 1) * 4);
      launch_coll_mark_heads(ka.get<long long>(), K(va), n, seg_key ? 1 : 0,
                             mark.get<uint8_t>(), stream_);
      scan_mask_positions(mark.get<uint8_t>(), n, pos.get<uint32_t>(), &stmp,
                          stream_);
      for (DevBuf* arr : {&ka, &pa, &va}) {
        if (!*arr) continue;
        launch_compact_u64(K(*arr), mark.get<uint8_t>(),
                           pos.get<uint32_t>(), n, scr.get<u64>(), stream_);
        AURON_HIP(hipMemcpyAsync(arr->get(), scr.get(), n * 8,
                                 hipMemcpyDeviceToDevice, stream_));
      }
      // new count = scan total (slot n of pos)
      AURON_HIP(hipMemcpyAsync(pinned_meta_.get(), pos.get<uint32_t>() + n,
                               4, hipMemcpyDeviceToHost, stream_));
      AURON_HIP(hipStreamSynchronize(stream_));
      n = (int64_t)*pinned_meta_.get<uint32_t>();
      if (n == 0) return 0;
      pass(pa);  // restore prio order
    }
    if (seg_key) {
      // final pass: sign-biased key order, stable (prio asc within key)
      launch_bias_i64(K(ka), n, K(biased), stream_);
      sort_pass(K(biased), n, K(ka), nullptr, K(va), skey.get<u64>() + at,
                nullptr, sval.get<u64>() + at);
    } else {
      AURON_HIP(hipMemcpyAsync(sval.get<u64>() + at, va.get(), n * 8,
                               hipMemcpyDeviceToDevice, stream_));
    }
    AURON_HIP(hipStreamSynchronize(stream_));  // temps return to the pool
    return n;
  };

  n0 = sort_segment(key, prio, val, n0, 0);
  // the back segment's arrival order is reversed in memory; the prio sort
  // restores it regardless
  n1 = sort_segment(nullptr, prio + (cap - n1), val + (cap - n1), n1, n0);
  return {n0, n1};
}

// device counters must match the sorted views' binary-search bounds
void AggOp::upload_pool_counts(unsigned long long* d_n, int64_t n0,
                               int64_t n1) {
  unsigned long long* h = pinned_meta_.get<unsigned long long>();
  h[0] = (unsigned long long)n0;
  h[1] = (unsigned long long)n1;
  AURON_HIP(hipMemcpyAsync(d_n, h, 16, hipMemcpyHostToDevice, stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
}

// Sort the legacy COLLECT pool (sort_collect_pool) and point the table's
// c_key/c_val views at the sorted arrays. One-shot before any emit.
void AggOp::prepare_collect() {
  if (!has_coll_ || coll_sorted_) return;
  coll_sorted_ = true;
  if (pinned_meta_.size() < 32) pinned_meta_.alloc(32);
  AURON_HIP(hipMemcpyAsync(pinned_meta_.get(), d_cn_.get(), 16,
                           hipMemcpyDeviceToHost, stream_));
  uint32_t* errp = pinned_meta_.get<uint32_t>() + 4;
  AURON_HIP(hipMemcpyAsync(errp, t_.error_flag, 4, hipMemcpyDeviceToHost,
                           stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
  int64_t n0 = (int64_t)pinned_meta_.get<unsigned long long>()[0];
  int64_t n1 = (int64_t)pinned_meta_.get<unsigned long long>()[1];
  // the per-append guard reads the opposing counter non-atomically (an
  // approximate early trip); this is the exact post-hoc check
  if ((*errp & 4u) || n0 + n1 > coll_cap_)
    FAIL("collect pool overflow: raise AURON_HIP_COLLECT_POOL");
  std::tie(coll_n0_, coll_n1_) =
      sort_collect_pool(t_.c_key, t_.c_prio, t_.c_val, coll_cap_, n0, n1,
                        coll_set_, d_cskey_, d_csval_);
  upload_pool_counts(d_cn_.get<unsigned long long>(), coll_n0_, coll_n1_);
  t_.c_key = d_cskey_.get<long long>();
  t_.c_val = d_csval_.get<unsigned long long>();
  t_.c_cap = coll_n0_ + coll_n1_;  // null segment ends the sorted view
}

// Sort each multi-arg collect pool like prepare_collect sorts the legacy
// one (COLLECT_SET pools dedup). The sorted views replace the raw pool
// pointers in mp_ (no further appends happen after finish) and the device
// counters are updated to the post-dedup counts.
void AggOp::prepare_ma_pools() {
  if (!ma_mode_ || ma_pools_sorted_) return;
  ma_pools_sorted_ = true;
  if (pinned_meta_.size() < MA_MAX_POOLS * 16)
    pinned_meta_.alloc(MA_MAX_POOLS * 16);
  unsigned long long* h_n = pinned_meta_.get<unsigned long long>();
  AURON_HIP(hipMemcpyAsync(h_n, d_mp_n_.get(), MA_MAX_POOLS * 16,
                           hipMemcpyDeviceToHost, stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
  for (int p = 0; p < MA_MAX_POOLS; p++) {  // raw until the pool is sorted
    mp_counts_[p][0] = (int64_t)h_n[2 * p];
    mp_counts_[p][1] = (int64_t)h_n[2 * p + 1];
  }
  for (int j = 0; j < ma_desc_.n; j++) {
    uint8_t p = ma_desc_.a[j].pool;
    if (p >= MA_MAX_POOLS) continue;
    int64_t n0 = mp_counts_[p][0], n1 = mp_counts_[p][1];
    if (n0 + n1 > mp_.cap) FAIL("collect pool overflow (ma mode)");
    std::tie(n0, n1) = sort_collect_pool(
        mp_.key[p], mp_.prio[p], mp_.val[p], mp_.cap, n0, n1,
        ma_desc_.a[j].kind == AGGL_CSET, d_mp_skey_[p], d_mp_sval_[p]);
    upload_pool_counts(d_mp_n_.get<unsigned long long>() + 2 * p, n0, n1);
    mp_.key[p] = d_mp_skey_[p].get<long long>();
    mp_.val[p] = d_mp_sval_[p].get<unsigned long long>();
    mp_counts_[p][0] = n0;
    mp_counts_[p][1] = n1;
  }
}

std::vector<HostOutBatch> AggOp::finish() {
  std::vector<HostOutBatch> out;
  drain_timing();
  if (spill_.empty()) {
    emit_table(&out, false);
  } else {
    // a9 analog (agg_table.rs:540-588 spill + RadixQueue merge): drain the
    // live table into the buckets, then merge+emit bucket by bucket so
    // peak table size is one bucket's groups. Output order is per-bucket
    // (the reference's own spill path also gives up global insertion
    // order), first-occurrence-ordered within each bucket.
    spill_table();
    for (size_t b = 0; b < spill_.size(); b++) {
      SpillBucket& sb = spill_[b];
      int64_t n = (int64_t)sb.keys.size();
      if (n > 0) {
        std::vector<int32_t> offs(n + 1, 0);
        for (int64_t i = 0; i < n; i++) offs[i + 1] = offs[i] + sb.lens[i];
        DevBuf d_keys(n * 8), d_first(n * 8), d_offs((n + 1) * 4),
            d_data(offs[n] ? offs[n] : 1);
        AURON_HIP(hipMemcpyAsync(d_keys.get(), sb.keys.data(), n * 8,
                                 hipMemcpyHostToDevice, stream_));
        AURON_HIP(hipMemcpyAsync(d_first.get(), sb.first_rows.data(), n * 8,
                                 hipMemcpyHostToDevice, stream_));
        AURON_HIP(hipMemcpyAsync(d_offs.get(), offs.data(), (n + 1) * 4,
                                 hipMemcpyHostToDevice, stream_));
        if (offs[n])
          AURON_HIP(hipMemcpyAsync(d_data.get(), sb.data.data(), offs[n],
                                   hipMemcpyHostToDevice, stream_));
        for (int64_t done2 = 0; done2 < n;) {
          ensure_capacity((int64_t)ng_bound_ +
                          std::min<int64_t>(n - done2, 1 << 20));
          int64_t free2 = t_.cap * 3 / 4 - (int64_t)ng_bound_;
          if (free2 <= 0)
            FAIL("spill bucket exceeds VRAM budget: raise "
                 "AURON_HIP_SPILL_BUCKETS");
          int64_t piece = std::min(n - done2, free2);
          launch_agg_merge_spill(t_, d_keys.get<int64_t>() + done2,
                                 d_data.get<uint8_t>(),
                                 d_offs.get<int32_t>() + done2,
                                 d_first.get<unsigned long long>() + done2,
                                 piece, layout_, stream_);
          if (has_first_)  // pass B with the records' preserved priorities
            launch_first_capture_frozen(
                t_, d_keys.get<int64_t>() + done2, nullptr,
                d_data.get<uint8_t>(), d_offs.get<int32_t>() + done2,
                d_first.get<unsigned long long>() + done2, piece, 0,
                layout_, stream_);
          done2 += piece;
          ng_bound_ += (uint64_t)piece;
        }
        AURON_HIP(hipStreamSynchronize(stream_));
      }
      bool last = (b + 1 == spill_.size());
      emit_table(&out, /*exclude_specials=*/!last);
      if (!last) {
        reset_main();
        // the pool holds this bucket's merged items + the resident
        // specials; keep only the specials for the next bucket
        if (has_coll_) reset_collect_pool();
      }
    }
    spill_.clear();
  }
  // 2) partial-skipped pass-through batches (agg_ctx.rs:428-462)
  for (DevBatch& b : skipped_) {
    out.emplace_back(emit_skipped(b));
  }
  skipped_.clear();
  held_.clear();
  return out;
}

std::vector<DevOutBatch> AggOp::finish_dev() {
  std::vector<DevOutBatch> out;
  drain_timing();
  prepare_collect();
  if (gkey_ || ma_mode_)
    FAIL("AURON_HIP_DEVICE_OUTPUT with generalized keys / multi-argument "
         "aggregates unsupported (unset the conf)");
  if (!spill_.empty())
    FAIL("AURON_HIP_DEVICE_OUTPUT with spill unsupported (unset the conf)");
  if (!skipped_.empty())
    FAIL("AURON_HIP_DEVICE_OUTPUT with partial skipping unsupported");
  DevBuf order, first;
  int64_t ng = table_order(&order, &first);
  for (int64_t beg = 0; beg < ng; beg += batch_size_) {
    int64_t len = std::min(batch_size_, ng - beg);
    out.emplace_back(emit_groups_dev(order.get<uint32_t>() + beg, len));
  }
  AURON_HIP(hipStreamSynchronize(stream_));  // order/first return to pool
  held_.clear();
  return out;
}

DevOutBatch AggOp::emit_groups_dev(const uint32_t* order_slots, int64_t n) {
  size_t bm = (n + 7) / 8;
  std::vector<DevOutCol> cols(2);
  DevOutCol& kc = cols[0];
  DevOutCol& bc = cols[1];
  kc.dt = key_out_dt();
  DevBuf keys(n * 8), wide, sums(n * 8), svalid(bm), cnts(n * 8);
  kc.validity.alloc(bm);
  launch_agg_gather_out(t_, order_slots, n, keys.get<int64_t>(),
                        kc.validity.get<uint8_t>(), sums.get<double>(),
                        svalid.get<uint8_t>(), cnts.get<long long>(),
                        nullptr, nullptr, nullptr, nullptr, nullptr,
                        stream_);
  narrow_keys(keys, wide, n);
  kc.values = std::move(keys);
  // freeze lens -> device exclusive scan -> offsets (+ total in slot n)
  bc.dt = DType::Binary;
  DevBuf lens((n + 1) * 4);
  bc.offsets.alloc((n + 1) * 4);
  launch_agg_freeze_len(t_, order_slots, n, lens.get<int32_t>(), layout_,
                        stream_);
  DevBuf scan_tmp;
  if (pinned_meta_.size() < 16) pinned_meta_.alloc(16);
  bc.data_len = scan_lens_offsets(lens.get<uint32_t>(), n,
                                  bc.offsets.get<uint32_t>(), &scan_tmp,
                                  pinned_meta_.get<uint32_t>(), stream_);
  bc.values.alloc(bc.data_len ? bc.data_len : 1);
  launch_agg_freeze_write(t_, order_slots, n, bc.offsets.get<int32_t>(),
                          bc.values.get<uint8_t>(), layout_, stream_);
  return {n, std::move(cols)};
}

uint64_t AggOp::num_groups_host() {
  if (!pinned_meta_.get()) pinned_meta_.alloc(16);
  uint64_t* ng = pinned_meta_.get<uint64_t>();
  uint32_t* err = (uint32_t*)(pinned_meta_.get<uint8_t>() + 8);
  AURON_HIP(hipMemcpyAsync(ng, t_.num_groups, 8, hipMemcpyDeviceToHost,
                           stream_));
  AURON_HIP(hipMemcpyAsync(err, t_.error_flag, 4, hipMemcpyDeviceToHost,
                           stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
  if (*err) {
    // bit 1: table probe exhausted; 16: gkey pool publish spin; 32:
    // scatter tile bound; 64: reserved (was the removed ring scatter's
    // retry bound) — do not reuse
    if (*err & ~1u)
      FAIL("agg device error flags 0x" +
           ([](uint32_t v) {
             char b[16];
             snprintf(b, sizeof b, "%x", v);
             return std::string(b);
           })(*err));
    FAIL("agg hash table probe exhausted (table full/corrupt)");
  }
  return *ng;
}

void AggOp::init_table(int64_t slots) {
  int64_t cap = 1;
  while (cap < slots) cap <<= 1;
  t_.cap = cap;
  d_slots_.alloc((cap + 2) * sizeof(AggSlot));
  d_special_.alloc(2 * 4);
  d_ng_.alloc(8);
  d_err_.alloc(4);
  t_.slots = d_slots_.get<AggSlot>();
  t_.special_used = d_special_.get<uint32_t>();
  t_.num_groups = d_ng_.get<unsigned long long>();
  t_.error_flag = d_err_.get<uint32_t>();
  AURON_HIP(hipMemsetAsync(d_err_.get(), 0, 4, stream_));
  AURON_HIP(hipMemsetAsync(d_special_.get(), 0, 2 * 4, stream_));
  AURON_HIP(hipMemsetAsync(d_ng_.get(), 0, 8, stream_));
  launch_slots_init(t_.slots, cap + 2, stream_);
  if (has_mm_) {
    d_mm_.alloc((cap + 2) * 16);
    t_.mm = d_mm_.get<unsigned long long>();
    launch_mm_init(t_.mm, cap + 2, stream_);
  }
  if (has_first_) {
    d_frow_.alloc((cap + 2) * 16);
    d_fval_.alloc((cap + 2) * 16);
    d_fst_.alloc((cap + 2) * 2);
    t_.f_row = d_frow_.get<unsigned long long>();
    t_.f_val = d_fval_.get<double>();
    t_.f_st = d_fst_.get<uint8_t>();
    launch_first_init(t_.f_row, t_.f_val, t_.f_st, cap + 2, stream_);
  }
  if (ma_mode_) {  // per-agg accumulator bank (growth re-allocs)
    int64_t cap2 = cap + 2;
    d_ma_acc_.alloc((int64_t)ma_desc_.n * cap2 * 8);
    d_ma_meta_.alloc((int64_t)ma_desc_.n * cap2 * 8);
    d_ma_st_.alloc((int64_t)ma_desc_.n * cap2);
    ma_.acc = d_ma_acc_.get<unsigned long long>();
    ma_.meta = d_ma_meta_.get<unsigned long long>();
    ma_.st = d_ma_st_.get<uint8_t>();
    ma_.stride = cap2;
    launch_ma_init(ma_desc_, ma_, cap2, stream_);
    if (!d_mp_n_) {  // pools survive growth (keyed by VALUE not slot)
      int64_t pc = std::max<int64_t>(1024, conf_coll_cap_ / 4);
      for (int j = 0; j < ma_desc_.n; j++) {
        uint8_t p = ma_desc_.a[j].pool;
        if (p >= MA_MAX_POOLS) continue;
        d_mp_key_[p].alloc(pc * 8);
        d_mp_prio_[p].alloc(pc * 8);
        d_mp_val_[p].alloc(pc * 8);
        mp_.cap = pc;
      }
      d_mp_n_.alloc(MA_MAX_POOLS * 16);
      AURON_HIP(hipMemsetAsync(d_mp_n_.get(), 0, MA_MAX_POOLS * 16,
                               stream_));
    }
    for (int p = 0; p < MA_MAX_POOLS; p++) {
      if (!d_mp_key_[p]) continue;
      mp_.key[p] = d_mp_key_[p].get<long long>();
      mp_.prio[p] = d_mp_prio_[p].get<unsigned long long>();
      mp_.val[p] = d_mp_val_[p].get<unsigned long long>();
    }
    mp_.n = d_mp_n_.get<unsigned long long>();
  }
  if (gkey_) {  // growth re-allocs the off array; pool survives
    d_gkoff_.alloc(cap * 8);
    AURON_HIP(hipMemsetAsync(d_gkoff_.get(), 0, cap * 8, stream_));
    g_.off = d_gkoff_.get<unsigned long long>();
  }
  if (has_coll_ && !d_ckey_) {  // pool survives grows (keys, not slots)
    coll_cap_ = conf_coll_cap_;
    d_ckey_.alloc(coll_cap_ * 8);
    d_cprio_.alloc(coll_cap_ * 8);
    d_cval_.alloc(coll_cap_ * 8);
    d_cn_.alloc(16);
    AURON_HIP(hipMemsetAsync(d_cn_.get(), 0, 16, stream_));
  }
  if (has_coll_) {
    t_.c_key = d_ckey_.get<long long>();
    t_.c_prio = d_cprio_.get<unsigned long long>();
    t_.c_val = d_cval_.get<unsigned long long>();
    t_.c_n = d_cn_.get<unsigned long long>();
    t_.c_cap = coll_cap_;
  }
}

// ---- multi-argument chunk (kernels_maarg.hip) --------------------------
void AggOp::ma_chunk(const DevBatch& b, int64_t done, int64_t chunk) {
  const DevColumn& key = b.cols.at(key_col_);
  const int64_t* keys = (const int64_t*)key.values + done;
  const uint8_t* kv = key.validity ? key.validity + done / 8 : nullptr;
  if (d_ma_slots_.size() < (size_t)chunk * 4) d_ma_slots_.alloc(chunk * 4);
  MaArgs args;
  if (!merge_mode_) {
    for (int j = 0; j < ma_desc_.n; j++) {
      if (ma_arg_cols_[j] < 0) continue;
      const DevColumn& c = b.cols.at(ma_arg_cols_[j]);
      size_t w = dtype_width(c.dt);
      args.vals[j] = (const uint8_t*)c.values + (size_t)done * w;
      args.valid[j] = c.validity ? c.validity + done / 8 : nullptr;
    }
  }
  timed([&] {
    launch_slots_upsert(t_, keys, kv, chunk, row_cursor_,
                        d_ma_slots_.get<uint32_t>(), stream_);
    bool any_first = false;
    for (int j = 0; j < ma_desc_.n; j++)
      any_first |= (ma_desc_.a[j].kind == AGGL_FIRST ||
                    ma_desc_.a[j].kind == AGGL_FIRSTIN);
    if (merge_mode_) {
      const DevColumn& buf = b.cols.at(1);
      if (buf.dt != DType::Binary) FAIL("agg-buf column must be Binary");
      launch_ma_merge_frozen(t_, ma_desc_, ma_, mp_, keys, kv,
                             d_ma_slots_.get<uint32_t>(),
                             (const uint8_t*)buf.values, buf.offsets + done,
                             chunk, row_cursor_, stream_);
      if (any_first)
        launch_ma_first_capture_frozen(t_, ma_desc_, ma_,
                                       d_ma_slots_.get<uint32_t>(),
                                       (const uint8_t*)buf.values,
                                       buf.offsets + done, chunk,
                                       row_cursor_, stream_);
    } else {
      launch_ma_update(t_, ma_desc_, ma_, mp_, args, keys, kv,
                       d_ma_slots_.get<uint32_t>(), chunk, row_cursor_,
                       stream_);
      if (any_first)
        launch_ma_first_capture(t_, ma_desc_, ma_, args,
                                d_ma_slots_.get<uint32_t>(), chunk,
                                row_cursor_, stream_);
      update_rows_ += chunk;
    }
  });
}

// ---- generalized-key machinery (kernels_gkey.hip) ----------------------
void AggOp::init_gkey() {
  gk_pool_cap_ = 64 << 20;
  d_gkpool_.alloc(gk_pool_cap_);
  d_gkpn_.alloc(8);
  AURON_HIP(hipMemsetAsync(d_gkpn_.get(), 0, 8, stream_));
  d_gkoff_.alloc(t_.cap * 8);
  AURON_HIP(hipMemsetAsync(d_gkoff_.get(), 0, t_.cap * 8, stream_));
  g_.off = d_gkoff_.get<unsigned long long>();
  g_.pool = d_gkpool_.get<uint8_t>();
  g_.pool_n = d_gkpn_.get<unsigned long long>();
  g_.pool_cap = gk_pool_cap_;
  uint8_t dts[GKEY_MAX_COLS] = {};
  for (size_t k = 0; k < key_dts_.size(); k++) {
    switch (key_dts_[k]) {
      case DType::Int64: dts[k] = GK_I64; break;
      case DType::Int32: dts[k] = GK_I32; break;
      case DType::Float64: dts[k] = GK_F64; break;
      default: dts[k] = GK_UTF8; break;  // Utf8/Binary
    }
  }
  d_gkdts_.alloc(GKEY_MAX_COLS);
  AURON_HIP(hipMemcpyAsync(d_gkdts_.get(), dts, GKEY_MAX_COLS,
                           hipMemcpyHostToDevice, stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
}

void AggOp::gk_ensure_pool(int64_t need_more) {
  if (gk_used_bound_ + need_more <= gk_pool_cap_) return;
  // refresh the true cursor (the bound counts every row as a new group)
  if (pinned_meta_.size() < 16) pinned_meta_.alloc(16);
  AURON_HIP(hipMemcpyAsync(pinned_meta_.get(), d_gkpn_.get(), 8,
                           hipMemcpyDeviceToHost, stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
  gk_used_bound_ = (int64_t)*pinned_meta_.get<unsigned long long>();
  if (gk_used_bound_ + need_more <= gk_pool_cap_) return;
  int64_t new_cap = gk_pool_cap_;
  while (new_cap < gk_used_bound_ + need_more) new_cap *= 2;
  DevBuf np(new_cap);
  AURON_HIP(hipMemcpyAsync(np.get(), d_gkpool_.get(), gk_pool_cap_,
                           hipMemcpyDeviceToDevice, stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
  d_gkpool_ = std::move(np);
  gk_pool_cap_ = new_cap;
  g_.pool = d_gkpool_.get<uint8_t>();
  g_.pool_cap = gk_pool_cap_;
}

GKeyCols AggOp::gk_cols(const DevBatch& b, int64_t done) const {
  GKeyCols gc;
  gc.ncols = (int)key_cols_.size();
  for (size_t k = 0; k < key_cols_.size(); k++) {
    const DevColumn& c = b.cols.at(key_cols_[k]);
    switch (key_dts_[k]) {
      case DType::Int64:
      case DType::Float64:
        gc.dt[k] = key_dts_[k] == DType::Int64 ? GK_I64 : GK_F64;
        gc.values[k] = (const uint8_t*)c.values + done * 8;
        break;
      case DType::Int32:
        gc.dt[k] = GK_I32;
        gc.values[k] = (const uint8_t*)c.values + done * 4;
        break;
      default:  // Utf8/Binary: offsets are absolute into the data buffer
        gc.dt[k] = GK_UTF8;
        gc.values[k] = c.values;
        gc.offsets[k] = c.offsets + done;
        break;
    }
    gc.validity[k] = c.validity ? c.validity + done / 8 : nullptr;
  }
  return gc;
}

// one bounded-size chunk of the generalized-key path: encode the key
// tuples -> scan -> upsert (slot per row) -> slot-indexed accumulate or
// frozen merge
void AggOp::gkey_chunk(const DevBatch& b, int64_t done, int64_t chunk) {
  GKeyCols gc = gk_cols(b, done);
  if (d_enclens_.size() < (size_t)(chunk + 1) * 4) {
    d_enclens_.alloc((chunk + 1) * 4);
    d_encoffs_.alloc((chunk + 1) * 4);
    d_gkslots_.alloc(chunk * 4);
  }
  launch_gkey_enc_lens(gc, chunk, d_enclens_.get<uint32_t>(), stream_);
  if (pinned_meta_.size() < 16) pinned_meta_.alloc(16);
  int64_t total = scan_lens_offsets(
      d_enclens_.get<uint32_t>(), chunk, d_encoffs_.get<uint32_t>(),
      &d_gkscan_tmp_, pinned_meta_.get<uint32_t>(), stream_);
  if (d_encbytes_.size() < (size_t)total + 8)
    d_encbytes_.alloc(total + 8);
  launch_gkey_enc_write(gc, d_encoffs_.get<uint32_t>(),
                        d_encbytes_.get<uint8_t>(), chunk, stream_);
  gk_ensure_pool(total + 4 * chunk);  // worst case: every row a new group
  timed([&] {
    launch_gkey_upsert(t_, g_, d_encoffs_.get<uint32_t>(),
                       d_encbytes_.get<uint8_t>(), chunk, row_cursor_,
                       d_gkslots_.get<uint32_t>(), stream_);
    if (merge_mode_) {
      const DevColumn& buf = b.cols.back();
      if (buf.dt != DType::Binary) FAIL("agg-buf column must be Binary");
      launch_gkey_merge_frozen_idx(t_, d_gkslots_.get<uint32_t>(),
                                   (const uint8_t*)buf.values,
                                   buf.offsets + done, chunk, layout_,
                                   stream_);
    } else {
      const DevColumn& val = b.cols.at(val_col_);
      launch_gkey_update_idx(t_, d_gkslots_.get<uint32_t>(),
                             (const double*)val.values + done,
                             val.validity ? val.validity + done / 8 : nullptr,
                             chunk, stream_);
      update_rows_ += chunk;
    }
  });
  gk_used_bound_ += total + 4 * chunk;
}

// Read the two-phase tuning knobs once, BEFORE the first chunk size is
// computed (the scratch buffers are sized from agg2_chunk_max_, so the
// bound must be final by then).
void AggOp::init_agg2_conf() {
  if (agg2_conf_read_) return;
  agg2_conf_read_ = true;
  const char* cm = getenv("AURON_AGG2_CHUNK_M");  // millions of rows
  if (cm && cm[0]) {
    int64_t m = atoll(cm);
    if (m >= 4 && m <= 1024) agg2_chunk_max_ = m << 20;
  }
  const char* p16 = getenv("AURON_AGG2_P16");
  agg2_p16_en_ = !(p16 && p16[0] == '0');
}

// Merge a COUNTED list of n table inserts (staged groups or leftover
// rows) piecewise, so a VRAM budget (spill) smaller than the list still
// works; launch(done, piece) enqueues entries [done, done+piece).
template <class Launch>
void AggOp::merge_counted(int64_t n, Launch launch) {
  for (int64_t done2 = 0; done2 < n;) {
    ensure_capacity((int64_t)ng_bound_ +
                    std::min<int64_t>(n - done2, 1 << 20));
    int64_t free2 = t_.cap * 3 / 4 - (int64_t)ng_bound_;
    if (free2 < (1 << 14)) {
      refresh_ng();
      free2 = t_.cap * 3 / 4 - (int64_t)ng_true_;
      if (free2 < (1 << 14)) {
        spill_table();
        continue;
      }
    }
    int64_t piece = std::min(n - done2, free2);
    launch(done2, piece);
    done2 += piece;
    ng_bound_ += (uint64_t)piece;
  }
}

// Two-phase aggregation of rows [done, done+chunk) of batch b:
// histogram -> line-padded scan -> LDS-staged packet scatter -> 4096-slot
// per-bucket LDS aggregate (kernels_agg3.hip) -> merge counted staged
// groups / leftover rows into the slot table (kernels_agg2.hip).
void AggOp::two_phase_chunk(const DevBatch& b, int64_t done, int64_t chunk) {
  const DevColumn& key = b.cols.at(key_col_);
  const DevColumn& val = b.cols.at(val_col_);
  const int64_t* keys = (const int64_t*)key.values + done;
  const double* vals = (const double*)val.values + done;
  const uint8_t* kv = key.validity ? key.validity + done / 8 : nullptr;
  const uint8_t* vv = val.validity ? val.validity + done / 8 : nullptr;
  const int64_t mat = (int64_t)AGG3_NBUCK << AGG3_GRID_LOG2;
  // the merges below insert rows of this chunk and may spill (table_order)
  // before the caller advances row_cursor_
  first_row_bound_ = row_cursor_ + (uint64_t)chunk;

  if (!d_partkv_) {
    // 24B records + one line of alignment padding per (block,bucket)
    d_partkv_.alloc(agg2_chunk_max_ * 24 + mat * 64);
    d_leftover_.alloc(agg2_chunk_max_ * sizeof(PartRow));
    d_counts_.alloc((mat + 1) * 4);   // +1: scan total slot
    d_scanned_.alloc((mat + 1) * 4);
    d_linesz_.alloc((mat + 1) * 4);
    size_t tb = 0;
    scan_counts_matrix(d_linesz_.get<uint32_t>(), d_scanned_.get<uint32_t>(),
                       mat + 1, nullptr, &tb, stream_);
    d_scan_tmp_.alloc(tb);
    d_staged_.alloc(AGG3_STAGED_CAP * sizeof(StagedGroup));
    d_counters_.alloc(24);  // staged_n, lo_n, special_rows
    // layout: counters[3] u64 (copy of d_counters_) | num_groups u64
    pinned_agg2_.alloc(32);
  }
  timed([&] {
    // ONE host sync per chunk: the special/staged/leftover counters are read
    // back together after the bucket aggregation.
    AURON_HIP(hipMemsetAsync(d_counters_.get(), 0, 24, stream_));
    // adaptive packed-16B records: if the normal-key range fits u32, chunks
    // store (key - base) u32 — 33% less partition traffic. Out-of-range keys
    // in later chunks take the counted leftover bypass, so the choice is a
    // pure optimization, never a correctness bet.
    // The range comes out of the first chunk's histogram pass (one
    // atomicMin/atomicMax per wave), so even the FIRST chunk runs the packed
    // layout and no pass over the keys is spent on the decision.
    const bool probe = agg2_p16_en_ && !p16_decided_;
    if (probe) {
      if (!d_kminmax_) d_kminmax_.alloc(16);
      AURON_HIP(hipMemsetAsync(d_kminmax_.get(), 0xFF, 8, stream_));
      AURON_HIP(hipMemsetAsync(d_kminmax_.get<uint8_t>() + 8, 0, 8, stream_));
    }
    launch_agg2_hist(keys, kv, chunk, AGG3_NBUCK_LOG2, AGG3_GRID_LOG2,
                     d_counts_.get<uint32_t>(),
                     (uint32_t*)(d_counters_.get<uint8_t>() + 16),
                     probe ? d_kminmax_.get<unsigned long long>() : nullptr,
                     stream_);
    if (probe) {
      // pinned_agg2_'s four words are free until the counter readback below
      uint64_t* h_kmm = pinned_agg2_.get<uint64_t>();
      AURON_HIP(hipMemcpyAsync(h_kmm, d_kminmax_.get(), 16,
                               hipMemcpyDeviceToHost, stream_));
      AURON_HIP(hipStreamSynchronize(stream_));
      p16_decided_ = true;
      // an empty range (no normal key in the chunk) reads ~0 > 0: stays 24B
      if (h_kmm[0] <= h_kmm[1] && h_kmm[1] - h_kmm[0] <= 0xFFFFFFFFull) {
        packed16_ = true;
        key_base16_ = (int64_t)(h_kmm[0] ^ 0x8000000000000000ull);
        DBG("agg.p16 enabled: key range %llu",
            (unsigned long long)(h_kmm[1] - h_kmm[0]));
      }
    }
    const int rec = packed16_ ? 16 : 24;
    launch_agg3_line_sizes(d_counts_.get<uint32_t>(), mat + 1,
                           d_linesz_.get<uint32_t>(), rec, stream_);
    size_t tb = d_scan_tmp_.size();
    scan_counts_matrix(d_linesz_.get<uint32_t>(), d_scanned_.get<uint32_t>(),
                       mat + 1, d_scan_tmp_.get(), &tb, stream_);
    launch_agg3_scatter(keys, kv, vals, vv, chunk, AGG3_NBUCK_LOG2,
                        AGG3_GRID_LOG2, d_scanned_.get<uint32_t>(),
                        d_partkv_.get<uint8_t>(), d_leftover_.get<PartRow>(),
                        d_counters_.get<unsigned long long>() + 1,
                        d_linesz_.get<uint32_t>(),  // free after the scan
                        t_.error_flag, rec, key_base16_, stream_);
    launch_agg3_bucket(d_partkv_.get<uint8_t>(), d_counts_.get<uint32_t>(),
                       d_linesz_.get<uint32_t>(), d_scanned_.get<uint32_t>(),
                       AGG3_GRID_LOG2, val_is_int_ ? 1 : 0, AGG3_NBUCK,
                       d_staged_.get<StagedGroup>(),
                       d_counters_.get<unsigned long long>(), AGG3_STAGED_CAP,
                       d_leftover_.get<PartRow>(),
                       d_counters_.get<unsigned long long>() + 1,
                       t_.error_flag, rec, key_base16_, stream_);
    unsigned long long* h_ctr = pinned_agg2_.get<unsigned long long>();
    AURON_HIP(hipMemcpyAsync(h_ctr, d_counters_.get(), 24,
                             hipMemcpyDeviceToHost, stream_));
    uint64_t* h_ng = (uint64_t*)(h_ctr + 3);
    AURON_HIP(hipMemcpyAsync(h_ng, t_.num_groups, 8, hipMemcpyDeviceToHost,
                             stream_));
    AURON_HIP(hipStreamSynchronize(stream_));
    int64_t staged_n = (int64_t)h_ctr[0];
    int64_t lo_n = (int64_t)h_ctr[1];
    uint32_t special_rows = (uint32_t)h_ctr[2];
    if (special_rows)
      launch_agg2_specials(t_, keys, kv, vals, vv, chunk, row_cursor_, stream_);
    // true cardinality from the piggybacked pre-merge read (no extra sync);
    // the piecewise merges below grow the bound as they go
    ng_true_ = *h_ng;
    ng_bound_ = *h_ng + (special_rows ? 2u : 0u);
    // merge: table inserts bounded by the COUNTED lists
    merge_counted(staged_n, [&](int64_t at, int64_t piece) {
      launch_agg2_merge_groups(t_, d_staged_.get<StagedGroup>() + at, piece,
                               row_cursor_, stream_);
    });
    merge_counted(lo_n, [&](int64_t at, int64_t piece) {
      launch_agg2_leftovers(t_, d_leftover_.get<PartRow>() + at, piece,
                            row_cursor_, stream_);
    });
    DBG("agg.2phase chunk=%lld staged=%lld leftover=%lld special=%u",
        (long long)chunk, (long long)staged_n, (long long)lo_n, special_rows);
  });
  update_rows_ += chunk;
}

// compact the table and return (order_slots sorted by first_row, ng);
// device buffers owned by the out-params
int64_t AggOp::table_order(DevBuf* slots_sorted, DevBuf* first_sorted) {
  uint64_t ng = num_groups_host();
  if (ng == 0) return 0;
  DevBuf slots_u(ng * 4), first(ng * 8), dcount(8);
  slots_sorted->alloc(ng * 4);
  first_sorted->alloc(ng * 8);
  AURON_HIP(hipMemsetAsync(dcount.get(), 0, 8, stream_));
  launch_agg_compact(t_, slots_u.get<uint32_t>(),
                     first.get<unsigned long long>(),
                     dcount.get<unsigned long long>(), (int64_t)ng, stream_);
  // every first_row is the global index of a consumed row or record
  // (spilled groups keep theirs from before the spill), so all of them are
  // below row_cursor_ — or, when a two-phase chunk spills while it merges,
  // below that chunk's end, which row_cursor_ reaches only afterwards:
  // sort only the bits that can be set
  const uint64_t bound = std::max(row_cursor_, first_row_bound_);
  int end_bit = 1;
  while (end_bit < 64 && (bound >> end_bit) != 0) end_bit++;
  DevBuf tmp;
  sort_pairs(first.get<unsigned long long>(), slots_u.get<uint32_t>(),
             first_sorted->get<unsigned long long>(),
             slots_sorted->get<uint32_t>(), (int64_t)ng, end_bit, &tmp,
             stream_);
  // pooled buffers (slots_u/first/tmp) must not be recycled while the sort
  // still reads them — the pool, unlike hipFree, does not synchronize
  AURON_HIP(hipStreamSynchronize(stream_));
  return (int64_t)ng;
}

// freeze the main-region groups to host spill buckets and reset the main
// region (the two special groups stay resident across spills)
void AggOp::spill_table() {
  drain_timing();
  // COLLECT pool drain (collect.rs spill analog): sort the pool so the
  // freeze kernels can binary-search each group's item run — the frozen
  // records then CARRY the items into the spill buckets; afterwards the
  // pool is reset to the resident specials' items only
  prepare_collect();
  DevBuf order, first;
  int64_t ng = table_order(&order, &first);
  if (ng == 0) return;
  std::vector<uint32_t> h_order(ng);
  std::vector<unsigned long long> h_first(ng);
  AURON_HIP(hipMemcpyAsync(h_order.data(), order.get(), ng * 4,
                           hipMemcpyDeviceToHost, stream_));
  AURON_HIP(hipMemcpyAsync(h_first.data(), first.get(), ng * 8,
                           hipMemcpyDeviceToHost, stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
  // filter out the special slots (they stay in the table)
  std::vector<uint32_t> main_order;
  std::vector<unsigned long long> main_first;
  for (int64_t i = 0; i < ng; i++) {
    if (h_order[i] < (uint32_t)t_.cap) {
      main_order.push_back(h_order[i]);
      main_first.push_back(h_first[i]);
    }
  }
  int64_t n = (int64_t)main_order.size();
  specials_count_ = ng - n;
  if (n > 0) {
    DevBuf d_order(n * 4), keys(n * 8);
    AURON_HIP(hipMemcpyAsync(d_order.get(), main_order.data(), n * 4,
                             hipMemcpyHostToDevice, stream_));
    launch_agg_gather_out(t_, d_order.get<uint32_t>(), n,
                          keys.get<int64_t>(), nullptr, nullptr, nullptr,
                          nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, stream_);
    std::vector<int64_t> h_keys(n);
    AURON_HIP(hipMemcpyAsync(h_keys.data(), keys.get(), n * 8,
                             hipMemcpyDeviceToHost, stream_));
    HostOutCol rec = freeze_agg_buf(d_order.get<uint32_t>(), n);
    emit_.sync();  // h_keys and the frozen bytes are on the host
    const int32_t* rec_offs = rec.offs();
    if (spill_.empty()) spill_.resize(num_spill_buckets_);
    for (int64_t i = 0; i < n; i++) {
      SpillBucket& b =
          spill_[host_mix64((uint64_t)h_keys[i]) % num_spill_buckets_];
      b.keys.push_back(h_keys[i]);
      b.first_rows.push_back(main_first[i]);
      b.lens.push_back(rec_offs[i + 1] - rec_offs[i]);
      b.data.insert(b.data.end(), rec.values.data() + rec_offs[i],
                    rec.values.data() + rec_offs[i + 1]);
    }
    spill_count_++;
  }
  reset_main();
  if (has_coll_) reset_collect_pool();
  DBG("agg.spill n=%lld buckets=%d", (long long)n, num_spill_buckets_);
}

// Rebuild the pool to hold exactly the two RESIDENT special groups' items
// (taken from the sorted views, order preserved; re-assigned prios 0..m
// stay below every future row/record priority) and restore the original
// pool arrays as the append target.
void AggOp::reset_collect_pool() {
  if (!has_coll_ || !coll_sorted_) return;
  uint32_t spec[2] = {(uint32_t)t_.cap, (uint32_t)(t_.cap + 1)};
  DevBuf d_spec(8), cnts(8), items;
  AURON_HIP(hipMemcpyAsync(d_spec.get(), spec, 8, hipMemcpyHostToDevice,
                           stream_));
  launch_coll_counts(t_, d_spec.get<uint32_t>(), 2, cnts.get<int32_t>(),
                     stream_);
  int32_t h_cnts[2];
  AURON_HIP(hipMemcpyAsync(h_cnts, cnts.get(), 8, hipMemcpyDeviceToHost,
                           stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
  int64_t m0 = h_cnts[0], m1 = h_cnts[1];
  int32_t h_offs[3] = {0, (int32_t)m0, (int32_t)(m0 + m1)};
  DevBuf d_offs(12);
  AURON_HIP(hipMemcpyAsync(d_offs.get(), h_offs, 12, hipMemcpyHostToDevice,
                           stream_));
  items.alloc((m0 + m1) * 8 + 8);
  launch_coll_gather(t_, d_spec.get<uint32_t>(), 2, d_offs.get<int32_t>(),
                     items.get<unsigned long long>(), stream_);
  // restore the ORIGINAL pool arrays as the live pool, then refill
  t_.c_key = d_ckey_.get<long long>();
  t_.c_prio = d_cprio_.get<unsigned long long>();
  t_.c_val = d_cval_.get<unsigned long long>();
  t_.c_cap = coll_cap_;
  launch_coll_refill(t_, items.get<unsigned long long>(), m0, m1, stream_);
  unsigned long long nn[2] = {(unsigned long long)m0,
                              (unsigned long long)m1};
  AURON_HIP(hipMemcpyAsync(d_cn_.get(), nn, 16, hipMemcpyHostToDevice,
                           stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
  coll_sorted_ = false;
  coll_n0_ = coll_n1_ = 0;
  d_cskey_ = DevBuf();
  d_csval_ = DevBuf();
}

void AggOp::reset_main() {
  launch_slots_init(t_.slots, t_.cap, stream_);  // specials untouched
  if (has_mm_) launch_mm_init(t_.mm, t_.cap, stream_);
  if (has_first_) launch_first_init(t_.f_row, t_.f_val, t_.f_st, t_.cap,
                                    stream_);
  uint64_t ng0 = (uint64_t)specials_count_;
  AURON_HIP(hipMemcpyAsync(t_.num_groups, &ng0, 8, hipMemcpyHostToDevice,
                           stream_));
  AURON_HIP(hipStreamSynchronize(stream_));
  ng_true_ = ng0;
  ng_bound_ = ng0;
}

void AggOp::refresh_ng() {
  ng_true_ = num_groups_host();
  ng_bound_ = ng_true_;
}

void AggOp::drain_timing() {
  if (ev_pairs_.empty()) return;
  AURON_HIP(hipStreamSynchronize(stream_));
  for (auto& [e0, e1] : ev_pairs_) {
    float ms = 0.f;
    AURON_HIP(hipEventElapsedTime(&ms, e0, e1));
    update_ns_ += (int64_t)(ms * 1e6);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  ev_pairs_.clear();
}

void AggOp::ensure_capacity(int64_t need) {
  while (t_.cap * 3 / 4 < need && t_.cap < max_cap_) grow(t_.cap * 4);
  if (t_.cap * 3 / 4 < need &&
      (int64_t)num_groups_host() > specials_count_) {
    if (gkey_)
      FAIL("spill with Utf8/multi-column grouping keys unsupported "
           "(raise AURON_HIP_MEM_BUDGET)");
    if (ma_mode_)
      FAIL("spill with multi-argument aggregates unsupported "
           "(raise AURON_HIP_MEM_BUDGET)");
    spill_table();  // frees the main region; caller re-checks free space
  }
}

void AggOp::grow(int64_t new_cap) {
  AggTable old = t_;
  GKeyTable oldg = g_;
  DevBuf oslots = std::move(d_slots_), os = std::move(d_special_),
         ong = std::move(d_ng_), oerr = std::move(d_err_),
         omm = std::move(d_mm_), ofrow = std::move(d_frow_),
         ofval = std::move(d_fval_), ofst = std::move(d_fst_),
         ogkoff = std::move(d_gkoff_);
  MaAcc oldma = ma_;
  DevBuf oma = std::move(d_ma_acc_), omam = std::move(d_ma_meta_),
         omas = std::move(d_ma_st_);
  init_table(new_cap);
  if (ma_mode_)
    launch_ma_rebuild(t_, ma_, old, oldma, ma_desc_.n, stream_);
  else if (gkey_)
    launch_gkey_rebuild(t_, g_, old, oldg, stream_);
  else
    launch_agg_rebuild(t_, old, stream_);
  AURON_HIP(hipStreamSynchronize(stream_));
}

// emit every group in the table, first-occurrence-ordered, in
// batch_size_-row output chunks
void AggOp::emit_table(std::vector<HostOutBatch>* out,
                       bool exclude_specials) {
  prepare_collect();  // one-shot per pool state (coll_sorted_ guard)
  prepare_ma_pools();
  DevBuf order, first;
  int64_t ng = table_order(&order, &first);
  DBG("agg.finish ng=%lld excl=%d", (long long)ng, (int)exclude_specials);
  if (ng == 0) return;
  DevBuf filtered;
  const uint32_t* order_ptr = order.get<uint32_t>();
  if (exclude_specials) {
    std::vector<uint32_t> h_order(ng);
    AURON_HIP(hipMemcpyAsync(h_order.data(), order.get(), ng * 4,
                             hipMemcpyDeviceToHost, stream_));
    AURON_HIP(hipStreamSynchronize(stream_));
    std::vector<uint32_t> keep;
    for (int64_t i = 0; i < ng; i++)
      if (h_order[i] < (uint32_t)t_.cap) keep.push_back(h_order[i]);
    ng = (int64_t)keep.size();
    if (ng == 0) return;
    filtered.alloc(ng * 4);
    AURON_HIP(hipMemcpyAsync(filtered.get(), keep.data(), ng * 4,
                             hipMemcpyHostToDevice, stream_));
    order_ptr = filtered.get<uint32_t>();
  }
  for (int64_t beg = 0; beg < ng; beg += batch_size_) {
    int64_t len = std::min(batch_size_, ng - beg);
    out->emplace_back(emit_groups(order_ptr + beg, len));
  }
}

// Variable-width (Binary) column of n rows from a pair of kernels:
// write_lens(int32_t* lens) sizes each row, write_bytes(const int32_t* offs,
// uint8_t* data) fills the rows at the scanned offsets. The data bytes are
// on the host after the caller's next sync.
template <class LensFn, class BytesFn>
HostOutCol AggOp::freeze_binary_col(int64_t n, LensFn write_lens,
                                    BytesFn write_bytes) {
  HostOutCol col;
  col.dt = DType::Binary;
  DevBuf lens(n * 4), offs((n + 1) * 4);
  write_lens(lens.get<int32_t>());
  col.offsets.alloc((size_t)(n + 1) * 4);
  lens_to_offsets_into(lens.get(), n, col.offsets.as<int32_t>(),
                       offs.get<int32_t>(), stream_);
  emit_.d2h_bytes += n * 4;
  size_t total = (size_t)col.offs()[n];
  DevBuf data(total ? total : 1);
  write_bytes(offs.get<int32_t>(), data.get<uint8_t>());
  emit_.d2h(&col.values, data.get(), total);
  emit_.keep(std::move(lens));
  emit_.keep(std::move(offs));
  emit_.keep(std::move(data));
  return col;
}

// the legacy table's a8 partial agg-buf column for the ordered groups
HostOutCol AggOp::freeze_agg_buf(const uint32_t* order_slots, int64_t n) {
  return freeze_binary_col(
      n,
      [&](int32_t* lens) {
        launch_agg_freeze_len(t_, order_slots, n, lens, layout_, stream_);
      },
      [&](const int32_t* offs, uint8_t* data) {
        launch_agg_freeze_write(t_, order_slots, n, offs, data, layout_,
                                stream_);
      });
}

// COLLECT list column for the ordered groups, read through an AggTable
// view `tv` of a sorted pool; item_dt Int32 narrows the 8-byte pool items
HostOutCol AggOp::coll_list_col(const AggTable& tv,
                                const uint32_t* order_slots, int64_t n,
                                DType item_dt) {
  HostOutCol col;
  col.dt = item_dt;
  col.is_list = true;
  DevBuf cnts(n * 4), d_off((n + 1) * 4);
  launch_coll_counts(tv, order_slots, n, cnts.get<int32_t>(), stream_);
  col.offsets.alloc((size_t)(n + 1) * 4);
  lens_to_offsets_into(cnts.get(), n, col.offsets.as<int32_t>(),
                       d_off.get<int32_t>(), stream_);
  emit_.d2h_bytes += n * 4;
  int64_t m = col.offs()[n];
  DevBuf items(m * 8 + 8);
  launch_coll_gather(tv, order_slots, n, d_off.get<int32_t>(),
                     items.get<unsigned long long>(), stream_);
  if (item_dt == DType::Int32) {
    DevBuf narrow(m * 4 + 4);
    launch_narrow_i64_i32(items.get<int64_t>(), m, narrow.get<int32_t>(),
                          stream_);
    emit_.d2h(&col.values, narrow.get(), (size_t)m * 4);
    emit_.keep(std::move(narrow));
  } else {
    emit_.d2h(&col.values, items.get(), (size_t)m * 8);
  }
  emit_.keep(std::move(cnts));
  emit_.keep(std::move(d_off));
  emit_.keep(std::move(items));
  return col;
}

DType AggOp::key_out_dt() const {
  return key_dt_ == DType::Unsupported ? DType::Int64 : key_dt_;
}

// Int32 keys sit widened in the i64 slots: narrow the gathered `keys` back
// to the declared type. The narrowed buffer replaces `keys`; the i64 one
// moves to `wide`, which the launch still reads until the caller syncs.
void AggOp::narrow_keys(DevBuf& keys, DevBuf& wide, int64_t n) {
  if (key_out_dt() != DType::Int32) return;
  wide = std::move(keys);
  keys.alloc(n * 4);
  launch_narrow_i64_i32(wide.get<int64_t>(), n, keys.get<int32_t>(),
                        stream_);
}

// decode the generalized-key grouping columns for the ordered groups
std::vector<HostOutCol> AggOp::emit_gkey_cols(const uint32_t* order_slots,
                                              int64_t n) {
  std::vector<HostOutCol> out;
  size_t bm = (n + 7) / 8;
  for (size_t k = 0; k < key_cols_.size(); k++) {
    HostOutCol c;
    DType dt = key_dts_[k];
    DevBuf bmbuf(bm);
    const int slot = emit_.null_slots(1);
    if (dt == DType::Utf8 || dt == DType::Binary) {
      c = freeze_binary_col(
          n,
          [&](int32_t* lens) {
            launch_gkey_out_lens(g_, order_slots, n, d_gkdts_.get<uint8_t>(),
                                 (int)key_cols_.size(), (int)k,
                                 (uint32_t*)lens, bmbuf.get<uint8_t>(),
                                 emit_.null_ctr(slot), stream_);
          },
          [&](const int32_t* offs, uint8_t* data) {
            launch_gkey_out_bytes(g_, order_slots, n,
                                  d_gkdts_.get<uint8_t>(),
                                  (int)key_cols_.size(), (int)k, offs, data,
                                  stream_);
          });
    } else {
      size_t w = dtype_width(dt);
      DevBuf vals(n * w);
      launch_gkey_out_fixed(g_, order_slots, n, d_gkdts_.get<uint8_t>(),
                            (int)key_cols_.size(), (int)k,
                            vals.get<uint8_t>(), bmbuf.get<uint8_t>(),
                            emit_.null_ctr(slot), stream_);
      emit_.d2h(&c.values, vals.get(), n * w);
      emit_.keep(std::move(vals));
    }
    c.dt = dt;
    emit_.col_validity(&c, bmbuf.get(), n, slot);
    emit_.keep(std::move(bmbuf));
    out.push_back(std::move(c));
  }
  return out;
}

// multi-arg emit: per-agg columns from the accumulator bank; partial mode
// freezes the per-agg wire instead (ma_freeze_*). Collect aggs read their
// sorted pool views through the legacy coll kernels (the AggTable's c_*
// pointers are temporarily re-aimed per pool).
void AggOp::emit_ma_aggs(const uint32_t* order_slots, int64_t n,
                         std::vector<HostOutCol>* cols) {
  size_t bm = (n + 7) / 8;
  if (!final_output_) {
    // partial: ONE Binary agg-buf column with the per-agg wire
    cols->push_back(freeze_binary_col(
        n,
        [&](int32_t* lens) {
          launch_ma_freeze_len(t_, ma_desc_, ma_, mp_, order_slots, n, lens,
                               stream_);
        },
        [&](const int32_t* offs, uint8_t* data) {
          launch_ma_freeze_write(t_, ma_desc_, ma_, mp_, order_slots, n,
                                 offs, data, stream_);
        }));
    return;
  }
  for (int j = 0; j < ma_desc_.n; j++) {
    const MaAgg& ag = ma_desc_.a[j];
    if (ag.kind == AGGL_CLIST || ag.kind == AGGL_CSET) {
      // re-aim the legacy collect view at this pool's sorted arrays
      AggTable tv = t_;
      uint8_t p = ag.pool;
      tv.c_key = mp_.key[p];
      tv.c_val = mp_.val[p];
      tv.c_n = d_mp_n_.get<unsigned long long>() + 2 * p;
      tv.c_cap = mp_counts_[p][0] + mp_counts_[p][1];
      cols->push_back(coll_list_col(tv, order_slots, n, ma_out_dt(j)));
      continue;
    }
    HostOutCol ac;
    int w = (ag.kind == AGGL_CNT) ? 8 : (ag.acc_t == 2 ? 4 : 8);
    DevBuf vals(n * w), bmbuf(bm);
    // COUNT is never null: its bitmap is built but not exported
    const int slot = (ag.kind != AGGL_CNT) ? emit_.null_slots(1) : -1;
    launch_ma_gather_out(ma_desc_, ma_, j, order_slots, n,
                         vals.get<uint8_t>(), bmbuf.get<uint8_t>(),
                         slot >= 0 ? emit_.null_ctr(slot) : nullptr, stream_);
    ac.dt = (ag.kind == AGGL_CNT) ? DType::Int64
            : (ag.kind == AGGL_AVG) ? DType::Float64
                                    : ma_out_dt(j);
    emit_.d2h(&ac.values, vals.get(), (size_t)n * w);
    if (slot >= 0) emit_.col_validity(&ac, bmbuf.get(), n, slot);
    emit_.keep(std::move(vals));
    emit_.keep(std::move(bmbuf));
    cols->push_back(std::move(ac));
  }
}

HostOutBatch AggOp::emit_groups(const uint32_t* order_slots, int64_t n) {
  DBG("agg.emit n=%lld final=%d", (long long)n, (int)final_output_);
  emit_.begin();
  std::vector<HostOutCol> cols;
  size_t bm = (n + 7) / 8;
  DevBuf keys(n * 8), kvalid(bm), sums(n * 8), svalid(bm), cnts(n * 8);
  DevBuf mins, mvalid, maxs, xvalid, avgs, wide, fvals[2], fvalid[2];
  if (has_mm_ && final_output_) {
    mins.alloc(n * 8);
    mvalid.alloc(bm);
    maxs.alloc(n * 8);
    xvalid.alloc(bm);
  }
  // gather_out's counters: {key, sum, min, max} nulls
  const int gslot = emit_.null_slots(4);
  launch_agg_gather_out(t_, order_slots, n, keys.get<int64_t>(),
                        kvalid.get<uint8_t>(), sums.get<double>(),
                        svalid.get<uint8_t>(), cnts.get<long long>(),
                        mins.get<double>(), mvalid.get<uint8_t>(),
                        maxs.get<double>(), xvalid.get<uint8_t>(),
                        emit_.null_ctr(gslot), stream_);
  HostOutCol key_col;
  key_col.dt = key_out_dt();
  if (!gkey_) {
    narrow_keys(keys, wide, n);
    emit_.d2h(&key_col.values, keys.get(), n * dtype_width(key_col.dt));
    emit_.col_validity(&key_col, kvalid.get(), n, gslot);
  }
  if (ma_mode_) {
    cols.push_back(std::move(key_col));
    emit_ma_aggs(order_slots, n, &cols);
  } else if (final_output_) {
    if (gkey_) {
      cols = emit_gkey_cols(order_slots, n);
    } else {
      cols.push_back(std::move(key_col));
    }
    const DType vdt = val_is_int_ ? DType::Int64 : DType::Float64;
    // each source goes down once, into the first column that shows it; a
    // later column over the same source is cloned from that one
    int sum_at = -1, cnt_at = -1, avg_at = -1, sv_at = -1, min_at = -1,
        max_at = -1, first_at[2] = {-1, -1}, coll_at = -1;
    auto values_once = [&](HostOutCol* ac, int* at, const DevBuf& src) {
      if (*at < 0) {
        emit_.d2h(&ac->values, src.get(), n * 8);
        *at = (int)cols.size();
      } else {
        ac->values_from = *at;
      }
    };
    auto validity_once = [&](HostOutCol* ac, int* at, const DevBuf& src,
                             int slot) {
      if (*at < 0) {
        emit_.col_validity(ac, src.get(), n, slot);
        *at = (int)cols.size();
      } else {
        ac->validity_from = *at;
      }
    };
    for (uint32_t k : agg_kinds_) {
      HostOutCol ac;
      if (k == AGGL_CNT) {
        ac.dt = DType::Int64;
        values_once(&ac, &cnt_at, cnts);
      } else if (k == AGGL_MIN) {
        ac.dt = vdt;
        int at = min_at;
        values_once(&ac, &min_at, mins);
        validity_once(&ac, &at, mvalid, gslot + 2);
      } else if (k == AGGL_MAX) {
        ac.dt = vdt;
        int at = max_at;
        values_once(&ac, &max_at, maxs);
        validity_once(&ac, &at, xvalid, gslot + 3);
      } else if (k == AGGL_FIRST || k == AGGL_FIRSTIN) {
        int w = (k == AGGL_FIRSTIN) ? 1 : 0;
        ac.dt = vdt;
        int at = first_at[w];
        int slot = -1;
        if (at < 0) {
          fvals[w].alloc(n * 8);
          fvalid[w].alloc(bm);
          slot = emit_.null_slots(1);
          launch_first_gather(t_, order_slots, n, w, fvals[w].get<double>(),
                              fvalid[w].get<uint8_t>(), emit_.null_ctr(slot),
                              stream_);
        }
        values_once(&ac, &first_at[w], fvals[w]);
        validity_once(&ac, &at, fvalid[w], slot);
      } else if (k == AGGL_CLIST || k == AGGL_CSET) {
        // the one legacy pool serves every collect agg
        if (coll_at < 0) {
          ac = coll_list_col(t_, order_slots, n, vdt);
          coll_at = (int)cols.size();
        } else {
          ac.dt = vdt;
          ac.is_list = true;
          ac.values_from = coll_at;
        }
      } else if (k == AGGL_AVG) {
        ac.dt = DType::Float64;
        if (avg_at < 0) {
          avgs.alloc(n * 8);
          launch_avg_div(sums.get<double>(), cnts.get<long long>(), n,
                         avgs.get<double>(), stream_);
        }
        values_once(&ac, &avg_at, avgs);
        validity_once(&ac, &sv_at, svalid, gslot + 1);
      } else {
        ac.dt = vdt;  // SUM output carries the accumulator type's raw bits
        values_once(&ac, &sum_at, sums);
        // null iff cnt==0 (shared column)
        validity_once(&ac, &sv_at, svalid, gslot + 1);
      }
      cols.push_back(std::move(ac));
    }
  } else {
    HostOutCol buf_col = freeze_agg_buf(order_slots, n);  // a8
    if (gkey_) {
      cols = emit_gkey_cols(order_slots, n);
    } else {
      cols.push_back(std::move(key_col));
    }
    cols.push_back(std::move(buf_col));
  }
  emit_.end(&cols);
  DBG("agg.emit d2h done");
  return {n, std::move(cols)};
}

HostOutBatch AggOp::emit_skipped(const DevBatch& b) {
  int64_t n = b.num_rows;
  const DevColumn& key = b.cols.at(key_col_);
  const DevColumn& val = b.cols.at(val_col_);
  emit_.begin();
  HostOutCol buf_col = freeze_binary_col(
      n,
      [&](int32_t* lens) {
        launch_skip_freeze_len(val.validity, n, lens, layout_, stream_);
      },
      [&](const int32_t* offs, uint8_t* data) {
        launch_skip_freeze_write((const double*)val.values, val.validity, n,
                                 offs, data, layout_, val_is_int_ ? 1 : 0,
                                 stream_);
      });
  HostOutCol key_col;
  key_col.dt = key.dt;
  emit_.d2h(&key_col.values, key.values, n * dtype_width(key.dt));
  // pass-through of the input's bitmap: counted, not rebuilt
  if (key.validity) {
    const int slot = emit_.null_slots(1);
    launch_bitmap_null_count(key.validity, n, emit_.null_ctr(slot), stream_);
    emit_.col_validity(&key_col, key.validity, n, slot);
  }
  std::vector<HostOutCol> cols;
  cols.push_back(std::move(key_col));
  cols.push_back(std::move(buf_col));
  emit_.end(&cols);
  return {n, std::move(cols)};
}

}  // namespace auron
