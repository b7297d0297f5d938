// engine.cpp — the MI355X-native Auron hot-path runtime behind the C ABI of
// include/auron_hip.h. Mirrors the reference runtime semantics:
//   NativeExecutionRuntime (auron/src/rt.rs:71-259): decode TaskDefinition →
//   operator tree → pull-model batch pump → Arrow FFI export per nextBatch.
// Operators implemented (the SURVEY.md §8 hot-path subset):
//   FFIReaderExec   (ffi_reader_exec.rs)        — input via callback
//   AggExec         (agg_exec.rs:141-278, agg_table.rs, agg_ctx.rs) — GPU
//   ShuffleWriterExec (shuffle_writer_exec.rs, sort_repartitioner.rs,
//                      buffered_data.rs) — GPU partition + host file emit
//   FilterExec / ProjectExec (filter_exec.rs, project_exec.rs) — GPU
// This file holds the Arrow import/export, the operators and the Runtime that
// drives the operator chain. The batch sources (ParquetScanExec,
// IpcReaderExec) are in sources.cpp, the types and helpers they share with
// this file in batch.h, the host-only auron_debug_* entry points in
// debug_abi.cpp.
// The GPU path is mandatory: any HIP failure aborts the task loudly; there is
// no CPU fallback anywhere in this library.
#include <chrono>
#include <tuple>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "batch.h"
#include "expr.h"
#include "kernels.h"
#include "kernels_expr.h"
#include "ipc_scalar.h"
#include "serde_host.h"

namespace auron {
namespace {

const char* dtype_format(DType t) {
  switch (t) {
    case DType::Int8: return "c";
    case DType::Int16: return "s";
    case DType::Int32: return "i";
    case DType::Int64: return "l";
    case DType::UInt8: return "C";
    case DType::UInt16: return "S";
    case DType::UInt32: return "I";
    case DType::UInt64: return "L";
    case DType::Float32: return "f";
    case DType::Float64: return "g";
    case DType::Utf8: return "u";
    case DType::Binary: return "z";
    default: return nullptr;
  }
}

DType format_dtype(const char* f) {
  if (!f || !f[0] || f[1]) return DType::Unsupported;
  switch (f[0]) {
    case 'c': return DType::Int8;
    case 's': return DType::Int16;
    case 'i': return DType::Int32;
    case 'l': return DType::Int64;
    case 'C': return DType::UInt8;
    case 'S': return DType::UInt16;
    case 'I': return DType::UInt32;
    case 'L': return DType::UInt64;
    case 'f': return DType::Float32;
    case 'g': return DType::Float64;
    case 'u': return DType::Utf8;
    case 'z': return DType::Binary;
    default: return DType::Unsupported;
  }
}

// ------------------------------------------------------------ arrow import --
DevColumn import_child(const ArrowArray* a, DType dt, bool device,
                       hipStream_t stream) {
  if (a->offset != 0) FAIL("ArrowArray with nonzero offset unsupported");
  const bool binary = dt == DType::Binary || dt == DType::Utf8;
  const size_t w = dtype_width(dt);
  if (binary && a->n_buffers < 3) FAIL("binary array needs 3 buffers");
  if (!binary && w == 0) FAIL("unsupported input dtype");
  const uint8_t* validity_src = a->n_buffers > 0 && a->null_count != 0
                                    ? (const uint8_t*)a->buffers[0]
                                    : nullptr;
  const int32_t* off_src = binary ? (const int32_t*)a->buffers[1] : nullptr;
  const void* val_src = binary             ? a->buffers[2]
                        : a->n_buffers > 1 ? a->buffers[1]
                                           : nullptr;
  if (!device)
    return upload_column(dt, a->length, val_src,
                         binary ? (size_t)off_src[a->length]
                                : (size_t)a->length * w,
                         off_src, validity_src, (a->length + 7) / 8, stream);
  // device-resident input: borrow the caller's buffers
  DevColumn c;
  c.dt = dt;
  c.len = a->length;
  c.values = val_src;
  c.validity = validity_src;
  if (binary) {
    c.offsets = off_src;
    int32_t dl = 0;
    AURON_HIP(hipMemcpyAsync(&dl, off_src + a->length, 4, hipMemcpyDeviceToHost,
                             stream));
    AURON_HIP(hipStreamSynchronize(stream));
    c.data_len = dl;
  }
  return c;
}

// Import a top-level struct batch (rt.rs:232-241 exports batches as
// StructArray). `schema_hint` gives dtypes when the caller passed no schema.
DevBatch import_batch(const ArrowArray* a, const ArrowSchema* schema,
                      const Schema& schema_hint, bool device,
                      hipStream_t stream) {
  DevBatch b;
  b.num_rows = a->length;
  for (int64_t i = 0; i < a->n_children; i++) {
    DType dt;
    if (schema && schema->n_children == a->n_children) {
      dt = format_dtype(schema->children[i]->format);
    } else if ((size_t)i < schema_hint.fields.size()) {
      dt = schema_hint.fields[i].dtype;
    } else {
      FAIL("cannot determine input column dtype");
    }
    b.cols.push_back(import_child(a->children[i], dt, device, stream));
  }
  if (!device) {
    // host buffers may be freed by the caller after return — drain the H2D
    // copies before handing the borrowed pointers back
    AURON_HIP(hipStreamSynchronize(stream));
  }
  return b;
}

// ------------------------------------------------------------ arrow export --
struct ExportPriv {
  // pool-backed host buffers taken over from the HostOutCols: (ptr, capacity)
  std::vector<std::pair<void*, size_t>> host_bufs;
  std::vector<const void*> buffer_ptrs;
  std::vector<ArrowArray> children_store;
  std::vector<ArrowArray*> children_ptrs;
  std::vector<std::vector<const void*>> child_buffer_ptrs;
  // list columns: one item array per column slot
  std::vector<ArrowArray> item_store;
  std::vector<ArrowArray*> item_ptrs;
  std::vector<std::vector<const void*>> item_buffer_ptrs;
};

void release_exported_array(ArrowArray* a) {
  if (!a || !a->release) return;
  ExportPriv* p = (ExportPriv*)a->private_data;
  for (auto& b : p->host_bufs) HostBuf::give_back(b.first, b.second);
  delete p;
  a->release = nullptr;
}

struct SchemaPriv {
  std::vector<ArrowSchema> children_store;
  std::vector<ArrowSchema*> children_ptrs;
  std::vector<std::string> names;
  std::vector<const char*> formats;
  // list fields: one item-schema per field slot (null when not a list)
  std::vector<ArrowSchema> item_store;
  std::vector<ArrowSchema*> item_ptrs;
};

void release_exported_schema(ArrowSchema* s) {
  if (!s || !s->release) return;
  delete (SchemaPriv*)s->private_data;
  s->release = nullptr;
}

struct OutField {
  std::string name;
  DType dt;        // list fields: the ITEM type
  bool nullable;
  bool is_list = false;  // Arrow list<dt> (COLLECT output)
};

void export_schema(const std::vector<OutField>& fields, ArrowSchema* out) {
  auto* priv = new SchemaPriv;
  priv->children_store.resize(fields.size());
  priv->item_store.resize(fields.size());
  priv->item_ptrs.resize(fields.size());
  for (size_t i = 0; i < fields.size(); i++) {
    priv->names.push_back(fields[i].name);
  }
  for (size_t i = 0; i < fields.size(); i++) {
    ArrowSchema& c = priv->children_store[i];
    memset(&c, 0, sizeof(c));
    c.name = priv->names[i].c_str();
    c.flags = fields[i].nullable ? ARROW_FLAG_NULLABLE : 0;
    c.release = [](ArrowSchema* s) { s->release = nullptr; };
    if (fields[i].is_list) {
      c.format = "+l";
      ArrowSchema& it = priv->item_store[i];
      memset(&it, 0, sizeof(it));
      it.format = dtype_format(fields[i].dt);
      it.name = "item";
      it.release = [](ArrowSchema* s) { s->release = nullptr; };
      priv->item_ptrs[i] = &it;
      c.n_children = 1;
      c.children = &priv->item_ptrs[i];
    } else {
      c.format = dtype_format(fields[i].dt);
    }
    priv->children_ptrs.push_back(&c);
  }
  memset(out, 0, sizeof(*out));
  out->format = "+s";
  out->name = "";
  out->n_children = (int64_t)fields.size();
  out->children = priv->children_ptrs.data();
  out->release = release_exported_schema;
  out->private_data = priv;
}

// host-side column staging for export
struct HostOutCol {
  DType dt;            // list cols: the ITEM type
  HostBuf values;      // list cols: child (item) values
  HostBuf validity;    // empty = no nulls
  HostBuf offsets;     // binary / list: (n+1) int32
  int64_t null_count = 0;  // exact; validity is attached only when > 0
  bool is_list = false;
  // emit bookkeeping, resolved at the batch's one sync (AggOp::emit_end):
  // the device null counter that belongs to `validity`, and the column of
  // the same batch whose values(+offsets) / validity this one duplicates
  int null_slot = -1;
  int values_from = -1, validity_from = -1;

  const int32_t* offs() const { return offsets.as<int32_t>(); }
};

// device-resident column staging: partial-agg output that stays in HBM and
// is exported through import_device_batch (buffers owned by the runtime,
// valid until auron_finalize — the documented contract for this harness).
struct DevOutCol {
  DType dt;
  DevBuf values;    // prim values / binary data bytes
  DevBuf offsets;   // binary only: (n+1) int32
  DevBuf validity;  // LSB bitmap or empty
  int64_t data_len = 0;
};


void export_batch(int64_t num_rows, std::vector<HostOutCol>&& cols,
                  ArrowArray* out) {
  auto* priv = new ExportPriv;
  priv->children_store.resize(cols.size());
  priv->child_buffer_ptrs.resize(cols.size());
  priv->item_store.resize(cols.size());
  priv->item_ptrs.resize(cols.size());
  priv->item_buffer_ptrs.resize(cols.size());
  for (size_t i = 0; i < cols.size(); i++) {
    HostOutCol& c = cols[i];
    ArrowArray& ch = priv->children_store[i];
    memset(&ch, 0, sizeof(ch));
    ch.length = num_rows;
    ch.offset = 0;
    // the export takes the buffers over; release_exported_array returns
    // them to the pool
    auto take = [&](HostBuf& hb) -> const void* {
      if (hb.empty()) hb.alloc(0);  // Arrow data buffers are never null
      size_t cap = 0;
      void* b = hb.release(&cap);
      priv->host_bufs.push_back({b, cap});
      return b;
    };
    std::vector<const void*>& bufs = priv->child_buffer_ptrs[i];
    const void* validity = nullptr;
    if (!c.validity.empty() && c.null_count > 0) validity = take(c.validity);
    ch.null_count = validity ? c.null_count : 0;
    if (c.is_list) {
      // list<prim>: parent {validity, offsets}; child = item values
      ArrowArray& it = priv->item_store[i];
      memset(&it, 0, sizeof(it));
      it.length = c.offsets.empty() ? 0 : c.offs()[num_rows];
      it.null_count = 0;
      bufs = {validity, take(c.offsets)};
      std::vector<const void*>& ibufs = priv->item_buffer_ptrs[i];
      ibufs = {nullptr, take(c.values)};
      it.n_buffers = 2;
      it.buffers = ibufs.data();
      it.release = [](ArrowArray* a) { a->release = nullptr; };
      priv->item_ptrs[i] = &it;
      ch.n_children = 1;
      ch.children = &priv->item_ptrs[i];
    } else if (c.dt == DType::Binary || c.dt == DType::Utf8) {
      const void* offs = take(c.offsets);
      bufs = {validity, offs, take(c.values)};
    } else {
      bufs = {validity, take(c.values)};
    }
    ch.n_buffers = (int64_t)bufs.size();
    ch.buffers = bufs.data();
    ch.release = [](ArrowArray* a) { a->release = nullptr; };
    priv->children_ptrs.push_back(&ch);
  }
  memset(out, 0, sizeof(*out));
  out->length = num_rows;
  out->null_count = 0;
  out->n_buffers = 1;
  priv->buffer_ptrs = {nullptr};
  out->buffers = priv->buffer_ptrs.data();
  out->n_children = (int64_t)cols.size();
  out->children = priv->children_ptrs.data();
  out->release = release_exported_array;
  out->private_data = priv;
}

// Variable-width output layout: device lens[n] (int32) -> host exclusive scan
// -> the n+1 offsets in the caller's offs[], uploaded to d_offs (the caller
// keeps offs alive until its next sync: it is the source of the upload).
// Arrow offsets are int32, so a total past INT32_MAX fails instead of
// wrapping.
void lens_to_offsets_into(const void* d_lens, int64_t n, int32_t* offs,
                          int32_t* d_offs, hipStream_t stream) {
  offs[0] = 0;
  AURON_HIP(hipMemcpyAsync(offs + 1, d_lens, n * 4, hipMemcpyDeviceToHost,
                           stream));
  AURON_HIP(hipStreamSynchronize(stream));
  int64_t total = 0;
  for (int64_t i = 0; i < n; i++) {
    total += offs[i + 1];
    if (total > INT32_MAX)
      FAIL("variable-width output exceeds 2 GiB in one batch (int32 offsets)");
    offs[i + 1] = (int32_t)total;
  }
  AURON_HIP(hipMemcpyAsync(d_offs, offs, (n + 1) * 4, hipMemcpyHostToDevice,
                           stream));
}

std::vector<int32_t> lens_to_offsets(const void* d_lens, int64_t n,
                                     int32_t* d_offs, hipStream_t stream) {
  std::vector<int32_t> offs(n + 1, 0);
  lens_to_offsets_into(d_lens, n, offs.data(), d_offs, stream);
  return offs;
}

// ------------------------------------------------------------------ AggOp --
// GPU AggExec (agg_exec.rs:141-278 semantics), HashAgg in one of four modes:
//   legacy shared-argument table — one numeric key, all aggs over one column;
//   multi-argument bank (ma_mode_) — per-agg argument columns and pools;
//   generalized keys (gkey_) — Utf8 / multi-column grouping tuples;
//   two-phase fast path — partition-then-merge for large numeric-key chunks.
class AggOp {
 public:
  AggOp(const AggNode& node, const Conf& conf, hipStream_t stream)
      : stream_(stream) {
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

  ~AggOp() {
    for (auto& [e0, e1] : ev_pairs_) {
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
    }
    (void)hipEventDestroy(ev_start_);
    (void)hipEventDestroy(ev_stop_);
  }

  void consume(DevBatch&& b) {
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
        // HIP-event timing on the launch stream (roofline evidence for the
        // dominant kernel; pairs are drained once at finish() so the hot
        // loop never synchronizes for timing)
        hipEvent_t e0, e1;
        AURON_HIP(hipEventCreate(&e0));
        AURON_HIP(hipEventCreate(&e1));
        AURON_HIP(hipEventRecord(e0, stream_));
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
        AURON_HIP(hipEventRecord(e1, stream_));
        ev_pairs_.push_back({e0, e1});
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
  bool maybe_enter_skipping(const DevBatch& b, int64_t done) {
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

  std::vector<OutField> key_fields() const {
    std::vector<OutField> f;
    for (size_t k = 0; k < key_cols_.size(); k++) {
      DType kd = k < key_dts_.size() ? key_dts_[k] : key_out_dt();
      f.push_back({key_names_[k], kd, true});
    }
    return f;
  }

  DType ma_out_dt(size_t i) const {  // per-agg declared type (ma mode)
    switch (ma_desc_.a[i].acc_t) {
      case 1: return DType::Int64;
      case 2: return DType::Int32;
      default: return DType::Float64;
    }
  }

  std::vector<OutField> output_fields() const {
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
  std::pair<int64_t, int64_t> sort_collect_pool(
      const long long* key, const unsigned long long* prio,
      const unsigned long long* val, int64_t cap, int64_t n0, int64_t n1,
      bool dedup, DevBuf& skey, DevBuf& sval) {
    using u64 = unsigned long long;
    if (!pinned_meta_.get()) pinned_meta_.alloc(16);
    int64_t nmax = std::max<int64_t>(std::max(n0, n1), 1);
    size_t tb0 = 0;
    sort_pairs_u64_u32(nullptr, nullptr, nullptr, nullptr, nmax, nullptr,
                       &tb0, stream_);
    DevBuf tmp(tb0), idx(nmax * 4), idxo(nmax * 4), scr(nmax * 8);
    skey.alloc(std::max<int64_t>(n0 + n1, 1) * 8);
    sval.alloc(std::max<int64_t>(n0 + n1, 1) * 8);

    // one stable radix pass over `by`, gathering key/prio/val (null = not
    // carried) into the given destinations
    auto sort_pass = [&](const u64* by, int64_t n, const u64* k, const u64* p,
                         const u64* v, u64* k_out, u64* p_out, u64* v_out) {
      launch_iota_u32(idx.get<uint32_t>(), n, stream_);
      size_t tb = tmp.size();
      sort_pairs_u64_u32(by, idx.get<uint32_t>(), scr.get<u64>(),
                         idxo.get<uint32_t>(), n, tmp.get(), &tb, stream_);
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
        size_t stb = 0;
        scan_mask_u8(mark.get<uint8_t>(), pos.get<uint32_t>(), n, nullptr,
                     &stb, stream_);
        DevBuf stmp(stb);
        scan_mask_u8(mark.get<uint8_t>(), pos.get<uint32_t>(), n, stmp.get(),
                     &stb, stream_);
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
  void upload_pool_counts(unsigned long long* d_n, int64_t n0, int64_t n1) {
    unsigned long long* h = pinned_meta_.get<unsigned long long>();
    h[0] = (unsigned long long)n0;
    h[1] = (unsigned long long)n1;
    AURON_HIP(hipMemcpyAsync(d_n, h, 16, hipMemcpyHostToDevice, stream_));
    AURON_HIP(hipStreamSynchronize(stream_));
  }

  // Sort the legacy COLLECT pool (sort_collect_pool) and point the table's
  // c_key/c_val views at the sorted arrays. One-shot before any emit.
  void prepare_collect() {
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
  void prepare_ma_pools() {
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

  // drain: produce all output batches (host-staged)
  std::vector<std::pair<int64_t, std::vector<HostOutCol>>> finish() {
    std::vector<std::pair<int64_t, std::vector<HostOutCol>>> out;
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

  // device-resident variant of finish(): partial (key + a8 Binary) batches
  // stay in HBM. Spill / partial-skipping fall outside this mode (the bench
  // and exchange paths that use it never enter them) and FAIL loudly.
  std::vector<std::pair<int64_t, std::vector<DevOutCol>>> finish_dev() {
    std::vector<std::pair<int64_t, std::vector<DevOutCol>>> out;
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

  std::pair<int64_t, std::vector<DevOutCol>> emit_groups_dev(
      const uint32_t* order_slots, int64_t n) {
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
    size_t tb = 0;
    scan_counts_matrix(lens.get<uint32_t>(), bc.offsets.get<uint32_t>(),
                       n + 1, nullptr, &tb, stream_);
    DevBuf scan_tmp(tb);
    scan_counts_matrix(lens.get<uint32_t>(), bc.offsets.get<uint32_t>(),
                       n + 1, scan_tmp.get(), &tb, stream_);
    if (pinned_meta_.size() < 16) pinned_meta_.alloc(16);
    AURON_HIP(hipMemcpyAsync(pinned_meta_.get(),
                             bc.offsets.get<uint32_t>() + n, 4,
                             hipMemcpyDeviceToHost, stream_));
    AURON_HIP(hipStreamSynchronize(stream_));
    bc.data_len = (int64_t)*pinned_meta_.get<uint32_t>();
    bc.values.alloc(bc.data_len ? bc.data_len : 1);
    launch_agg_freeze_write(t_, order_slots, n, bc.offsets.get<int32_t>(),
                            bc.values.get<uint8_t>(), layout_, stream_);
    return {n, std::move(cols)};
  }

  uint64_t num_groups_host() {
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

  int64_t batch_size() const { return batch_size_; }

 private:
  void init_table(int64_t slots) {
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

  static constexpr int64_t AGG2_MIN_CHUNK = 4 << 20;   // below: single-phase
  // partition-buffer rows per two-phase chunk: bigger chunks amortize launch
  // tails and per-chunk syncs (24 B/row + 24 B/row leftover scratch; 256M
  // rows = 12 GB of the 288 GB HBM). Runtime-tunable for A/B sweeps.
  int64_t agg2_chunk_max_ = 256 << 20;
  static constexpr int AGG3_NBUCK_LOG2 = 9;   // 512 buckets
  static constexpr int AGG3_NBUCK = 1 << AGG3_NBUCK_LOG2;
  static constexpr int AGG3_GRID_LOG2 = 8;    // hist/scatter grid: 256 blocks
                                              // x 1024 threads
  // staged-group capacity: every bucket's full 4096-slot LDS window
  static constexpr int64_t AGG3_STAGED_CAP = (int64_t)AGG3_NBUCK * 4096;

  // ---- multi-argument chunk (kernels_maarg.hip) --------------------------
  void ma_chunk(const DevBatch& b, int64_t done, int64_t chunk) {
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
    hipEvent_t e0, e1;
    AURON_HIP(hipEventCreate(&e0));
    AURON_HIP(hipEventCreate(&e1));
    AURON_HIP(hipEventRecord(e0, stream_));
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
    AURON_HIP(hipEventRecord(e1, stream_));
    ev_pairs_.push_back({e0, e1});
  }

  // ---- generalized-key machinery (kernels_gkey.hip) ----------------------
  void init_gkey() {
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

  void gk_ensure_pool(int64_t need_more) {
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

  GKeyCols gk_cols(const DevBatch& b, int64_t done) const {
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
  void gkey_chunk(const DevBatch& b, int64_t done, int64_t chunk) {
    GKeyCols gc = gk_cols(b, done);
    if (d_enclens_.size() < (size_t)(chunk + 1) * 4) {
      d_enclens_.alloc((chunk + 1) * 4);
      d_encoffs_.alloc((chunk + 1) * 4);
      d_gkslots_.alloc(chunk * 4);
    }
    launch_gkey_enc_lens(gc, chunk, d_enclens_.get<uint32_t>(), stream_);
    size_t tb = 0;
    scan_counts_matrix(d_enclens_.get<uint32_t>(), d_encoffs_.get<uint32_t>(),
                       chunk + 1, nullptr, &tb, stream_);
    if (d_gkscan_tmp_.size() < tb) d_gkscan_tmp_.alloc(tb);
    scan_counts_matrix(d_enclens_.get<uint32_t>(), d_encoffs_.get<uint32_t>(),
                       chunk + 1, d_gkscan_tmp_.get(), &tb, stream_);
    if (pinned_meta_.size() < 16) pinned_meta_.alloc(16);
    AURON_HIP(hipMemcpyAsync(pinned_meta_.get(),
                             d_encoffs_.get<uint32_t>() + chunk, 4,
                             hipMemcpyDeviceToHost, stream_));
    AURON_HIP(hipStreamSynchronize(stream_));
    int64_t total = (int64_t)*pinned_meta_.get<uint32_t>();
    if (d_encbytes_.size() < (size_t)total + 8)
      d_encbytes_.alloc(total + 8);
    launch_gkey_enc_write(gc, d_encoffs_.get<uint32_t>(),
                          d_encbytes_.get<uint8_t>(), chunk, stream_);
    gk_ensure_pool(total + 4 * chunk);  // worst case: every row a new group
    hipEvent_t e0, e1;
    AURON_HIP(hipEventCreate(&e0));
    AURON_HIP(hipEventCreate(&e1));
    AURON_HIP(hipEventRecord(e0, stream_));
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
    AURON_HIP(hipEventRecord(e1, stream_));
    ev_pairs_.push_back({e0, e1});
    gk_used_bound_ += total + 4 * chunk;
  }

  // Read the two-phase tuning knobs once, BEFORE the first chunk size is
  // computed (the scratch buffers are sized from agg2_chunk_max_, so the
  // bound must be final by then).
  void init_agg2_conf() {
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
  void merge_counted(int64_t n, Launch launch) {
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
  void two_phase_chunk(const DevBatch& b, int64_t done, int64_t chunk) {
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
    hipEvent_t e0, e1;
    AURON_HIP(hipEventCreate(&e0));
    AURON_HIP(hipEventCreate(&e1));
    AURON_HIP(hipEventRecord(e0, stream_));
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
    AURON_HIP(hipEventRecord(e1, stream_));
    ev_pairs_.push_back({e0, e1});
    update_rows_ += chunk;
    DBG("agg.2phase chunk=%lld staged=%lld leftover=%lld special=%u",
        (long long)chunk, (long long)staged_n, (long long)lo_n, special_rows);
  }

  static uint64_t host_mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
  }

  struct SpillBucket {
    std::vector<int64_t> keys;
    std::vector<unsigned long long> first_rows;
    std::vector<int32_t> lens;
    std::vector<uint8_t> data;
  };

  // compact the table and return (order_slots sorted by first_row, ng);
  // device buffers owned by the out-params
  int64_t table_order(DevBuf* slots_sorted, DevBuf* first_sorted) {
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
    size_t tmp_bytes = 0;
    sort_pairs_u64_u32(first.get<unsigned long long>(), slots_u.get<uint32_t>(),
                       first_sorted->get<unsigned long long>(),
                       slots_sorted->get<uint32_t>(), (int64_t)ng, nullptr,
                       &tmp_bytes, stream_, end_bit);
    DevBuf tmp(tmp_bytes);
    sort_pairs_u64_u32(first.get<unsigned long long>(), slots_u.get<uint32_t>(),
                       first_sorted->get<unsigned long long>(),
                       slots_sorted->get<uint32_t>(), (int64_t)ng, tmp.get(),
                       &tmp_bytes, stream_, end_bit);
    // pooled buffers (slots_u/first/tmp) must not be recycled while the sort
    // still reads them — the pool, unlike hipFree, does not synchronize
    AURON_HIP(hipStreamSynchronize(stream_));
    return (int64_t)ng;
  }

  // freeze the main-region groups to host spill buckets and reset the main
  // region (the two special groups stay resident across spills)
  void spill_table() {
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
      emit_sync();  // h_keys and the frozen bytes are on the host
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
  void reset_collect_pool() {
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

  void reset_main() {
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

  void refresh_ng() {
    ng_true_ = num_groups_host();
    ng_bound_ = ng_true_;
  }

  void drain_timing() {
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

  void ensure_capacity(int64_t need) {
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

  void grow(int64_t new_cap) {
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
  void emit_table(std::vector<std::pair<int64_t, std::vector<HostOutCol>>>* out,
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

  // ---- host emit -----------------------------------------------------------
  // One output batch = emit_begin(), any number of d2h() / col_validity()
  // enqueues straight into the columns' own export buffers, emit_end(): the
  // batch's ONE stream sync, after which the device null counters decide
  // which bitmaps stay attached. emit_d2h_bytes_ counts the column payload
  // (values, bitmaps, offsets) copied down; the 4-byte counters are not
  // payload.
  static constexpr int EMIT_NULL_SLOTS = 256;

  void emit_begin() {
    if (!d_emit_nulls_) {
      d_emit_nulls_.alloc(EMIT_NULL_SLOTS * 4);
      pinned_nulls_.alloc(EMIT_NULL_SLOTS * 4);
    }
    AURON_HIP(hipMemsetAsync(d_emit_nulls_.get(), 0, EMIT_NULL_SLOTS * 4,
                             stream_));
    emit_null_used_ = 0;
  }

  // reserve k consecutive device null counters; returns the first index
  int null_slots(int k) {
    if (emit_null_used_ + k > EMIT_NULL_SLOTS)
      FAIL("too many nullable output columns in one batch");
    int at = emit_null_used_;
    emit_null_used_ += k;
    return at;
  }
  uint32_t* null_ctr(int slot) {
    return d_emit_nulls_.get<uint32_t>() + slot;
  }

  // enqueue dev -> a fresh export buffer (no sync)
  void d2h(HostBuf* dst, const void* dev, size_t len) {
    dst->alloc(len);
    if (len == 0) return;
    AURON_HIP(hipMemcpyAsync(dst->data(), dev, len, hipMemcpyDeviceToHost,
                             stream_));
    emit_d2h_bytes_ += (int64_t)len;
  }

  // bitmap of n rows whose nulls a kernel adds to counter `slot`
  void col_validity(HostOutCol* col, const void* dev_bm, int64_t n, int slot) {
    d2h(&col->validity, dev_bm, (size_t)(n + 7) / 8);
    col->null_slot = slot;
  }

  // D2H sources live until the batch's sync: the device pool hands a freed
  // buffer to whoever asks next and does not synchronize
  void keep(DevBuf&& b) { emit_keep_.push_back(std::move(b)); }

  void emit_sync() {
    AURON_HIP(hipStreamSynchronize(stream_));
    emit_keep_.clear();
  }

  // The one sync of an output batch. Keeps the rule of the Arrow null_count
  // convention (and batch_serde's has_null header): validity is attached only
  // when nulls exist. Columns that duplicate another column's source are
  // cloned here, the only host copy of the emit path.
  void emit_end(std::vector<HostOutCol>* cols) {
    uint32_t* h_nulls = pinned_nulls_.get<uint32_t>();
    if (emit_null_used_)
      AURON_HIP(hipMemcpyAsync(h_nulls, d_emit_nulls_.get(),
                               (size_t)emit_null_used_ * 4,
                               hipMemcpyDeviceToHost, stream_));
    emit_sync();
    for (HostOutCol& c : *cols) {
      if (c.null_slot < 0) continue;
      c.null_count = (int64_t)h_nulls[c.null_slot];
      if (c.null_count == 0) c.validity.free();
      c.null_slot = -1;
    }
    for (HostOutCol& c : *cols) {
      if (c.values_from >= 0) {
        const HostOutCol& src = (*cols)[c.values_from];
        c.values = src.values.clone(&emit_host_copy_bytes_);
        c.offsets = src.offsets.clone(&emit_host_copy_bytes_);
        c.values_from = -1;
      }
      if (c.validity_from >= 0) {
        const HostOutCol& src = (*cols)[c.validity_from];
        c.validity = src.validity.clone(&emit_host_copy_bytes_);
        c.null_count = src.null_count;
        c.validity_from = -1;
      }
    }
  }

  // Variable-width (Binary) column of n rows from a pair of kernels:
  // write_lens(int32_t* lens) sizes each row, write_bytes(const int32_t* offs,
  // uint8_t* data) fills the rows at the scanned offsets. The data bytes are
  // on the host after the caller's next sync.
  template <class LensFn, class BytesFn>
  HostOutCol freeze_binary_col(int64_t n, LensFn write_lens,
                               BytesFn write_bytes) {
    HostOutCol col;
    col.dt = DType::Binary;
    DevBuf lens(n * 4), offs((n + 1) * 4);
    write_lens(lens.get<int32_t>());
    col.offsets.alloc((size_t)(n + 1) * 4);
    lens_to_offsets_into(lens.get(), n, col.offsets.as<int32_t>(),
                         offs.get<int32_t>(), stream_);
    emit_d2h_bytes_ += n * 4;
    size_t total = (size_t)col.offs()[n];
    DevBuf data(total ? total : 1);
    write_bytes(offs.get<int32_t>(), data.get<uint8_t>());
    d2h(&col.values, data.get(), total);
    keep(std::move(lens));
    keep(std::move(offs));
    keep(std::move(data));
    return col;
  }

  // the legacy table's a8 partial agg-buf column for the ordered groups
  HostOutCol freeze_agg_buf(const uint32_t* order_slots, int64_t n) {
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
  HostOutCol coll_list_col(const AggTable& tv, const uint32_t* order_slots,
                           int64_t n, DType item_dt) {
    HostOutCol col;
    col.dt = item_dt;
    col.is_list = true;
    DevBuf cnts(n * 4), d_off((n + 1) * 4);
    launch_coll_counts(tv, order_slots, n, cnts.get<int32_t>(), stream_);
    col.offsets.alloc((size_t)(n + 1) * 4);
    lens_to_offsets_into(cnts.get(), n, col.offsets.as<int32_t>(),
                         d_off.get<int32_t>(), stream_);
    emit_d2h_bytes_ += n * 4;
    int64_t m = col.offs()[n];
    DevBuf items(m * 8 + 8);
    launch_coll_gather(tv, order_slots, n, d_off.get<int32_t>(),
                       items.get<unsigned long long>(), stream_);
    if (item_dt == DType::Int32) {
      DevBuf narrow(m * 4 + 4);
      launch_narrow_i64_i32(items.get<int64_t>(), m, narrow.get<int32_t>(),
                            stream_);
      d2h(&col.values, narrow.get(), (size_t)m * 4);
      keep(std::move(narrow));
    } else {
      d2h(&col.values, items.get(), (size_t)m * 8);
    }
    keep(std::move(cnts));
    keep(std::move(d_off));
    keep(std::move(items));
    return col;
  }

  DType key_out_dt() const {
    return key_dt_ == DType::Unsupported ? DType::Int64 : key_dt_;
  }

  // Int32 keys sit widened in the i64 slots: narrow the gathered `keys` back
  // to the declared type. The narrowed buffer replaces `keys`; the i64 one
  // moves to `wide`, which the launch still reads until the caller syncs.
  void narrow_keys(DevBuf& keys, DevBuf& wide, int64_t n) {
    if (key_out_dt() != DType::Int32) return;
    wide = std::move(keys);
    keys.alloc(n * 4);
    launch_narrow_i64_i32(wide.get<int64_t>(), n, keys.get<int32_t>(),
                          stream_);
  }

  // decode the generalized-key grouping columns for the ordered groups
  std::vector<HostOutCol> emit_gkey_cols(const uint32_t* order_slots,
                                         int64_t n) {
    std::vector<HostOutCol> out;
    size_t bm = (n + 7) / 8;
    for (size_t k = 0; k < key_cols_.size(); k++) {
      HostOutCol c;
      DType dt = key_dts_[k];
      DevBuf bmbuf(bm);
      const int slot = null_slots(1);
      if (dt == DType::Utf8 || dt == DType::Binary) {
        c = freeze_binary_col(
            n,
            [&](int32_t* lens) {
              launch_gkey_out_lens(g_, order_slots, n, d_gkdts_.get<uint8_t>(),
                                   (int)key_cols_.size(), (int)k,
                                   (uint32_t*)lens, bmbuf.get<uint8_t>(),
                                   null_ctr(slot), stream_);
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
                              null_ctr(slot), stream_);
        d2h(&c.values, vals.get(), n * w);
        keep(std::move(vals));
      }
      c.dt = dt;
      col_validity(&c, bmbuf.get(), n, slot);
      keep(std::move(bmbuf));
      out.push_back(std::move(c));
    }
    return out;
  }

  // multi-arg emit: per-agg columns from the accumulator bank; partial mode
  // freezes the per-agg wire instead (ma_freeze_*). Collect aggs read their
  // sorted pool views through the legacy coll kernels (the AggTable's c_*
  // pointers are temporarily re-aimed per pool).
  void emit_ma_aggs(const uint32_t* order_slots, int64_t n,
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
      const int slot = (ag.kind != AGGL_CNT) ? null_slots(1) : -1;
      launch_ma_gather_out(ma_desc_, ma_, j, order_slots, n,
                           vals.get<uint8_t>(), bmbuf.get<uint8_t>(),
                           slot >= 0 ? null_ctr(slot) : nullptr, stream_);
      ac.dt = (ag.kind == AGGL_CNT) ? DType::Int64
              : (ag.kind == AGGL_AVG) ? DType::Float64
                                      : ma_out_dt(j);
      d2h(&ac.values, vals.get(), (size_t)n * w);
      if (slot >= 0) col_validity(&ac, bmbuf.get(), n, slot);
      keep(std::move(vals));
      keep(std::move(bmbuf));
      cols->push_back(std::move(ac));
    }
  }

  std::pair<int64_t, std::vector<HostOutCol>> emit_groups(
      const uint32_t* order_slots, int64_t n) {
    DBG("agg.emit n=%lld final=%d", (long long)n, (int)final_output_);
    emit_begin();
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
    const int gslot = null_slots(4);
    launch_agg_gather_out(t_, order_slots, n, keys.get<int64_t>(),
                          kvalid.get<uint8_t>(), sums.get<double>(),
                          svalid.get<uint8_t>(), cnts.get<long long>(),
                          mins.get<double>(), mvalid.get<uint8_t>(),
                          maxs.get<double>(), xvalid.get<uint8_t>(),
                          null_ctr(gslot), stream_);
    HostOutCol key_col;
    key_col.dt = key_out_dt();
    if (!gkey_) {
      narrow_keys(keys, wide, n);
      d2h(&key_col.values, keys.get(), n * dtype_width(key_col.dt));
      col_validity(&key_col, kvalid.get(), n, gslot);
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
          d2h(&ac->values, src.get(), n * 8);
          *at = (int)cols.size();
        } else {
          ac->values_from = *at;
        }
      };
      auto validity_once = [&](HostOutCol* ac, int* at, const DevBuf& src,
                               int slot) {
        if (*at < 0) {
          col_validity(ac, src.get(), n, slot);
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
            slot = null_slots(1);
            launch_first_gather(t_, order_slots, n, w, fvals[w].get<double>(),
                                fvalid[w].get<uint8_t>(), null_ctr(slot),
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
    emit_end(&cols);
    DBG("agg.emit d2h done");
    return {n, std::move(cols)};
  }

  std::pair<int64_t, std::vector<HostOutCol>> emit_skipped(const DevBatch& b) {
    int64_t n = b.num_rows;
    const DevColumn& key = b.cols.at(key_col_);
    const DevColumn& val = b.cols.at(val_col_);
    emit_begin();
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
    d2h(&key_col.values, key.values, n * dtype_width(key.dt));
    // pass-through of the input's bitmap: counted, not rebuilt
    if (key.validity) {
      const int slot = null_slots(1);
      launch_bitmap_null_count(key.validity, n, null_ctr(slot), stream_);
      col_validity(&key_col, key.validity, n, slot);
    }
    std::vector<HostOutCol> cols;
    cols.push_back(std::move(key_col));
    cols.push_back(std::move(buf_col));
    emit_end(&cols);
    return {n, std::move(cols)};
  }

 public:
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
  PinnedBuf pinned_meta_, pinned_nulls_;
  // host emit state (emit_begin .. emit_end)
  DevBuf d_emit_nulls_;
  int emit_null_used_ = 0;
  std::vector<DevBuf> emit_keep_;
  int64_t emit_d2h_bytes_ = 0, emit_host_copy_bytes_ = 0;
  // two-phase scratch (allocated on first large chunk)
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

// -------------------------------------------------------------- ShuffleOp --
class ShuffleOp {
 public:
  ShuffleOp(const ShuffleWriterNode& node, const Conf& conf, hipStream_t stream,
            uint32_t task_partition_id)
      : stream_(stream), node_(node), task_partition_id_(task_partition_id) {
    if (node.partitioning.kind == Repartition::Hash) {
      if (node.partitioning.hash_exprs.empty())
        FAIL("hash partitioning without exprs");
      for (const Expr& e : node.partitioning.hash_exprs) {
        if (e.kind != Expr::Column) FAIL("hash expr must be a Column");
        hash_cols_.push_back(e.col_index);
      }
    } else if (node.partitioning.kind != Repartition::Single &&
               node.partitioning.kind != Repartition::RoundRobin) {
      FAIL("unsupported partitioning kind");
    }
    if (node.partitioning.partition_count <= 0 ||
        node.partitioning.partition_count > (1 << 24))
      FAIL("ShuffleWriter: partition_count out of range");
    P_ = (uint32_t)node.partitioning.partition_count;
    batch_size_ = conf.get_i("BATCH_SIZE", 10000);
    if (batch_size_ <= 0) FAIL("invalid BATCH_SIZE conf");
    target_block_ = (size_t)conf.get_i("SHUFFLE_COMPRESSION_TARGET_BUF_SIZE",
                                       4194304);
    std::string codec = conf.get("SPARK_IO_COMPRESSION_CODEC", "lz4");
    if (codec == "lz4") codec_ = 0;
    else if (codec == "zstd") codec_ = 1;  // ipc_compression.rs:189-196
    else FAIL("unsupported shuffle codec (lz4/zstd on this path)");
    zstd_level_ = (int)conf.get_i("SPARK_IO_COMPRESSION_ZSTD_LEVEL", 1);
  }

  void consume(DevBatch&& b) {
    if (b.num_rows > 0) staged_.push_back(std::move(b));
  }

  // partition + write files; returns nothing (shuffle output goes to disk)
  void finish() {
    int64_t n = 0;
    for (const DevBatch& b : staged_) n += b.num_rows;
    std::vector<int64_t> part_offsets(P_ + 1, 0);
    if (n == 0) {
      write_files({}, part_offsets);
      return;
    }
    size_t ncols = staged_[0].cols.size();
    // concat columns (device)
    DevBatch all = concat();
    std::vector<int64_t> h_offsets;
    if (node_.partitioning.kind == Repartition::Single) {
      part_offsets[1] = n;
      for (uint32_t p = 1; p <= P_; p++) part_offsets[p] = n;
      // identity permutation
      DevBuf perm(n * 4);
      launch_iota_u32(perm.get<uint32_t>(), n, stream_);
      emit(all, perm, part_offsets, ncols, n);
      return;
    }
    DevBuf part_ids(n * 4);
    if (node_.partitioning.kind == Repartition::RoundRobin) {
      // evaluate_robin_partition_ids (shuffle/mod.rs:190-202) with
      // start_rows = partition_id * 1000193 (buffered_data.rs:291-293); one
      // continuous counter over all rows == the reference's per-flush chain
      uint32_t start = (uint32_t)(((uint64_t)task_partition_id_ * 1000193ull) %
                                  (uint64_t)P_);
      launch_robin_ids(n, start, P_, part_ids.get<uint32_t>(), stream_);
    } else {
      // murmur3 seed 42 fold over hash cols (shuffle/mod.rs:163-176)
      DevBuf hashes(n * 4);
      launch_hash_init(hashes.get<int32_t>(), 42, n, stream_);
      for (uint32_t ci : hash_cols_) {
        const DevColumn& c = all.cols.at(ci);
        if (c.dt == DType::Int64)
          launch_hash_fold_i64((const int64_t*)c.values, c.validity, n,
                               hashes.get<int32_t>(), stream_);
        else if (c.dt == DType::Int32)
          launch_hash_fold_i32((const int32_t*)c.values, c.validity, n,
                               hashes.get<int32_t>(), stream_);
        else if (c.dt == DType::Utf8 || c.dt == DType::Binary)
          launch_hash_fold_bytes(c.offsets, (const uint8_t*)c.values,
                                 c.validity, n, hashes.get<int32_t>(),
                                 stream_);
        else
          FAIL("hash expr column must be Int64/Int32/Utf8 (hot-path scope)");
      }
      launch_pmod(hashes.get<int32_t>(), n, (int32_t)P_,
                  part_ids.get<uint32_t>(), stream_);
      AURON_HIP(hipStreamSynchronize(stream_));  // hashes is pooled
    }
    // histogram → host scan
    DevBuf counts(P_ * 4);
    AURON_HIP(hipMemsetAsync(counts.get(), 0, P_ * 4, stream_));
    launch_histogram(part_ids.get<uint32_t>(), n, P_, counts.get<uint32_t>(),
                     stream_);
    std::vector<uint32_t> h_counts(P_);
    AURON_HIP(hipMemcpyAsync(h_counts.data(), counts.get(), P_ * 4,
                             hipMemcpyDeviceToHost, stream_));
    AURON_HIP(hipStreamSynchronize(stream_));
    for (uint32_t p = 0; p < P_; p++)
      part_offsets[p + 1] = part_offsets[p] + h_counts[p];
    // stable permutation: rocprim stable radix sort of (part_id, row)
    DevBuf iota(n * 4), keys_out(n * 4), perm(n * 4);
    launch_iota_u32(iota.get<uint32_t>(), n, stream_);
    int end_bit = 1;
    while ((1u << end_bit) < P_) end_bit++;
    size_t tmp_bytes = 0;
    sort_pairs_u32_u32(part_ids.get<uint32_t>(), iota.get<uint32_t>(),
                       keys_out.get<uint32_t>(), perm.get<uint32_t>(), n,
                       end_bit, nullptr, &tmp_bytes, stream_);
    DevBuf tmp(tmp_bytes);
    sort_pairs_u32_u32(part_ids.get<uint32_t>(), iota.get<uint32_t>(),
                       keys_out.get<uint32_t>(), perm.get<uint32_t>(), n,
                       end_bit, tmp.get(), &tmp_bytes, stream_);
    emit(all, perm, part_offsets, ncols, n);
  }

 private:
  DevBatch concat() {
    DevBatch all;
    int64_t n = 0;
    for (const DevBatch& b : staged_) n += b.num_rows;
    all.num_rows = n;
    size_t ncols = staged_[0].cols.size();
    for (size_t c = 0; c < ncols; c++) {
      const DevColumn& proto = staged_[0].cols[c];
      DevColumn col;
      col.dt = proto.dt;
      col.len = n;
      bool any_valid = false;
      for (const DevBatch& b : staged_)
        if (b.cols[c].validity) any_valid = true;
      if (col.dt == DType::Binary || col.dt == DType::Utf8) {
        int64_t total_data = 0;
        for (const DevBatch& b : staged_) total_data += b.cols[c].data_len;
        col.data_len = total_data;
        col.own_values.alloc(total_data ? total_data : 1);
        col.own_offsets.alloc((n + 1) * 4);
        // offsets rebased on host (few batches; lens path keeps it simple)
        std::vector<int32_t> h_off(n + 1, 0);
        int64_t row = 0, dpos = 0;
        for (const DevBatch& b : staged_) {
          const DevColumn& src = b.cols[c];
          std::vector<int32_t> so(src.len + 1);
          AURON_HIP(hipMemcpyAsync(so.data(), src.offsets, (src.len + 1) * 4,
                                   hipMemcpyDeviceToHost, stream_));
          AURON_HIP(hipStreamSynchronize(stream_));
          for (int64_t i = 0; i < src.len; i++)
            h_off[row + i + 1] = (int32_t)(dpos + so[i + 1]);
          if (src.data_len)
            AURON_HIP(hipMemcpyAsync(col.own_values.get<uint8_t>() + dpos,
                                     src.values, src.data_len,
                                     hipMemcpyDeviceToDevice, stream_));
          row += src.len;
          dpos += src.data_len;
        }
        AURON_HIP(hipMemcpyAsync(col.own_offsets.get(), h_off.data(),
                                 (n + 1) * 4, hipMemcpyHostToDevice, stream_));
        col.values = col.own_values.get();
        col.offsets = col.own_offsets.get<int32_t>();
      } else {
        size_t w = dtype_width(col.dt);
        col.own_values.alloc(n * w);
        int64_t row = 0;
        for (const DevBatch& b : staged_) {
          AURON_HIP(hipMemcpyAsync(col.own_values.get<uint8_t>() + row * w,
                                   b.cols[c].values, b.cols[c].len * w,
                                   hipMemcpyDeviceToDevice, stream_));
          row += b.cols[c].len;
        }
        col.values = col.own_values.get();
      }
      if (any_valid) {
        // merge validity bitmaps on host (bit shifts across batch boundaries)
        std::vector<uint8_t> bm((n + 7) / 8, 0xFF);
        int64_t row = 0;
        for (const DevBatch& b : staged_) {
          const DevColumn& src = b.cols[c];
          if (src.validity) {
            std::vector<uint8_t> sb((src.len + 7) / 8);
            AURON_HIP(hipMemcpyAsync(sb.data(), src.validity, sb.size(),
                                     hipMemcpyDeviceToHost, stream_));
            AURON_HIP(hipStreamSynchronize(stream_));
            for (int64_t i = 0; i < src.len; i++)
              if (!((sb[i >> 3] >> (i & 7)) & 1))
                bm[(row + i) >> 3] &= (uint8_t)~(1u << ((row + i) & 7));
          }
          row += src.len;
        }
        col.own_validity.alloc(bm.size());
        AURON_HIP(hipMemcpyAsync(col.own_validity.get(), bm.data(), bm.size(),
                                 hipMemcpyHostToDevice, stream_));
        col.validity = col.own_validity.get<uint8_t>();
      }
      all.cols.push_back(std::move(col));
    }
    return all;
  }

  void emit(const DevBatch& all, const DevBuf& perm,
            const std::vector<int64_t>& part_offsets, size_t ncols, int64_t n) {
    // gather columns into partition-contiguous order, D2H, serialize
    std::vector<std::vector<uint8_t>> h_values(ncols), h_validity(ncols);
    std::vector<std::vector<int32_t>> h_offsets(ncols);
    std::vector<HostCol> cols(ncols);
    for (size_t c = 0; c < ncols; c++) {
      const DevColumn& src = all.cols[c];
      if (src.dt == DType::Binary || src.dt == DType::Utf8) {
        DevBuf lens(n * 4);
        launch_gather_lens(src.offsets, perm.get<uint32_t>(), n,
                           lens.get<int32_t>(), stream_);
        DevBuf d_off((n + 1) * 4);
        h_offsets[c] =
            lens_to_offsets(lens.get(), n, d_off.get<int32_t>(), stream_);
        DevBuf d_data(h_offsets[c][n] ? h_offsets[c][n] : 1);
        launch_gather_bytes((const uint8_t*)src.values, src.offsets,
                            perm.get<uint32_t>(), d_off.get<int32_t>(), n,
                            d_data.get<uint8_t>(), stream_);
        h_values[c].resize(h_offsets[c][n]);
        AURON_HIP(hipMemcpyAsync(h_values[c].data(), d_data.get(),
                                 h_values[c].size(), hipMemcpyDeviceToHost,
                                 stream_));
        AURON_HIP(hipStreamSynchronize(stream_));
        cols[c].byte_width = 0;
        cols[c].values = h_values[c].data();
        cols[c].offsets = h_offsets[c].data();
      } else {
        size_t w = dtype_width(src.dt);
        DevBuf d_out(n * w);
        if (w == 8)
          launch_gather_8((const uint8_t*)src.values, perm.get<uint32_t>(), n,
                          d_out.get<uint8_t>(), stream_);
        else if (w == 4)
          launch_gather_4((const uint8_t*)src.values, perm.get<uint32_t>(), n,
                          d_out.get<uint8_t>(), stream_);
        else
          FAIL("shuffle gather supports 4/8-byte primitives (hot path)");
        h_values[c].resize(n * w);
        AURON_HIP(hipMemcpyAsync(h_values[c].data(), d_out.get(), n * w,
                                 hipMemcpyDeviceToHost, stream_));
        cols[c].byte_width = (int)w;
        cols[c].values = h_values[c].data();
      }
      if (src.validity) {
        DevBuf d_bits((n + 7) / 8);
        launch_gather_bits(src.validity, perm.get<uint32_t>(), n,
                           d_bits.get<uint8_t>(), stream_);
        h_validity[c].resize((n + 7) / 8);
        AURON_HIP(hipMemcpyAsync(h_validity[c].data(), d_bits.get(),
                                 h_validity[c].size(), hipMemcpyDeviceToHost,
                                 stream_));
        cols[c].validity = h_validity[c].data();
      }
    }
    AURON_HIP(hipStreamSynchronize(stream_));
    write_files(cols, part_offsets);
  }

  void write_files(const std::vector<HostCol>& cols,
                   const std::vector<int64_t>& part_offsets) {
    std::string err;
    if (!write_shuffle_files(cols, part_offsets, batch_size_,
                             node_.output_data_file, node_.output_index_file,
                             &err, codec_, zstd_level_))
      FAIL(err);
  }

  hipStream_t stream_;
  const ShuffleWriterNode& node_;
  uint32_t task_partition_id_ = 0;
  std::vector<uint32_t> hash_cols_;
  uint32_t P_ = 1;
  int64_t batch_size_ = 10000;
  size_t target_block_ = 4194304;
  int codec_ = 0, zstd_level_ = 1;
  std::vector<DevBatch> staged_;
};

// ------------------------------------------------------------- ExprRunner --
// Binds a compiled ExprProgram (expr.h) to the columns of one device batch
// and launches k_expr_eval. The caller owns the error flag and reads it back
// at its next host sync.
struct ExprRunner {
  ExprProgram prog;

  // fills prog / vals / valid / n; returns the nullable-slot mask
  uint32_t bind(const DevBatch& in, ExprKernArgs* a) const {
    memset((void*)a, 0, sizeof(*a));
    a->prog = prog;
    a->n = in.num_rows;
    uint32_t nullable = 0;
    for (int s = 0; s < prog.nslots; s++) {
      const DevColumn& c = in.cols.at(prog.slot_col[s]);
      if (c.dt != expr_ty_dtype((ExprTy)prog.slot_ty[s]))
        FAIL("expression input column " + std::to_string(prog.slot_col[s]) +
             " arrived with a dtype other than the plan's");
      if (c.len < in.num_rows) FAIL("expression input column too short");
      a->vals[s] = c.values;
      a->valid[s] = c.validity;
      if (c.validity) nullable |= 1u << s;
    }
    return nullable;
  }
};

// --------------------------------------------------------------- FilterOp --
// FilterExec (filter_exec.rs:174-198): ANDed predicates -> selection mask ->
// stable compaction. Column <op> Literal, IsNotNull/IsNull(Column) and And of
// those run the per-predicate mask kernels; any other predicate shape turns
// the whole predicate list into one ExprProgram evaluated in mask mode.
class FilterOp {
 public:
  FilterOp(const FilterNode& node, const std::vector<DType>* in_dtypes,
           hipStream_t stream)
      : stream_(stream) {
    try {
      for (const Expr& e : node.predicates) compile(e);
    } catch (const EngineError&) {
      preds_.clear();
      use_prog_ = true;
    }
    if (use_prog_) {
      if (!in_dtypes)
        FAIL("FilterExec: computed predicates need a statically typed input "
             "(not available above an Agg)");
      std::string err;
      if (!compile_filter_program(node.predicates, *in_dtypes, &runner_.prog,
                                  &err))
        FAIL("FilterExec: " + err);
      d_err_.alloc(4);
      AURON_HIP(hipMemsetAsync(d_err_.get(), 0, 4, stream_));
    } else if (preds_.empty()) {
      FAIL("FilterExec without usable predicates");
    }
  }

  DevBatch apply(DevBatch&& in) {
    int64_t n = in.num_rows;
    if (n == 0) return std::move(in);
    DevBuf mask(n);
    if (use_prog_) {
      ExprKernArgs a;
      runner_.bind(in, &a);
      a.out_mask = mask.get<uint8_t>();
      a.error_flag = d_err_.get<uint32_t>();
      launch_expr_eval(a, stream_);
    }
    for (size_t pi = 0; pi < preds_.size(); pi++) {
      const Pred& p = preds_[pi];
      const DevColumn& c = in.cols.at(p.col);
      bool first = pi == 0;
      if (p.kind == Pred::NotNull || p.kind == Pred::Null) {
        launch_is_not_null(c.validity, n, mask.get<uint8_t>(), first,
                           p.kind == Pred::Null, stream_);
      } else {
        if (c.dt != p.dtype) FAIL("filter literal/column dtype mismatch");
        launch_cmp_lit(c.dt, c.values, c.validity, n, p.op, p.lit_i, p.lit_f,
                       mask.get<uint8_t>(), first, stream_);
      }
    }
    // stable compaction: positions = exclusive scan of mask
    DevBuf positions((n + 1) * 4);
    scan_mask_positions(mask.get<uint8_t>(), n, positions.get<uint32_t>(),
                        &scan_tmp_, stream_);
    if (!pinned_.get()) pinned_.alloc(8);
    uint32_t* h_cnt = pinned_.get<uint32_t>();
    AURON_HIP(hipMemcpyAsync(h_cnt, positions.get<uint32_t>() + n, 4,
                             hipMemcpyDeviceToHost, stream_));
    h_cnt[1] = 0;
    if (use_prog_ && runner_.prog.can_poison)
      AURON_HIP(hipMemcpyAsync(h_cnt + 1, d_err_.get(), 4,
                               hipMemcpyDeviceToHost, stream_));
    AURON_HIP(hipStreamSynchronize(stream_));
    if (h_cnt[1]) FAIL("Divide by zero error");
    int64_t m = *h_cnt;
    DevBatch out;
    out.num_rows = m;
    if (m == 0) {
      for (auto& c : in.cols) {
        DevColumn oc;
        oc.dt = c.dt;
        oc.len = 0;
        out.cols.push_back(std::move(oc));
      }
      return out;
    }
    DevBuf sel(m * 4);
    launch_sel_rows(mask.get<uint8_t>(), positions.get<uint32_t>(), n,
                    sel.get<uint32_t>(), stream_);
    for (auto& c : in.cols) {
      out.cols.push_back(gather_col(c, sel.get<uint32_t>(), m));
    }
    // sel/mask/positions are pooled: drain the gathers before recycling
    AURON_HIP(hipStreamSynchronize(stream_));
    held_.push_back(std::move(in));  // borrowed inputs stay alive
    return out;
  }

 private:
  struct Pred {
    enum Kind { CmpLit, NotNull, Null } kind = CmpLit;
    uint32_t col = 0;
    CmpOp op = CMP_EQ;
    DType dtype = DType::Unsupported;
    int64_t lit_i = 0;
    double lit_f = 0;
  };

  void compile(const Expr& e) {
    if (e.kind == Expr::IsNotNull || e.kind == Expr::IsNull) {
      const Expr& c = e.children.at(0);
      if (c.kind != Expr::Column) FAIL("null-check operand must be a Column");
      Pred p;
      p.kind = e.kind == Expr::IsNull ? Pred::Null : Pred::NotNull;
      p.col = c.col_index;
      preds_.push_back(p);
      return;
    }
    if (e.kind != Expr::BinaryExpr || e.children.size() != 2)
      FAIL("unsupported filter predicate");
    const Expr& l = e.children[0];
    const Expr& r = e.children[1];
    if (e.op == "And") {  // nested AND: flatten
      compile(l);
      compile(r);
      return;
    }
    CmpOp op;
    if (e.op == "Eq") op = CMP_EQ;
    else if (e.op == "NotEq") op = CMP_NE;
    else if (e.op == "Lt") op = CMP_LT;
    else if (e.op == "LtEq") op = CMP_LE;
    else if (e.op == "Gt") op = CMP_GT;
    else if (e.op == "GtEq") op = CMP_GE;
    else FAIL("unsupported filter operator: " + e.op);
    const Expr* col = nullptr;
    const Expr* lit = nullptr;
    if (l.kind == Expr::Column && r.kind == Expr::Literal) {
      col = &l;
      lit = &r;
    } else if (l.kind == Expr::Literal && r.kind == Expr::Column) {
      col = &r;
      lit = &l;
      // flip: lit OP col == col FLIP(OP) lit
      op = op == CMP_LT ? CMP_GT : op == CMP_LE ? CMP_GE
           : op == CMP_GT ? CMP_LT : op == CMP_GE ? CMP_LE : op;
    } else {
      FAIL("filter predicate must be Column-vs-Literal on this path");
    }
    ScalarLit s;
    std::string err;
    if (!decode_ipc_scalar(lit->literal_ipc.data(), lit->literal_ipc.size(),
                           &s, &err))
      FAIL("literal decode: " + err);
    Pred p;
    p.kind = Pred::CmpLit;
    p.col = col->col_index;
    p.op = op;
    p.dtype = s.dtype;
    p.lit_i = s.i64;
    p.lit_f = s.f64;
    if (s.is_null) FAIL("null literal comparison unsupported");
    preds_.push_back(p);
  }

  DevColumn gather_col(const DevColumn& c, const uint32_t* sel, int64_t m) {
    DevColumn out;
    out.dt = c.dt;
    out.len = m;
    size_t w = dtype_width(c.dt);
    if (c.dt == DType::Binary || c.dt == DType::Utf8) {
      DevBuf lens(m * 4);
      launch_gather_lens(c.offsets, sel, m, lens.get<int32_t>(), stream_);
      out.own_offsets.alloc((m + 1) * 4);
      std::vector<int32_t> h_offs = lens_to_offsets(
          lens.get(), m, out.own_offsets.get<int32_t>(), stream_);
      out.offsets = out.own_offsets.get<int32_t>();
      out.data_len = h_offs[m];
      out.own_values.alloc(out.data_len ? out.data_len : 1);
      launch_gather_bytes((const uint8_t*)c.values, c.offsets, sel,
                          out.own_offsets.get<int32_t>(), m,
                          out.own_values.get<uint8_t>(), stream_);
      out.values = out.own_values.get();
    } else if (w == 8) {
      out.own_values.alloc(m * 8);
      launch_gather_8((const uint8_t*)c.values, sel, m,
                      out.own_values.get<uint8_t>(), stream_);
      out.values = out.own_values.get();
    } else if (w == 4) {
      out.own_values.alloc(m * 4);
      launch_gather_4((const uint8_t*)c.values, sel, m,
                      out.own_values.get<uint8_t>(), stream_);
      out.values = out.own_values.get();
    } else {
      FAIL("filter gather: unsupported column width");
    }
    if (c.validity) {
      out.own_validity.alloc((m + 7) / 8);
      launch_gather_bits(c.validity, sel, m, out.own_validity.get<uint8_t>(),
                         stream_);
      out.validity = out.own_validity.get<uint8_t>();
    }
    return out;
  }

  hipStream_t stream_;
  std::vector<Pred> preds_;
  bool use_prog_ = false;
  ExprRunner runner_;
  DevBuf d_err_;
  DevBuf scan_tmp_;
  PinnedBuf pinned_;
  std::vector<DevBatch> held_;
};

// -------------------------------------------------------------- ProjectOp --
// ProjectionExec (project_exec.rs): Column exprs are zero-copy views; every
// other expr is compiled to an ExprProgram and evaluated by k_expr_eval into
// an owned column. Also serves as the implicit stage that computes Agg
// grouping / argument expressions.
class ProjectOp {
 public:
  ProjectOp(const std::vector<Expr>& exprs, const std::vector<DType>* in_dtypes,
            hipStream_t stream)
      : stream_(stream) {
    for (const Expr& e : exprs) {
      Item it;
      if (e.kind == Expr::Column) {
        it.col = (int)e.col_index;
        if (in_dtypes && e.col_index < in_dtypes->size())
          it.dt = (*in_dtypes)[e.col_index];
      } else {
        if (!in_dtypes)
          FAIL("ProjectionExec: computed exprs need a statically typed input "
               "(not available above an Agg)");
        std::string err;
        if (!compile_value_program(e, *in_dtypes, &it.run.prog, &err))
          FAIL("ProjectionExec: " + err);
        it.dt = expr_ty_dtype((ExprTy)it.run.prog.root_ty);
        any_poison_ |= it.run.prog.can_poison != 0;
        any_computed_ = true;
      }
      items_.push_back(std::move(it));
    }
    if (any_computed_) {
      d_err_.alloc(4);
      AURON_HIP(hipMemsetAsync(d_err_.get(), 0, 4, stream_));
    }
  }

  // output dtypes (Unsupported where a Column's input type is not known)
  std::vector<DType> output_dtypes() const {
    std::vector<DType> d;
    for (const Item& it : items_) d.push_back(it.dt);
    return d;
  }

  DevBatch apply(DevBatch&& in) {
    DevBatch out;
    const int64_t n = in.num_rows;
    out.num_rows = n;
    for (const Item& it : items_) {
      if (it.col >= 0) {
        DevColumn& src = in.cols.at(it.col);
        DevColumn view;
        view.dt = src.dt;
        view.len = src.len;
        view.values = src.values;
        view.validity = src.validity;
        view.offsets = src.offsets;
        view.data_len = src.data_len;
        out.cols.push_back(std::move(view));
        continue;
      }
      DevColumn oc;
      oc.dt = it.dt;
      oc.len = n;
      if (n > 0) {
        ExprKernArgs a;
        uint32_t nullable = it.run.bind(in, &a);
        const size_t w = dtype_width(it.dt);
        oc.own_values.alloc((size_t)n * w);
        oc.values = oc.own_values.get();
        a.out_vals = oc.own_values.get();
        a.out_width = (int32_t)w;
        if (expr_result_nullable(it.run.prog, nullable)) {
          // whole 64-row words: one 8-byte store per wave
          oc.own_validity.alloc((size_t)((n + 63) / 64) * 8);
          oc.validity = oc.own_validity.get<uint8_t>();
          a.out_valid = oc.own_validity.get<uint64_t>();
        }
        a.error_flag = d_err_.get<uint32_t>();
        launch_expr_eval(a, stream_);
      }
      out.cols.push_back(std::move(oc));
    }
    if (any_poison_ && n > 0) {
      if (!pinned_.get()) pinned_.alloc(8);
      uint32_t* h_err = pinned_.get<uint32_t>();
      AURON_HIP(hipMemcpyAsync(h_err, d_err_.get(), 4, hipMemcpyDeviceToHost,
                               stream_));
      AURON_HIP(hipStreamSynchronize(stream_));
      if (*h_err) FAIL("Divide by zero error");
    }
    held_.push_back(std::move(in));  // owner of the viewed / read buffers
    return out;
  }

 private:
  struct Item {
    int col = -1;  // >= 0: zero-copy view of that input column
    DType dt = DType::Unsupported;
    ExprRunner run;
  };
  hipStream_t stream_;
  std::vector<Item> items_;
  bool any_computed_ = false, any_poison_ = false;
  DevBuf d_err_;
  PinnedBuf pinned_;
  std::vector<DevBatch> held_;
};

// ---------------------------------------------------------------- Runtime --
struct Runtime {
  std::unique_ptr<TaskDefinition> td;
  AuronCallbacks cb{};
  hipStream_t stream = nullptr;
  bool started = false;
  bool schema_sent = false;
  std::string error;
  struct Stage {
    enum Kind { AggS, ShuffleS, FilterS, ProjectS } kind = AggS;
    std::unique_ptr<AggOp> agg;
    std::unique_ptr<ShuffleOp> shuffle;
    std::unique_ptr<FilterOp> filter;
    std::unique_ptr<ProjectOp> project;
  };
  std::vector<Stage> stages_;
  bool terminal_transform_ = false;  // last stage is a Filter / Projection
  std::vector<OutField> out_fields;
  int ipc_codec_ = 0;  // IpcReader block codec (SPARK_IO_COMPRESSION_CODEC)
  std::vector<std::pair<int64_t, std::vector<HostOutCol>>> outputs;
  int64_t emit_d2h_bytes_ = 0;  // terminal Filter/Projection downloads
  size_t emit_idx = 0;
  // device-resident outputs (AURON_HIP_DEVICE_OUTPUT): exported through
  // import_device_batch; DevBufs stay owned here until finalize
  std::vector<std::pair<int64_t, std::vector<DevOutCol>>> outputs_dev;
  size_t emit_dev_idx = 0;
  std::map<std::string, int64_t> metrics;

  ~Runtime() {
    if (stream) (void)hipStreamDestroy(stream);
  }

  void set_error(const std::string& msg) {
    error = msg;
    if (cb.set_error) cb.set_error(cb.user, msg.c_str());
  }

  // run the whole pipeline (Agg is a pipeline breaker; outputs are staged)
  void run() {
    auto t0 = std::chrono::steady_clock::now();
    Conf conf{&cb};
    {
      std::string codec = conf.get("SPARK_IO_COMPRESSION_CODEC", "lz4");
      if (codec == "zstd") ipc_codec_ = 1;
      else if (codec != "lz4")
        FAIL("unsupported shuffle codec (lz4/zstd on this path)");
    }
    // collect plan chain root→leaf
    std::vector<const PlanNode*> chain;
    const PlanNode* p = td->plan.get();
    while (p) {
      chain.push_back(p);
      switch (p->kind) {
        case PlanNode::ShuffleWriter: p = p->shuffle_writer->input.get(); break;
        case PlanNode::Agg: p = p->agg->input.get(); break;
        case PlanNode::Filter: p = p->filter->input.get(); break;
        case PlanNode::Projection: p = p->projection->input.get(); break;
        case PlanNode::IpcReader:
        case PlanNode::ParquetScan:
        case PlanNode::FFIReader: p = nullptr; break;
      }
    }
    // leaf must be a source: FFIReader (Arrow in) or IpcReader (shuffle bytes)
    const PlanNode* leaf = chain.back();
    if (leaf->kind != PlanNode::FFIReader &&
        leaf->kind != PlanNode::IpcReader &&
        leaf->kind != PlanNode::ParquetScan)
      FAIL("plan leaf must be FFIReader/IpcReader/ParquetScan on this path");

    // static schema of the batches between stages: expression programs are
    // type-checked against it at plan build. An Agg fixes its output types
    // only when it sees data, so the schema is unknown above one.
    std::vector<OutField> cur;
    bool cur_known = true;
    {
      const Schema* ls = leaf->kind == PlanNode::FFIReader
                             ? &leaf->ffi_reader->schema
                         : leaf->kind == PlanNode::IpcReader
                             ? &leaf->ipc_reader->schema
                             : &leaf->parquet->schema;
      std::vector<uint32_t> pick;
      if (leaf->kind == PlanNode::ParquetScan) pick = leaf->parquet->projection;
      if (pick.empty())
        for (uint32_t i = 0; i < ls->fields.size(); i++) pick.push_back(i);
      for (uint32_t i : pick) {
        if (i >= ls->fields.size()) FAIL("scan projection out of range");
        cur.push_back({ls->fields[i].name, ls->fields[i].dtype, true});
      }
    }
    auto cur_dtypes = [&]() {
      std::vector<DType> d;
      for (const OutField& f : cur) d.push_back(f.dt);
      return d;
    };

    // middle ops (leaf-1 ... root), in execution order
    stages_.clear();
    terminal_transform_ = false;
    for (auto it = chain.rbegin() + 1; it != chain.rend(); ++it) {
      const PlanNode* node = *it;
      if (!stages_.empty() && stages_.back().kind == Stage::ShuffleS)
        FAIL("operator above ShuffleWriter unsupported");
      Stage st;
      std::vector<DType> in_dt = cur_dtypes();
      const std::vector<DType>* in_dtp = cur_known ? &in_dt : nullptr;
      switch (node->kind) {
        case PlanNode::Agg: {
          st.kind = Stage::AggS;
          AggNode lowered;
          std::vector<Expr> pre;
          if (lower_agg_inputs(*node->agg, &lowered, &pre)) {
            // implicit projection directly in front of the Agg: referenced
            // columns + computed grouping / argument columns
            Stage ps;
            ps.kind = Stage::ProjectS;
            ps.project = std::make_unique<ProjectOp>(pre, in_dtp, stream);
            stages_.push_back(std::move(ps));
            st.agg = std::make_unique<AggOp>(lowered, conf, stream);
          } else {
            st.agg = std::make_unique<AggOp>(*node->agg, conf, stream);
          }
          cur_known = false;
          break;
        }
        case PlanNode::ShuffleWriter:
          st.kind = Stage::ShuffleS;
          st.shuffle = std::make_unique<ShuffleOp>(*node->shuffle_writer, conf,
                                                   stream, td->partition_id);
          break;
        case PlanNode::Filter:
          st.kind = Stage::FilterS;
          st.filter = std::make_unique<FilterOp>(*node->filter, in_dtp, stream);
          break;
        case PlanNode::Projection: {
          const ProjectionNode& pn = *node->projection;
          st.kind = Stage::ProjectS;
          st.project = std::make_unique<ProjectOp>(pn.exprs, in_dtp, stream);
          std::vector<DType> od = st.project->output_dtypes();
          std::vector<OutField> next;
          for (size_t i = 0; i < od.size(); i++)
            next.push_back({i < pn.names.size() ? pn.names[i]
                                                : "col" + std::to_string(i),
                            od[i], true});
          cur = std::move(next);
          break;
        }
        default:
          FAIL("unsupported operator in plan chain");
      }
      stages_.push_back(std::move(st));
    }
    // A plan that ends in a Filter or Projection has no pipeline breaker to
    // stage its output: batches leaving the chain are emitted as ordinary
    // host task output, in input order.
    if (!stages_.empty() && (stages_.back().kind == Stage::FilterS ||
                             stages_.back().kind == Stage::ProjectS)) {
      if (!cur_known)
        FAIL("Filter/Projection above an Agg as the plan's last stage "
             "unsupported");
      if (conf.get_i("AURON_HIP_DEVICE_OUTPUT", 0) != 0)
        FAIL("AURON_HIP_DEVICE_OUTPUT on a plan ending in Filter/Projection "
             "unsupported (its output is host batches)");
      for (const OutField& f : cur)
        if (!dtype_format(f.dt) || f.dt == DType::Unsupported)
          FAIL("terminal Filter/Projection: unsupported output column dtype");
      terminal_transform_ = true;
      out_fields = cur;
    }

    // pump input through the chain
    int64_t input_rows = 0;
    const BatchSink sink = [&](DevBatch&& b) { feed(0, std::move(b)); };
    if (leaf->kind == PlanNode::FFIReader) {
      const FFIReaderNode& reader = *leaf->ffi_reader;
      while (true) {
        ArrowArray arr;
        ArrowSchema sch;
        ArrowDeviceArray dev;
        memset(&arr, 0, sizeof(arr));
        memset(&sch, 0, sizeof(sch));
        memset(&dev, 0, sizeof(dev));
        if (!cb.next_input_batch) break;
        int rc = cb.next_input_batch(cb.user, reader.resource_id.c_str(), &arr,
                                     &sch, &dev);
        DBG("reader rc=%d", rc);
        if (rc == 0) break;
        DevBatch b;
        if (rc == 2) {
          b = import_batch(&dev.array, sch.release ? &sch : nullptr,
                           reader.schema, true, stream);
        } else {
          b = import_batch(&arr, sch.release ? &sch : nullptr, reader.schema,
                           false, stream);
          if (arr.release) arr.release(&arr);
        }
        if (sch.release) sch.release(&sch);
        input_rows += b.num_rows;
        feed(0, std::move(b));
      }
    } else if (leaf->kind == PlanNode::IpcReader) {
      input_rows = read_ipc(*leaf->ipc_reader, cb, ipc_codec_, stream, sink);
    } else {
      input_rows = scan_parquet(*leaf->parquet, stream, sink);
    }
    // drain chain: pipeline breakers emit, transforms pass through
    AggOp* last_agg = nullptr;
    AggOp* first_agg = nullptr;
    bool has_shuffle = false;
    for (size_t i = 0; i < stages_.size(); i++) {
      Stage& st = stages_[i];
      if (st.kind == Stage::AggS) {
        if (!first_agg) first_agg = st.agg.get();
        last_agg = st.agg.get();
        bool terminal = i + 1 == stages_.size();
        if (st.agg->device_out_) {
          if (!terminal)
            FAIL("AURON_HIP_DEVICE_OUTPUT on a non-terminal Agg unsupported");
          if (!cb.import_device_batch)
            FAIL("AURON_HIP_DEVICE_OUTPUT set but import_device_batch is "
                 "NULL");
          outputs_dev = st.agg->finish_dev();
          out_fields = st.agg->output_fields();
        } else {
          auto outs = st.agg->finish();
          for (auto& ob : outs) {
            if (terminal) {
              outputs.push_back(std::move(ob));
            } else {
              DevBatch b = host_out_to_dev(ob);
              feed(i + 1, std::move(b));
            }
          }
          if (terminal) out_fields = st.agg->output_fields();
        }
      } else if (st.kind == Stage::ShuffleS) {
        st.shuffle->finish();
        has_shuffle = true;
        out_fields.clear();
      }
    }
    if (!has_shuffle && !last_agg && !terminal_transform_)
      FAIL("plan without Agg/ShuffleWriter sink unsupported");
    if (last_agg) {
      metrics["num_groups"] = (int64_t)last_agg->num_groups_host();
      metrics["agg_update_ns"] = first_agg->update_ns_;
      metrics["agg_update_rows"] = first_agg->update_rows_;
      metrics["spill_count"] = first_agg->spill_count_ + last_agg->spill_count_;
    }
    // host-emit accounting: payload bytes copied down into export buffers,
    // and payload bytes moved again by a host memcpy on the way out
    int64_t d2h_bytes = emit_d2h_bytes_, host_copy_bytes = 0;
    for (Stage& st : stages_)
      if (st.kind == Stage::AggS) {
        d2h_bytes += st.agg->emit_d2h_bytes_;
        host_copy_bytes += st.agg->emit_host_copy_bytes_;
      }
    metrics["emit_d2h_bytes"] = d2h_bytes;
    metrics["emit_host_copy_bytes"] = host_copy_bytes;
    metrics["input_rows"] = input_rows;
    int64_t out_rows = 0;
    for (auto& o : outputs) out_rows += o.first;
    for (auto& o : outputs_dev) out_rows += o.first;
    metrics["output_rows"] = out_rows;
    metrics["elapsed_compute_ns"] =
        std::chrono::duration_cast<std::chrono::nanoseconds>(
            std::chrono::steady_clock::now() - t0)
            .count();
  }

  void feed(size_t idx, DevBatch&& b) {
    while (idx < stages_.size()) {
      Stage& st = stages_[idx];
      switch (st.kind) {
        case Stage::AggS:
          st.agg->consume(std::move(b));
          return;
        case Stage::ShuffleS:
          st.shuffle->consume(std::move(b));
          return;
        case Stage::FilterS:
          b = st.filter->apply(std::move(b));
          idx++;
          break;
        case Stage::ProjectS:
          b = st.project->apply(std::move(b));
          idx++;
          break;
      }
    }
    if (!terminal_transform_) FAIL("batch fed past end of chain");
    emit_host(std::move(b));
  }

  // Agg inputs that are not plain Columns (Partial mode only: a merging Agg
  // reads the accumulator column, never its argument exprs). Returns false
  // when there is nothing to lower. Otherwise *pre is the projection list —
  // each referenced Column once, then each computed expr — and *out is the
  // AggNode with every grouping expr / argument rewritten to a Column of
  // that projection. NULL-literal arguments stay as they are.
  static bool lower_agg_inputs(const AggNode& node, AggNode* out,
                               std::vector<Expr>* pre) {
    if (node.modes.empty() || node.modes[0] != AggMode::Partial) return false;
    bool any = false;
    for (const Expr& g : node.grouping_exprs) any |= g.kind != Expr::Column;
    for (const Expr& a : node.agg_exprs)
      if (!a.children.empty())
        any |= a.children[0].kind != Expr::Column &&
               a.children[0].kind != Expr::Literal;
    if (!any) return false;
    out->exec_mode = node.exec_mode;
    out->grouping_exprs = node.grouping_exprs;
    out->agg_exprs = node.agg_exprs;
    out->modes = node.modes;
    out->grouping_names = node.grouping_names;
    out->agg_names = node.agg_names;
    out->initial_input_buffer_offset = node.initial_input_buffer_offset;
    out->supports_partial_skipping = node.supports_partial_skipping;
    std::map<uint32_t, uint32_t> col_at;  // input column -> projection index
    auto rewrite = [&](Expr& e, const std::string& name) {
      if (e.kind == Expr::Literal) return;
      uint32_t at;
      if (e.kind == Expr::Column) {
        auto f = col_at.find(e.col_index);
        if (f == col_at.end()) {
          at = (uint32_t)pre->size();
          col_at[e.col_index] = at;
          pre->push_back(e);
        } else {
          at = f->second;
        }
      } else {
        at = (uint32_t)pre->size();
        pre->push_back(e);
      }
      Expr c;
      c.kind = Expr::Column;
      c.col_name = e.kind == Expr::Column ? e.col_name : name;
      c.col_index = at;
      e = std::move(c);
    };
    for (size_t i = 0; i < out->grouping_exprs.size(); i++)
      rewrite(out->grouping_exprs[i], "#group" + std::to_string(i));
    for (size_t i = 0; i < out->agg_exprs.size(); i++)
      if (!out->agg_exprs[i].children.empty())
        rewrite(out->agg_exprs[i].children[0], "#arg" + std::to_string(i));
    return true;
  }

  // terminal Filter/Projection output: download one device batch into the
  // host output queue (export buffers filled by the D2H, one sync)
  void emit_host(DevBatch&& b) {
    const int64_t n = b.num_rows;
    if (n == 0) return;
    std::vector<HostOutCol> cols(b.cols.size());
    DevBuf d_nulls(b.cols.size() * 4);
    PinnedBuf h_nulls(b.cols.size() * 4);
    AURON_HIP(hipMemsetAsync(d_nulls.get(), 0, b.cols.size() * 4, stream));
    auto d2h = [&](HostBuf* dst, const void* dev, size_t len) {
      dst->alloc(len);
      if (len == 0) return;
      AURON_HIP(hipMemcpyAsync(dst->data(), dev, len, hipMemcpyDeviceToHost,
                               stream));
      emit_d2h_bytes_ += (int64_t)len;
    };
    for (size_t i = 0; i < b.cols.size(); i++) {
      const DevColumn& c = b.cols[i];
      HostOutCol& h = cols[i];
      h.dt = c.dt;
      if (c.dt == DType::Binary || c.dt == DType::Utf8) {
        d2h(&h.offsets, c.offsets, (size_t)(n + 1) * 4);
        d2h(&h.values, c.values, (size_t)c.data_len);
      } else {
        const size_t w = dtype_width(c.dt);
        if (w == 0) FAIL("terminal output: unsupported column dtype");
        d2h(&h.values, c.values, (size_t)n * w);
      }
      if (c.validity) {
        launch_bitmap_null_count(c.validity, n, d_nulls.get<uint32_t>() + i,
                                 stream);
        d2h(&h.validity, c.validity, (size_t)(n + 7) / 8);
      }
    }
    AURON_HIP(hipMemcpyAsync(h_nulls.get(), d_nulls.get(), b.cols.size() * 4,
                             hipMemcpyDeviceToHost, stream));
    AURON_HIP(hipStreamSynchronize(stream));
    for (size_t i = 0; i < cols.size(); i++) {
      cols[i].null_count = (int64_t)h_nulls.get<uint32_t>()[i];
      if (cols[i].null_count == 0) cols[i].validity.free();
    }
    outputs.emplace_back(n, std::move(cols));
  }

  // a non-terminal Agg's staged host output, back up for the next stage
  DevBatch host_out_to_dev(
      const std::pair<int64_t, std::vector<HostOutCol>>& ob) {
    DevBatch b;
    b.num_rows = ob.first;
    for (const HostOutCol& h : ob.second) {
      const bool binary = h.dt == DType::Binary || h.dt == DType::Utf8;
      b.cols.push_back(upload_column(
          h.dt, ob.first, h.values.data(), h.values.size(),
          binary ? h.offs() : nullptr, h.validity.data(), h.validity.size(),
          stream));
    }
    // the sources are pinned, so the uploads are truly asynchronous: drain
    // them before the caller lets the buffers go back to the pool
    AURON_HIP(hipStreamSynchronize(stream));
    return b;
  }

  int32_t next_batch() {
    try {
      if (!started) {
        started = true;
        run();
      }
      if (!schema_sent && !out_fields.empty() && cb.import_schema) {
        ArrowSchema s;
        export_schema(out_fields, &s);
        cb.import_schema(cb.user, &s);
        schema_sent = true;
      }
      if (emit_dev_idx < outputs_dev.size()) {
        auto& ob = outputs_dev[emit_dev_idx++];
        // per-call export scaffolding: child arrays point at the DevBufs
        // (owned by outputs_dev until finalize); the struct itself is only
        // valid during the callback — the consumer copies the pointers out.
        std::vector<ArrowArray> children(ob.second.size());
        std::vector<ArrowArray*> child_ptrs(ob.second.size());
        std::vector<std::array<const void*, 3>> bufs(ob.second.size());
        for (size_t ci = 0; ci < ob.second.size(); ci++) {
          DevOutCol& oc = ob.second[ci];
          ArrowArray& ch = children[ci];
          memset(&ch, 0, sizeof(ch));
          ch.length = ob.first;
          ch.null_count = -1;  // unknown; validity bitmap always attached
          bufs[ci][0] = oc.validity.size() ? oc.validity.get() : nullptr;
          if (oc.dt == DType::Binary || oc.dt == DType::Utf8) {
            bufs[ci][1] = oc.offsets.get();
            bufs[ci][2] = oc.values.get();
            ch.n_buffers = 3;
            // Arrow C has no data-length field; stash it for the consumer
            ch.private_data = (void*)(intptr_t)oc.data_len;
          } else {
            bufs[ci][1] = oc.values.get();
            ch.n_buffers = 2;
          }
          ch.buffers = (const void**)bufs[ci].data();
          child_ptrs[ci] = &ch;
        }
        ArrowDeviceArray dev;
        memset(&dev, 0, sizeof(dev));
        dev.array.length = ob.first;
        dev.array.n_children = (int64_t)children.size();
        dev.array.children = child_ptrs.data();
        int did = 0;
        (void)hipGetDevice(&did);
        dev.device_id = did;
        dev.device_type = 10;  // ARROW_DEVICE_ROCM
        cb.import_device_batch(cb.user, &dev, nullptr);
        return 1;
      }
      if (emit_idx >= outputs.size()) return 0;
      auto& ob = outputs[emit_idx++];
      ArrowArray a;
      export_batch(ob.first, std::move(ob.second), &a);
      if (cb.import_batch) cb.import_batch(cb.user, &a);
      return 1;
    } catch (const std::exception& e) {
      set_error(e.what());
      return 0;
    }
  }
};

std::mutex g_mu;
std::map<int64_t, std::unique_ptr<Runtime>> g_runtimes;
int64_t g_next_handle = 1;

}  // namespace
}  // namespace auron

using namespace auron;

extern "C" {

int64_t auron_call_native(const uint8_t* task_definition, size_t len,
                          AuronCallbacks* callbacks) {
  auto rt = std::make_unique<Runtime>();
  if (callbacks) rt->cb = *callbacks;
  try {
    DBG("call_native len=%zu", len);
    int ndev = 0;
    hip_check(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
    if (ndev == 0) throw EngineError("no HIP device visible");
    AURON_HIP(hipStreamCreate(&rt->stream));
    std::string err;
    rt->td = decode_task_definition(task_definition, len, &err);
    if (!rt->td) throw EngineError("plan decode failed: " + err);
    DBG("call_native ready");
  } catch (const std::exception& e) {
    rt->set_error(e.what());
    return 0;
  }
  std::lock_guard<std::mutex> lk(g_mu);
  int64_t h = g_next_handle++;
  g_runtimes[h] = std::move(rt);
  return h;
}

int32_t auron_next_batch(int64_t handle) {
  Runtime* rt;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_runtimes.find(handle);
    if (it == g_runtimes.end()) return 0;
    rt = it->second.get();
  }
  return rt->next_batch();
}

void auron_finalize(int64_t handle) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_runtimes.erase(handle);
}

void auron_on_exit(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_runtimes.clear();
  DevPool::inst().clear([](void* p) { (void)hipFree(p); });
}

const char* auron_version(void) { return "auron-hip 0.1 gfx950"; }

// Compute murmur3(seed 42) + pmod partition ids for host-resident i64 keys on
// the GPU (shuffle/mod.rs:163-188). Used by bench.py's RCCL exchange leg to
// route partial-agg records to their owner rank. Returns 0 on success.
int32_t auron_partition_ids(const int64_t* keys, int64_t n, int32_t P,
                            uint32_t* out) {
  try {
    // cached stream + pinned staging: this helper runs once per bench step
    // and pageable H2D/D2H of the ~1M-group arrays costs milliseconds
    static hipStream_t s = nullptr;
    static PinnedBuf pin_in, pin_out;
    if (!s) AURON_HIP(hipStreamCreate(&s));
    if (pin_in.size() < (size_t)n * 8) {
      pin_in.alloc(n * 8);
      pin_out.alloc(n * 4);
    }
    memcpy(pin_in.get(), keys, n * 8);
    DevBuf d_keys(n * 8), d_hash(n * 4), d_out(n * 4);
    AURON_HIP(hipMemcpyAsync(d_keys.get(), pin_in.get(), n * 8,
                             hipMemcpyHostToDevice, s));
    launch_hash_init(d_hash.get<int32_t>(), 42, n, s);
    launch_hash_fold_i64(d_keys.get<int64_t>(), nullptr, n,
                         d_hash.get<int32_t>(), s);
    launch_pmod(d_hash.get<int32_t>(), n, P, d_out.get<uint32_t>(), s);
    AURON_HIP(hipMemcpyAsync(pin_out.get(), d_out.get(), n * 4,
                             hipMemcpyDeviceToHost, s));
    AURON_HIP(hipStreamSynchronize(s));
    memcpy(out, pin_out.get(), n * 4);
    return 0;
  } catch (const std::exception&) {
    return -1;
  }
}

// ---- device repartition (in-memory exchange prep) --------------------------
// The multi-GPU exchange analog of sort_batches_by_partition_id +
// create_batch_interleaver (buffered_data.rs:284-351, selection.rs:65-300):
// murmur3(seed 42) partition ids -> stable sort by (dest rank = pid % world,
// pid) -> gather the (key, a8 accbuf) records into dest-rank-major,
// partition-ordered layout entirely in HBM, returning the per-rank row/byte
// splits the RCCL all-to-all needs. Input/output pointers are device memory;
// output buffers are owned by the returned handle until
// auron_repartition_free.
namespace auron {
namespace {
struct RepartOut {
  DevBuf keys, kvalid, offsets, data;
  hipStream_t stream = nullptr;
};
std::mutex g_rp_mu;
std::map<int64_t, std::unique_ptr<RepartOut>> g_repart;
int64_t g_rp_next = 1;
}  // namespace
}  // namespace auron

extern "C" {

int64_t auron_repartition_device(int64_t n, const void* keys,
                                 const void* key_validity,
                                 const void* offsets, const void* data,
                                 int32_t num_partitions, int32_t world,
                                 const void** out_keys,
                                 const void** out_key_validity,
                                 const void** out_offsets,
                                 const void** out_data,
                                 int64_t* rank_rows, int64_t* rank_bytes) {
  try {
    if (n <= 0 || num_partitions <= 0 || world <= 0 || world > 64) return 0;
    auto rp = std::make_unique<RepartOut>();
    AURON_HIP(hipStreamCreate(&rp->stream));
    hipStream_t s = rp->stream;
    DevBuf hash(n * 4), pids(n * 4), ord(n * 4), ord_sorted(n * 4);
    DevBuf idx(n * 4), perm(n * 4), counts(world * 16);
    launch_hash_init(hash.get<int32_t>(), 42, n, s);
    launch_hash_fold_i64((const int64_t*)keys, nullptr, n, hash.get<int32_t>(),
                         s);
    launch_pmod(hash.get<int32_t>(), n, num_partitions, pids.get<uint32_t>(),
                s);
    launch_exchange_ord(pids.get<uint32_t>(), n, (uint32_t)num_partitions,
                        (uint32_t)world, ord.get<uint32_t>(), s);
    AURON_HIP(hipMemsetAsync(counts.get(), 0, world * 16, s));
    launch_dest_counts(pids.get<uint32_t>(), (const int32_t*)offsets, n,
                       (uint32_t)world, counts.get<unsigned long long>(),
                       counts.get<unsigned long long>() + world, s);
    launch_iota_u32(idx.get<uint32_t>(), n, s);
    // ord < world * P: sort only the live bits
    int end_bit = 1;
    while ((1u << end_bit) < (uint32_t)world * (uint32_t)num_partitions &&
           end_bit < 32)
      end_bit++;
    size_t tb = 0;
    sort_pairs_u32_u32(ord.get<uint32_t>(), idx.get<uint32_t>(),
                       ord_sorted.get<uint32_t>(), perm.get<uint32_t>(), n,
                       end_bit, nullptr, &tb, s);
    DevBuf tmp(tb);
    sort_pairs_u32_u32(ord.get<uint32_t>(), idx.get<uint32_t>(),
                       ord_sorted.get<uint32_t>(), perm.get<uint32_t>(), n,
                       end_bit, tmp.get(), &tb, s);
    rp->keys.alloc(n * 8);
    launch_gather_8((const uint8_t*)keys, perm.get<uint32_t>(), n,
                    rp->keys.get<uint8_t>(), s);
    if (key_validity) {
      rp->kvalid.alloc((n + 7) / 8);
      launch_gather_bits((const uint8_t*)key_validity, perm.get<uint32_t>(), n,
                         rp->kvalid.get<uint8_t>(), s);
    }
    if (offsets && data) {
      DevBuf lens((n + 1) * 4);
      rp->offsets.alloc((n + 1) * 4);
      launch_gather_lens((const int32_t*)offsets, perm.get<uint32_t>(), n,
                         lens.get<int32_t>(), s);
      size_t stb = 0;
      scan_counts_matrix(lens.get<uint32_t>(), rp->offsets.get<uint32_t>(),
                         n + 1, nullptr, &stb, s);
      DevBuf stmp(stb);
      scan_counts_matrix(lens.get<uint32_t>(), rp->offsets.get<uint32_t>(),
                         n + 1, stmp.get(), &stb, s);
      PinnedBuf pin;
      pin.alloc(16);
      AURON_HIP(hipMemcpyAsync(pin.get(), rp->offsets.get<uint32_t>() + n, 4,
                               hipMemcpyDeviceToHost, s));
      AURON_HIP(hipStreamSynchronize(s));
      int64_t total = (int64_t)*pin.get<uint32_t>();
      rp->data.alloc(total ? total : 1);
      launch_gather_bytes((const uint8_t*)data, (const int32_t*)offsets,
                          perm.get<uint32_t>(), rp->offsets.get<int32_t>(), n,
                          rp->data.get<uint8_t>(), s);
    }
    std::vector<unsigned long long> h_counts(world * 2);
    AURON_HIP(hipMemcpyAsync(h_counts.data(), counts.get(), world * 16,
                             hipMemcpyDeviceToHost, s));
    AURON_HIP(hipStreamSynchronize(s));
    for (int32_t w = 0; w < world; w++) {
      if (rank_rows) rank_rows[w] = (int64_t)h_counts[w];
      if (rank_bytes) rank_bytes[w] = (int64_t)h_counts[world + w];
    }
    if (out_keys) *out_keys = rp->keys.get();
    if (out_key_validity)
      *out_key_validity = key_validity ? rp->kvalid.get() : nullptr;
    if (out_offsets) *out_offsets = rp->offsets.get();
    if (out_data) *out_data = rp->data.get();
    std::lock_guard<std::mutex> lk(g_rp_mu);
    int64_t h = g_rp_next++;
    g_repart[h] = std::move(rp);
    return h;
  } catch (const std::exception&) {
    return 0;
  }
}

void auron_repartition_free(int64_t handle) {
  std::lock_guard<std::mutex> lk(g_rp_mu);
  auto it = g_repart.find(handle);
  if (it != g_repart.end()) {
    if (it->second->stream) {
      (void)hipStreamSynchronize(it->second->stream);
      (void)hipStreamDestroy(it->second->stream);
    }
    g_repart.erase(it);
  }
}

}  // extern "C"

int64_t auron_get_metric(int64_t handle, const char* name) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_runtimes.find(handle);
  if (it == g_runtimes.end()) return -1;
  auto mit = it->second->metrics.find(name);
  return mit == it->second->metrics.end() ? -1 : mit->second;
}

}  // extern "C"
