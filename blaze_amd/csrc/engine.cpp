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
// This file holds the Arrow import/export, the Shuffle / Filter / Projection
// operators and the Runtime that drives the operator chain. AggOp is in
// agg.cpp (agg.h), the output staging it shares with the Runtime in emit.h.
// The batch sources (ParquetScanExec, IpcReaderExec) are in sources.cpp, the
// types and helpers they share with this file in batch.h, the host-only
// auron_debug_* entry points in debug_abi.cpp.
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

#include "agg.h"
#include "batch.h"
#include "emit.h"
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
    DevBuf tmp;
    sort_pairs(part_ids.get<uint32_t>(), iota.get<uint32_t>(),
               keys_out.get<uint32_t>(), perm.get<uint32_t>(), n, end_bit,
               &tmp, stream_);
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
      const bool binary =
          all.cols[c].dt == DType::Binary || all.cols[c].dt == DType::Utf8;
      // the gathered buffers go back to the pool at the end of the iteration;
      // every later use of them is on this stream, behind the downloads
      DevColumn g = gather_column(all.cols[c], perm.get<uint32_t>(), n, stream_,
                                  binary ? &h_offsets[c] : nullptr);
      h_values[c].resize(binary ? (size_t)g.data_len
                                : (size_t)n * dtype_width(g.dt));
      AURON_HIP(hipMemcpyAsync(h_values[c].data(), g.values,
                               h_values[c].size(), hipMemcpyDeviceToHost,
                               stream_));
      if (binary) {
        AURON_HIP(hipStreamSynchronize(stream_));
        cols[c].offsets = h_offsets[c].data();
      }
      cols[c].byte_width = binary ? 0 : (int)dtype_width(g.dt);
      cols[c].values = h_values[c].data();
      if (g.validity) {
        h_validity[c].resize((n + 7) / 8);
        AURON_HIP(hipMemcpyAsync(h_validity[c].data(), g.validity,
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
      out.cols.push_back(gather_column(c, sel.get<uint32_t>(), m, stream_));
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
  std::vector<HostOutBatch> outputs;
  HostEmit emit_;  // terminal Filter/Projection downloads
  size_t emit_idx = 0;
  // device-resident outputs (AURON_HIP_DEVICE_OUTPUT): exported through
  // import_device_batch; DevBufs stay owned here until finalize
  std::vector<DevOutBatch> outputs_dev;
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
    emit_.stream = stream;
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
        if (st.agg->device_out()) {
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
      metrics["agg_update_ns"] = first_agg->metrics().update_ns;
      metrics["agg_update_rows"] = first_agg->metrics().update_rows;
      metrics["spill_count"] = first_agg->metrics().spill_count +
                               last_agg->metrics().spill_count;
    }
    // host-emit accounting: payload bytes copied down into export buffers,
    // and payload bytes moved again by a host memcpy on the way out
    int64_t d2h_bytes = emit_.d2h_bytes;
    int64_t host_copy_bytes = emit_.host_copy_bytes;
    for (Stage& st : stages_)
      if (st.kind == Stage::AggS) {
        d2h_bytes += st.agg->metrics().emit_d2h_bytes;
        host_copy_bytes += st.agg->metrics().emit_host_copy_bytes;
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
  // host output queue (export buffers filled by the D2H, one sync). An input
  // bitmap passes through: counted, not rebuilt.
  void emit_host(DevBatch&& b) {
    const int64_t n = b.num_rows;
    if (n == 0) return;
    std::vector<HostOutCol> cols(b.cols.size());
    emit_.begin();
    for (size_t i = 0; i < b.cols.size(); i++) {
      const DevColumn& c = b.cols[i];
      HostOutCol& h = cols[i];
      h.dt = c.dt;
      if (c.dt == DType::Binary || c.dt == DType::Utf8) {
        emit_.d2h(&h.offsets, c.offsets, (size_t)(n + 1) * 4);
        emit_.d2h(&h.values, c.values, (size_t)c.data_len);
      } else {
        const size_t w = dtype_width(c.dt);
        if (w == 0) FAIL("terminal output: unsupported column dtype");
        emit_.d2h(&h.values, c.values, (size_t)n * w);
      }
      if (c.validity) {
        const int slot = emit_.null_slots(1);
        launch_bitmap_null_count(c.validity, n, emit_.null_ctr(slot), stream);
        emit_.col_validity(&h, c.validity, n, slot);
      }
    }
    emit_.end(&cols);
    outputs.emplace_back(n, std::move(cols));
  }

  // a non-terminal Agg's staged host output, back up for the next stage
  DevBatch host_out_to_dev(const HostOutBatch& ob) {
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
    DevBuf tmp;
    sort_pairs(ord.get<uint32_t>(), idx.get<uint32_t>(),
               ord_sorted.get<uint32_t>(), perm.get<uint32_t>(), n, end_bit,
               &tmp, s);
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
      DevBuf stmp;
      PinnedBuf pin(16);
      int64_t total =
          scan_lens_offsets(lens.get<uint32_t>(), n,
                            rp->offsets.get<uint32_t>(), &stmp,
                            pin.get<uint32_t>(), s);
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
