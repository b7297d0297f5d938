// emit.h — output staging shared by AggOp (agg.cpp) and the Runtime
// (engine.cpp): the output schema field, the host and device column staging
// types, and HostEmit, the one mechanism that downloads an output batch into
// its export buffers.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "batch.h"

namespace auron {

struct OutField {
  std::string name;
  DType dt;        // list fields: the ITEM type
  bool nullable;
  bool is_list = false;  // Arrow list<dt> (COLLECT output)
};

// host-side column staging for export
struct HostOutCol {
  DType dt;            // list cols: the ITEM type
  HostBuf values;      // list cols: child (item) values
  HostBuf validity;    // empty = no nulls
  HostBuf offsets;     // binary / list: (n+1) int32
  int64_t null_count = 0;  // exact; validity is attached only when > 0
  bool is_list = false;
  // emit bookkeeping, resolved at the batch's one sync (HostEmit::end): the
  // device null counter that belongs to `validity`, and the column of the
  // same batch whose values(+offsets) / validity this one duplicates
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

// one output batch: (rows, columns)
using HostOutBatch = std::pair<int64_t, std::vector<HostOutCol>>;
using DevOutBatch = std::pair<int64_t, std::vector<DevOutCol>>;

// Host emit of one output batch on `stream`: begin(), any number of d2h() /
// col_validity() enqueues straight into the columns' own export buffers,
// end(): the batch's ONE stream sync, after which the device null counters
// decide which bitmaps stay attached. d2h_bytes counts the column payload
// (values, bitmaps, offsets) copied down; the 4-byte counters are not
// payload.
struct HostEmit {
  static constexpr int NULL_SLOTS = 256;

  hipStream_t stream = nullptr;
  int64_t d2h_bytes = 0, host_copy_bytes = 0;

  void begin() {
    if (!d_nulls_) {
      d_nulls_.alloc(NULL_SLOTS * 4);
      pinned_nulls_.alloc(NULL_SLOTS * 4);
    }
    AURON_HIP(hipMemsetAsync(d_nulls_.get(), 0, NULL_SLOTS * 4, stream));
    null_used_ = 0;
  }

  // reserve k consecutive device null counters; returns the first index
  int null_slots(int k) {
    if (null_used_ + k > NULL_SLOTS)
      FAIL("too many nullable output columns in one batch");
    int at = null_used_;
    null_used_ += k;
    return at;
  }
  uint32_t* null_ctr(int slot) { return d_nulls_.get<uint32_t>() + slot; }

  // enqueue dev -> a fresh export buffer (no sync)
  void d2h(HostBuf* dst, const void* dev, size_t len) {
    dst->alloc(len);
    if (len == 0) return;
    AURON_HIP(hipMemcpyAsync(dst->data(), dev, len, hipMemcpyDeviceToHost,
                             stream));
    d2h_bytes += (int64_t)len;
  }

  // bitmap of n rows whose nulls a kernel adds to counter `slot`
  void col_validity(HostOutCol* col, const void* dev_bm, int64_t n, int slot) {
    d2h(&col->validity, dev_bm, (size_t)(n + 7) / 8);
    col->null_slot = slot;
  }

  // D2H sources live until the batch's sync: the device pool hands a freed
  // buffer to whoever asks next and does not synchronize
  void keep(DevBuf&& b) { keep_.push_back(std::move(b)); }

  void sync() {
    AURON_HIP(hipStreamSynchronize(stream));
    keep_.clear();
  }

  // The one sync of an output batch. Keeps the rule of the Arrow null_count
  // convention (and batch_serde's has_null header): validity is attached only
  // when nulls exist. Columns that duplicate another column's source are
  // cloned here, the only host copy of the emit path.
  void end(std::vector<HostOutCol>* cols) {
    uint32_t* h_nulls = pinned_nulls_.get<uint32_t>();
    if (null_used_)
      AURON_HIP(hipMemcpyAsync(h_nulls, d_nulls_.get(), (size_t)null_used_ * 4,
                               hipMemcpyDeviceToHost, stream));
    sync();
    for (HostOutCol& c : *cols) {
      if (c.null_slot < 0) continue;
      c.null_count = (int64_t)h_nulls[c.null_slot];
      if (c.null_count == 0) c.validity.free();
      c.null_slot = -1;
    }
    for (HostOutCol& c : *cols) {
      if (c.values_from >= 0) {
        const HostOutCol& src = (*cols)[c.values_from];
        c.values = src.values.clone(&host_copy_bytes);
        c.offsets = src.offsets.clone(&host_copy_bytes);
        c.values_from = -1;
      }
      if (c.validity_from >= 0) {
        const HostOutCol& src = (*cols)[c.validity_from];
        c.validity = src.validity.clone(&host_copy_bytes);
        c.null_count = src.null_count;
        c.validity_from = -1;
      }
    }
  }

 private:
  DevBuf d_nulls_;
  PinnedBuf pinned_nulls_;
  int null_used_ = 0;
  std::vector<DevBuf> keep_;
};

}  // namespace auron
