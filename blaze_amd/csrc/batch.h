// batch.h — what the engine's translation units share: the error and trace
// plumbing, the device batch, the conf reader, and the batch sources of
// sources.cpp with the helpers that more than one file uses.
#pragma once

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/auron_hip.h"
#include "dev.h"
#include "plan.h"

namespace auron {

struct EngineError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// AURON_DEBUG=1 traces engine stages (with ms timestamps) to stderr
inline bool debug_on() {
  static bool v = getenv("AURON_DEBUG") != nullptr;
  return v;
}
inline double dbg_ms() {
  static auto t0 = std::chrono::steady_clock::now();
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now() - t0)
      .count();
}
#define DBG(...)                                             \
  do {                                                       \
    if (::auron::debug_on()) {                               \
      fprintf(stderr, "[auron %9.2f] ", ::auron::dbg_ms());  \
      fprintf(stderr, __VA_ARGS__);                          \
      fprintf(stderr, "\n");                                 \
      fflush(stderr);                                        \
    }                                                        \
  } while (0)

#define FAIL(msg) throw ::auron::EngineError(msg)

// ---------------------------------------------------------------- columns --
struct DevColumn {
  DType dt = DType::Unsupported;
  int64_t len = 0;
  // non-owning views (point into own_* when owned)
  const void* values = nullptr;       // prim: len*w; binary: data bytes
  const uint8_t* validity = nullptr;  // LSB bitmap or null
  const int32_t* offsets = nullptr;   // binary: len+1
  int64_t data_len = 0;               // binary data bytes
  DevBuf own_values, own_validity, own_offsets;
};

struct DevBatch {
  int64_t num_rows = 0;
  std::vector<DevColumn> cols;
};

// ------------------------------------------------------------------- conf --
struct Conf {
  AuronCallbacks* cb;
  std::string get(const char* key, const std::string& dflt) const {
    char buf[256];
    buf[0] = '\0';
    if (cb && cb->get_conf &&
        cb->get_conf(cb->user, key, buf, sizeof(buf)) == 0 && buf[0] != '\0')
      return std::string(buf);
    return dflt;
  }
  int64_t get_i(const char* key, int64_t dflt) const {
    std::string v = get(key, "");
    return v.empty() ? dflt : (int64_t)strtoll(v.c_str(), nullptr, 10);
  }
  double get_d(const char* key, double dflt) const {
    std::string v = get(key, "");
    return v.empty() ? dflt : strtod(v.c_str(), nullptr);
  }
};

// ---------------------------------------------------------------- helpers --
// Host column -> owned DevColumn with its views aimed. `offsets` (rows+1
// int32) marks a binary column, whose data_len is values_len — a binary
// column needs non-null offsets even at 0 rows, a null pointer makes the
// column fixed-width; validity is
// uploaded when it is non-null and validity_len > 0. An empty values buffer
// still gets a 1-byte allocation so the view is never null. Every buffer
// goes through PinnedUploader; nothing here synchronises — the caller drains
// the stream before the host buffers die.
DevColumn upload_column(DType dt, int64_t rows, const void* values,
                        size_t values_len, const int32_t* offsets,
                        const uint8_t* validity, size_t validity_len,
                        hipStream_t stream);

// positions[0..n] = exclusive scan of the byte mask (positions[n] = number of
// set rows). `tmp` is the caller's grow-only scan scratch.
void scan_mask_positions(const uint8_t* mask, int64_t n, uint32_t* positions,
                         DevBuf* tmp, hipStream_t stream);

// Device lens -> offsets: offsets[0..n] = exclusive scan of lens[0..n), the
// total in slot n. Both buffers have n+1 slots (slot n of lens is only read).
// `tmp` is the caller's grow-only scan scratch, `pinned_total` a pinned
// 4-byte landing slot. Returns the total after its one stream sync.
int64_t scan_lens_offsets(const uint32_t* lens, int64_t n, uint32_t* offsets,
                          DevBuf* tmp, uint32_t* pinned_total,
                          hipStream_t stream);

// The stable radix sorts of kernels.h (only key bits [0, end_bit) compared)
// with the scratch-size query done here; `tmp` is grow-only and may be
// reused across calls on one stream.
void sort_pairs(const uint32_t* keys_in, const uint32_t* vals_in,
                uint32_t* keys_out, uint32_t* vals_out, int64_t n, int end_bit,
                DevBuf* tmp, hipStream_t stream);
void sort_pairs(const unsigned long long* keys_in, const uint32_t* vals_in,
                unsigned long long* keys_out, uint32_t* vals_out, int64_t n,
                int end_bit, DevBuf* tmp, hipStream_t stream);

// Variable-width output layout: device lens[n] (int32) -> host exclusive scan
// -> the n+1 offsets in the caller's offs[], uploaded to d_offs (the caller
// keeps offs alive until its next sync: it is the source of the upload).
// Arrow offsets are int32, so a total past INT32_MAX fails instead of
// wrapping.
void lens_to_offsets_into(const void* d_lens, int64_t n, int32_t* offs,
                          int32_t* d_offs, hipStream_t stream);
std::vector<int32_t> lens_to_offsets(const void* d_lens, int64_t n,
                                     int32_t* d_offs, hipStream_t stream);

// Rows sel[0..m) of column c as an owned column (validity carried when c has
// one); binary offsets are scanned on the host (lens_to_offsets), which
// syncs the stream once. A non-null host_offsets receives that host copy of
// the m+1 offsets. 4/8-byte primitives and Binary/Utf8 only.
DevColumn gather_column(const DevColumn& c, const uint32_t* sel, int64_t m,
                        hipStream_t stream,
                        std::vector<int32_t>* host_offsets = nullptr);

// ---------------------------------------------------------------- sources --
// Each source pushes its batches into `sink` and returns the input row count.
using BatchSink = std::function<void(DevBatch&&)>;

// ParquetScanExec: footer/pages on host, page decompression, validity and
// dictionary expansion on the GPU; one batch per surviving row group.
int64_t scan_parquet(const ParquetScanNode& node, hipStream_t stream,
                     const BatchSink& sink);

// IpcReaderExec: shuffle block streams from cb.next_ipc_bytes, decoded and
// deserialized on host (codec: 0 lz4, 1 zstd), one batch per serde batch.
int64_t read_ipc(const IpcReaderNode& reader, const AuronCallbacks& cb,
                 int codec, hipStream_t stream, const BatchSink& sink);

}  // namespace auron
