// sources.cpp — the batch sources behind the operator chain (batch.h): the
// ParquetScanExec scan and the IpcReaderExec reader, and the helpers of
// batch.h that more than one file uses: column upload and gather, the
// one-call scans and sorts.
#include <algorithm>
#include <atomic>
#include <future>
#include <mutex>
#include <thread>

#include "batch.h"
#include "ipc_scalar.h"
#include "kernels.h"
#include "parquet.h"
#include "serde_host.h"

namespace auron {

DevColumn upload_column(DType dt, int64_t rows, const void* values,
                        size_t values_len, const int32_t* offsets,
                        const uint8_t* validity, size_t validity_len,
                        hipStream_t stream) {
  PinnedUploader& up = PinnedUploader::inst();
  DevColumn c;
  c.dt = dt;
  c.len = rows;
  if (offsets) {
    c.own_offsets.alloc((rows + 1) * 4);
    up.copy(c.own_offsets.get(), offsets, (rows + 1) * 4, stream);
    c.offsets = c.own_offsets.get<int32_t>();
    c.data_len = (int64_t)values_len;
  }
  c.own_values.alloc(values_len ? values_len : 1);
  up.copy(c.own_values.get(), values, values_len, stream);
  c.values = c.own_values.get();
  if (validity && validity_len) {
    c.own_validity.alloc(validity_len);
    up.copy(c.own_validity.get(), validity, validity_len, stream);
    c.validity = c.own_validity.get<uint8_t>();
  }
  return c;
}

void scan_mask_positions(const uint8_t* mask, int64_t n, uint32_t* positions,
                         DevBuf* tmp, hipStream_t stream) {
  size_t tb = 0;
  scan_mask_u8(mask, positions, n, nullptr, &tb, stream);
  if (tb > tmp->size()) tmp->alloc(tb);
  scan_mask_u8(mask, positions, n, tmp->get(), &tb, stream);
}

int64_t scan_lens_offsets(const uint32_t* lens, int64_t n, uint32_t* offsets,
                          DevBuf* tmp, uint32_t* pinned_total,
                          hipStream_t stream) {
  size_t tb = 0;
  scan_counts_matrix(lens, offsets, n + 1, nullptr, &tb, stream);
  if (tb > tmp->size()) tmp->alloc(tb);
  scan_counts_matrix(lens, offsets, n + 1, tmp->get(), &tb, stream);
  AURON_HIP(hipMemcpyAsync(pinned_total, offsets + n, 4, hipMemcpyDeviceToHost,
                           stream));
  AURON_HIP(hipStreamSynchronize(stream));
  return (int64_t)*pinned_total;
}

void sort_pairs(const uint32_t* keys_in, const uint32_t* vals_in,
                uint32_t* keys_out, uint32_t* vals_out, int64_t n, int end_bit,
                DevBuf* tmp, hipStream_t stream) {
  size_t tb = 0;
  sort_pairs_u32_u32(keys_in, vals_in, keys_out, vals_out, n, end_bit, nullptr,
                     &tb, stream);
  if (tb > tmp->size()) tmp->alloc(tb);
  sort_pairs_u32_u32(keys_in, vals_in, keys_out, vals_out, n, end_bit,
                     tmp->get(), &tb, stream);
}

void sort_pairs(const unsigned long long* keys_in, const uint32_t* vals_in,
                unsigned long long* keys_out, uint32_t* vals_out, int64_t n,
                int end_bit, DevBuf* tmp, hipStream_t stream) {
  size_t tb = 0;
  sort_pairs_u64_u32(keys_in, vals_in, keys_out, vals_out, n, nullptr, &tb,
                     stream, end_bit);
  if (tb > tmp->size()) tmp->alloc(tb);
  sort_pairs_u64_u32(keys_in, vals_in, keys_out, vals_out, n, tmp->get(), &tb,
                     stream, end_bit);
}

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

DevColumn gather_column(const DevColumn& c, const uint32_t* sel, int64_t m,
                        hipStream_t stream,
                        std::vector<int32_t>* host_offsets) {
  DevColumn out;
  out.dt = c.dt;
  out.len = m;
  size_t w = dtype_width(c.dt);
  if (c.dt == DType::Binary || c.dt == DType::Utf8) {
    DevBuf lens(m * 4);
    launch_gather_lens(c.offsets, sel, m, lens.get<int32_t>(), stream);
    out.own_offsets.alloc((m + 1) * 4);
    std::vector<int32_t> h_offs = lens_to_offsets(
        lens.get(), m, out.own_offsets.get<int32_t>(), stream);
    out.offsets = out.own_offsets.get<int32_t>();
    out.data_len = h_offs[m];
    out.own_values.alloc(out.data_len ? out.data_len : 1);
    launch_gather_bytes((const uint8_t*)c.values, c.offsets, sel,
                        out.own_offsets.get<int32_t>(), m,
                        out.own_values.get<uint8_t>(), stream);
    if (host_offsets) *host_offsets = std::move(h_offs);
  } else if (w == 8) {
    out.own_values.alloc(m * 8);
    launch_gather_8((const uint8_t*)c.values, sel, m,
                    out.own_values.get<uint8_t>(), stream);
  } else if (w == 4) {
    out.own_values.alloc(m * 4);
    launch_gather_4((const uint8_t*)c.values, sel, m,
                    out.own_values.get<uint8_t>(), stream);
  } else {
    FAIL("column gather supports Binary/Utf8 and 4/8-byte primitives");
  }
  out.values = out.own_values.get();
  if (c.validity) {
    out.own_validity.alloc((m + 7) / 8);
    launch_gather_bits(c.validity, sel, m, out.own_validity.get<uint8_t>(),
                       stream);
    out.validity = out.own_validity.get<uint8_t>();
  }
  return out;
}

namespace {

// ---------------------------------------------------------- parquet scan --
// Evaluate a Column-vs-Literal pruning predicate against row-group stats:
// returns false only when the predicate PROVABLY excludes every row
// (parquet_exec.rs row-group stats pruning analog; conservative on any
// unsupported shape).
bool rg_may_match(const Expr& e, const ParquetFile& pf, int rg) {
  if (e.kind != Expr::BinaryExpr || e.children.size() != 2) return true;
  if (e.op == "And")
    return rg_may_match(e.children[0], pf, rg) &&
           rg_may_match(e.children[1], pf, rg);
  const Expr* col = nullptr;
  const Expr* lit = nullptr;
  bool flipped = false;
  if (e.children[0].kind == Expr::Column &&
      e.children[1].kind == Expr::Literal) {
    col = &e.children[0];
    lit = &e.children[1];
  } else if (e.children[1].kind == Expr::Column &&
             e.children[0].kind == Expr::Literal) {
    col = &e.children[1];
    lit = &e.children[0];
    flipped = true;
  } else {
    return true;
  }
  if (col->col_index >= pf.columns().size()) return true;
  PqColStats s = pf.column_stats(rg, (int)col->col_index);
  if (!s.has_minmax) return true;
  ScalarLit sl;
  std::string err2;
  if (!decode_ipc_scalar(lit->literal_ipc.data(), lit->literal_ipc.size(),
                         &sl, &err2) ||
      sl.is_null)
    return true;
  std::string op = e.op;
  if (flipped) {
    op = op == "Lt" ? "Gt" : op == "LtEq" ? "GtEq"
         : op == "Gt" ? "Lt" : op == "GtEq" ? "LtEq" : op;
  }
  int pt = pf.columns()[col->col_index].physical_type;
  if (pt == 1 || pt == 2) {
    // compare in the int64 domain: a round-trip through double loses
    // precision past 2^53 and could prune a row group that matches
    int64_t lo = s.min_i, hi = s.max_i, v = sl.i64;
    if (op == "Lt") return lo < v;
    if (op == "LtEq") return lo <= v;
    if (op == "Gt") return hi > v;
    if (op == "GtEq") return hi >= v;
    if (op == "Eq") return lo <= v && v <= hi;
    return true;
  }
  if (pt != 4 && pt != 5) return true;
  double lo = s.min_f, hi = s.max_f, v = sl.f64;
  if (op == "Lt") return lo < v;
  if (op == "LtEq") return lo <= v;
  if (op == "Gt") return hi > v;
  if (op == "GtEq") return hi >= v;
  if (op == "Eq") return lo <= v && v <= hi;
  return true;
}

// Host decode of chunks [jlo, jhi) of the row-group-major `decoded` array on
// up to 48 threads; the first failure lands in *err.
void decode_chunks(const ParquetFile& pf, const std::vector<uint32_t>& proj,
                   std::vector<PqColumnChunkData>* decoded, size_t jlo,
                   size_t jhi, std::string* err, std::mutex* err_mu) {
  const size_t width = proj.size();
  std::atomic<size_t> next{jlo};
  auto worker = [&]() {
    for (;;) {
      size_t i = next.fetch_add(1);
      if (i >= jhi) break;
      try {
        (*decoded)[i] = pf.read_chunk((int)(i / width), (int)proj[i % width]);
      } catch (const std::exception& ex) {
        std::lock_guard<std::mutex> lk(*err_mu);
        if (err->empty()) *err = ex.what();
      }
    }
  };
  unsigned nw = std::min<unsigned>(
      std::min(48u, std::max(1u, std::thread::hardware_concurrency())),
      (unsigned)(jhi - jlo));
  std::vector<std::thread> ws;
  for (unsigned w = 0; w < nw; w++) ws.emplace_back(worker);
  for (auto& w : ws) w.join();
}

// Result of the device page decompression of one window: two blobs
// (validity bitmaps / dense non-null values) that stay resident while the
// window's row groups are assembled, and where each gpu_comp chunk's share
// of them lies.
struct GcWindow {
  struct Chunk {
    uint64_t valid_base = 0, dense_base = 0;
    int64_t total_nn = 0, null_total = 0;
    bool ready = false;
  };
  DevBuf valid, dense;
  std::vector<Chunk> chunks;  // one per chunk of the window
};

// GPU page decompression (kernels_pq.hip): every gpu_comp chunk's
// PLAIN-suffix pages across ALL row groups of the window go into ONE
// wave-per-page decompress+decode launch set (per-chunk launches would leave
// the chip nearly idle: ~30 pages per chunk).
GcWindow decompress_window(const PqColumnChunkData* chunks, size_t nchunks,
                           hipStream_t stream) {
  GcWindow win;
  win.chunks.resize(nchunks);
  std::vector<PqGpuPage> pages;
  std::vector<PqGpuChunk> chmeta;
  std::vector<size_t> ch_di;
  uint64_t comp_total = 0, scratch_total = 0, valid_total = 0,
           dense_total = 0;
  auto al8 = [](uint64_t v) { return (v + 7) & ~7ull; };
  for (size_t di = 0; di < nchunks; di++) {
    const PqColumnChunkData& cd = chunks[di];
    if (!cd.gpu_comp) continue;
    const int vw = cd.value_width;
    int64_t values = cd.prefix_values + cd.suffix_values;
    PqGpuChunk ch;
    ch.page0 = (uint32_t)pages.size();
    ch.npages = (uint32_t)cd.comp_pages.size();
    ch.valid_base = valid_total;
    ch.dense_base = dense_total;
    ch.prefix_nn = (uint32_t)(cd.plain.size() / (size_t)vw);
    ch.vw = (uint32_t)vw;
    uint32_t vbase = (uint32_t)cd.prefix_values;
    for (const auto& pg : cd.comp_pages) {
      PqGpuPage p;
      p.comp_off = comp_total + (uint64_t)(pg.src - cd.comp_pages[0].src);
      p.uncomp_off = scratch_total;
      p.comp_len = pg.comp_len;
      p.uncomp_len = pg.uncomp_len;
      p.num_values = pg.num_values;
      p.value_base = vbase;
      p.has_def = cd.nullable ? 1u : 0u;
      p.chunk_id = (uint32_t)chmeta.size();
      pages.push_back(p);
      vbase += pg.num_values;
      scratch_total += al8(pg.uncomp_len);
    }
    const auto& lastp = cd.comp_pages.back();
    comp_total += al8((uint64_t)(lastp.src - cd.comp_pages[0].src) +
                      lastp.comp_len);
    valid_total += al8(((uint64_t)values + 7) / 8);
    dense_total += al8((uint64_t)values * vw);
    chmeta.push_back(ch);
    ch_di.push_back(di);
  }
  if (pages.empty()) return win;

  PinnedUploader& up = PinnedUploader::inst();
  DevBuf d_comp(comp_total), d_scratch(scratch_total);
  win.valid.alloc(valid_total ? valid_total : 8);
  win.dense.alloc(dense_total);
  DevBuf d_pages(pages.size() * sizeof(PqGpuPage));
  DevBuf d_chunks(chmeta.size() * sizeof(PqGpuChunk));
  DevBuf d_nn(pages.size() * 4), d_voff(pages.size() * 4);
  DevBuf d_pdense(pages.size() * 4), d_chunknn(chmeta.size() * 4);
  DevBuf d_gcerr(4);
  AURON_HIP(hipMemsetAsync(win.valid.get(), 0, valid_total, stream));
  AURON_HIP(hipMemsetAsync(d_gcerr.get(), 0, 4, stream));
  up.copy(d_pages.get(), pages.data(), pages.size() * sizeof(PqGpuPage),
          stream);
  up.copy(d_chunks.get(), chmeta.data(), chmeta.size() * sizeof(PqGpuChunk),
          stream);
  std::vector<std::vector<uint8_t>> pvbits(chmeta.size());
  for (size_t c = 0; c < chmeta.size(); c++) {
    const PqColumnChunkData& cd = chunks[ch_di[c]];
    // compressed span (pages of a chunk are contiguous in the file)
    const auto& p0 = cd.comp_pages[0];
    const auto& pl = cd.comp_pages.back();
    size_t span = (size_t)(pl.src - p0.src) + pl.comp_len;
    up.copy(d_comp.get<uint8_t>() + pages[chmeta[c].page0].comp_off, p0.src,
            span, stream);
    // host-decoded prefix: dense values + validity bits
    up.copy(win.dense.get<uint8_t>() + chmeta[c].dense_base, cd.plain.data(),
            cd.plain.size(), stream);
    if (!cd.nullable || cd.prefix_values <= 0) continue;
    size_t pb = ((size_t)cd.prefix_values + 7) / 8;
    auto& vb = pvbits[c];
    if (!cd.validity.empty()) {
      vb.assign(cd.validity.begin(), cd.validity.begin() + pb);
    } else {
      vb.assign(pb, 0xFF);
    }
    if (cd.prefix_values & 7)  // clear bits beyond the prefix:
      vb[pb - 1] &= (uint8_t)((1u << (cd.prefix_values & 7)) - 1);
    up.copy(win.valid.get<uint8_t>() + chmeta[c].valid_base, vb.data(), pb,
            stream);
  }
  launch_pq_pages_decode(d_comp.get<uint8_t>(), d_pages.get<PqGpuPage>(),
                         (int)pages.size(), d_scratch.get<uint8_t>(),
                         win.valid.get<uint8_t>(), d_chunks.get<PqGpuChunk>(),
                         d_nn.get<uint32_t>(), d_voff.get<uint32_t>(),
                         d_gcerr.get<uint32_t>(), stream);
  launch_pq_page_offsets(d_chunks.get<PqGpuChunk>(), (int)chmeta.size(),
                         d_nn.get<uint32_t>(), d_pdense.get<uint32_t>(),
                         d_chunknn.get<uint32_t>(), stream);
  launch_pq_pages_compact(d_pages.get<PqGpuPage>(), (int)pages.size(),
                          d_scratch.get<uint8_t>(), d_chunks.get<PqGpuChunk>(),
                          d_nn.get<uint32_t>(), d_voff.get<uint32_t>(),
                          d_pdense.get<uint32_t>(), win.dense.get<uint8_t>(),
                          stream);
  std::vector<uint32_t> h_chunknn(chmeta.size());
  uint32_t h_err = 0;
  AURON_HIP(hipMemcpyAsync(h_chunknn.data(), d_chunknn.get(),
                           chmeta.size() * 4, hipMemcpyDeviceToHost, stream));
  AURON_HIP(hipMemcpyAsync(&h_err, d_gcerr.get(), 4, hipMemcpyDeviceToHost,
                           stream));
  AURON_HIP(hipStreamSynchronize(stream));
  if (h_err) FAIL("parquet: GPU page decode failed (flags " +
                  std::to_string(h_err) + ")");
  for (size_t c = 0; c < chmeta.size(); c++) {
    const PqColumnChunkData& cd = chunks[ch_di[c]];
    GcWindow::Chunk& r = win.chunks[ch_di[c]];
    r.valid_base = chmeta[c].valid_base;
    r.dense_base = chmeta[c].dense_base;
    r.total_nn = (int64_t)chmeta[c].prefix_nn + h_chunknn[c];
    r.null_total = cd.prefix_values + cd.suffix_values - r.total_nn;
    r.ready = true;
  }
  return win;
}

// Device temporaries of one chunk's assembly. DevBuf is pooled: a buffer
// freed before the stream drains is recycled under a running kernel, so the
// assembling function keeps these until it has synchronised.
struct ChunkTemps {
  DevBuf mask, positions;     // byte mask / exclusive positions of validity
  DevBuf runs, run_bytes;     // def-level or dictionary-index RLE runs
  DevBuf packed, idx_packed;  // dense non-null values / dictionary indices
  DevBuf indices, dict;       // row-aligned indices, dictionary values
};

// validity bitmap -> byte mask + exclusive positions of the non-null rows
void validity_positions(const uint8_t* validity, int64_t rows, ChunkTemps* t,
                        DevBuf* scan_tmp, hipStream_t stream) {
  t->mask.alloc(rows);
  t->positions.alloc((rows + 1) * 4);
  launch_bits_to_mask(validity, rows, t->mask.get<uint8_t>(), stream);
  scan_mask_positions(t->mask.get<uint8_t>(), rows,
                      t->positions.get<uint32_t>(), scan_tmp, stream);
}

// Dense non-null dictionary indices in t->idx_packed -> row-aligned values
// in `out`: scatter by validity (or straight copy), upload the dictionary,
// gather at the value width.
void gather_dictionary(const PqColumnChunkData& cd, bool has_nulls,
                       int64_t rows, int w, ChunkTemps* t, uint8_t* out,
                       hipStream_t stream) {
  t->indices.alloc((size_t)rows * 4);
  if (has_nulls) {
    launch_scatter_packed(4, t->idx_packed.get<uint8_t>(),
                          t->positions.get<uint32_t>(),
                          t->mask.get<uint8_t>(), rows,
                          t->indices.get<uint8_t>(), stream);
  } else {
    AURON_HIP(hipMemcpyAsync(t->indices.get(), t->idx_packed.get(),
                             (size_t)rows * 4, hipMemcpyDeviceToDevice,
                             stream));
  }
  t->dict.alloc(cd.dict_values.empty() ? 1 : cd.dict_values.size());
  if (!cd.dict_values.empty())
    AURON_HIP(hipMemcpyAsync(t->dict.get(), cd.dict_values.data(),
                             cd.dict_values.size(), hipMemcpyHostToDevice,
                             stream));
  if (w == 8)
    launch_gather_8(t->dict.get<uint8_t>(), t->indices.get<uint32_t>(), rows,
                    out, stream);
  else
    launch_gather_4(t->dict.get<uint8_t>(), t->indices.get<uint32_t>(), rows,
                    out, stream);
}

// Device-decompressed chunk: its validity bitmap and dense values are
// already resident in the window's blobs.
DevColumn assemble_gpu_comp(const PqColumnChunkData& cd,
                            const GcWindow& win, const GcWindow::Chunk& r,
                            DType dt, int64_t rows, DevBuf* scan_tmp,
                            hipStream_t stream) {
  if (!r.ready) FAIL("parquet: gpu page results missing");
  if (cd.prefix_values + cd.suffix_values != rows)
    FAIL("parquet: gpu chunk row count mismatch");
  DevColumn c;
  c.dt = dt;
  c.len = rows;
  const int w = (int)dtype_width(dt);
  c.own_values.alloc((size_t)rows * w);
  c.values = c.own_values.get();
  const uint8_t* dense = win.dense.get<uint8_t>() + r.dense_base;
  if (r.null_total == 0) {
    AURON_HIP(hipMemcpyAsync(c.own_values.get(), dense, (size_t)rows * w,
                             hipMemcpyDeviceToDevice, stream));
    return c;
  }
  c.own_validity.alloc((rows + 7) / 8);
  AURON_HIP(hipMemcpyAsync(c.own_validity.get(),
                           win.valid.get<uint8_t>() + r.valid_base,
                           (size_t)(rows + 7) / 8, hipMemcpyDeviceToDevice,
                           stream));
  c.validity = c.own_validity.get<uint8_t>();
  ChunkTemps t;
  validity_positions(c.validity, rows, &t, scan_tmp, stream);
  launch_scatter_packed(w, dense, t.positions.get<uint32_t>(),
                        t.mask.get<uint8_t>(), rows,
                        c.own_values.get<uint8_t>(), stream);
  AURON_HIP(hipStreamSynchronize(stream));  // temps die here
  return c;
}

// Host-decoded fixed-width chunk: validity (def-level runs expanded on
// device, or the host bitmap), then PLAIN values or dictionary indices
// (run-expanded on device, or host-decoded) scattered to their rows.
DevColumn assemble_fixed(const PqColumnChunkData& cd, DType dt, int64_t rows,
                         DevBuf* scan_tmp, hipStream_t stream) {
  PinnedUploader& up = PinnedUploader::inst();
  DevColumn c;
  c.dt = dt;
  c.len = rows;
  const int w = (int)dtype_width(dt);
  const bool has_nulls = cd.null_count > 0;
  c.own_values.alloc((size_t)rows * w);
  c.values = c.own_values.get();
  ChunkTemps t;
  if (cd.gpu_def) {
    // def levels expand to the validity bitmap ON DEVICE (the host only
    // walked the run headers — parquet.cpp rle_bp_runs)
    t.runs.alloc(cd.def_runs.size() * sizeof(PqRun));
    up.copy(t.runs.get(), cd.def_runs.data(),
            cd.def_runs.size() * sizeof(PqRun), stream);
    t.run_bytes.alloc(cd.def_bytes.empty() ? 8 : cd.def_bytes.size());
    up.copy(t.run_bytes.get(), cd.def_bytes.data(), cd.def_bytes.size(),
            stream);
    c.own_validity.alloc((rows + 7) / 8);
    launch_def_expand_validity(t.runs.get(), (int)cd.def_runs.size(),
                               t.run_bytes.get<uint8_t>(), rows,
                               c.own_validity.get<uint8_t>(), stream);
  } else if (has_nulls) {
    c.own_validity.alloc(cd.validity.size());
    AURON_HIP(hipMemcpyAsync(c.own_validity.get(), cd.validity.data(),
                             cd.validity.size(), hipMemcpyHostToDevice,
                             stream));
  }
  if (cd.gpu_def || has_nulls) {
    c.validity = c.own_validity.get<uint8_t>();
    validity_positions(c.validity, rows, &t, scan_tmp, stream);
  }
  if (cd.gpu_dict) {
    // dictionary indices: host walked run headers only; expand the dense
    // non-null index array on device
    DevBuf d_iruns(cd.idx_runs.size() * sizeof(PqRun));
    up.copy(d_iruns.get(), cd.idx_runs.data(),
            cd.idx_runs.size() * sizeof(PqRun), stream);
    DevBuf d_ibytes(cd.idx_bytes.empty() ? 8 : cd.idx_bytes.size());
    up.copy(d_ibytes.get(), cd.idx_bytes.data(), cd.idx_bytes.size(), stream);
    t.idx_packed.alloc((cd.nn_count ? cd.nn_count : 1) * 4);
    launch_runs_expand_u32(d_iruns.get(), (int)cd.idx_runs.size(),
                           d_ibytes.get<uint8_t>(), cd.nn_count,
                           t.idx_packed.get<uint32_t>(), stream);
    gather_dictionary(cd, has_nulls, rows, w, &t, c.own_values.get<uint8_t>(),
                      stream);
    AURON_HIP(hipStreamSynchronize(stream));  // temps die below
  } else if (cd.uses_dict) {
    // host-decoded dictionary indices
    t.idx_packed.alloc(cd.dict_indices.empty() ? 4
                                               : cd.dict_indices.size() * 4);
    up.copy(t.idx_packed.get(), cd.dict_indices.data(),
            cd.dict_indices.size() * 4, stream);
    gather_dictionary(cd, has_nulls, rows, w, &t, c.own_values.get<uint8_t>(),
                      stream);
  } else if (!has_nulls) {
    // PLAIN without nulls: the packed values are the column
    up.copy(c.own_values.get(), cd.plain.data(), cd.plain.size(), stream);
  } else {
    // PLAIN: non-null values packed densely
    t.packed.alloc(cd.plain.empty() ? 1 : cd.plain.size());
    up.copy(t.packed.get(), cd.plain.data(), cd.plain.size(), stream);
    launch_scatter_packed(w, t.packed.get<uint8_t>(),
                          t.positions.get<uint32_t>(), t.mask.get<uint8_t>(),
                          rows, c.own_values.get<uint8_t>(), stream);
  }
  AURON_HIP(hipStreamSynchronize(stream));  // host cd dies here
  return c;
}

// One column chunk -> a row-aligned DevColumn of `rows` rows.
DevColumn assemble_chunk(const PqColumnChunkData& cd, const GcWindow& win,
                         const GcWindow::Chunk& gc, DType dt, int64_t rows,
                         DevBuf* scan_tmp, hipStream_t stream) {
  if (cd.gpu_comp)
    return assemble_gpu_comp(cd, win, gc, dt, rows, scan_tmp, stream);
  if (dt != DType::Utf8 && dt != DType::Binary)
    return assemble_fixed(cd, dt, rows, scan_tmp, stream);
  // row-aligned offsets/data assembled on host (parquet.cpp)
  DevColumn c = upload_column(
      dt, rows, cd.bin_data.data(), cd.bin_data.size(), cd.bin_offsets.data(),
      cd.null_count > 0 ? cd.validity.data() : nullptr, cd.validity.size(),
      stream);
  AURON_HIP(hipStreamSynchronize(stream));  // host cd dies here
  return c;
}

// Row groups per decode window (AURON_PARQUET_WIN: 0 = the whole file)
int window_row_groups(const ParquetFile& pf) {
  const int nrg = pf.num_row_groups();
  const char* e = getenv("AURON_PARQUET_WIN");
  if (e && e[0] == '0') return nrg > 0 ? nrg : 1;  // one window
  if (e && atoi(e) > 0) return atoi(e);
  // ~128M rows per window measured best at 1B rows (same-box A/B:
  // 16-rg windows 1341 ms/step vs whole-file 1619, 8-rg 1679)
  return std::max(
      1, (int)((512u << 20) / std::max<int64_t>(1, pf.row_group_rows(0) * 8)));
}

// One file: per window of row groups — decode, pre-pass, prune, assemble,
// feed. Host decode overlaps the device work: while window k's
// uploads/kernels/consume run on the stream, the host cores decode window
// k+1 (the host page-header walk + dict-prefix decode and the GPU page
// decompression are comparable in wall time — serializing them was ~40% of
// the config-3 step).
int64_t scan_file(const std::string& path, const ParquetScanNode& node,
                  DevBuf* scan_tmp, hipStream_t stream,
                  const BatchSink& sink) {
  ParquetFile pf(path);
  const auto& fcols = pf.columns();
  std::vector<uint32_t> proj = node.projection;
  if (proj.empty())
    for (uint32_t i = 0; i < fcols.size(); i++) proj.push_back(i);
  for (uint32_t ci : proj)
    if (ci >= fcols.size()) FAIL("parquet: projection out of range");
  const int nrg = pf.num_row_groups();
  const size_t width = proj.size();
  const int rg_win = window_row_groups(pf);
  std::vector<PqColumnChunkData> decoded((size_t)nrg * width);
  std::string decode_err;
  std::mutex err_mu;
  auto decode_window = [&](int rg_lo, int rg_hi) {
    decode_chunks(pf, proj, &decoded, (size_t)rg_lo * width,
                  (size_t)rg_hi * width, &decode_err, &err_mu);
  };
  std::future<void> pending = std::async(std::launch::async, decode_window, 0,
                                         std::min(rg_win, nrg));
  int64_t input_rows = 0;
  for (int win_lo = 0; win_lo < nrg; win_lo += rg_win) {
    const int win_hi = std::min(win_lo + rg_win, nrg);
    pending.get();  // this window's host decode is complete
    if (!decode_err.empty()) FAIL(decode_err);
    if (win_hi < nrg)  // overlap: decode the NEXT window on host cores
      pending = std::async(std::launch::async, decode_window, win_hi,
                           std::min(win_hi + rg_win, nrg));
    GcWindow gc = decompress_window(decoded.data() + (size_t)win_lo * width,
                                    (size_t)(win_hi - win_lo) * width, stream);
    for (int rg = win_lo; rg < win_hi; rg++) {
      bool keep = true;
      for (const Expr& pr : node.pruning)
        keep = keep && rg_may_match(pr, pf, rg);
      if (!keep) {
        DBG("parquet: pruned row group %d", rg);
        continue;
      }
      DevBatch b;
      b.num_rows = pf.row_group_rows(rg);
      for (size_t pi = 0; pi < width; pi++) {
        const size_t wi = (size_t)(rg - win_lo) * width + pi;
        // the host chunk is released as soon as its column is on the device
        PqColumnChunkData cd = std::move(decoded[(size_t)rg * width + pi]);
        b.cols.push_back(assemble_chunk(cd, gc, gc.chunks[wi],
                                        fcols[proj[pi]].dtype(), b.num_rows,
                                        scan_tmp, stream));
      }
      input_rows += b.num_rows;
      sink(std::move(b));
    }
  }
  return input_rows;
}

}  // namespace

int64_t scan_parquet(const ParquetScanNode& node, hipStream_t stream,
                     const BatchSink& sink) {
  int64_t input_rows = 0;
  DevBuf scan_tmp;
  for (const std::string& path : node.files)
    input_rows += scan_file(path, node, &scan_tmp, stream, sink);
  return input_rows;
}

// ------------------------------------------------------------ ipc reader --
// (ipc_reader_exec.rs:62-120)
int64_t read_ipc(const IpcReaderNode& reader, const AuronCallbacks& cb,
                 int codec, hipStream_t stream, const BatchSink& sink) {
  if (!cb.next_ipc_bytes)
    FAIL("plan holds IpcReaderExec but no next_ipc_bytes callback was given");
  std::vector<int> widths;
  for (const Field& f : reader.schema.fields) {
    if (f.dtype == DType::Binary || f.dtype == DType::Utf8)
      widths.push_back(0);
    else if (dtype_width(f.dtype) > 0)
      widths.push_back((int)dtype_width(f.dtype));
    else
      FAIL("IpcReader: unsupported column dtype");
  }
  int64_t input_rows = 0;
  while (true) {
    const uint8_t* data = nullptr;
    size_t len = 0;
    int rc = cb.next_ipc_bytes(cb.user, reader.resource_id.c_str(), &data,
                               &len);
    DBG("ipc reader rc=%d len=%zu", rc, len);
    if (rc == 0) break;
    std::vector<uint8_t> payload;
    std::string err;
    if (!ipc_decode_blocks(data, len, &payload, &err, codec)) FAIL(err);
    size_t used = 0;
    while (used < payload.size()) {
      int64_t rows = 0;
      std::vector<OwnedCol> cols;
      if (!serde_read_batch(payload.data(), payload.size(), &used, widths,
                            &rows, &cols, &err))
        FAIL(err);
      DevBatch b;
      b.num_rows = rows;
      for (size_t ci = 0; ci < cols.size(); ci++) {
        const OwnedCol& oc = cols[ci];
        b.cols.push_back(upload_column(
            reader.schema.fields[ci].dtype, rows, oc.values.data(),
            oc.values.size(),
            oc.byte_width == 0 ? oc.offsets.data() : nullptr,
            oc.validity.data(), oc.validity.size(), stream));
        AURON_HIP(hipStreamSynchronize(stream));  // host vectors die below
      }
      input_rows += rows;
      sink(std::move(b));
    }
  }
  return input_rows;
}

}  // namespace auron
