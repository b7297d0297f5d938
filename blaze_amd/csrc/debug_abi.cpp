// debug_abi.cpp — the test-only auron_debug_* entry points of
// include/auron_hip.h that need neither a Runtime nor a device: host-side
// serde / parquet / scalar / conf / plan decode checks and the expression
// compiler and interpreter.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch.h"
#include "expr.h"
#include "ipc_scalar.h"
#include "parquet.h"
#include "serde_host.h"

using namespace auron;

extern "C" {

// test-only: host-side batch_serde + IPC block codec roundtrip over a
// 3-column batch (i64 key, f64 val, binary) — CPU-checkable byte parity
// against the oracle writer plus write->read self-consistency, covering the
// engine's IpcReader decode path without a GPU. Returns the block-stream
// length (copied into out up to cap), or -1 with the error text in out.
int64_t auron_debug_serde_roundtrip(const int64_t* k, const uint8_t* kvalid,
                                    const double* v, const uint8_t* vvalid,
                                    const int32_t* boffs, const uint8_t* bdata,
                                    int64_t n, int64_t batch_size, uint8_t* out,
                                    size_t cap) {
  auto fail = [&](const std::string& m) -> int64_t {
    snprintf((char*)out, cap, "%s", m.c_str());
    return -1;
  };
  std::string err;
  std::vector<HostCol> cols(3);
  cols[0] = {8, (const uint8_t*)k, kvalid, nullptr};
  cols[1] = {8, (const uint8_t*)v, vvalid, nullptr};
  cols[2] = {0, bdata, nullptr, boffs};
  IpcBlockWriter w;
  for (int64_t beg = 0; beg < n; beg += batch_size) {
    int64_t end = std::min(n, beg + batch_size);
    std::vector<uint8_t> payload;
    serde_write_batch(cols, beg, end, &payload);
    if (!w.write_payload(payload.data(), payload.size(), &err))
      return fail(err);
  }
  if (!w.finish_block(&err)) return fail(err);
  std::vector<uint8_t> stream = w.take();

  // decode side: blocks -> payload -> batches; verify every row round-trips
  std::vector<uint8_t> payload;
  if (!ipc_decode_blocks(stream.data(), stream.size(), &payload, &err))
    return fail(err);
  size_t pos = 0;
  int64_t row = 0;
  while (pos < payload.size()) {
    size_t used = 0;
    int64_t rows = 0;
    std::vector<OwnedCol> rc;
    if (!serde_read_batch(payload.data() + pos, payload.size() - pos, &used,
                          {8, 8, 0}, &rows, &rc, &err))
      return fail(err);
    pos += used;
    for (int64_t i = 0; i < rows; i++, row++) {
      bool kv2 = rc[0].validity.empty() ||
                 ((rc[0].validity[i >> 3] >> (i & 7)) & 1);
      bool kv1 = !kvalid || ((kvalid[row >> 3] >> (row & 7)) & 1);
      if (kv1 != kv2) return fail("key validity mismatch");
      if (kv1 && memcmp(rc[0].values.data() + i * 8, (const uint8_t*)&k[row],
                        8) != 0)
        return fail("key value mismatch");
      bool vv2 = rc[1].validity.empty() ||
                 ((rc[1].validity[i >> 3] >> (i & 7)) & 1);
      bool vv1 = !vvalid || ((vvalid[row >> 3] >> (row & 7)) & 1);
      if (vv1 != vv2) return fail("val validity mismatch");
      if (vv1 && memcmp(rc[1].values.data() + i * 8, (const uint8_t*)&v[row],
                        8) != 0)
        return fail("val value mismatch");
      int32_t l1 = boffs[row + 1] - boffs[row];
      int32_t l2 = rc[2].offsets[i + 1] - rc[2].offsets[i];
      if (l1 != l2) return fail("binary length mismatch");
      if (l1 && memcmp(rc[2].values.data() + rc[2].offsets[i],
                       bdata + boffs[row], l1) != 0)
        return fail("binary bytes mismatch");
    }
  }
  if (row != n) return fail("row count mismatch");
  if (stream.size() <= cap) memcpy(out, stream.data(), stream.size());
  return (int64_t)stream.size();
}

// test-only: parse a parquet file on the host and summarize chunk decode
// results (CPU-checkable against pyarrow metadata — no GPU needed)
int32_t auron_debug_parquet_summary(const char* path, char* out, size_t cap) {
  std::string r;
  try {
    ParquetFile pf(path);
    r = "cols=";
    for (const auto& c : pf.columns())
      r += c.name + ":" + std::to_string(c.physical_type) +
           (c.nullable ? "?" : "") + ",";
    r += " rgs=" + std::to_string(pf.num_row_groups());
    for (int rg = 0; rg < pf.num_row_groups(); rg++) {
      r += " [rg" + std::to_string(rg) + " rows=" +
           std::to_string(pf.row_group_rows(rg));
      for (size_t c = 0; c < pf.columns().size(); c++) {
        PqColumnChunkData cd = pf.read_chunk(rg, (int)c);
        pq_materialize_gpu_staging(&cd);  // host-expand staged GPU runs
        // value checksum: wrapping i64 sum of the raw fixed-width values
        // (sign-extended for narrow ints) over the dense non-null stream —
        // lets CPU tests verify DECODED VALUES against numpy ground truth,
        // not just counts
        int64_t csum = 0;
        const size_t w = dtype_width(pf.columns()[c].dtype());
        auto add_vals = [&](const uint8_t* v, size_t cnt) {
          for (size_t i = 0; i < cnt; i++) {
            int64_t x = 0;
            if (w == 8) {
              memcpy(&x, v + i * 8, 8);
            } else if (w == 4) {
              int32_t x32;
              memcpy(&x32, v + i * 4, 4);
              x = x32;
            }
            csum = (int64_t)((uint64_t)csum + (uint64_t)x);
          }
        };
        if (w > 0) {
          if (cd.uses_dict) {
            for (uint32_t ix : cd.dict_indices)
              add_vals(cd.dict_values.data() + (size_t)ix * w, 1);
          } else {
            add_vals(cd.plain.data(), cd.plain.size() / w);
          }
        } else if (!cd.bin_offsets.empty()) {
          // byte-array columns: position-weighted rolling checksum over the
          // row-aligned lengths and data bytes
          for (size_t i = 0; i + 1 < cd.bin_offsets.size(); i++) {
            int64_t l = cd.bin_offsets[i + 1] - cd.bin_offsets[i];
            csum = (int64_t)((uint64_t)csum + (uint64_t)(l * (int64_t)(i + 1)));
          }
          for (size_t j = 0; j < cd.bin_data.size(); j++)
            csum = (int64_t)((uint64_t)csum +
                             (uint64_t)((int64_t)cd.bin_data[j] *
                                        (int64_t)(j + 1)));
        }
        r += " c" + std::to_string(c) + "{n=" + std::to_string(cd.num_values) +
             ",nulls=" + std::to_string(cd.null_count) +
             ",dict=" + std::to_string(cd.uses_dict ? cd.dict_count : 0) +
             ",csum=" + std::to_string(csum) + "}";
      }
      r += "]";
    }
  } catch (const std::exception& ex) {
    r = std::string("ERROR: ") + ex.what();
  }
  if (r.size() + 1 > cap) return -1;
  memcpy(out, r.c_str(), r.size() + 1);
  return (int32_t)r.size();
}

// test-only: decode a ScalarValue ipc_bytes literal and render it
int32_t auron_debug_decode_scalar(const uint8_t* data, size_t len, char* out,
                                  size_t cap) {
  ScalarLit s;
  std::string err;
  std::string r;
  if (!decode_ipc_scalar(data, len, &s, &err)) {
    r = "ERROR: " + err;
  } else if (s.is_null) {
    r = "null dtype=" + std::to_string((int)s.dtype);
  } else if (s.dtype == DType::Utf8 || s.dtype == DType::Binary) {
    r = "str:" + s.utf8;
  } else if (s.dtype == DType::Float64 || s.dtype == DType::Float32) {
    char buf[64];
    snprintf(buf, sizeof(buf), "f:%.17g", s.f64);
    r = buf;
  } else {
    r = "i:" + std::to_string(s.i64) + " dtype=" + std::to_string((int)s.dtype);
  }
  if (r.size() + 1 > cap) return -1;
  memcpy(out, r.c_str(), r.size() + 1);
  return (int32_t)r.size();
}

// test-only: exercise the get_conf callback plumbing from the C side (the
// ctypes out-param contract is easy to get wrong — see GET_CONF note)
int32_t auron_debug_conf_roundtrip(AuronCallbacks* cb, const char* key,
                                   char* out, size_t cap) {
  Conf conf{cb};
  std::string v = conf.get(key, "<default>");
  if (v.size() + 1 > cap) return -1;
  memcpy(out, v.c_str(), v.size() + 1);
  return (int32_t)v.size();
}

// test-only introspection: decode a TaskDefinition and render a one-line
// summary (verifies the hand-rolled proto reader against encoders)
int32_t auron_debug_decode_plan(const uint8_t* data, size_t len, char* out,
                                size_t out_cap) {
  std::string err;
  auto td = decode_task_definition(data, len, &err);
  std::string s;
  if (!td) {
    s = "ERROR: " + err;
  } else {
    s = "task stage=" + std::to_string(td->stage_id) +
        " part=" + std::to_string(td->partition_id) +
        " tid=" + std::to_string(td->task_id) + " plan=";
    const PlanNode* p = td->plan.get();
    while (p) {
      switch (p->kind) {
        case PlanNode::ShuffleWriter: {
          const auto& sw = *p->shuffle_writer;
          s += "ShuffleWriter(kind=" + std::to_string((int)sw.partitioning.kind) +
               ",P=" + std::to_string(sw.partitioning.partition_count) +
               ",nhash=" + std::to_string(sw.partitioning.hash_exprs.size()) +
               ",data=" + sw.output_data_file + ")->";
          p = sw.input.get();
          break;
        }
        case PlanNode::Agg: {
          const auto& ag = *p->agg;
          s += "Agg(mode=" +
               std::to_string(ag.modes.empty() ? -1 : (int)ag.modes[0]) +
               ",ngroup=" + std::to_string(ag.grouping_exprs.size()) +
               ",nagg=" + std::to_string(ag.agg_exprs.size());
          for (const auto& e : ag.agg_exprs)
            s += ",fn" + std::to_string(e.agg_function) + "rt" +
                 std::to_string((int)e.return_type);
          s += ",skip=" + std::to_string((int)ag.supports_partial_skipping) +
               ")->";
          p = ag.input.get();
          break;
        }
        case PlanNode::Filter: {
          s += "Filter(npred=" +
               std::to_string(p->filter->predicates.size()) + ")->";
          p = p->filter->input.get();
          break;
        }
        case PlanNode::Projection: {
          s += "Project(ncols=" +
               std::to_string(p->projection->exprs.size()) + ")->";
          p = p->projection->input.get();
          break;
        }
        case PlanNode::ParquetScan: {
          const auto& pq = *p->parquet;
          s += "ParquetScan(nfiles=" + std::to_string(pq.files.size()) +
               ",nfields=" + std::to_string(pq.schema.fields.size()) +
               ",nproj=" + std::to_string(pq.projection.size()) + ")";
          p = nullptr;
          break;
        }
        case PlanNode::IpcReader: {
          const auto& ir = *p->ipc_reader;
          s += "IpcReader(nfields=" + std::to_string(ir.schema.fields.size()) +
               ",rid=" + ir.resource_id + ")";
          p = nullptr;
          break;
        }
        case PlanNode::FFIReader: {
          const auto& fr = *p->ffi_reader;
          s += "FFIReader(nfields=" + std::to_string(fr.schema.fields.size()) +
               ",rid=" + fr.resource_id + ")";
          p = nullptr;
          break;
        }
      }
    }
  }
  // expression trees of Filter / Projection nodes, root to leaf, appended
  // after the chain summary
  if (td) {
    std::string ex;
    const PlanNode* p = td->plan.get();
    while (p) {
      switch (p->kind) {
        case PlanNode::ShuffleWriter: p = p->shuffle_writer->input.get(); break;
        case PlanNode::Agg: p = p->agg->input.get(); break;
        case PlanNode::Filter:
          ex += " Filter[";
          for (size_t i = 0; i < p->filter->predicates.size(); i++)
            ex += (i ? "; " : "") + expr_tree_text(p->filter->predicates[i]);
          ex += "]";
          p = p->filter->input.get();
          break;
        case PlanNode::Projection:
          ex += " Project[";
          for (size_t i = 0; i < p->projection->exprs.size(); i++)
            ex += (i ? "; " : "") + expr_tree_text(p->projection->exprs[i]);
          ex += "]";
          p = p->projection->input.get();
          break;
        default: p = nullptr;
      }
    }
    if (!ex.empty()) s += " exprs:" + ex;
  }
  if (s.size() + 1 > out_cap) return -1;
  memcpy(out, s.c_str(), s.size() + 1);
  return (int32_t)s.size();
}

namespace auron {
namespace {
// Programs of a plan whose root is a Filter or a Projection directly over a
// reader: one AND-ed mask program for a Filter, one value program per
// non-Column expr for a Projection (Column exprs yield no program). The same
// compile entry points the operators use.
bool debug_compile_programs(const uint8_t* data, size_t len,
                            std::vector<ExprProgram>* progs,
                            std::vector<int>* expr_index, std::string* err) {
  auto td = decode_task_definition(data, len, err);
  if (!td) return false;
  const PlanNode* root = td->plan.get();
  const PlanNode* in = nullptr;
  if (root->kind == PlanNode::Filter) in = root->filter->input.get();
  else if (root->kind == PlanNode::Projection)
    in = root->projection->input.get();
  else {
    *err = "plan root must be a Filter or a Projection";
    return false;
  }
  const Schema* sc = nullptr;
  if (in && in->kind == PlanNode::FFIReader) sc = &in->ffi_reader->schema;
  else if (in && in->kind == PlanNode::IpcReader) sc = &in->ipc_reader->schema;
  if (!sc) {
    *err = "the Filter / Projection input must be an FFIReader or IpcReader";
    return false;
  }
  std::vector<DType> dts;
  for (const Field& f : sc->fields) dts.push_back(f.dtype);
  if (root->kind == PlanNode::Filter) {
    ExprProgram p;
    if (!compile_filter_program(root->filter->predicates, dts, &p, err))
      return false;
    progs->push_back(p);
    expr_index->push_back(0);
    return true;
  }
  const auto& exprs = root->projection->exprs;
  for (size_t i = 0; i < exprs.size(); i++) {
    if (exprs[i].kind == Expr::Column) continue;
    ExprProgram p;
    if (!compile_value_program(exprs[i], dts, &p, err)) {
      *err = "expr " + std::to_string(i) + ": " + *err;
      return false;
    }
    progs->push_back(p);
    expr_index->push_back((int)i);
  }
  return true;
}
}  // namespace
}  // namespace auron

// test-only: compile the expressions of a Filter / Projection plan and render
// the programs, one per line; "ERROR: <cause>" on a plan-build failure.
// Host-only: needs no GPU.
int32_t auron_debug_compile_expr(const uint8_t* data, size_t len, char* out,
                                 size_t out_cap) {
  std::vector<ExprProgram> progs;
  std::vector<int> idx;
  std::string err, s;
  if (!debug_compile_programs(data, len, &progs, &idx, &err)) {
    s = "ERROR: " + err;
  } else {
    for (size_t i = 0; i < progs.size(); i++)
      s += "expr" + std::to_string(idx[i]) + " " +
           expr_program_text(progs[i]) + "\n";
  }
  if (s.size() + 1 > out_cap) return -1;
  memcpy(out, s.c_str(), s.size() + 1);
  return (int32_t)s.size();
}

// test-only: run the compiled program of expression `expr_index` (0 for a
// Filter) on host arrays through the interpreter that shares the kernel's
// per-row evaluator. col_values[c] holds n values at column c's width,
// col_valid[c] one byte per row or NULL. Writes n value bit patterns and n
// states (0 valid, 1 null, 2 poison); returns the root type code (0 Int32,
// 1 Int64, 2 Float64, 3 Bool) or -1 with the cause in err.
int32_t auron_debug_eval_expr(const uint8_t* data, size_t len,
                              int32_t expr_index, int32_t ncols,
                              const void* const* col_values,
                              const uint8_t* const* col_valid, int64_t n,
                              uint64_t* out_bits, uint8_t* out_state,
                              char* err_out, size_t err_cap) {
  std::vector<ExprProgram> progs;
  std::vector<int> idx;
  std::string err;
  const ExprProgram* prog = nullptr;
  if (debug_compile_programs(data, len, &progs, &idx, &err)) {
    for (size_t i = 0; i < progs.size(); i++)
      if (idx[i] == expr_index) prog = &progs[i];
    if (!prog) err = "no computed expression at index " +
                     std::to_string(expr_index);
  }
  if (prog)
    for (int s = 0; s < prog->nslots; s++)
      if ((int64_t)prog->slot_col[s] >= ncols || !col_values[prog->slot_col[s]]) {
        err = "input column " + std::to_string(prog->slot_col[s]) +
              " not supplied";
        prog = nullptr;
        break;
      }
  if (!prog) {
    snprintf(err_out, err_cap, "%s", err.c_str());
    return -1;
  }
  std::vector<ExprHostCol> cols((size_t)ncols);
  for (int32_t c = 0; c < ncols; c++)
    cols[c] = ExprHostCol{col_values[c], col_valid ? col_valid[c] : nullptr};
  expr_eval_host(*prog, cols, n, out_bits, out_state);
  return (int32_t)prog->root_ty;
}

}  // extern "C"
