// expr_fuzz.cpp — stand-alone sanitizer driver for the host half of the
// expression engine: the compiler (expr.cpp) and the interpreter that shares
// the kernel's per-row evaluator (expr_ops.h).
//
// It builds random expression trees, valid and invalid (mismatched types,
// Utf8 operands, deep and long trees, unknown ops), compiles each one, and
// runs every program that compiles over random arrays with nulls and the
// integer / float edge values. Build with AddressSanitizer and UBSan and run
// on the CPU (`make -C blaze_amd/csrc expr_fuzz_run`); it links no HIP code
// and is never loaded into Python.
//
//   expr_fuzz <tests/golden/expr_literals.bin> [iterations] [seed]
//
// Besides the sanitizers it checks invariants: a failed compile names a
// cause; a program respects the instruction / stack limits; a result the
// nullable analysis calls non-nullable has no null row; a program that
// cannot poison yields no poison row; null and poison rows carry value 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../blaze_amd/csrc/expr.h"

using namespace auron;

namespace {

struct Lit {
  int type;  // 0 Int32, 1 Int64, 2 Float64, 3 Bool, 4 Utf8
  bool is_null;
  std::vector<uint8_t> ipc;
};

std::vector<Lit> load_literals(const char* path) {
  std::vector<Lit> lits;
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  for (;;) {
    uint8_t hdr[6];
    if (fread(hdr, 1, 6, f) != 6) break;
    uint32_t len;
    memcpy(&len, hdr + 2, 4);
    Lit l;
    l.type = hdr[0];
    l.is_null = hdr[1] != 0;
    l.ipc.resize(len);
    if (fread(l.ipc.data(), 1, len, f) != len) {
      fprintf(stderr, "truncated literal fixture\n");
      exit(2);
    }
    lits.push_back(std::move(l));
  }
  fclose(f);
  return lits;
}

// input schema: two columns of each value type, one Utf8, one Float32
const std::vector<DType> kSchema = {
    DType::Int32, DType::Int32, DType::Int64, DType::Int64,
    DType::Float64, DType::Float64, DType::Utf8, DType::Float32};

struct Gen {
  std::mt19937_64 rng;
  const std::vector<Lit>& lits;
  int chaos;  // percent of nodes that ignore the requested type

  int pick(int n) { return (int)(rng() % (uint64_t)n); }
  bool coin(int pct) { return pick(100) < pct; }

  Expr column(int ty) {  // ty: 0..2 value types, 4 Utf8, 5 Float32
    Expr e;
    e.kind = Expr::Column;
    int base = ty == 4 ? 6 : ty == 5 ? 7 : ty * 2 + pick(2);
    e.col_index = (uint32_t)base;
    if (coin(1)) e.col_index = 99;  // out of range
    e.col_name = "c" + std::to_string(e.col_index);
    return e;
  }

  Expr literal(int ty) {
    std::vector<const Lit*> fit;
    for (const Lit& l : lits)
      if (l.type == ty) fit.push_back(&l);
    Expr e;
    e.kind = Expr::Literal;
    if (!fit.empty()) e.literal_ipc = fit[pick((int)fit.size())]->ipc;
    if (coin(1) && !e.literal_ipc.empty())
      e.literal_ipc.resize(e.literal_ipc.size() / 2);  // truncated stream
    return e;
  }

  static DType dtype_of(int ty) {
    switch (ty) {
      case 0: return DType::Int32;
      case 1: return DType::Int64;
      case 2: return DType::Float64;
      case 3: return DType::Bool;
      case 4: return DType::Utf8;
      default: return DType::Float32;
    }
  }

  // a tree meant to have type `ty` (0 Int32, 1 Int64, 2 Float64, 3 Bool)
  Expr gen(int ty, int depth) {
    if (coin(chaos)) ty = pick(6);
    if (ty > 3) return coin(70) ? column(ty) : literal(4);
    if (depth <= 0 || coin(15)) {
      if (ty == 3 || coin(35)) return literal(ty);
      return column(ty);
    }
    Expr e;
    if (ty == 3) {
      switch (pick(8)) {
        case 0: case 1: {
          static const char* ops[] = {"Eq", "NotEq", "Lt", "LtEq", "Gt",
                                      "GtEq"};
          int ot = pick(3);
          e.kind = Expr::BinaryExpr;
          e.op = ops[pick(6)];
          e.children = {gen(ot, depth - 1), gen(ot, depth - 1)};
          return e;
        }
        case 2: case 3:
          e.kind = Expr::BinaryExpr;
          e.op = coin(50) ? "And" : "Or";
          e.children = {gen(3, depth - 1), gen(3, depth - 1)};
          return e;
        case 4:
          e.kind = coin(50) ? Expr::SCAnd : Expr::SCOr;
          e.children = {gen(3, depth - 1), gen(3, depth - 1)};
          return e;
        case 5:
          e.kind = Expr::Not;
          e.children = {gen(3, depth - 1)};
          return e;
        case 6:
          e.kind = coin(50) ? Expr::IsNull : Expr::IsNotNull;
          e.children = {gen(pick(4), depth - 1)};
          return e;
        default: break;  // CASE yielding Bool, below
      }
    }
    switch (ty == 3 ? 4 : pick(6)) {
      case 0: case 1: {
        static const char* ops[] = {"Plus", "Minus", "Multiply", "Divide",
                                    "Modulo", "BitwiseAnd", ""};
        e.kind = Expr::BinaryExpr;
        e.op = coin(2) ? ops[5 + pick(2)] : ops[pick(5)];
        e.children = {gen(ty, depth - 1), gen(ty, depth - 1)};
        if (coin(1)) e.children.pop_back();  // malformed: one operand
        return e;
      }
      case 2:
        e.kind = Expr::Negative;
        e.children = {gen(ty, depth - 1)};
        return e;
      case 3:
        e.kind = coin(50) ? Expr::Cast : Expr::TryCast;
        e.cast_type = dtype_of(coin(3) ? pick(6) : ty);
        e.children = {gen(pick(3), depth - 1)};
        return e;
      default: {
        e.kind = Expr::Case;
        e.case_has_base = coin(30);
        e.case_has_else = coin(60);
        int bt = pick(3);
        if (e.case_has_base) e.children.push_back(gen(bt, depth - 1));
        int arms = 1 + pick(3);
        if (coin(1)) arms = 0;  // malformed: no WHEN
        for (int i = 0; i < arms; i++) {
          e.children.push_back(gen(e.case_has_base ? bt : 3, depth - 1));
          e.children.push_back(gen(ty, depth - 1));
        }
        if (e.case_has_else) e.children.push_back(gen(ty, depth - 1));
        return e;
      }
    }
  }
};

int fail(const char* what, const Expr& e, const ExprProgram* p) {
  fprintf(stderr, "INVARIANT VIOLATED: %s\n  tree: %s\n", what,
          expr_tree_text(e).c_str());
  if (p) fprintf(stderr, "  prog: %s\n", expr_program_text(*p).c_str());
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: expr_fuzz <expr_literals.bin> [iters] [seed]\n");
    return 2;
  }
  std::vector<Lit> lits = load_literals(argv[1]);
  if (lits.empty()) {
    fprintf(stderr, "no literals in %s\n", argv[1]);
    return 2;
  }
  const long iters = argc > 2 ? atol(argv[2]) : 20000;
  const uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 1;

  // random input arrays: edge values first, ~20% nulls
  const int64_t n = 97;
  std::mt19937_64 rng(seed);
  std::vector<int32_t> i32[2];
  std::vector<int64_t> i64[2];
  std::vector<double> f64[2];
  std::vector<uint8_t> valid[6];
  const int32_t e32[] = {INT32_MIN, INT32_MAX, -1, 0, 1};
  const int64_t e64[] = {INT64_MIN, INT64_MAX, -1, 0, 1, 1LL << 31};
  const double ef[] = {1e30, -1e30, std::nan(""), 0.0, -0.0, 0.5,
                       std::numeric_limits<double>::infinity(), 9.3e18};
  for (int c = 0; c < 2; c++) {
    for (int64_t r = 0; r < n; r++) {
      i32[c].push_back(r < 5 ? e32[(r + c) % 5] : (int32_t)(rng() % 21) - 10);
      i64[c].push_back(r < 6 ? e64[(r + 2 * c) % 6]
                             : (int64_t)(rng() % 2001) - 1000);
      f64[c].push_back(r < 8 ? ef[(r + 3 * c) % 8]
                             : ((double)(rng() % 20001) - 10000.0) / 64.0);
    }
  }
  for (auto& v : valid)
    for (int64_t r = 0; r < n; r++) v.push_back(rng() % 5 != 0);
  std::vector<ExprHostCol> cols(8);
  cols[0] = {i32[0].data(), valid[0].data()};
  cols[1] = {i32[1].data(), nullptr};  // a column without validity
  cols[2] = {i64[0].data(), valid[2].data()};
  cols[3] = {i64[1].data(), valid[3].data()};
  cols[4] = {f64[0].data(), valid[4].data()};
  cols[5] = {f64[1].data(), valid[5].data()};
  const uint32_t col_nullable = 0b111101;  // by input column

  Gen g{std::mt19937_64(seed * 7919 + 1), lits, 0};
  long compiled = 0, rejected = 0, poisoned = 0;
  std::vector<uint64_t> bits(n);
  std::vector<uint8_t> state(n);
  for (long it = 0; it < iters; it++) {
    g.chaos = it % 3 == 0 ? 0 : (it % 3 == 1 ? 3 : 15);
    int depth = 1 + g.pick(it % 50 == 0 ? 12 : 5);
    int ty = g.pick(4);
    Expr e = g.gen(ty, depth);
    ExprProgram p;
    std::string err;
    bool ok;
    int mode = g.pick(3);
    if (mode == 0) ok = compile_expr(e, kSchema, &p, &err);
    else if (mode == 1) ok = compile_value_program(e, kSchema, &p, &err);
    else ok = compile_filter_program({e, e}, kSchema, &p, &err);
    if (!ok) {
      if (err.empty()) return fail("compile failed without a cause", e, nullptr);
      rejected++;
      continue;
    }
    compiled++;
    if (p.n <= 0 || p.n > EXPR_MAX_INS || p.nslots > EXPR_MAX_SLOTS)
      return fail("program exceeds its limits", e, &p);
    (void)expr_program_text(p);
    uint32_t slot_nullable = 0;
    for (int s = 0; s < p.nslots; s++) {
      if (p.slot_col[s] >= 6) return fail("slot reads a non-value column", e, &p);
      if ((col_nullable >> p.slot_col[s]) & 1) slot_nullable |= 1u << s;
    }
    bool nullable = expr_result_nullable(p, slot_nullable);
    expr_eval_host(p, cols, n, bits.data(), state.data());
    for (int64_t r = 0; r < n; r++) {
      if (state[r] > ES_POISON) return fail("state out of range", e, &p);
      if (state[r] == ES_NULL && !nullable)
        return fail("null row in a result analysed as non-nullable", e, &p);
      if (state[r] == ES_POISON && !p.can_poison)
        return fail("poison row from a program that cannot poison", e, &p);
      if (state[r] != ES_VALID && bits[r] != 0)
        return fail("null / poison row with a nonzero value", e, &p);
      if (state[r] == ES_VALID && p.root_ty == ET_BOOL && bits[r] > 1)
        return fail("Bool value other than 0 / 1", e, &p);
      if (state[r] == ES_VALID && p.root_ty == ET_I32 &&
          (int64_t)bits[r] != (int64_t)(int32_t)bits[r])
        return fail("Int32 value not sign-extended", e, &p);
      poisoned += state[r] == ES_POISON;
    }
  }
  printf("expr_fuzz: %ld trees, %ld compiled, %ld rejected, %ld poison rows\n",
         iters, compiled, rejected, poisoned);
  if (compiled == 0 || rejected == 0) {
    fprintf(stderr, "fuzzer degenerate: both outcomes must occur\n");
    return 1;
  }
  return 0;
}
