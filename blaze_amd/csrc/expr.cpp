// expr.cpp — expression compiler, program printer and host interpreter.
#include "expr.h"

#include <cstdio>
#include <cstring>

#include "ipc_scalar.h"

namespace auron {

const char* expr_ty_name(ExprTy t) {
  switch (t) {
    case ET_I32: return "Int32";
    case ET_I64: return "Int64";
    case ET_F64: return "Float64";
    case ET_BOOL: return "Bool";
  }
  return "?";
}

DType expr_ty_dtype(ExprTy t) {
  switch (t) {
    case ET_I32: return DType::Int32;
    case ET_I64: return DType::Int64;
    case ET_F64: return DType::Float64;
    default: return DType::Unsupported;
  }
}

namespace {

const char* dtype_name(DType t) {
  static const char* names[] = {
      "Unsupported", "Null", "Bool", "UInt8", "Int8", "UInt16", "Int16",
      "UInt32", "Int32", "UInt64", "Int64", "Float16", "Float32", "Float64",
      "Utf8", "Binary"};
  int i = (int)t;
  return (i >= 0 && i <= 15) ? names[i] : "Unsupported";
}

bool value_ty(DType dt, ExprTy* ty) {
  switch (dt) {
    case DType::Int32: *ty = ET_I32; return true;
    case DType::Int64: *ty = ET_I64; return true;
    case DType::Float64: *ty = ET_F64; return true;
    default: return false;
  }
}

const char* op_name(uint8_t op) {
  static const char* names[] = {
      "LOAD", "LIT", "ADD", "SUB", "MUL", "DIV", "MOD", "NEG", "EQ", "NE",
      "LT", "LE", "GT", "GE", "AND", "OR", "SCAND", "SCOR", "NOT", "ISNULL",
      "ISNOTNULL", "CAST", "SELECT"};
  return op <= EOP_SELECT ? names[op] : "?";
}

struct Compiler {
  const std::vector<DType>& in;
  std::vector<ExprIns> ins;
  std::vector<uint64_t> imm;
  std::vector<uint32_t> slot_col;
  std::vector<uint8_t> slot_ty;
  int depth = 0, max_depth = 0;
  bool can_poison = false;
  std::string err;

  explicit Compiler(const std::vector<DType>& d) : in(d) {}

  bool fail(const std::string& m) {
    if (err.empty()) err = m;
    return false;
  }

  void emit(uint8_t op, uint8_t ty, uint8_t a, uint8_t b, int delta) {
    ins.push_back(ExprIns{op, ty, a, b});
    depth += delta;
    if (depth > max_depth) max_depth = depth;
  }

  int imm_index(uint64_t bits) {
    for (size_t i = 0; i < imm.size(); i++)
      if (imm[i] == bits) return (int)i;
    imm.push_back(bits);
    return (int)imm.size() - 1;
  }

  void emit_null(ExprTy ty) { emit(EOP_LIT, ty, 0, 1, +1); }

  bool gen_column(const Expr& e, ExprTy* ty) {
    if (e.col_index >= in.size())
      return fail("column index " + std::to_string(e.col_index) +
                  " out of range (input has " + std::to_string(in.size()) +
                  " columns)");
    DType dt = in[e.col_index];
    if (!value_ty(dt, ty))
      return fail(std::string(dtype_name(dt)) + " column '" + e.col_name +
                  "' cannot be used in a computed expression (value types are "
                  "Int32, Int64, Float64)");
    size_t s = 0;
    for (; s < slot_col.size(); s++)
      if (slot_col[s] == e.col_index) break;
    if (s == slot_col.size()) {
      slot_col.push_back(e.col_index);
      slot_ty.push_back((uint8_t)*ty);
    }
    emit(EOP_LOAD, *ty, (uint8_t)(s & 0xff), 0, +1);
    return true;
  }

  bool gen_literal(const Expr& e, ExprTy* ty) {
    ScalarLit s;
    std::string lerr;
    if (!decode_ipc_scalar(e.literal_ipc.data(), e.literal_ipc.size(), &s,
                           &lerr))
      return fail("literal decode: " + lerr);
    uint64_t bits = 0;
    if (s.dtype == DType::Bool) {
      *ty = ET_BOOL;
      bits = s.i64 ? 1 : 0;
    } else if (!value_ty(s.dtype, ty)) {
      return fail(std::string(dtype_name(s.dtype)) +
                  " literal cannot be used in a computed expression (value "
                  "types are Int32, Int64, Float64, Bool)");
    } else if (*ty == ET_F64) {
      bits = ev_bits(s.f64);
    } else {
      bits = (uint64_t)s.i64;  // Int32 decodes sign-extended
    }
    if (s.is_null) {
      emit_null(*ty);
    } else {
      emit(EOP_LIT, *ty, (uint8_t)(imm_index(bits) & 0xff), 0, +1);
    }
    return true;
  }

  bool gen_bool(const Expr& e, const char* what) {
    ExprTy t;
    if (!gen(e, &t)) return false;
    if (t != ET_BOOL)
      return fail(std::string(what) + " needs a Bool operand, got " +
                  expr_ty_name(t));
    return true;
  }

  bool gen_binary(const Expr& e, ExprTy* ty) {
    if (e.children.size() != 2)
      return fail("binary expression '" + e.op + "' without two operands");
    uint8_t op;
    enum { Arith, Cmp, Logic } cls;
    if (e.op == "Plus") { op = EOP_ADD; cls = Arith; }
    else if (e.op == "Minus") { op = EOP_SUB; cls = Arith; }
    else if (e.op == "Multiply") { op = EOP_MUL; cls = Arith; }
    else if (e.op == "Divide") { op = EOP_DIV; cls = Arith; }
    else if (e.op == "Modulo") { op = EOP_MOD; cls = Arith; }
    else if (e.op == "Eq") { op = EOP_EQ; cls = Cmp; }
    else if (e.op == "NotEq") { op = EOP_NE; cls = Cmp; }
    else if (e.op == "Lt") { op = EOP_LT; cls = Cmp; }
    else if (e.op == "LtEq") { op = EOP_LE; cls = Cmp; }
    else if (e.op == "Gt") { op = EOP_GT; cls = Cmp; }
    else if (e.op == "GtEq") { op = EOP_GE; cls = Cmp; }
    else if (e.op == "And") { op = EOP_AND; cls = Logic; }
    else if (e.op == "Or") { op = EOP_OR; cls = Logic; }
    else return fail("unsupported binary operator '" + e.op + "'");
    ExprTy lt, rt;
    if (!gen(e.children[0], &lt) || !gen(e.children[1], &rt)) return false;
    if (lt != rt)
      return fail("type mismatch in " + e.op + ": " + expr_ty_name(lt) +
                  " vs " + expr_ty_name(rt) +
                  " (operands must be cast to one type)");
    if (cls == Logic) {
      if (lt != ET_BOOL)
        return fail(e.op + " needs Bool operands, got " + expr_ty_name(lt));
      *ty = ET_BOOL;
    } else {
      if (lt == ET_BOOL)
        return fail(e.op + " on Bool operands is unsupported");
      *ty = cls == Cmp ? ET_BOOL : lt;
      if ((op == EOP_DIV || op == EOP_MOD) && lt != ET_F64) can_poison = true;
    }
    emit(op, (uint8_t)lt, 0, 0, -1);
    return true;
  }

  bool gen_cast(const Expr& e, ExprTy* ty) {
    if (e.children.size() != 1) return fail("Cast without an operand");
    ExprTy from, to;
    if (!gen(e.children[0], &from)) return false;
    if (from == ET_BOOL || !value_ty(e.cast_type, &to))
      return fail(std::string("unsupported cast ") + expr_ty_name(from) +
                  " -> " + dtype_name(e.cast_type));
    if (from != to) emit(EOP_CAST, (uint8_t)from, (uint8_t)to, 0, 0);
    *ty = to;
    return true;
  }

  // CASE [base] WHEN c THEN t ... [ELSE e]: emitted innermost-first as
  //   else, (cond_n, then_n, SELECT), ..., (cond_1, then_1, SELECT)
  // so the stack holds three values at most whatever the number of arms.
  bool gen_case(const Expr& e, ExprTy* ty) {
    size_t lo = e.case_has_base ? 1 : 0;
    size_t hi = e.children.size() - (e.case_has_else ? 1 : 0);
    if (e.children.size() < lo + (e.case_has_else ? 1 : 0) || hi <= lo ||
        (hi - lo) % 2 != 0)
      return fail("CASE without WHEN/THEN arms");
    ExprTy out;
    size_t else_at = ins.size();
    if (e.case_has_else) {
      if (!gen(e.children.back(), &out)) return false;
    } else {
      emit_null(ET_I32);  // type patched once the first THEN is known
    }
    bool out_known = e.case_has_else;
    for (size_t i = hi; i > lo; i -= 2) {
      const Expr& when = e.children[i - 2];
      const Expr& then = e.children[i - 1];
      if (e.case_has_base) {
        ExprTy bt, wt;
        if (!gen(e.children[0], &bt) || !gen(when, &wt)) return false;
        if (bt != wt)
          return fail(std::string("type mismatch in CASE base vs WHEN: ") +
                      expr_ty_name(bt) + " vs " + expr_ty_name(wt));
        if (bt == ET_BOOL) return fail("CASE base of type Bool is unsupported");
        emit(EOP_EQ, (uint8_t)bt, 0, 0, -1);
      } else if (!gen_bool(when, "CASE WHEN")) {
        return false;
      }
      ExprTy tt;
      if (!gen(then, &tt)) return false;
      if (!out_known) {
        out = tt;
        out_known = true;
        ins[else_at].ty = (uint8_t)tt;
      } else if (tt != out) {
        return fail(std::string("type mismatch in CASE branches: ") +
                    expr_ty_name(out) + " vs " + expr_ty_name(tt));
      }
      emit(EOP_SELECT, (uint8_t)out, 0, 0, -2);
    }
    *ty = out;
    return true;
  }

  bool gen(const Expr& e, ExprTy* ty) {
    switch (e.kind) {
      case Expr::Column: return gen_column(e, ty);
      case Expr::Literal: return gen_literal(e, ty);
      case Expr::BinaryExpr: return gen_binary(e, ty);
      case Expr::IsNull: case Expr::IsNotNull: {
        if (e.children.size() != 1) return fail("null check without operand");
        ExprTy t;
        if (!gen(e.children[0], &t)) return false;
        emit(e.kind == Expr::IsNull ? EOP_ISNULL : EOP_ISNOTNULL, (uint8_t)t,
             0, 0, 0);
        *ty = ET_BOOL;
        return true;
      }
      case Expr::Not:
        if (e.children.size() != 1) return fail("Not without operand");
        if (!gen_bool(e.children[0], "Not")) return false;
        emit(EOP_NOT, ET_BOOL, 0, 0, 0);
        *ty = ET_BOOL;
        return true;
      case Expr::Negative: {
        if (e.children.size() != 1) return fail("Negative without operand");
        if (!gen(e.children[0], ty)) return false;
        if (*ty == ET_BOOL) return fail("Negative on a Bool operand");
        emit(EOP_NEG, (uint8_t)*ty, 0, 0, 0);
        return true;
      }
      case Expr::Cast: case Expr::TryCast: return gen_cast(e, ty);
      case Expr::Case: return gen_case(e, ty);
      case Expr::SCAnd: case Expr::SCOr: {
        const char* nm = e.kind == Expr::SCAnd ? "SCAnd" : "SCOr";
        if (e.children.size() != 2)
          return fail(std::string(nm) + " without two operands");
        if (!gen_bool(e.children[0], nm) || !gen_bool(e.children[1], nm))
          return false;
        emit(e.kind == Expr::SCAnd ? EOP_SCAND : EOP_SCOR, ET_BOOL, 0, 0, -1);
        *ty = ET_BOOL;
        return true;
      }
      case Expr::AggExpr:
        return fail("aggregate expression inside a computed expression");
    }
    return fail("unknown expression kind");
  }

  bool finish(ExprTy root, ExprProgram* out) {
    if (max_depth > EXPR_MAX_STACK)
      return fail("expression needs operand stack depth " +
                  std::to_string(max_depth) + " (limit " +
                  std::to_string(EXPR_MAX_STACK) + ")");
    if (ins.size() > (size_t)EXPR_MAX_INS)
      return fail("expression compiles to " + std::to_string(ins.size()) +
                  " instructions (limit " + std::to_string(EXPR_MAX_INS) + ")");
    if (slot_col.size() > (size_t)EXPR_MAX_SLOTS)
      return fail("expression reads " + std::to_string(slot_col.size()) +
                  " distinct columns (limit " +
                  std::to_string(EXPR_MAX_SLOTS) + ")");
    if (imm.size() > (size_t)EXPR_MAX_IMM)
      return fail("expression holds " + std::to_string(imm.size()) +
                  " distinct literals (limit " + std::to_string(EXPR_MAX_IMM) +
                  ")");
    *out = ExprProgram{};
    out->n = (int32_t)ins.size();
    out->nslots = (int32_t)slot_col.size();
    out->root_ty = (uint8_t)root;
    out->can_poison = can_poison ? 1 : 0;
    for (size_t i = 0; i < ins.size(); i++) out->ins[i] = ins[i];
    for (size_t i = 0; i < imm.size(); i++) out->imm[i] = imm[i];
    for (size_t i = 0; i < slot_col.size(); i++) {
      out->slot_col[i] = slot_col[i];
      out->slot_ty[i] = slot_ty[i];
    }
    return true;
  }
};

}  // namespace

bool compile_expr(const Expr& e, const std::vector<DType>& in_dtypes,
                  ExprProgram* out, std::string* err) {
  Compiler c(in_dtypes);
  ExprTy root;
  if (!c.gen(e, &root) || !c.finish(root, out)) {
    *err = c.err;
    return false;
  }
  return true;
}

bool compile_filter_program(const std::vector<Expr>& predicates,
                            const std::vector<DType>& in_dtypes,
                            ExprProgram* out, std::string* err) {
  if (predicates.empty()) {
    *err = "FilterExec without predicates";
    return false;
  }
  Compiler c(in_dtypes);
  for (size_t i = 0; i < predicates.size(); i++) {
    ExprTy t;
    if (!c.gen(predicates[i], &t)) {
      *err = c.err;
      return false;
    }
    if (t != ET_BOOL) {
      *err = std::string("filter predicate ") + std::to_string(i) +
             " is " + expr_ty_name(t) + ", not Bool";
      return false;
    }
    if (i > 0) c.emit(EOP_AND, ET_BOOL, 0, 0, -1);
  }
  if (!c.finish(ET_BOOL, out)) {
    *err = c.err;
    return false;
  }
  return true;
}

bool compile_value_program(const Expr& e, const std::vector<DType>& in_dtypes,
                           ExprProgram* out, std::string* err) {
  if (!compile_expr(e, in_dtypes, out, err)) return false;
  if (out->root_ty == ET_BOOL) {
    *err = "expression yields Bool, which has no column type here (wrap in "
           "CASE to produce a number)";
    return false;
  }
  return true;
}

bool expr_result_nullable(const ExprProgram& p, uint32_t slot_nullable) {
  bool st[EXPR_MAX_STACK + 1] = {};
  int sp = 0;  // programs are depth-checked at compile time
  for (int pc = 0; pc < p.n; pc++) {
    const ExprIns in = p.ins[pc];
    switch (in.op) {
      case EOP_LOAD: st[sp++] = (slot_nullable >> in.a) & 1; break;
      case EOP_LIT: st[sp++] = in.b != 0; break;
      case EOP_NEG: case EOP_NOT: break;
      case EOP_ISNULL: case EOP_ISNOTNULL: st[sp - 1] = false; break;
      case EOP_CAST:
        if (in.ty == ET_I64 && in.a == ET_I32) st[sp - 1] = true;
        break;
      case EOP_SELECT:  // then (top) or else (third); the condition is dropped
        st[sp - 3] = st[sp - 1] || st[sp - 3];
        sp -= 2;
        break;
      default:  // binary ops
        st[sp - 2] = st[sp - 2] || st[sp - 1];
        sp -= 1;
    }
  }
  return sp > 0 ? st[sp - 1] : true;
}

std::string expr_program_text(const ExprProgram& p) {
  std::string s = std::string("root=") + expr_ty_name((ExprTy)p.root_ty) +
                  " n=" + std::to_string(p.n) +
                  " poison=" + std::to_string((int)p.can_poison) + " :";
  for (int pc = 0; pc < p.n; pc++) {
    const ExprIns in = p.ins[pc];
    s += std::string(" ") + op_name(in.op);
    if (in.op == EOP_LOAD) {
      s += "(col" + std::to_string(p.slot_col[in.a]) + ":" +
           expr_ty_name((ExprTy)in.ty) + ")";
    } else if (in.op == EOP_LIT) {
      s += std::string("(") + expr_ty_name((ExprTy)in.ty) + ":";
      if (in.b) s += "null";
      else if (in.ty == ET_F64) {
        char buf[40];
        snprintf(buf, sizeof(buf), "%.17g", ev_f64(p.imm[in.a]));
        s += buf;
      } else {
        s += std::to_string((int64_t)p.imm[in.a]);
      }
      s += ")";
    } else if (in.op == EOP_CAST) {
      s += std::string("(") + expr_ty_name((ExprTy)in.ty) + "->" +
           expr_ty_name((ExprTy)in.a) + ")";
    } else if (in.op != EOP_SELECT && in.op < EOP_AND) {
      s += std::string(".") + expr_ty_name((ExprTy)in.ty);
    }
  }
  return s;
}

std::string expr_tree_text(const Expr& e) {
  auto kids = [&](size_t from) {
    std::string s;
    for (size_t i = from; i < e.children.size(); i++) {
      if (i > from) s += ",";
      s += expr_tree_text(e.children[i]);
    }
    return s;
  };
  switch (e.kind) {
    case Expr::Column:
      return "Column(" + e.col_name + "#" + std::to_string(e.col_index) + ")";
    case Expr::Literal: {
      ScalarLit s;
      std::string err;
      if (!decode_ipc_scalar(e.literal_ipc.data(), e.literal_ipc.size(), &s,
                             &err))
        return "Literal(?)";
      std::string v;
      if (s.is_null) v = "null";
      else if (s.dtype == DType::Utf8 || s.dtype == DType::Binary)
        v = "'" + s.utf8 + "'";
      else if (s.dtype == DType::Float64 || s.dtype == DType::Float32) {
        char buf[40];
        snprintf(buf, sizeof(buf), "%.17g", s.f64);
        v = buf;
      } else {
        v = std::to_string(s.i64);
      }
      return std::string("Literal(") + dtype_name(s.dtype) + ":" + v + ")";
    }
    case Expr::BinaryExpr: return e.op + "(" + kids(0) + ")";
    case Expr::IsNull: return "IsNull(" + kids(0) + ")";
    case Expr::IsNotNull: return "IsNotNull(" + kids(0) + ")";
    case Expr::Not: return "Not(" + kids(0) + ")";
    case Expr::Negative: return "Negative(" + kids(0) + ")";
    case Expr::Cast:
      return std::string("Cast(") + kids(0) + " AS " +
             dtype_name(e.cast_type) + ")";
    case Expr::TryCast:
      return std::string("TryCast(") + kids(0) + " AS " +
             dtype_name(e.cast_type) + ")";
    case Expr::SCAnd: return "SCAnd(" + kids(0) + ")";
    case Expr::SCOr: return "SCOr(" + kids(0) + ")";
    case Expr::AggExpr:
      return "Agg" + std::to_string(e.agg_function) + "(" + kids(0) + ")";
    case Expr::Case: {
      std::string s = "Case(";
      size_t lo = e.case_has_base ? 1 : 0;
      size_t hi = e.children.size() - (e.case_has_else ? 1 : 0);
      if (e.case_has_base && !e.children.empty())
        s += "base=" + expr_tree_text(e.children[0]) + ",";
      for (size_t i = lo; i + 1 < hi && hi <= e.children.size(); i += 2)
        s += "when=" + expr_tree_text(e.children[i]) +
             ",then=" + expr_tree_text(e.children[i + 1]) + ",";
      if (e.case_has_else && !e.children.empty())
        s += "else=" + expr_tree_text(e.children.back());
      else
        s += "else=none";
      return s + ")";
    }
  }
  return "?";
}

void expr_eval_host(const ExprProgram& p, const std::vector<ExprHostCol>& cols,
                    int64_t n, uint64_t* out_bits, uint8_t* out_state) {
  for (int64_t row = 0; row < n; row++) {
    auto load = [&](uint8_t slot, uint8_t ty) -> EVal {
      const ExprHostCol& c = cols[p.slot_col[slot]];
      if (c.valid && !c.valid[row]) return EVal{0, ES_NULL};
      uint64_t b;
      if (ty == ET_I32) {
        int32_t v;
        memcpy(&v, (const uint8_t*)c.values + row * 4, 4);
        b = (uint64_t)(int64_t)v;
      } else {
        memcpy(&b, (const uint8_t*)c.values + row * 8, 8);
      }
      return EVal{b, ES_VALID};
    };
    EVal r = expr_eval_row(p, load);
    out_bits[row] = r.st == ES_VALID ? r.b : 0;
    out_state[row] = (uint8_t)r.st;
  }
}

}  // namespace auron
