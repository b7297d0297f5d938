// expr_ops.h — the expression program format and its per-row evaluator,
// shared verbatim by k_expr_eval (kernels_expr.hip) and the host interpreter
// (expr.cpp). Host-pure: no HIP headers; EXPR_HD adds the device attributes
// only under hipcc.
//
// A program is a type-checked postfix sequence over an operand stack of at
// most EXPR_MAX_STACK values. Every value carries a state: valid, null, or
// poison (an integer division error on that row). Poison outranks null and
// only the ops that discard an operand (SELECT, SCAND, SCOR) can drop it.
#pragma once

#include <cstdint>

#include <math.h>

#if defined(__HIPCC__)
#define EXPR_HD __host__ __device__
#else
#define EXPR_HD
#endif

// The reference materialises every intermediate array, so a multiply feeding
// an add rounds twice, while hipcc contracts device code to FMA by default.
// EXPR_NO_FMA opens every function that does float arithmetic: instructions
// emitted under it carry no contract flag, so they never fuse, wherever they
// are inlined. (Function scope, so including this header changes no other
// code in the translation unit.)
#if defined(__clang__)
#define EXPR_NO_FMA _Pragma("clang fp contract(off)")
#else
#define EXPR_NO_FMA
#endif

namespace auron {

constexpr int EXPR_MAX_INS = 64;
constexpr int EXPR_MAX_STACK = 8;
constexpr int EXPR_MAX_SLOTS = 8;   // distinct input columns
constexpr int EXPR_MAX_IMM = 16;    // literals

enum ExprTy : uint8_t { ET_I32 = 0, ET_I64 = 1, ET_F64 = 2, ET_BOOL = 3 };
enum ExprState : uint32_t { ES_VALID = 0, ES_NULL = 1, ES_POISON = 2 };

enum ExprOp : uint8_t {
  EOP_LOAD,    // a = input slot, ty = column type
  EOP_LIT,     // a = imm index, ty = literal type, b = 1 for a typed NULL
  EOP_ADD, EOP_SUB, EOP_MUL, EOP_DIV, EOP_MOD,   // ty = operand type
  EOP_NEG,                                       // ty = operand type
  EOP_EQ, EOP_NE, EOP_LT, EOP_LE, EOP_GT, EOP_GE,  // ty = operand type
  EOP_AND, EOP_OR, EOP_SCAND, EOP_SCOR, EOP_NOT,
  EOP_ISNULL, EOP_ISNOTNULL,
  EOP_CAST,    // ty = source type, a = target type
  EOP_SELECT,  // pops then, cond, else (top first); pushes the taken one
};

struct ExprIns {
  uint8_t op, ty, a, b;
};

struct ExprProgram {
  int32_t n = 0;
  int32_t nslots = 0;
  uint8_t root_ty = ET_I32;
  uint8_t can_poison = 0;
  uint8_t slot_ty[EXPR_MAX_SLOTS] = {};
  uint32_t slot_col[EXPR_MAX_SLOTS] = {};  // input column index per slot
  ExprIns ins[EXPR_MAX_INS] = {};
  uint64_t imm[EXPR_MAX_IMM] = {};
};

// I32 values live sign-extended in the low half of `b`; BOOL is 0 or 1;
// F64 is the IEEE bit pattern. A null or poison value has b == 0.
struct EVal {
  uint64_t b;
  uint32_t st;
};

EXPR_HD inline double ev_f64(uint64_t b) {
  return __builtin_bit_cast(double, b);
}
EXPR_HD inline uint64_t ev_bits(double d) {
  return __builtin_bit_cast(uint64_t, d);
}
EXPR_HD inline uint64_t ev_sext32(uint32_t x) {
  return (uint64_t)(int64_t)(int32_t)x;
}

EXPR_HD inline uint32_t ev_state2(const EVal& x, const EVal& y) {
  if (x.st == ES_POISON || y.st == ES_POISON) return ES_POISON;
  if (x.st == ES_NULL || y.st == ES_NULL) return ES_NULL;
  return ES_VALID;
}

// Plus / Minus / Multiply: integers wrap at the operand width.
EXPR_HD inline EVal ev_arith(uint8_t op, uint8_t ty, const EVal& x,
                             const EVal& y) {
  EXPR_NO_FMA
  EVal r{0, ev_state2(x, y)};
  if (r.st != ES_VALID) return r;
  if (ty == ET_F64) {
    double a = ev_f64(x.b), c = ev_f64(y.b), d;
    if (op == EOP_ADD) d = a + c;
    else if (op == EOP_SUB) d = a - c;
    else d = a * c;
    r.b = ev_bits(d);
  } else if (ty == ET_I64) {
    uint64_t a = x.b, c = y.b;
    r.b = op == EOP_ADD ? a + c : op == EOP_SUB ? a - c : a * c;
  } else {
    uint32_t a = (uint32_t)x.b, c = (uint32_t)y.b;
    uint32_t d = op == EOP_ADD ? a + c : op == EOP_SUB ? a - c : a * c;
    r.b = ev_sext32(d);
  }
  return r;
}

// Divide / Modulo: integers truncate toward zero, the remainder takes the
// dividend's sign; a zero divisor or MIN op -1 poisons the row.
EXPR_HD inline EVal ev_divmod(uint8_t op, uint8_t ty, const EVal& x,
                              const EVal& y) {
  EXPR_NO_FMA
  EVal r{0, ev_state2(x, y)};
  if (r.st != ES_VALID) return r;
  if (ty == ET_F64) {
    double a = ev_f64(x.b), c = ev_f64(y.b);
    r.b = ev_bits(op == EOP_DIV ? a / c : fmod(a, c));
  } else if (ty == ET_I64) {
    int64_t a = (int64_t)x.b, c = (int64_t)y.b;
    if (c == 0 || (a == INT64_MIN && c == -1)) {
      r.st = ES_POISON;
    } else {
      r.b = (uint64_t)(op == EOP_DIV ? a / c : a % c);
    }
  } else {
    int32_t a = (int32_t)(uint32_t)x.b, c = (int32_t)(uint32_t)y.b;
    if (c == 0 || (a == INT32_MIN && c == -1)) {
      r.st = ES_POISON;
    } else {
      r.b = ev_sext32((uint32_t)(op == EOP_DIV ? a / c : a % c));
    }
  }
  return r;
}

EXPR_HD inline EVal ev_neg(uint8_t ty, const EVal& x) {
  EXPR_NO_FMA
  EVal r{0, x.st};
  if (r.st != ES_VALID) return r;
  if (ty == ET_F64) r.b = ev_bits(-ev_f64(x.b));
  else if (ty == ET_I64) r.b = 0 - x.b;
  else r.b = ev_sext32(0u - (uint32_t)x.b);
  return r;
}

// Comparisons use the plain C++ operators, as k_cmp_lit does: NaN compares
// false under everything but NotEq, and -0.0 equals 0.0.
EXPR_HD inline EVal ev_cmp(uint8_t op, uint8_t ty, const EVal& x,
                           const EVal& y) {
  EVal r{0, ev_state2(x, y)};
  if (r.st != ES_VALID) return r;
  bool t;
  if (ty == ET_F64) {
    double a = ev_f64(x.b), c = ev_f64(y.b);
    t = op == EOP_EQ ? a == c : op == EOP_NE ? a != c : op == EOP_LT ? a < c
        : op == EOP_LE ? a <= c : op == EOP_GT ? a > c : a >= c;
  } else {  // I32 is sign-extended, so both integer widths compare as i64
    int64_t a = (int64_t)x.b, c = (int64_t)y.b;
    t = op == EOP_EQ ? a == c : op == EOP_NE ? a != c : op == EOP_LT ? a < c
        : op == EOP_LE ? a <= c : op == EOP_GT ? a > c : a >= c;
  }
  r.b = t ? 1 : 0;
  return r;
}

// Kleene And / Or. `sc` drops poison on the right where the left decides.
EXPR_HD inline EVal ev_logic(bool is_or, bool sc, const EVal& x,
                             const EVal& y) {
  const uint64_t decides = is_or ? 1 : 0;  // the absorbing truth value
  if (x.st == ES_POISON) return EVal{0, ES_POISON};
  bool x_decides = x.st == ES_VALID && x.b == decides;
  if (y.st == ES_POISON) {
    if (sc && x_decides) return EVal{decides, ES_VALID};
    return EVal{0, ES_POISON};
  }
  bool y_decides = y.st == ES_VALID && y.b == decides;
  if (x_decides || y_decides) return EVal{decides, ES_VALID};
  if (x.st == ES_NULL || y.st == ES_NULL) return EVal{0, ES_NULL};
  return EVal{decides ^ 1, ES_VALID};
}

// Float64 -> integer: truncate toward zero, saturate, NaN -> 0 (Rust `as`).
EXPR_HD inline int64_t ev_f64_to_i64(double d) {
  if (d != d) return 0;
  if (d >= 9223372036854775808.0) return INT64_MAX;
  if (d <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)d;
}
EXPR_HD inline int32_t ev_f64_to_i32(double d) {
  if (d != d) return 0;
  if (d >= 2147483647.0) return INT32_MAX;
  if (d <= -2147483648.0) return INT32_MIN;
  return (int32_t)d;
}

EXPR_HD inline EVal ev_cast(uint8_t from, uint8_t to, const EVal& x) {
  EVal r{0, x.st};
  if (r.st != ES_VALID || from == to) {
    r.b = r.st == ES_VALID ? x.b : 0;
    return r;
  }
  if (from == ET_I32) {
    // sign-extended already: Int64 takes the bits as they are
    r.b = to == ET_I64 ? x.b : ev_bits((double)(int32_t)(uint32_t)x.b);
  } else if (from == ET_I64) {
    int64_t v = (int64_t)x.b;
    if (to == ET_F64) {
      r.b = ev_bits((double)v);
    } else if (v < INT32_MIN || v > INT32_MAX) {
      r.st = ES_NULL;  // arrow's safe cast: out of range -> null
    } else {
      r.b = x.b;
    }
  } else {
    double d = ev_f64(x.b);
    r.b = to == ET_I64 ? (uint64_t)ev_f64_to_i64(d)
                       : ev_sext32((uint32_t)ev_f64_to_i32(d));
  }
  return r;
}

// Evaluate one row. `load(slot, ty)` returns the row's value of an input
// column. The stack is eight named values moved by constant index (a shift
// stack), so on the device it stays in registers.
template <class Load>
EXPR_HD inline EVal expr_eval_row(const ExprProgram& p, Load& load) {
  EVal s0{0, ES_NULL}, s1 = s0, s2 = s0, s3 = s0, s4 = s0, s5 = s0, s6 = s0,
       s7 = s0;
#define EV_PUSH(v)                                                         \
  do {                                                                     \
    EVal nv_ = (v);                                                        \
    s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0;         \
    s0 = nv_;                                                              \
  } while (0)
#define EV_BIN(v)                                                          \
  do {                                                                     \
    EVal nv_ = (v);                                                        \
    s0 = nv_;                                                              \
    s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;                  \
  } while (0)
  for (int pc = 0; pc < p.n; pc++) {
    const ExprIns in = p.ins[pc];
    switch (in.op) {
      case EOP_LOAD: EV_PUSH(load(in.a, in.ty)); break;
      case EOP_LIT:
        EV_PUSH((in.b ? EVal{0, ES_NULL} : EVal{p.imm[in.a], ES_VALID}));
        break;
      case EOP_ADD: case EOP_SUB: case EOP_MUL:
        EV_BIN(ev_arith(in.op, in.ty, s1, s0));
        break;
      case EOP_DIV: case EOP_MOD:
        EV_BIN(ev_divmod(in.op, in.ty, s1, s0));
        break;
      case EOP_NEG: s0 = ev_neg(in.ty, s0); break;
      case EOP_EQ: case EOP_NE: case EOP_LT: case EOP_LE: case EOP_GT:
      case EOP_GE:
        EV_BIN(ev_cmp(in.op, in.ty, s1, s0));
        break;
      case EOP_AND: EV_BIN(ev_logic(false, false, s1, s0)); break;
      case EOP_OR: EV_BIN(ev_logic(true, false, s1, s0)); break;
      case EOP_SCAND: EV_BIN(ev_logic(false, true, s1, s0)); break;
      case EOP_SCOR: EV_BIN(ev_logic(true, true, s1, s0)); break;
      case EOP_NOT:
        if (s0.st == ES_VALID) s0.b ^= 1;
        break;
      case EOP_ISNULL: case EOP_ISNOTNULL:
        if (s0.st != ES_POISON) {
          bool isnull = s0.st == ES_NULL;
          s0 = EVal{(uint64_t)((in.op == EOP_ISNULL) == isnull), ES_VALID};
        }
        break;
      case EOP_CAST: s0 = ev_cast(in.ty, in.a, s0); break;
      case EOP_SELECT: {
        // s2 = else, s1 = cond, s0 = then. A poisoned condition poisons the
        // row; a null one is not taken. Only the taken branch survives.
        EVal r = s1.st == ES_POISON ? EVal{0, ES_POISON}
                 : (s1.st == ES_VALID && s1.b) ? s0 : s2;
        s0 = r;
        s1 = s3; s2 = s4; s3 = s5; s4 = s6; s5 = s7;
        break;
      }
      default: break;
    }
  }
#undef EV_PUSH
#undef EV_BIN
  return s0;
}

}  // namespace auron
