// expr.h — host-side expression compiler: Expr tree + input column dtypes ->
// type-checked postfix ExprProgram (expr_ops.h), plus a host interpreter that
// runs the same per-row evaluator as the kernel. Host-pure (no HIP).
#pragma once

#include <string>
#include <vector>

#include "expr_ops.h"
#include "plan.h"

namespace auron {

const char* expr_ty_name(ExprTy t);
DType expr_ty_dtype(ExprTy t);  // Bool has no column type: Unsupported

// Compile `e` over input columns of the given dtypes. On failure returns
// false with the cause in *err.
bool compile_expr(const Expr& e, const std::vector<DType>& in_dtypes,
                  ExprProgram* out, std::string* err);

// FilterExec: all predicates AND-ed into one program with a Bool root.
bool compile_filter_program(const std::vector<Expr>& predicates,
                            const std::vector<DType>& in_dtypes,
                            ExprProgram* out, std::string* err);

// ProjectionExec / Agg input: one computed output column. A Bool root has no
// column type and fails ("wrap in CASE").
bool compile_value_program(const Expr& e, const std::vector<DType>& in_dtypes,
                           ExprProgram* out, std::string* err);

// Can the root be null, given which input slots carry a validity bitmap
// (bit s of slot_nullable)? False lets the kernel skip the output bitmap.
bool expr_result_nullable(const ExprProgram& p, uint32_t slot_nullable);

std::string expr_program_text(const ExprProgram& p);
std::string expr_tree_text(const Expr& e);

// Host column for the interpreter: values at the column's width, one
// validity byte per row (nullptr = all valid).
struct ExprHostCol {
  const void* values = nullptr;
  const uint8_t* valid = nullptr;
};

// Run `p` over n rows. cols is indexed by input column. out_bits receives the
// value bits (0 on null / poison rows), out_state the ExprState per row.
void expr_eval_host(const ExprProgram& p, const std::vector<ExprHostCol>& cols,
                    int64_t n, uint64_t* out_bits, uint8_t* out_state);

}  // namespace auron
