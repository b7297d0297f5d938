// kernels_expr.h — launch API of k_expr_eval (kernels_expr.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "expr_ops.h"

namespace auron {

// Everything k_expr_eval needs, passed by value. vals/valid are indexed by
// program slot (prog.slot_col maps a slot to its input column).
struct ExprKernArgs {
  ExprProgram prog;
  const void* vals[EXPR_MAX_SLOTS];
  const uint8_t* valid[EXPR_MAX_SLOTS];  // LSB bitmap; nullptr = all valid
  int64_t n;
  // mask mode: out_mask[n], 1 only where the root is valid and true
  uint8_t* out_mask;
  // value mode: out_vals[n] at out_width (4 or 8) bytes, null rows 0;
  // out_valid holds (n+63)/64 words, or nullptr for a non-nullable result
  void* out_vals;
  uint64_t* out_valid;
  int32_t out_width;
  uint32_t* error_flag;  // set to 1 if poison reaches the root of any row
};

void launch_expr_eval(const ExprKernArgs& a, hipStream_t s);

}  // namespace auron
