// kernels_expr.hip — k_expr_eval: one fused pass per root expression.
//
//  * The program travels by value in the kernel arguments, so every opcode
//    and operand index is wave-uniform: the switch in expr_eval_row branches
//    on scalars and no lane diverges inside an instruction.
//  * The operand stack is the shift stack of expr_ops.h: eight named values
//    moved by constant index, held in VGPRs (no private-memory array).
//  * Each wave owns 64 consecutive rows per iteration, aligned to 64. Input
//    validity is one 64-bit word per wave and column; output validity is one
//    ballot and one 8-byte store by lane 0, with no atomics. Rows past n vote
//    0, so the tail word's high bits are zero.
//  * Streaming and memory-bound: per row it reads the referenced columns once
//    (4 B or 8 B each) and writes the result once.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "kernels_expr.h"
#include "launch_check.h"

namespace auron {

static constexpr int EXPR_BLOCK = 256;
static constexpr int64_t EXPR_MAX_BLOCKS = 256 * 8;

// The validity word of rows [base, base+64) of one column. `base` is a
// multiple of 64. Whole words of an 8-byte-aligned bitmap are one load; an
// unaligned bitmap or the tail word is assembled from the bytes that exist,
// so nothing past (n+7)/8 bytes is read.
__device__ __forceinline__ uint64_t valid_word(const uint8_t* v, int64_t base,
                                               int64_t n) {
  if (!v) return ~0ull;
  const uint8_t* p = v + (base >> 3);
  if (base + 64 <= n && (((uintptr_t)p) & 7) == 0)
    return *(const uint64_t*)p;
  int64_t nbytes = ((n + 7) >> 3) - (base >> 3);
  if (nbytes > 8) nbytes = 8;
  uint64_t w = 0;
  for (int64_t i = 0; i < nbytes; i++) w |= (uint64_t)p[i] << (8 * i);
  return w;
}

__global__ __launch_bounds__(EXPR_BLOCK) void k_expr_eval(ExprKernArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t n = a.n;
  uint32_t poisoned = 0;
  for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
    const bool active = base + lane < n;
    // lanes past n recompute the last row: every load stays in bounds and no
    // lane leaves the wave-uniform instruction stream
    const int64_t row = active ? base + lane : n - 1;
    const int64_t vbit = row - base;
    auto load = [&](uint8_t slot, uint8_t ty) -> EVal {
      uint64_t w = valid_word(a.valid[slot], base, n);
      uint64_t bits;
      if (ty == ET_I32)
        bits = (uint64_t)(int64_t)((const int32_t*)a.vals[slot])[row];
      else
        bits = ((const uint64_t*)a.vals[slot])[row];
      bool ok = (w >> vbit) & 1;
      return EVal{ok ? bits : 0, ok ? (uint32_t)ES_VALID : (uint32_t)ES_NULL};
    };
    EVal r = expr_eval_row(a.prog, load);
    const bool ok = active && r.st == ES_VALID;
    if (active && r.st == ES_POISON) poisoned = 1;
    const uint64_t bits = ok ? r.b : 0;
    if (a.out_mask) {
      if (active) a.out_mask[row] = (uint8_t)(ok && bits != 0);
    } else {
      if (active) {
        if (a.out_width == 4) ((uint32_t*)a.out_vals)[row] = (uint32_t)bits;
        else ((uint64_t*)a.out_vals)[row] = bits;
      }
      if (a.out_valid) {
        uint64_t word = __ballot(ok);
        if (lane == 0) a.out_valid[base >> 6] = word;
      }
    }
  }
  if (poisoned) *a.error_flag = 1u;  // same value from every writer
}

void launch_expr_eval(const ExprKernArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  if (a.prog.n <= 0 || a.prog.n > EXPR_MAX_INS ||
      a.prog.nslots > EXPR_MAX_SLOTS)
    throw std::runtime_error("k_expr_eval: malformed program");
  if (!a.error_flag || (!a.out_mask && !a.out_vals))
    throw std::runtime_error("k_expr_eval: missing output buffers");
  for (int i = 0; i < a.prog.nslots; i++)
    if (!a.vals[i]) throw std::runtime_error("k_expr_eval: null input column");
  int64_t blocks = (a.n + EXPR_BLOCK - 1) / EXPR_BLOCK;
  if (blocks > EXPR_MAX_BLOCKS) blocks = EXPR_MAX_BLOCKS;
  hipLaunchKernelGGL(k_expr_eval, dim3((unsigned)blocks), dim3(EXPR_BLOCK), 0,
                     s, a);
  check_launch("k_expr_eval");
}

}  // namespace auron
