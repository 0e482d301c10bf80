// Packed copies of constant B operands (weights, the bank) for the f16x3 mode, one registry for both GEMM kernels:
//   SP8 copy + per-row power-of-two scales (sp8.h): what the LDS-DMA kernel (gemm_sp.h) and the fused MLP read by DMA;
//   split copy: every aligned group of 4 floats replaced by its 4 fp16 hi + 4 fp16 lo halves (same byte layout, same
//   offsets), so the convert-on-load kernel (gemm_kernel.h) moves ready halves instead of converting the same weights
//   in every block; rows with an SP8 copy are stored scaled by 1 / wscale[row].
// An owner registers the base pointer of a buffer it allocated, refreshes a range after writing it, and unregisters
// before freeing.  Unregistered operands are split on the fly.
#pragma once
#include "common.h"

namespace mtgv {

// [n_floats / row_k][row_k] f32 at W (16-byte aligned).  The SP8 copy is kept when row_k is a positive multiple of 8 that
// divides n_floats; the split copy when `split` is set, and then only buffers of >= 64 floats, a multiple of 4, are
// registered at all (small vectors are skipped).  Registering the same base with the same shape again keeps the copies.
void operand_register(const float* W, size_t n_floats, int row_k, bool split = true);
// packs whole rows of the range on `s`: SP8 (which computes the rows' scales) first, then the split copy scaled by them
void operand_refresh(const float* W, size_t offset_floats, size_t n_floats, hipStream_t s);
void operand_unregister(const float* W);
bool operand_registered(const float* W);  // by base pointer
// SP8 rows and scales for the operand at `W` (base or a row-aligned interior pointer of a registered buffer) when its
// rows are K long; false if there is none
bool operand_sp8(const float* W, int K, const char** sp8, const float** wscale);
// split copy for a launch with rows of K floats, by exact base pointer only: unscaled copies always (*wscale = null),
// scaled ones only when K is their row length, with their scales; null if there is none
const float* operand_split(const float* W, int K, const float** wscale);

}  // namespace mtgv
