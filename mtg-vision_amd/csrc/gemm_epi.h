// Convert-on-load GEMM epilogue that is a function of its own: the LayerNorm store (EPI 2).
// Included by gemm_kernel.h, which defines f32x16, gemm_c_row and gemm_scale_bias.  The top-k epilogue and the GRN partial
// sums are written in the kernel body on purpose: as functions they cost scratch or time (profiles/gemm_kernel_phases.txt).
#pragma once

namespace mtgv {

// LayerNorm over the row, interior tiles only (the tile holds all N = BN columns of its rows: gemm_ln_fusable): a row's
// values sit in the 32 lanes of one half-wave x TN column blocks; sums over the blocks in j order, then a butterfly over
// the lanes (the same two-pass form as ln_rows_kernel: mean, then the squared deviations).
// obase + loff: this lane's element of the wave's first output row (the interior store's addressing)
template <int TN, int PREC>
__device__ __forceinline__ void gemm_epi_ln(const f32x16 (&acc)[TN], const float (&bv)[TN], const float (&wsv)[TN], const float* ln_w,
                                            const float* ln_b, float ln_eps, float* obase, int ldo, unsigned loff, int col) {
#pragma clang fp contract(off)
  constexpr int BN = 32 * TN;
  float lw[TN], lb[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) lw[j] = ln_w[j * 32 + col], lb[j] = ln_b[j * 32 + col];
  const float inv_n = 1.0f / (float)BN;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long rr = gemm_c_row(r);
    float v[TN];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      v[j] = gemm_scale_bias<PREC>(acc[j][r], wsv[j], bv[j]);
      sum += v[j];
    }
#pragma unroll
    for (int m = 16; m > 0; m >>= 1) sum += __shfl_xor(sum, m);
    const float mean = sum * inv_n;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      v[j] -= mean;
      sq += v[j] * v[j];
    }
#pragma unroll
    for (int m = 16; m > 0; m >>= 1) sq += __shfl_xor(sq, m);
    const float rstd = 1.0f / sqrtf(sq * inv_n + ln_eps);
#pragma unroll
    for (int j = 0; j < TN; ++j) (obase + rr * ldo + j * 32)[loff] = v[j] * rstd * lw[j] + lb[j];
  }
}

}  // namespace mtgv
