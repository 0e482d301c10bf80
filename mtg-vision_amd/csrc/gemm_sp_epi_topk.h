// Split GEMM epilogue: the fused top-k of the match path (SP_EPI_TOPK, and SP_EPI_TOPK_LABELS over labelled bank rows).
// Included by gemm_sp_kernel.h, which defines SpDev, spf16 and the helpers used here.
//
// LDS: none - the scores never leave registers, so the launch is sized by the ring alone (gemm_sp_cfg.h, sp_ring).
//
// A lane holds 16 TN columns of its row, its partner lane ^ 32 the other 16 TN; each round picks the (score desc, column
// asc) maximum of the wave's 32 TN columns and retires it.  Candidates: cand[m][(tile_n * WN + wn) * topk + kk];
// topk_merge_kernel finishes.
//
// LABELS (Bank::topk_labelled): a column whose tags fail the row's (all_of, any_of, none_of) masks scores -inf like a
// column past N; with g.distinct the winner's group travels with (score, column) through the lane exchange and the retire
// step retires every column of that group (group >= 0), so a wave range reports its best eligible rows of pairwise
// different groups.  A lane keeps the groups of its 16 TN columns in registers (the operand registers are dead); tags are
// read once per tile and dropped.
//
// One function for both: the scale / -inf pass, the select step, the lane-pair exchange, the candidate store and the
// retire step are shared; LABELS adds the eligibility test and the group that travels with the winner.  Both name a column
// by its compile-time offset sp_topk_off(j, q) from the lane's first column ncolh and take the first strict maximum in
// ascending column order, which is the lowest column among equal scores.
#pragma once

namespace mtgv {

// column of accumulator register q of column block j, counted from the lane's first column
constexpr int sp_topk_off(int j, int q) { return j * 32 + (q >> 2) * 8 + (q & 3); }

// mrow0 / ncol0: first row / column of this wave; cslot: its candidate range, tile_n * WN + wn, of `slots` per row
template <bool LABELS, int TM, int TN>
__device__ __forceinline__ void sp_epi_topk(const SpDev& g, spf16 (&acc)[TM][TN], int mrow0, int ncol0, long cslot, long slots, int r, int h) {
#pragma clang fp contract(off)
  const int ncolh = ncol0 + 4 * h;  // the lane's first column; its columns are ncolh + 32 j + 8 gq + e
  unsigned long m_all[TM], m_any[TM], m_none[TM];
  int grp[TN][16];
  if constexpr (LABELS) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = mrow0 + i * 32 + r;
      const bool mok = g.row_masks != nullptr && m < g.M;
      m_all[i] = mok ? g.row_masks[3 * (long)m] : 0ul;
      m_any[i] = mok ? g.row_masks[3 * (long)m + 1] : 0ul;
      m_none[i] = mok ? g.row_masks[3 * (long)m + 2] : 0ul;
    }
  }
  typedef unsigned long sp_u2 __attribute__((ext_vector_type(2)));
  typedef int sp_i4 __attribute__((ext_vector_type(4)));
  // scale the scores; columns past N (and ineligible ones) score -inf
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int n = ncolh + j * 32 + gq * 8;
      unsigned long tg[4] = {0ul, 0ul, 0ul, 0ul};
      sp_i4 gr = {-1, -1, -1, -1};
      if constexpr (LABELS) {
        if (n + 3 < g.N) {  // a whole quad of columns: 16-byte loads (n % 4 == 0; gemm_sp_topk_labels_launch checks the bases)
          if (g.row_masks != nullptr) {
            const sp_u2 t0 = *reinterpret_cast<const sp_u2*>(g.col_tags + n), t1 = *reinterpret_cast<const sp_u2*>(g.col_tags + n + 2);
            tg[0] = t0[0], tg[1] = t0[1], tg[2] = t1[0], tg[3] = t1[1];
          }
          if (g.distinct != 0) gr = *reinterpret_cast<const sp_i4*>(g.col_groups + n);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (g.row_masks != nullptr && n + e < g.N) tg[e] = g.col_tags[n + e];
            if (g.distinct != 0 && n + e < g.N) gr[e] = g.col_groups[n + e];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool nok = n + e < g.N;
        const float ws = (g.wscale != nullptr && nok) ? g.wscale[n + e] * g.a_unmul : g.a_unmul;
        if constexpr (LABELS) grp[j][4 * gq + e] = gr[e];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          if constexpr (LABELS) {
            // (short-circuit form on purpose: written with & and | the step becomes one straight line, the compiler takes all
            // 48 columns' loads and tests at once and the kernel needs 256 VGPRs and 344 bytes of scratch per lane; in this
            // form it is 236 VGPRs without scratch.  tests/test_gpu_match_labels.py::test_filter runs it at b = 130.)
            const bool el = (tg[e] & m_all[i]) == m_all[i] && (m_any[i] == 0ul || (tg[e] & m_any[i]) != 0ul) && (tg[e] & m_none[i]) == 0ul;
            acc[i][j][4 * gq + e] = (nok && el) ? acc[i][j][4 * gq + e] * ws : -INFINITY;
          } else {
            acc[i][j][4 * gq + e] = nok ? acc[i][j][4 * gq + e] * ws : -INFINITY;
          }
        }
      }
    }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = mrow0 + i * 32 + r;
    for (int kk = 0; kk < g.topk; ++kk) {
      // select: the lane's columns are named by their compile-time offset from ncolh (no register per column index);
      // ascending column order inside the lane, so the first strict maximum has the lowest column
      float bs = -INFINITY;
      int br = -1, bg = -1;
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float v = acc[i][j][q];
          if (v > bs) {
            bs = v, br = sp_topk_off(j, q);
            if constexpr (LABELS) bg = grp[j][q];
          }
        }
      int bi = br >= 0 ? ncolh + br : 0x7fffffff;
      // the better of the lane pair
      const float os = __shfl_xor(bs, 32);
      const int oi = __shfl_xor(bi, 32);
      int og = -1;
      if constexpr (LABELS) og = __shfl_xor(bg, 32);
      if (os > bs || (os == bs && oi < bi)) bs = os, bi = oi, bg = og;
      if (h == 0 && m < g.M) {
        const long o = ((long)m * slots + cslot) * g.topk + kk;
        g.cand_s[o] = bs;
        g.cand_i[o] = (bs == -INFINITY) ? -1 : bi;
      }
      // retire the winner, and with it every column of its group (the partner's winner is 4 columns off every column of
      // this lane: rr matches none of them).  A select per register on purpose: written as `if (hit) acc = -inf` the plain
      // form keeps a branch and a copy of the accumulators per column (profiles/gemm_sp_phases.txt).
      const int rr = bi - ncolh;
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          bool hit = sp_topk_off(j, q) == rr;
          if constexpr (LABELS) hit = hit || (bg >= 0 && grp[j][q] == bg);
          acc[i][j][q] = hit ? -INFINITY : acc[i][j][q];
        }
    }
  }
}

}  // namespace mtgv
