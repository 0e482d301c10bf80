// Exact cosine top-k over the whole card bank (what Qdrant's HNSW index approximates;
// mtgvision/qdrant.py:76-95).  Bank rows are stored L2-normalised, so cosine = dot:
//   1. l2norm_rows_kernel        q -> q/|q|
//   2. gemm_f32 (EPI=1)          S tile = Q B^T on f32 MFMA, per-tile top-k in registers
//   3. topk_merge_kernel         tiles_n*k candidates per query -> top k (score desc, id asc)
#include "match.h"
#include "gemm_sp.h"
#include "operand_registry.h"
#include "rowops.h"
#include "sp8.h"

#include <stdlib.h>

namespace mtgv {

// One result slot.  out_scores == nullptr selects the exchange format of the sharded match (mtgv/dist.py): out_ids is
// then [slots][2] int64 = (id, the score's float32 bit pattern zero-extended) - one buffer, one all-gather.
__device__ __forceinline__ void store_result(long* __restrict__ out_ids, float* __restrict__ out_scores, long slot, long id, float score) {
  if (out_scores != nullptr) {
    out_scores[slot] = score;
    out_ids[slot] = id;
  } else {
    out_ids[2 * slot] = id;
    out_ids[2 * slot + 1] = (long)__float_as_uint(score);
  }
}

// The labelled exchange format (Bank::topk_packed_labelled): word 1 also carries the row's group in its high half (uint32;
// -1 = 0xFFFFFFFF, pads too), which is all the cross-shard merge needs to dedupe; readers of the unlabelled format take
// the low half only.
__device__ __forceinline__ long pack_score_group(float score, int group) {
  return (long)(((unsigned long)(unsigned)group << 32) | (unsigned long)__float_as_uint(score));
}
__device__ __forceinline__ void store_result(long* __restrict__ packed, long slot, long id, float score, int group) {
  packed[2 * slot] = id;
  packed[2 * slot + 1] = pack_score_group(score, group);
}

// the labelled exchange message of an empty shard: every slot a pad (id -1, -inf, group -1)
__global__ __launch_bounds__(256) void packed_pads_kernel(long* __restrict__ packed, long slots) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < slots) store_result(packed, i, -1, -INFINITY, -1);
}

// ---------------------------------------------------------------------------
// The one selection step and the one merge body of every top-k merge.  The contract, on a single bank and across
// shards alike (same ids, same score bits): order by score descending, then id ascending; an id < 0 is a pad and never
// takes part; the threshold is applied last - a representative below it becomes a pad and is not replaced; a picked
// group >= 0 retires its other candidates; picks never depend on which rank a candidate came from.
// ---------------------------------------------------------------------------
template <typename IdT>
__device__ __forceinline__ bool better(float v, IdT i, float bs, IdT bi) {
  return v > bs || (v == bs && i < bi);
}

// a thread's proposal rule: candidate (v, i) at position p replaces the thread's best so far unless it is a pad (i < 0)
// or retired (-inf)
template <typename IdT>
__device__ __forceinline__ void propose(float v, IdT i, int p, float& bs, IdT& bi, int& bp) {
  if (i >= 0 && v > -INFINITY && better(v, i, bs, bi)) bs = v, bi = i, bp = p;
}

// Block selection: every thread hands in its best (score, id, position), position < 0 for none; a 256-thread LDS tree
// leaves the block's winner in rs[0], ri[0], rp[0] (rp[0] < 0: nothing left), visible to every thread on return.
// CONTAINS BARRIERS: call it from block-uniform control flow only, and put a barrier between the last read of the
// winner and the next call, which overwrites it.
template <typename IdT>
__device__ __forceinline__ void block_pick(float bs, IdT bi, int bp, float* rs, IdT* ri, int* rp, int tid) {
  rs[tid] = bs, ri[tid] = bi, rp[tid] = bp;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      const float os = rs[tid + st];
      const IdT oi = ri[tid + st];
      const int op = rp[tid + st];
      if (op >= 0 && (rp[tid] < 0 || better(os, oi, rs[tid], ri[tid]))) rs[tid] = os, ri[tid] = oi, rp[tid] = op;
    }
    __syncthreads();
  }
}

// The k rounds of a merge over the candidates of one query: pick, apply the threshold, emit, retire the winner - with
// DISTINCT the winner's whole group, if it has one (>= 0).  View: n candidates with score(p), id(p), group(p) (read with
// DISTINCT only) and retire(p); LAZY_ID views keep their ids far away, so an id is read only where its candidate leads
// or ties.  emit(kk, ok, id, score) writes result kk; !ok: a pad.  CONTAINS BARRIERS, like block_pick.
template <bool DISTINCT, typename View, typename Emit>
__device__ __forceinline__ void merge_rounds(View c, int k, float thr, Emit emit) {
  __shared__ float rs[256];
  __shared__ long ri[256];
  __shared__ int rp[256];
  const int tid = threadIdx.x;
  for (int kk = 0; kk < k; ++kk) {
    float bs = -INFINITY;
    long bi = 0x7fffffffffffffffL;
    int bp = -1;
    for (int p = tid; p < c.n; p += 256) {
      const float v = c.score(p);
      if (View::LAZY_ID && !(v > -INFINITY && v >= bs)) continue;
      propose(v, c.id(p), p, bs, bi, bp);
    }
    block_pick(bs, bi, bp, rs, ri, rp, tid);
    const int wp = rp[0];  // the winner is overwritten only after the barrier below
    // score_threshold (qdrant.py:83,93): candidates below it are not results - id -1 / score -inf pads, like a bank with
    // fewer than k rows.  It comes last: a representative below it is a pad, not replaced.
    if (tid == 0) emit(kk, wp >= 0 && rs[0] >= thr, ri[0], rs[0]);
    if (wp >= 0) {
      int wg = -1;
      if constexpr (DISTINCT) wg = c.group(wp);
      if (wg >= 0) {
        for (int p = tid; p < c.n; p += 256)
          if (c.group(p) == wg) c.retire(p);  // the winner with its group
      } else if (tid == 0) {
        c.retire(wp);
      }
    }
    __syncthreads();
  }
}

// Candidates in HBM, ids are bank rows: a candidate's group is groups[id] (a pad has none).
template <typename IdT>
struct HbmCandidates {
  static constexpr bool LAZY_ID = false;
  float* __restrict__ s;
  const IdT* __restrict__ ids;
  const int* __restrict__ groups;
  int n;
  __device__ __forceinline__ float score(int p) const { return s[p]; }
  __device__ __forceinline__ long id(int p) const { return (long)ids[p]; }
  __device__ __forceinline__ int group(int p) const { return ids[p] >= 0 ? groups[ids[p]] : -1; }
  __device__ __forceinline__ void retire(int p) const { s[p] = -INFINITY; }
};

// DISTINCT (labelled matches, Bank::topk_labelled): after a pick every candidate of the winner's group (>= 0) is retired
// with it.  The candidate ranges dedupe too (gemm_sp_kernel.h SP_EPI_TOPK_LABELS, gemm_kernel.h EPI 3): a merge-only
// dedupe would miss rows hidden inside a range.
// PACK_GROUP: out_ids is the labelled exchange format (out_scores is not read).
template <typename IdT, bool DISTINCT = false, bool PACK_GROUP = false>
__global__ __launch_bounds__(256) void topk_merge_kernel(float* __restrict__ cs, const IdT* __restrict__ ci, int ncand, int k,
                                                        long id_base, float thr, long* __restrict__ out_ids,
                                                        float* __restrict__ out_scores, const int* __restrict__ groups = nullptr) {
  const int b = blockIdx.x;
  const HbmCandidates<IdT> c{cs + (long)b * ncand, ci + (long)b * ncand, groups, ncand};
  merge_rounds<DISTINCT>(c, k, thr, [&](int kk, bool ok, long id, float score) {
    if constexpr (PACK_GROUP)
      store_result(out_ids, (long)b * k + kk, ok ? id + id_base : -1, ok ? score : -INFINITY, ok ? groups[id] : -1);
    else
      store_result(out_ids, out_scores, (long)b * k + kk, ok ? id + id_base : -1, ok ? score : -INFINITY);
  });
}

// ---------------------------------------------------------------------------
// Two-pass match for query batches (>= 128 queries, K % 64 == 0, k <= 4).
//   pass 1  gemm_sp_kernel<..., AMODE 6, EPI 16>: fp16 x fp16 products of the hi halves only (one MFMA per product instead
//           of three, half the bank bytes: 154 MB for 100k x 768, which stays in the Infinity Cache); per 96-column wave
//           range the KP = 2 best approximate scores
//   pass 2  rerank_kernel, one block per query: the R = 8 best reported candidates are scored exactly (f32 master rows,
//           float64 accumulation) and the top k of those are the answer - PROVIDED no other column can beat them:
//           every column that was not re-ranked has an approximate score <= B = max(a_R, max over ranges of the range's
//           last reported score), and approximate and exact scores differ by at most EPS (both operands rounded to
//           fp16: 2 * 2^-11 * sum |q_k b_k| <= 2^-10 for unit vectors, plus f32 accumulation).  If the k-th exact score
//           is below B + EPS the block scores exactly every row that could still enter: the reported candidates whose own
//           approximate score comes within EPS of it and all columns of the wave ranges whose cut-off does (typically
//           one or two ranges; banks with many near-duplicates of a query's best match scan more).
// The answer is therefore always the exact top k (score desc, id asc), like the one-pass path's.
// ---------------------------------------------------------------------------
constexpr int PRE_KP = 2;     // candidates per wave range
constexpr int PRE_R = 8;      // candidates re-ranked per query
constexpr float PRE_EPS = 1.1e-3f;

__global__ __launch_bounds__(256) void f32_to_f16_rows_kernel(const float* __restrict__ in, const float* __restrict__ wscale,
                                                             _Float16* __restrict__ out, long rows, int K) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // one thread per 8 elements
  const int k8 = K / 8;
  if (i >= rows * k8) return;
  const long row = i / k8;
  const float sc = wscale != nullptr ? 1.0f / wscale[row] : 1.0f;  // exact: a power of two
  const sp_f4 a = *reinterpret_cast<const sp_f4*>(in + i * 8) * sc, b = *reinterpret_cast<const sp_f4*>(in + i * 8 + 4) * sc;
  sp_h8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (_Float16)a[e], o[4 + e] = (_Float16)b[e];
  *reinterpret_cast<sp_h8*>(out + i * 8) = o;
}

static void f32_to_f16_rows_launch(const float* in, const float* wscale, _Float16* out, long rows, int K, hipStream_t s) {
  const long n8 = rows * (K / 8);
  hipLaunchKernelGGL(f32_to_f16_rows_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, in, wscale, out, rows, K);
  HIP_OK(hipGetLastError());
}

// exact score of (query, bank row): float64 sum of the f32 products, 64 lanes over k, fixed reduction order
__device__ __forceinline__ float exact_dot_wave(const float* __restrict__ q, const float* __restrict__ row, int K, int lane) {
  double acc = 0.0;
  for (int k = lane * 4; k < K; k += 256) {
    const sp_f4 a = *reinterpret_cast<const sp_f4*>(q + k), b = *reinterpret_cast<const sp_f4*>(row + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += (double)a[e] * (double)b[e];
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
  return (float)acc;
}

// four rows at once, 16 lanes each (the rescoring scan: independent loads in flight); lane group g = lane >> 4 scores
// rows[g] (< 0: none) and every lane of the group returns the row's score
__device__ __forceinline__ float exact_dot_quad(const float* __restrict__ q, const float* __restrict__ bank, long row, int K, int lane) {
  double acc = 0.0;
  if (row >= 0) {
    const float* r = bank + row * K;
    for (int k = (lane & 15) * 4; k < K; k += 64) {
      const sp_f4 a = *reinterpret_cast<const sp_f4*>(q + k), b = *reinterpret_cast<const sp_f4*>(r + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc += (double)a[e] * (double)b[e];
    }
  }
#pragma unroll
  for (int m = 8; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
  return (float)acc;
}

// insert (e, i) into a descending (score desc, id asc) list of k entries held in registers (every lane of the wave alike)
__device__ __forceinline__ void topk_insert(float (&bs)[8], long (&bi)[8], int k, float e, long i) {
  for (int kk = 0; kk < k; ++kk)
    if (bi[kk] < 0 || e > bs[kk] || (e == bs[kk] && i < bi[kk])) {
      const float te = bs[kk];
      const long ti = bi[kk];
      bs[kk] = e, bi[kk] = i, e = te, i = ti;
      if (i < 0) break;
    }
}

__global__ __launch_bounds__(256) void rerank_kernel(const float* __restrict__ qn, const float* __restrict__ bank, long nrows, int K,
                                                    const float* __restrict__ cand_s, const int* __restrict__ cand_i, int slots,
                                                    int range_cols, int k, long id_base, float thr, long* __restrict__ out_ids,
                                                    float* __restrict__ out_scores, int* __restrict__ n_fallback) {
  __shared__ float rs[256];
  __shared__ int ri[256], rp[256];
  __shared__ int sel_p[PRE_R];
  __shared__ float fs[4][8];
  __shared__ long fi[4][8];
  __shared__ float s_cut, s_kth, s_aR;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncand = slots * PRE_KP;
  const float* cs = cand_s + (long)b * ncand;
  const int* ci = cand_i + (long)b * ncand;
  const float* q = qn + (long)b * K;
  // A query without a direction (all zeros: a row that a budgeted tracker step pads its queries with) scores exactly 0 on
  // every row, so its exact answer is known: the k first rows.  Without this the bound below can prove nothing - every
  // approximate score ties at 0 - and the block would score the whole bank exactly and count as a fallback.
  {
    bool nonzero = false;
    for (int c = tid; c < K; c += 256) nonzero |= q[c] != 0.f;
    if (!__syncthreads_or(nonzero)) {  // (the whole block)
      if (tid == 0)
        for (int kk = 0; kk < k; ++kk) {
          const bool ok = kk < nrows && 0.f >= thr;
          store_result(out_ids, out_scores, (long)b * k + kk, ok ? kk + id_base : -1, ok ? 0.f : -INFINITY);
        }
      return;
    }
  }
  // bound of everything a wave range did not report: its last reported score (-inf when the range ran out of columns)
  float cut = -INFINITY;
  for (int w = tid; w < slots; w += 256) cut = fmaxf(cut, cs[w * PRE_KP + PRE_KP - 1]);
  rs[tid] = cut;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) rs[tid] = fmaxf(rs[tid], rs[tid + st]);
    __syncthreads();
  }
  if (tid == 0) s_cut = rs[0];
  if (tid < PRE_R) sel_p[tid] = -1;
  __syncthreads();
  // the R best reported candidates by approximate score (score desc, id asc)
  for (int rr = 0; rr < PRE_R; ++rr) {
    float bs = -INFINITY;
    int bi = 0x7fffffff, bp = -1;
    for (int p = tid; p < ncand; p += 256) {
      const float v = cs[p];
      const int i = ci[p];
      bool taken = false;
      for (int t = 0; t < rr; ++t) taken |= sel_p[t] == p;
      if (!taken) propose(v, i, p, bs, bi, bp);
    }
    block_pick(bs, bi, bp, rs, ri, rp, tid);
    if (tid == 0) {
      sel_p[rr] = rp[0];
      if (rr == PRE_R - 1) s_aR = rp[0] >= 0 ? rs[0] : -INFINITY;  // bounds the reported candidates that were not selected
    }
    __syncthreads();
  }
  // exact scores: every wave keeps the k best (score desc, id asc) of the rows it has scored
  float bs[8];
  long bi[8];
  for (int kk = 0; kk < 8; ++kk) bs[kk] = -INFINITY, bi[kk] = -1;
  for (int rr = wave; rr < PRE_R; rr += 4) {
    const int p = sel_p[rr];
    if (p >= 0) topk_insert(bs, bi, k, exact_dot_wave(q, bank + (long)ci[p] * K, K, lane), (long)ci[p]);
  }
  auto publish = [&]() {  // block-wide k-th best so far -> s_kth; the merged list -> fs[0], fi[0]
    if (lane == 0)
      for (int kk = 0; kk < k; ++kk) fs[wave][kk] = bs[kk], fi[wave][kk] = bi[kk];
    __syncthreads();
    if (tid == 0) {
      float ms[8];
      long mi[8];
      for (int kk = 0; kk < k; ++kk) ms[kk] = -INFINITY, mi[kk] = -1;
      for (int w = 0; w < 4; ++w)
        for (int j = 0; j < k; ++j)
          if (fi[w][j] >= 0) topk_insert(ms, mi, k, fs[w][j], fi[w][j]);
      for (int kk = 0; kk < k; ++kk) fs[0][kk] = ms[kk], fi[0][kk] = mi[kk];
      s_kth = mi[k - 1] >= 0 ? ms[k - 1] : -INFINITY;
    }
    __syncthreads();
  };
  publish();
  // Any row not scored yet has an approximate score <= max(a_R, s_cut), hence an exact score <= that + EPS.
  const float bound = fmaxf(s_aR, s_cut);
  if (bound > -INFINITY && !(s_kth > bound + PRE_EPS)) {
    // The bound does not prove the answer (near-duplicate rows, or two strong rows inside one wave range): score exactly
    // every row that could still enter - reported candidates whose own approximate score comes within EPS of the k-th
    // best, and all columns of the ranges whose cut-off does.  Each is scored once: the lists cannot hold duplicates.
    if (tid == 0 && n_fallback != nullptr) atomicAdd(n_fallback, 1);
    const float need = s_kth - PRE_EPS;  // fixed for the scan: scoring more rows only raises the k-th best
    if (wave == 0)  // wave 0 restarts from the merged list, the others from nothing: every scored row lives in one list
      for (int kk = 0; kk < k; ++kk) bs[kk] = fs[0][kk], bi[kk] = fi[0][kk];
    else
      for (int kk = 0; kk < k; ++kk) bs[kk] = -INFINITY, bi[kk] = -1;
    __syncthreads();
    for (int p = wave; p < ncand; p += 4) {
      const int i = ci[p];
      if (i < 0 || !(cs[p] >= need)) continue;
      bool taken = false;
      for (int t = 0; t < PRE_R; ++t) taken |= sel_p[t] == p;
      if (!taken) topk_insert(bs, bi, k, exact_dot_wave(q, bank + (long)i * K, K, lane), (long)i);
    }
    for (int w = 0; w < slots; ++w) {  // every wave walks the ranges; a dangerous range's columns are dealt out 16 at a time
      if (!(cs[w * PRE_KP + PRE_KP - 1] >= need)) continue;
      const long c0 = (long)w * range_cols;
      for (long cb = c0 + wave * 4; cb < c0 + range_cols; cb += 16) {
        long c = cb + (lane >> 4);
        bool skip = c >= nrows || c >= c0 + range_cols;
        for (int j = 0; j < PRE_KP; ++j) skip |= (long)ci[w * PRE_KP + j] == c;
        if (skip) c = -1;
        const float e = exact_dot_quad(q, bank, c, K, lane);
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const long cg = __shfl(c, gq * 16);
          const float eg = __shfl(e, gq * 16);
          if (cg >= 0) topk_insert(bs, bi, k, eg, cg);
        }
      }
    }
    publish();
  }
  if (tid == 0)
    for (int kk = 0; kk < k; ++kk) {
      const bool ok = fi[0][kk] >= 0 && fs[0][kk] >= thr;
      store_result(out_ids, out_scores, (long)b * k + kk, ok ? fi[0][kk] + id_base : -1, ok ? fs[0][kk] : -INFINITY);
    }
}

// Candidates of one query in the all-gathered exchange buffer (gathered[R][b_total][k][2], either exchange format):
// LDS holds the score and, for distinct merges, the group (the high half of word 1) per candidate - 32 KiB at the
// 4096-candidate cap, so with the reduction scratch the block stays inside the 64 KiB a launch gets without an opt-in;
// ids stay in the gathered buffer (LAZY_ID).  A pad (id < 0) is staged as -inf whatever its score word says: it never
// takes part.
struct GatheredCandidates {
  static constexpr bool LAZY_ID = true;
  const long* __restrict__ query;  // candidate (rank 0, kk 0) of this query
  long rank_stride;                // words from one rank's candidates to the next rank's
  int k, n;
  float* cs;
  int* cg;
  __device__ __forceinline__ const long* cand(int p) const {
    const int r = p / k;
    return query + r * rank_stride + (p - r * k) * 2;
  }
  template <bool DISTINCT>
  __device__ __forceinline__ void stage(int tid) const {
    for (int p = tid; p < n; p += 256) {
      const long* e = cand(p);
      const long w = e[1];
      cs[p] = e[0] >= 0 ? __uint_as_float((unsigned)w) : -INFINITY;
      if constexpr (DISTINCT) cg[p] = (int)(w >> 32);
    }
    __syncthreads();
  }
  __device__ __forceinline__ float score(int p) const { return cs[p]; }
  __device__ __forceinline__ long id(int p) const { return cand(p)[0]; }
  __device__ __forceinline__ int group(int p) const { return cg[p]; }
  __device__ __forceinline__ void retire(int p) const { cs[p] = -INFINITY; }
};

// Merge of the all-gathered per-shard candidates (mtgv/dist.py step 4): block b merges the R * k candidates of query
// row0 + b (ids are global already).  Plain: either exchange format, the high half of word 1 is ignored.  DISTINCT: the
// labelled exchange format (Bank::topk_packed_labelled); after a pick every other candidate of the winner's group (>= 0)
// is retired with it - two shards may each report a row of one card, and only the better one represents it.
template <bool DISTINCT>
__global__ __launch_bounds__(256) void topk_merge_gathered_kernel(const long* __restrict__ gathered, int R, int b_total, int k, int row0,
                                                                 float thr, long* __restrict__ out_ids, float* __restrict__ out_scores) {
  extern __shared__ __attribute__((aligned(16))) char gm_sm[];
  const int b = blockIdx.x, ncand = R * k;
  const GatheredCandidates c{gathered + (long)(row0 + b) * k * 2, (long)b_total * k * 2, k, ncand, reinterpret_cast<float*>(gm_sm),
                             reinterpret_cast<int*>(gm_sm + (size_t)ncand * sizeof(float))};
  c.stage<DISTINCT>(threadIdx.x);
  merge_rounds<DISTINCT>(c, k, thr, [&](int kk, bool ok, long id, float score) {
    store_result(out_ids, out_scores, (long)b * k + kk, ok ? id : -1, ok ? score : -INFINITY);
  });
}

void topk_merge_gathered_launch(const int64_t* gathered, int R, int b_total, int k, int row0, int b, float thr, bool distinct, int64_t* ids,
                                float* scores, hipStream_t s) {
  MTGV_CHECK(R > 0 && k > 0 && b > 0 && row0 >= 0 && row0 + b <= b_total, ERR_INVALID, "topk_merge_gathered: R=%d k=%d rows [%d, %d) of %d", R,
             k, row0, row0 + b, b_total);
  MTGV_CHECK((long)R * k <= 4096, ERR_INVALID, "topk_merge_gathered: %d x %d candidates per query (at most 4096)", R, k);
  const size_t lds = (size_t)R * k * (sizeof(float) + (distinct ? sizeof(int) : 0));
  hipLaunchKernelGGL(distinct ? topk_merge_gathered_kernel<true> : topk_merge_gathered_kernel<false>, dim3(b), dim3(256), lds, s,
                     (const long*)gathered, R, b_total, k, row0, thr, (long*)ids, scores);
  HIP_OK(hipGetLastError());
}

// the merge of a bank's own candidates (ids are bank rows; groups: the bank's, read with distinct or pack_group only)
static void local_merge_launch(bool distinct, bool pack_group, float* cs, const int* ci, int b, int ncand, int k, int64_t id_base, float thr,
                               int64_t* ids, float* scores, const int* groups, hipStream_t s) {
  const auto kernel = pack_group ? (distinct ? topk_merge_kernel<int, true, true> : topk_merge_kernel<int, false, true>)
                                 : (distinct ? topk_merge_kernel<int, true> : topk_merge_kernel<int>);
  hipLaunchKernelGGL(kernel, dim3(b), dim3(256), 0, s, cs, ci, ncand, k, (long)id_base, thr, (long*)ids, scores, groups);
  HIP_OK(hipGetLastError());
}

void topk_merge_launch_i64(float* cs, const int64_t* ci, int b, int ncand, int k, float thr, int64_t* ids, float* scores,
                           hipStream_t s) {
  MTGV_CHECK(b > 0 && ncand > 0 && k > 0, ERR_INVALID, "topk_merge: b=%d ncand=%d k=%d", b, ncand, k);
  hipLaunchKernelGGL((topk_merge_kernel<long>), dim3(b), dim3(256), 0, s, cs, (const long*)ci, ncand, k, 0L, thr, (long*)ids, scores,
                     (const int*)nullptr);
  HIP_OK(hipGetLastError());
}

Bank::Bank(int dim, int64_t capacity) : dim_(dim), cap_(capacity) {
  MTGV_CHECK(dim > 0 && dim % 4 == 0, ERR_INVALID, "bank: dim=%d must be a positive multiple of 4", dim);
  MTGV_CHECK(capacity > 0 && capacity < (1ll << 31), ERR_INVALID, "bank: capacity=%lld", (long long)capacity);
  vecs_.alloc((size_t)capacity * dim);
  // the bank is the B operand of the match GEMM; rows of `dim` floats get per-row scaled split copies
  operand_register(vecs_.p, (size_t)capacity * dim, dim % 8 == 0 ? dim : 0);
  // workspace for the usual query batches up front (1024 queries, k <= 8, the candidate layout with the most groups:
  // 64-column tiles), so that topk does not allocate on the hot path; larger requests still grow it once
  stat_.alloc(4);
  HIP_OK(hipMemset(stat_.p, 0, 4 * sizeof(float)));
  const size_t groups = (size_t)ceil_div((int)capacity, 64);
  if (groups * 8 * 1024 * sizeof(float) <= ((size_t)256 << 20)) {
    qn_.ensure((size_t)1024 * dim);
    qhi_.ensure((size_t)1024 * dim / 2 + 8);
    cand_s_.ensure((size_t)1024 * groups * 8);
    cand_i_.ensure((size_t)1024 * groups * 8);
  }
}

Bank::~Bank() { operand_unregister(vecs_.p); }

// fp16 hi halves of rows [row0, row0 + rows) of the (row-scaled) bank: what the SP8 copy holds as its hi pieces, contiguous
void Bank::refresh_hi(int64_t row0, int64_t rows, hipStream_t s) {
  if (dim_ % 64 != 0 || rows <= 0) return;
  hi_.ensure((size_t)cap_ * dim_ / 2 + 8);
  const float* wsc = nullptr;
  if (!operand_sp8(vecs_.p + (size_t)row0 * dim_, dim_, nullptr, &wsc)) return;
  f32_to_f16_rows_launch(vecs_.p + (size_t)row0 * dim_, wsc, reinterpret_cast<_Float16*>(hi_.p) + (size_t)row0 * dim_, (long)rows, dim_, s);
}

int64_t Bank::prepass_fallbacks() const {
  int v = 0;
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(&v, stat_.p, sizeof(int), hipMemcpyDeviceToHost));
  return v;
}

bool Bank::prepass_ok(int b, int k) const {
  const bool on = env_int("MTGV_MATCH_PREPASS", 1) != 0;  // read per call: tests and tools compare the two paths in one process
  return on && gemm_sp_active() && b >= 128 && k <= 4 && dim_ % 64 == 0 && size_ >= 4096 && hi_.p != nullptr;
}

void Bank::prepass_layout(int* slots, int* range_cols, int* per_range) const {
  *slots = gemm_sp_topk_hi16_slots((int)size_);
  *range_cols = gemm_sp_topk_hi16_range_cols();
  *per_range = PRE_KP;
}

// TEST SURFACE: what topk_prepass runs before the re-rank - the same launches with the same arguments - with the candidates
// in the caller's buffers instead of the bank's (not recorded by the launch profiler: topk_prepass's record stands for the
// match).  Refuses, before anything is written, a bank or batch that topk would not give to the first pass.
void Bank::prepass_candidates(const float* q, int b, float* cand_s, int* cand_i, int* slots, int* range_cols, hipStream_t s) {
  MTGV_CHECK(b > 0 && q != nullptr && cand_s != nullptr && cand_i != nullptr, ERR_INVALID, "bank: prepass_candidates b=%d or a null tensor", b);
  MTGV_CHECK(gemm_sp_active() && b >= 128 && dim_ % 64 == 0 && size_ >= 4096 && hi_.p != nullptr, ERR_INVALID,
             "bank: no fp16 first pass here (f16x3 mode %d, b=%d >= 128, dim=%d %% 64 == 0, size=%lld >= 4096, fp16 copy %d)",
             gemm_sp_active() ? 1 : 0, b, dim_, (long long)size_, hi_.p != nullptr ? 1 : 0);
  const int N = (int)size_;
  qn_.ensure((size_t)b * dim_);
  qhi_.ensure((size_t)b * dim_ / 2 + 8);
  l2norm_rows_launch(q, qn_.p, b, dim_, s);
  f32_to_f16_rows_launch(qn_.p, nullptr, reinterpret_cast<_Float16*>(qhi_.p), (long)b, dim_, s);
  const float* wsc = nullptr;
  MTGV_CHECK(operand_sp8(vecs_.p, dim_, nullptr, &wsc), ERR_RUNTIME, "bank: row scales missing");
  int sl = 0;
  gemm_sp_topk_hi16_launch(qhi_.p, hi_.p, wsc, b, N, dim_, PRE_KP, cand_s, cand_i, &sl, s);
  if (slots != nullptr) *slots = sl;
  if (range_cols != nullptr) *range_cols = gemm_sp_topk_hi16_range_cols();
}

void Bank::topk_prepass(const float* q, int b, int k, int64_t id_base, float thr, int64_t* ids, float* scores, hipStream_t s) {
  const int N = (int)size_;
  const int slots = gemm_sp_topk_hi16_slots(N);
  const size_t ncand = (size_t)slots * PRE_KP;
  qn_.ensure((size_t)b * dim_);
  qhi_.ensure((size_t)b * dim_ / 2 + 8);
  cand_s_.ensure((size_t)b * ncand);
  cand_i_.ensure((size_t)b * ncand);
  l2norm_rows_launch(q, qn_.p, b, dim_, s);
  f32_to_f16_rows_launch(qn_.p, nullptr, reinterpret_cast<_Float16*>(qhi_.p), (long)b, dim_, s);
  const float* wsc = nullptr;
  MTGV_CHECK(operand_sp8(vecs_.p, dim_, nullptr, &wsc), ERR_RUNTIME, "bank: row scales missing");
  int sl = 0;
  {  // recorded for the roofline like the one-pass launch it replaces (sp = 3: one fp16 MFMA per product, fp16 bank bytes)
    GemmArgs rec;
    rec.M = b, rec.N = N, rec.K = dim_, rec.topk = PRE_KP;
    const double tiles = (double)ceil_div(b, 128) * ceil_div(N, 192);
    gemm_profile_begin(rec, s, 3, tiles * (128 + 192) * dim_ * 2.0, 2.0 * ((double)N * dim_ + (double)b * dim_) + 8.0 * b * slots * PRE_KP);
  }
  gemm_sp_topk_hi16_launch(qhi_.p, hi_.p, wsc, b, N, dim_, PRE_KP, cand_s_.p, reinterpret_cast<int*>(cand_i_.p), &sl, s);
  gemm_profile_end(s);
  hipLaunchKernelGGL(rerank_kernel, dim3(b), dim3(256), 0, s, qn_.p, vecs_.p, (long)N, dim_, (const float*)cand_s_.p,
                     (const int*)cand_i_.p, sl, gemm_sp_topk_hi16_range_cols(), k, (long)id_base, thr, (long*)ids, scores,
                     reinterpret_cast<int*>(stat_.p));
  HIP_OK(hipGetLastError());
}

void Bank::append(const float* v, int64_t n, bool is_device, hipStream_t s) {
  MTGV_CHECK(n >= 0 && size_ + n <= cap_, ERR_INVALID, "bank: %lld + %lld rows exceed capacity %lld", (long long)size_,
             (long long)n, (long long)cap_);
  if (n == 0) return;
  float* dst = vecs_.p + (size_t)size_ * dim_;
  HIP_OK(hipMemcpyAsync(dst, v, (size_t)n * dim_ * sizeof(float), is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  l2norm_rows_launch(dst, dst, n, dim_, s);
  operand_refresh(vecs_.p, (size_t)size_ * dim_, (size_t)n * dim_, s);
  refresh_hi(size_, n, s);
  if (!is_device) HIP_OK(hipStreamSynchronize(s));  // host buffer may be freed by the caller
  size_ += n;
}

void Bank::set_row(int64_t row, const float* v_host, hipStream_t s) {
  MTGV_CHECK(row >= 0 && row < size_, ERR_INVALID, "bank: row %lld outside [0, %lld)", (long long)row, (long long)size_);
  float* dst = vecs_.p + (size_t)row * dim_;
  HIP_OK(hipMemcpyAsync(dst, v_host, (size_t)dim_ * sizeof(float), hipMemcpyHostToDevice, s));
  l2norm_rows_launch(dst, dst, 1, dim_, s);
  operand_refresh(vecs_.p, (size_t)row * dim_, (size_t)dim_, s);
  refresh_hi(row, 1, s);
  HIP_OK(hipStreamSynchronize(s));
}

void Bank::get_rows(int64_t row, int64_t n, float* out_host) const {
  MTGV_CHECK(row >= 0 && n >= 0 && row + n <= size_, ERR_INVALID, "bank: rows [%lld, %lld) outside [0, %lld)", (long long)row,
             (long long)(row + n), (long long)size_);
  if (n == 0) return;
  HIP_OK(hipMemcpy(out_host, vecs_.p + (size_t)row * dim_, (size_t)n * dim_ * sizeof(float), hipMemcpyDeviceToHost));
}

// ---- row labels ----
// Invariant: once allocated, every row at or beyond size_ holds the defaults (tags 0, group -1), so append has nothing to do.
void Bank::ensure_labels() {
  if (tags_.p != nullptr) return;
  tags_.alloc((size_t)cap_ * 2);  // uint64 per row
  groups_.alloc((size_t)cap_);    // int32 per row
  HIP_OK(hipMemset(tags_.p, 0, (size_t)cap_ * sizeof(uint64_t)));
  HIP_OK(hipMemset(groups_.p, 0xff, (size_t)cap_ * sizeof(int32_t)));  // -1
  HIP_OK(hipStreamSynchronize(nullptr));  // the caller's stream need not wait on the null stream by itself
}

void Bank::clear() {
  if (tags_.p != nullptr && size_ > 0) {
    HIP_OK(hipDeviceSynchronize());  // matches in flight still read the labels
    HIP_OK(hipMemset(tags_.p, 0, (size_t)size_ * sizeof(uint64_t)));
    HIP_OK(hipMemset(groups_.p, 0xff, (size_t)size_ * sizeof(int32_t)));
    HIP_OK(hipStreamSynchronize(nullptr));
  }
  size_ = 0;
}

void Bank::set_labels(int64_t row0, int64_t n, const uint64_t* tags_host, const int32_t* groups_host, hipStream_t s) {
  MTGV_CHECK(row0 >= 0 && n >= 0 && row0 + n <= size_, ERR_INVALID, "bank: label rows [%lld, %lld) outside [0, %lld)", (long long)row0,
             (long long)(row0 + n), (long long)size_);
  if (groups_host != nullptr)
    for (int64_t i = 0; i < n; ++i)
      MTGV_CHECK(groups_host[i] >= -1, ERR_INVALID, "bank: group %d of row %lld (groups are >= 0, or -1 for none)", groups_host[i],
                 (long long)(row0 + i));
  if (n == 0 || (tags_host == nullptr && groups_host == nullptr)) return;
  ensure_labels();
  if (tags_host != nullptr)
    HIP_OK(hipMemcpyAsync(reinterpret_cast<uint64_t*>(tags_.p) + row0, tags_host, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  if (groups_host != nullptr)
    HIP_OK(hipMemcpyAsync(reinterpret_cast<int32_t*>(groups_.p) + row0, groups_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));  // host buffers may be freed by the caller
}

void Bank::get_labels(int64_t row0, int64_t n, uint64_t* tags_host, int32_t* groups_host) const {
  MTGV_CHECK(row0 >= 0 && n >= 0 && row0 + n <= size_, ERR_INVALID, "bank: label rows [%lld, %lld) outside [0, %lld)", (long long)row0,
             (long long)(row0 + n), (long long)size_);
  if (n == 0) return;
  if (tags_.p == nullptr) {  // never labelled: all defaults
    for (int64_t i = 0; i < n; ++i) {
      if (tags_host != nullptr) tags_host[i] = 0;
      if (groups_host != nullptr) groups_host[i] = -1;
    }
    return;
  }
  if (tags_host != nullptr)
    HIP_OK(hipMemcpy(tags_host, reinterpret_cast<const uint64_t*>(tags_.p) + row0, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (groups_host != nullptr)
    HIP_OK(hipMemcpy(groups_host, reinterpret_cast<const int32_t*>(groups_.p) + row0, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
}

// One-pass exact match: normalise the queries, one GEMM launch with the fused top-k epilogue, one merge.  labelled: the
// launch and the merge honour the row labels (masks may be null: no filter; distinct: one row per group) - every candidate
// range reports its kt best eligible rows, with `distinct` of pairwise different groups, and the merge dedupes again: the
// result is the exact filtered / distinct top k (match).  labelled with scores == nullptr: ids receives the
// labelled exchange format, (id, group << 32 | score bits) per result.
void Bank::topk_one_pass(const float* q, int b, int k, int64_t id_base, float thr, bool labelled, const uint64_t* masks, bool distinct,
                         int64_t* ids, float* scores, hipStream_t s) {
  qn_.ensure((size_t)b * dim_);
  GemmArgs g = linear_args(qn_.p, dim_, vecs_.p, nullptr, nullptr, 0, b, (int)size_, dim_, ACT_NONE);
  if (labelled) {
    g.col_tags = reinterpret_cast<const uint64_t*>(tags_.p);
    g.col_groups = reinterpret_cast<const int*>(groups_.p);
    g.row_masks = masks;
    g.topk_distinct = distinct ? 1 : 0;
  }
  // candidate groups: 64-column tiles of the convert-on-load kernel, or the per-wave column ranges of the LDS-DMA kernel
  int slots = 0, cols = 0;
  g.topk = 1;
  gemm_topk_layout(g, &slots, &cols);
  const int kt = k < cols ? k : cols;  // a group cannot contribute more candidates than it has columns
  const size_t ncand = (size_t)slots * kt;
  cand_s_.ensure((size_t)b * ncand);
  cand_i_.ensure((size_t)b * ncand);
  l2norm_rows_launch(q, qn_.p, b, dim_, s);
  g.cand_s = cand_s_.p;
  g.cand_i = reinterpret_cast<int*>(cand_i_.p);
  g.topk = kt;
  gemm_launch(g, s);
  // labelled with scores == nullptr: the labelled exchange format, every result with its row's group
  local_merge_launch(labelled && distinct, labelled && scores == nullptr, cand_s_.p, (const int*)cand_i_.p, b, (int)ncand, k, id_base, thr,
                     ids, scores, g.col_groups, s);
}

// what every Bank::topk* entry checks first; labels_ok: a labelled entry got masks or distinct
static void check_topk_args(int b, int k, bool tensors_ok, bool labels_ok = true) {
  MTGV_CHECK(b > 0 && k > 0 && k <= 65536, ERR_INVALID, "bank: b=%d k=%d (k must be in [1,65536])", b, k);
  MTGV_CHECK(tensors_ok, ERR_INVALID, "bank: null tensor");
  MTGV_CHECK(labels_ok, ERR_INVALID, "bank: a labelled match needs masks or distinct");
}

// Labelled match: always the one-pass kernel with the labelled epilogue (the fp16 pre-pass's bound does not cover labels).
void Bank::topk_labelled(const float* q, int b, int k, int64_t id_base, float thr, const uint64_t* masks, bool distinct, int64_t* ids,
                         float* scores, hipStream_t s) {
  check_topk_args(b, k, q != nullptr && ids != nullptr && scores != nullptr, masks != nullptr || distinct);
  MTGV_CHECK(size_ > 0, ERR_RUNTIME, "bank is empty");
  ensure_labels();  // (first labelled call on a bank without labels: allocates and synchronises once)
  topk_one_pass(q, b, k, id_base, thr, true, masks, distinct, ids, scores, s);
}

// The labelled match of a row shard in the exchange format (topk_one_pass, labelled, scores == nullptr).  No threshold here:
// it belongs to the merge.  An empty shard answers with pads instead of an error - a rank that raised would leave the
// others waiting in the collective.
void Bank::topk_packed_labelled(const float* q, int b, int k, int64_t id_base, const uint64_t* masks, bool distinct, int64_t* packed,
                                hipStream_t s) {
  check_topk_args(b, k, q != nullptr && packed != nullptr, masks != nullptr || distinct);
  if (size_ == 0) {
    const long slots = (long)b * k;
    hipLaunchKernelGGL(packed_pads_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, (long*)packed, slots);
    HIP_OK(hipGetLastError());
    return;
  }
  ensure_labels();  // (first labelled call on a bank without labels: allocates and synchronises once)
  topk_one_pass(q, b, k, id_base, -INFINITY, true, masks, distinct, packed, nullptr, s);
}

void Bank::topk(const float* q, int b, int k, int64_t id_base, float thr, int64_t* ids, float* scores, hipStream_t s) {
  check_topk_args(b, k, q != nullptr && ids != nullptr);  // scores == nullptr: exchange format in ids (store_result)
  MTGV_CHECK(size_ > 0, ERR_RUNTIME, "bank is empty");
  if (prepass_ok(b, k)) {
    topk_prepass(q, b, k, id_base, thr, ids, scores, s);
    return;
  }
  topk_one_pass(q, b, k, id_base, thr, false, nullptr, false, ids, scores, s);
}

}  // namespace mtgv
