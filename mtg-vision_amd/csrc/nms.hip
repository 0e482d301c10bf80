// Per-image class-aware NMS on decoded predictions, one workgroup per image: the axis-aligned greedy sweep of the
// segment / detect family (nms_kernel), and the rotated rule of the OBB family (nms_rotated_kernel, further down).
// (third-party `non_max_suppression` of ultralytics 8.3.x behind CardSegmenter,
//  mtgvision/od_export.py:147-150; defaults conf 0.25, iou 0.7, max_det 300, max_wh 7680.)
//
//   1. candidates: max class score > conf; key = score bits << 32 | ~anchor  (u64)
//   2. bitonic sort of the keys in LDS, descending -> score desc, anchor asc (deterministic)
//   3. sorted boxes -> xyxy + class offset, areas (workspace in HBM, L2-resident)
//   4. greedy sweep, 64 sorted boxes at a time: one wave resolves the word in order (readlane broadcast + __ballot),
//      then all waves apply the word's kept boxes to the later words, one __ballot per word into the suppression
//      bitmask (no atomics)
//
// All box arithmetic uses explicitly rounded single operations (no FMA contraction), so the
// kept indices are bit-identical to the float32 CPU oracle (oracle/detector_ref.py nms_single).
//
// Two forms of the kernel.  ROWS = false reads decoded predictions `pred` (n, 4 + nc + nm, na).  ROWS = true reads the
// segment head's raw rows instead (head_decode.h): step 1 takes the class scores of every anchor from the rows' class
// logits, step 3 decodes the boxes of the sorted candidates only, and the kept detections copy their coefficients from
// their rows - the values decode_kernel would have written to `pred`, bit for bit, without the pass over every anchor.
#include "nms.h"
#include "probiou.h"

#include <algorithm>

namespace mtgv {

static constexpr int NMS_THREADS = 1024;

__device__ __forceinline__ float box_iou_rn(float ax1, float ay1, float ax2, float ay2, float aarea, float bx1, float by1,
                                            float bx2, float by2, float barea) {
  const float iw = fmaxf(0.f, __fsub_rn(fminf(ax2, bx2), fmaxf(ax1, bx1)));
  const float ih = fmaxf(0.f, __fsub_rn(fminf(ay2, by2), fmaxf(ay1, by1)));
  const float inter = __fmul_rn(iw, ih);
  return __fdiv_rn(inter, __fsub_rn(__fadd_rn(aarea, barea), inter));
}

// what the sweep needs of anchor a, from either source
template <bool ROWS>
struct NmsSrc {
  const float* P;  // pred of this image (ROWS = false)
  HeadRows h;      // (ROWS = true)
  int img, na;
  __device__ __forceinline__ HeadAnchor anchor(int a) const { return ROWS ? head_anchor(h, img, a) : HeadAnchor{}; }
  __device__ __forceinline__ float score(const HeadAnchor& an, int a, int c) const {
    if constexpr (ROWS) return head_score(an.row[h.cls + c]);
    else return P[(long)(4 + c) * na + a];
  }
  __device__ __forceinline__ void xywh(const HeadAnchor& an, int a, float b[4]) const {
    if constexpr (ROWS) head_box(an, b);
    else b[0] = P[a], b[1] = P[(long)na + a], b[2] = P[(long)2 * na + a], b[3] = P[(long)3 * na + a];
  }
  __device__ __forceinline__ float coef(const HeadAnchor& an, int a, int nc, int c) const {
    if constexpr (ROWS) return an.row[h.coef + c];
    else return P[(long)(4 + nc + c) * na + a];
  }
};

// Steps 1 and 2, shared by the axis-aligned and the rotated kernel: the anchors whose best class score exceeds conf as
// keys = score bits << 32 | ~anchor, sorted descending in LDS (score desc, anchor asc).  `score(a, c)`: class score c of
// anchor a.  Returns the candidate count; keys[count, cap) are zero.  Ends with a block barrier.
template <typename Score>
__device__ __forceinline__ int nms_sorted_keys(Score score, int nc, int na, int cap, float conf_thres, unsigned long long* keys,
                                               int* s_count) {
  const int tid = threadIdx.x;
  if (tid == 0) *s_count = 0;
  for (int i = tid; i < cap; i += NMS_THREADS) keys[i] = 0ull;
  __syncthreads();

  // 1. candidates
  for (int a = tid; a < na; a += NMS_THREADS) {
    float best = score(a, 0);
    for (int c = 1; c < nc; ++c) {
      const float v = score(a, c);
      if (v > best) best = v;
    }
    if (best > conf_thres) {
      const int slot = atomicAdd(s_count, 1);
      keys[slot] = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)(~(unsigned)a);
    }
  }
  __syncthreads();
  const int count = *s_count;
  int n2 = 1;
  while (n2 < count) n2 <<= 1;

  // 2. bitonic sort, descending
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += NMS_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = keys[i], b = keys[l];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) keys[i] = b, keys[l] = a;
        }
      }
      __syncthreads();
    }
  }
  return count;
}

template <bool ROWS>
__device__ __forceinline__ int nms_sorted_candidates(const NmsSrc<ROWS>& src, int nc, int na, int cap, float conf_thres,
                                                     unsigned long long* keys, int* s_count) {
  return nms_sorted_keys([&](int a, int c) { return src.score(src.anchor(a), a, c); }, nc, na, cap, conf_thres, keys, s_count);
}

// ws layout per image (floats): obox[cap][4], area[cap], then ints: sidx[cap], scls[cap]
template <bool ROWS>
__global__ __launch_bounds__(NMS_THREADS) void nms_kernel(const float* __restrict__ pred, HeadRows rows, int nc, int nm, int na, int cap,
                                                         float conf_thres, float iou_thres, int max_det, float max_wh,
                                                         int* __restrict__ n_det, float* __restrict__ boxes,
                                                         float* __restrict__ conf_out, int* __restrict__ cls_out,
                                                         int* __restrict__ keep_idx, float* __restrict__ coef_out,
                                                         int* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];  // [cap] (cap = pow2 >= na)
  __shared__ int s_count;
  __shared__ int s_nkeep;
  __shared__ int s_keep[1024];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int no = 4 + nc + nm;
  const NmsSrc<ROWS> src{ROWS ? nullptr : pred + (long)img * no * na, rows, img, na};

  float* obox = reinterpret_cast<float*>(ws) + (long)img * cap * 7;
  float* area = obox + (long)cap * 4;
  int* sidx = reinterpret_cast<int*>(area + cap);
  int* scls = sidx + cap;

  if (tid == 0) s_nkeep = 0;
  const int count = nms_sorted_candidates(src, nc, na, cap, conf_thres, keys, &s_count);

  // 3. sorted boxes
  for (int i = tid; i < count; i += NMS_THREADS) {
    const int a = (int)(~(unsigned)(keys[i] & 0xffffffffull));
    const HeadAnchor an = src.anchor(a);
    float b[4];
    src.xywh(an, a, b);
    const float x = b[0], y = b[1], w = b[2], h = b[3];
    float best = src.score(an, a, 0);
    int cls = 0;
    for (int c = 1; c < nc; ++c) {
      const float v = src.score(an, a, c);
      if (v > best) best = v, cls = c;
    }
    const float hw = __fmul_rn(w, 0.5f), hh = __fmul_rn(h, 0.5f);
    const float off = __fmul_rn((float)cls, max_wh);
    const float x1 = __fadd_rn(__fsub_rn(x, hw), off), y1 = __fadd_rn(__fsub_rn(y, hh), off);
    const float x2 = __fadd_rn(__fadd_rn(x, hw), off), y2 = __fadd_rn(__fadd_rn(y, hh), off);
    obox[(long)i * 4 + 0] = x1, obox[(long)i * 4 + 1] = y1, obox[(long)i * 4 + 2] = x2, obox[(long)i * 4 + 3] = y2;
    area[i] = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
    sidx[i] = a;
    scls[i] = cls;
  }
  __syncthreads();  // global writes by this block are visible to it after the barrier

  // 4. greedy sweep, one 64-box word of the sorted list at a time; the key buffer is reused as the suppression bitmask.
  //    (a) wave 0 resolves the word in order: the lowest surviving lane is kept (v_readlane broadcasts its box) and
  //        knocks out the later lanes it overlaps, published with one __ballot per keep - no block barrier;
  //    (b) every wave then applies the word's kept boxes (parked in LDS) to its share of the later words.
  //    Same keep list as the box-at-a-time sweep: a box is kept iff no earlier kept box overlaps it beyond the
  //    threshold; two block barriers per word instead of two per kept box.
  unsigned long long* supp = keys;
  __shared__ float kbox[64 * 5];  // x1 y1 x2 y2 area of the word being resolved
  __shared__ unsigned long long s_kmask;
  const int nwords = (count + 63) >> 6;
  for (int i = tid; i < nwords; i += NMS_THREADS) supp[i] = 0ull;
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, nwaves = NMS_THREADS >> 6;
  for (int w0 = 0; w0 < nwords; ++w0) {
    if (wave == 0) {
      const int j = (w0 << 6) + lane;
      const bool valid = j < count;
      const float bx1 = valid ? obox[(long)j * 4] : 0.f, by1 = valid ? obox[(long)j * 4 + 1] : 0.f;
      const float bx2 = valid ? obox[(long)j * 4 + 2] : 0.f, by2 = valid ? obox[(long)j * 4 + 3] : 0.f;
      const float barea = valid ? area[j] : 0.f;
      kbox[lane * 5 + 0] = bx1, kbox[lane * 5 + 1] = by1, kbox[lane * 5 + 2] = bx2, kbox[lane * 5 + 3] = by2, kbox[lane * 5 + 4] = barea;
      unsigned long long alive = __ballot(valid) & ~supp[w0];
      unsigned long long kept = 0ull;
      int nk = s_nkeep;
      while (alive != 0ull && nk < max_det) {
        const int k = __builtin_ctzll(alive);  // wave-uniform: the earliest surviving box of the word
        if (lane == 0) s_keep[nk] = (w0 << 6) + k;
        nk += 1;
        kept |= 1ull << k;
        alive &= ~(1ull << k);
        if (nk >= max_det) break;
        const float ax1 = __shfl(bx1, k), ay1 = __shfl(by1, k), ax2 = __shfl(bx2, k), ay2 = __shfl(by2, k), aarea = __shfl(barea, k);
        const bool s = lane > k && ((alive >> lane) & 1ull) && box_iou_rn(ax1, ay1, ax2, ay2, aarea, bx1, by1, bx2, by2, barea) > iou_thres;
        alive &= ~__ballot(s);
      }
      if (lane == 0) s_nkeep = nk, s_kmask = kept;
    }
    __syncthreads();
    const unsigned long long kept = s_kmask;
    if (s_nkeep >= max_det) break;  // block-uniform
    if (kept != 0ull) {
      for (int wd = w0 + 1 + wave; wd < nwords; wd += nwaves) {
        const int j = (wd << 6) + lane;
        bool s = false;
        if (j < count) {
          const float bx1 = obox[(long)j * 4], by1 = obox[(long)j * 4 + 1], bx2 = obox[(long)j * 4 + 2], by2 = obox[(long)j * 4 + 3];
          const float barea = area[j];
          unsigned long long m = kept;
          while (m != 0ull && !s) {  // any kept box of the word suffices; the order of the tests does not matter
            const int k = __builtin_ctzll(m);
            m &= m - 1;
            s = box_iou_rn(kbox[k * 5], kbox[k * 5 + 1], kbox[k * 5 + 2], kbox[k * 5 + 3], kbox[k * 5 + 4], bx1, by1, bx2, by2, barea) > iou_thres;
          }
        }
        const unsigned long long mk = __ballot(s);
        if (lane == 0 && mk) supp[wd] |= mk;  // one writer per word per step
      }
    }
    __syncthreads();  // supp of the next word is complete; kbox and s_kmask may be rewritten
  }
  __syncthreads();

  // outputs, score-descending
  const int nkeep = s_nkeep;
  if (tid == 0) n_det[img] = nkeep;
  for (int t = tid; t < nkeep; t += NMS_THREADS) {
    const int k = s_keep[t];
    const int a = sidx[k], cls = scls[k];
    const float off = __fmul_rn((float)cls, max_wh);
    const long o = (long)img * max_det + t;
    // un-offset boxes are recomputed from the prediction so they carry no offset rounding
    const HeadAnchor an = src.anchor(a);
    float b[4];
    src.xywh(an, a, b);
    const float x = b[0], y = b[1], w = b[2], h = b[3];
    const float hw = __fmul_rn(w, 0.5f), hh = __fmul_rn(h, 0.5f);
    boxes[o * 4 + 0] = __fsub_rn(x, hw);
    boxes[o * 4 + 1] = __fsub_rn(y, hh);
    boxes[o * 4 + 2] = __fadd_rn(x, hw);
    boxes[o * 4 + 3] = __fadd_rn(y, hh);
    (void)off;
    conf_out[o] = src.score(an, a, cls);
    cls_out[o] = cls;
    keep_idx[o] = a;
  }
  // slots beyond the kept detections: zeros, so callers may hand in uninitialised output tensors
  for (int t = nkeep + tid; t < max_det; t += NMS_THREADS) {
    const long o = (long)img * max_det + t;
    boxes[o * 4 + 0] = 0.f, boxes[o * 4 + 1] = 0.f, boxes[o * 4 + 2] = 0.f, boxes[o * 4 + 3] = 0.f;
    conf_out[o] = 0.f;
    cls_out[o] = 0;
    keep_idx[o] = 0;
  }
  if (coef_out != nullptr) {
    // mask coefficients of the kept detections, (max_det, nm) per image, zero beyond n_det
    for (int t = tid; t < max_det * nm; t += NMS_THREADS) {
      const int d = t / nm, c = t - d * nm;
      float v = 0.f;
      if (d < nkeep) {
        const int a = sidx[s_keep[d]];
        v = src.coef(src.anchor(a), a, nc, c);
      }
      coef_out[((long)img * max_det + d) * nm + c] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// Rotated NMS on OBB predictions pred (n, 4 + nc + 1, na) = xywh, class scores, angle
// (ultralytics 8.3.x non_max_suppression(rotated=True) -> ops.nms_rotated) [external - recalled; unpinned].
// The rule is NOT the greedy sweep above: nms_rotated takes the upper triangle of the pairwise ProbIoU matrix of the
// score-sorted candidates and keeps candidate j iff no candidate i < j has probiou(i, j) >= iou - whether or not i was
// itself dropped.  So there is no serial dependence: after the shared candidate and sort stages,
//   3. per sorted candidate: x, y + class offset and the covariance (a, b, c) of probiou.h, once (workspace in HBM)
//   4. one lane per candidate j tests the candidates before it (the loop index i is wave-uniform: every lane of a wave
//      reads the same candidate i) and stops at its first hit; __ballot collects a 64-candidate word of keep flags
//   5. ranks from the words' population counts; the first max_det kept are reported
// Pairs of different classes are skipped.  Proof that such a pair never suppresses, for max_wh = 7680, sides <= 1024 px
// and centres within [-512, 1536] (the head's: sides <= 30 bins x 32, centres within 240 px of the 640 frame): both
// coordinates of the two centres differ by at least 7680 - 2048, so |d|^2 >= 2 x 5632^2 = 6.3e7; with S = S1 + S2 the
// summed covariance, t1 + t2 = 1/8 d^T S^-1 d >= 1/8 |d|^2 / lambda_max(S), and lambda_max(S) <= 2 x 1024^2 / 12 = 1.75e5, so
// t1 + t2 > 45 > 25; t3 >= 0 (Minkowski: det(S1 + S2) >= 4 sqrt(det S1 det S2)); hence bd > 25, exp(-bd) < 1.4e-11 and
// hd = sqrt(1 - exp(-bd) + eps) >= 1, in float32 as well (1 - 1.4e-11 rounds to 1): probiou <= 0 < iou.  The launcher
// therefore requires iou > 0 and max_wh >= 7680.  No other pair is skipped, so the cost is quadratic in the candidates of
// a class, on one CU per image.  Measured (profiles/README.md, "OBB family"): 0.70 ms at 898 candidates, 31.7 ms at 8400
// dissimilar candidates of one class - 30 x the batch-1 forward of the same run; the rule is left exact.
// ws layout per image (floats): ox[cap], oy[cap], ca[cap], cb[cap], cc[cap], then ints: sidx[cap], scls[cap]
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NMS_THREADS) void nms_rotated_kernel(const float* __restrict__ pred, int nc, int na, int cap, float conf_thres,
                                                                 float iou_thres, int max_det, float max_wh, int* __restrict__ n_det,
                                                                 float* __restrict__ rboxes, float* __restrict__ conf_out,
                                                                 int* __restrict__ cls_out, int* __restrict__ keep_idx,
                                                                 int* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];  // [cap] (cap = pow2 >= na)
  __shared__ int s_count;
  __shared__ int s_nkeep;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int no = 4 + nc + 1;
  const float* P = pred + (long)img * no * na;

  float* ox = reinterpret_cast<float*>(ws) + (long)img * cap * 7;
  float* oy = ox + cap;
  float* ca = oy + cap;
  float* cb = ca + cap;
  float* cc = cb + cap;
  int* sidx = reinterpret_cast<int*>(cc + cap);
  int* scls = sidx + cap;

  const int count = nms_sorted_keys([&](int a, int c) { return P[(long)(4 + c) * na + a]; }, nc, na, cap, conf_thres, keys, &s_count);

  // 3. sorted candidates: offset centre, covariance, anchor, class (first maximum on ties)
  for (int i = tid; i < count; i += NMS_THREADS) {
    const int a = (int)(~(unsigned)(keys[i] & 0xffffffffull));
    float best = P[(long)4 * na + a];
    int cls = 0;
    for (int c = 1; c < nc; ++c) {
      const float v = P[(long)(4 + c) * na + a];
      if (v > best) best = v, cls = c;
    }
    const float off = __fmul_rn((float)cls, max_wh);
    float a_, b_, c_;
    probiou_cov(P[(long)2 * na + a], P[(long)3 * na + a], P[(long)(4 + nc) * na + a], a_, b_, c_);
    ox[i] = __fadd_rn(P[a], off), oy[i] = __fadd_rn(P[(long)na + a], off);
    ca[i] = a_, cb[i] = b_, cc[i] = c_;
    sidx[i] = a, scls[i] = cls;
  }
  __syncthreads();  // global writes by this block are visible to it after the barrier; the keys are no longer needed

  // 4. keep flags, one 64-candidate word per wave and pass; the key buffer is reused for the words
  unsigned long long* kept = keys;
  const int nwords = (count + 63) >> 6;
  const int lane = tid & 63, wave = tid >> 6, nwaves = NMS_THREADS >> 6;
  for (int wd = wave; wd < nwords; wd += nwaves) {
    const int j = (wd << 6) + lane;
    const bool valid = j < count;
    const float xj = valid ? ox[j] : 0.f, yj = valid ? oy[j] : 0.f;
    const float aj = valid ? ca[j] : 0.f, bj = valid ? cb[j] : 0.f, cj = valid ? cc[j] : 0.f;
    const int clsj = valid ? scls[j] : -1;
    bool hit = false;
    const int iend = min(count, (wd << 6) + 63);  // candidates before the word's last
    for (int i = 0; i < iend; ++i) {
      if (__ballot(valid && !hit && i < j) == 0ull) break;  // every lane of the word is settled
      if (valid && !hit && i < j && scls[i] == clsj)
        hit = probiou_pair(ox[i], oy[i], ca[i], cb[i], cc[i], xj, yj, aj, bj, cj) >= iou_thres;
    }
    const unsigned long long m = __ballot(valid && !hit);
    if (lane == 0) kept[wd] = m;
  }
  __syncthreads();

  // 5. ranks: exclusive prefix of the words' counts (one thread: at most cap / 64 words), then every kept candidate
  //    below max_det writes its row
  int* base = reinterpret_cast<int*>(kept + nwords);  // [nwords], behind the words (cap >= 2 nwords holds for cap >= 2)
  if (tid == 0) {
    int acc = 0;
    for (int w = 0; w < nwords; ++w) {
      base[w] = acc;
      acc += __popcll(kept[w]);
    }
    s_nkeep = acc < max_det ? acc : max_det;
  }
  __syncthreads();
  const int nkeep = s_nkeep;
  if (tid == 0) n_det[img] = nkeep;
  for (int j = tid; j < count; j += NMS_THREADS) {
    const unsigned long long m = kept[j >> 6];
    if (!((m >> (j & 63)) & 1ull)) continue;
    const int t = base[j >> 6] + __popcll(m & ((1ull << (j & 63)) - 1ull));
    if (t >= max_det) continue;
    const int a = sidx[j], cls = scls[j];
    const long o = (long)img * max_det + t;
    // copies of the prediction: no offset, no rounding
    rboxes[o * 5 + 0] = P[a], rboxes[o * 5 + 1] = P[(long)na + a], rboxes[o * 5 + 2] = P[(long)2 * na + a];
    rboxes[o * 5 + 3] = P[(long)3 * na + a], rboxes[o * 5 + 4] = P[(long)(4 + nc) * na + a];
    conf_out[o] = P[(long)(4 + cls) * na + a];
    cls_out[o] = cls;
    keep_idx[o] = a;
  }
  // slots beyond the kept detections: zeros, so callers may hand in uninitialised output tensors
  for (int t = nkeep + tid; t < max_det; t += NMS_THREADS) {
    const long o = (long)img * max_det + t;
    for (int e = 0; e < 5; ++e) rboxes[o * 5 + e] = 0.f;
    conf_out[o] = 0.f;
    cls_out[o] = 0;
    keep_idx[o] = 0;
  }
}

__global__ __launch_bounds__(256) void probiou_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                     long m) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  float a1, b1, c1, a2, b2, c2;
  probiou_cov(a[i * 5 + 2], a[i * 5 + 3], a[i * 5 + 4], a1, b1, c1);
  probiou_cov(b[i * 5 + 2], b[i * 5 + 3], b[i * 5 + 4], a2, b2, c2);
  out[i] = probiou_pair(a[i * 5], a[i * 5 + 1], a1, b1, c1, b[i * 5], b[i * 5 + 1], a2, b2, c2);
}

static int pow2_ge(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

size_t nms_workspace_bytes(int n, int na) { return (size_t)n * pow2_ge(na) * 7 * sizeof(float); }

template <bool ROWS>
static void nms_launch_form(const float* pred, const HeadRows& rows, int n, int nc, int nm, int na, float conf, float iou, int max_det,
                            float max_wh, int* n_det, float* boxes, float* conf_out, int* cls_out, int* keep_idx, float* coef_out, int* ws,
                            size_t ws_bytes, hipStream_t s) {
  MTGV_CHECK(n > 0 && nc > 0 && nm >= 0 && na > 0, ERR_INVALID, "nms: n=%d nc=%d nm=%d na=%d", n, nc, nm, na);
  MTGV_CHECK(max_det > 0 && max_det <= 1024, ERR_INVALID, "nms: max_det=%d outside [1,1024]", max_det);
  const int cap = pow2_ge(na);
  const size_t lds = (size_t)cap * sizeof(unsigned long long);
  MTGV_CHECK(lds <= 150 * 1024, ERR_INVALID, "nms: %d anchors exceed the LDS sort capacity", na);
  MTGV_CHECK(ws != nullptr && ws_bytes >= nms_workspace_bytes(n, na), ERR_INVALID, "nms: workspace too small");
  lds_opt_in<nms_kernel<ROWS>>(lds, 150 * 1024);
  hipLaunchKernelGGL(nms_kernel<ROWS>, dim3(n), dim3(NMS_THREADS), lds, s, pred, rows, nc, nm, na, cap, conf, iou, max_det, max_wh, n_det,
                     boxes, conf_out, cls_out, keep_idx, coef_out, ws);
  HIP_OK(hipGetLastError());
}

void nms_launch(const float* pred, int n, int nc, int nm, int na, float conf, float iou, int max_det, float max_wh, int* n_det,
                float* boxes, float* conf_out, int* cls_out, int* keep_idx, float* coef_out, int* ws, size_t ws_bytes,
                hipStream_t s) {
  nms_launch_form<false>(pred, HeadRows{}, n, nc, nm, na, conf, iou, max_det, max_wh, n_det, boxes, conf_out, cls_out, keep_idx, coef_out,
                         ws, ws_bytes, s);
}

void nms_rotated_launch(const float* pred, int n, int nc, int na, float conf, float iou, int max_det, float max_wh, int* n_det,
                        float* rboxes, float* conf_out, int* cls_out, int* keep_idx, int* ws, size_t ws_bytes, hipStream_t s) {
  MTGV_CHECK(n > 0 && nc > 0 && na > 0, ERR_INVALID, "nms_rotated: n=%d nc=%d na=%d", n, nc, na);
  MTGV_CHECK(max_det > 0 && max_det <= 1024, ERR_INVALID, "nms_rotated: max_det=%d outside [1,1024]", max_det);
  // (what the proof of the skipped cross-class pairs needs, see nms_rotated_kernel)
  MTGV_CHECK(iou > 0.f && max_wh >= 7680.f, ERR_INVALID, "nms_rotated: iou=%g must be > 0 and max_wh=%g >= 7680", (double)iou, (double)max_wh);
  const int cap = pow2_ge(na);
  const size_t lds = (size_t)std::max(cap, 2) * sizeof(unsigned long long);
  MTGV_CHECK(lds <= 150 * 1024, ERR_INVALID, "nms_rotated: %d anchors exceed the LDS sort capacity", na);
  MTGV_CHECK(ws != nullptr && ws_bytes >= nms_workspace_bytes(n, na), ERR_INVALID, "nms_rotated: workspace too small");
  lds_opt_in<nms_rotated_kernel>(lds, 150 * 1024);
  hipLaunchKernelGGL(nms_rotated_kernel, dim3(n), dim3(NMS_THREADS), lds, s, pred, nc, na, cap, conf, iou, max_det, max_wh, n_det, rboxes,
                     conf_out, cls_out, keep_idx, ws);
  HIP_OK(hipGetLastError());
}

int head_rows_anchors(const HeadRows& rows) {
  const int h = rows.in_h(), w = rows.in_w();
  return (h / 8) * (w / 8) + (h / 16) * (w / 16) + (h / 32) * (w / 32);
}

void head_rows_check(const HeadRows& rows, int nc, int nm) {
  MTGV_CHECK(rows.r0 && rows.r1 && rows.r2 && rows.imgsz > 0 && rows.imgsz % 32 == 0 && nc > 0 && nm >= 0, ERR_INVALID,
             "head rows: imgsz=%d nc=%d nm=%d", rows.imgsz, nc, nm);
  MTGV_CHECK((rows.h == 0 && rows.w == 0) || (rows.h > 0 && rows.w > 0 && rows.h % 32 == 0 && rows.w % 32 == 0), ERR_INVALID,
             "head rows: h=%d w=%d (both 0: imgsz x imgsz; otherwise multiples of 32)", rows.h, rows.w);
  MTGV_CHECK(rows.ct % 4 == 0 && rows.cls % 4 == 0 && rows.coef % 4 == 0 && rows.cls >= 64 && rows.coef >= 64 && rows.cls + nc <= rows.ct &&
                 rows.coef + nm <= rows.ct && (((uintptr_t)rows.r0 | (uintptr_t)rows.r1 | (uintptr_t)rows.r2) & 15) == 0,
             ERR_INVALID, "head rows: layout ct=%d cls=%d coef=%d (nc=%d nm=%d; 16-byte aligned rows)", rows.ct, rows.cls, rows.coef, nc, nm);
}

void nms_rows_launch(const HeadRows& rows, int n, int nc, int nm, float conf, float iou, int max_det, float max_wh, int* n_det,
                     float* boxes, float* conf_out, int* cls_out, int* keep_idx, float* coef_out, int* ws, size_t ws_bytes,
                     hipStream_t s) {
  head_rows_check(rows, nc, nm);
  nms_launch_form<true>(nullptr, rows, n, nc, nm, head_rows_anchors(rows), conf, iou, max_det, max_wh, n_det, boxes, conf_out, cls_out,
                        keep_idx, coef_out, ws, ws_bytes, s);
}

}  // namespace mtgv

extern "C" {
MTGV_API size_t mtgv_nms_workspace_bytes(int32_t n, int32_t na) {
  if (n <= 0 || na <= 0) return 0;
  return mtgv::nms_workspace_bytes(n, na);
}
MTGV_API size_t mtgv_nms_rotated_workspace_bytes(int32_t n, int32_t na) {
  if (n <= 0 || na <= 0) return 0;
  return mtgv::nms_workspace_bytes(n, na);  // seven words per sort slot, like the axis-aligned kernel
}
MTGV_API int mtgv_nms_rotated(const float* pred_dev, int32_t n, int32_t nc, int32_t na, float conf, float iou, int32_t max_det, float max_wh,
                              int32_t* n_det_dev, float* rboxes_dev, float* conf_dev, int32_t* cls_dev, int32_t* keep_idx_dev,
                              int32_t* workspace_dev, size_t workspace_bytes, void* stream) {
  return mtgv::guarded([&] {
    MTGV_CHECK(pred_dev && n_det_dev && rboxes_dev && conf_dev && cls_dev && keep_idx_dev, mtgv::ERR_INVALID, "null argument");
    mtgv::nms_rotated_launch(pred_dev, n, nc, na, conf, iou, max_det, max_wh, n_det_dev, rboxes_dev, conf_dev, cls_dev, keep_idx_dev,
                             workspace_dev, workspace_bytes, (hipStream_t)stream);
  });
}
MTGV_API int mtgv_op_probiou(const float* a_dev, const float* b_dev, int64_t m, float* out_dev, void* stream) {
  return mtgv::guarded([&] {
    MTGV_CHECK(m >= 0, mtgv::ERR_INVALID, "probiou: m=%lld", (long long)m);
    if (m == 0) return;
    MTGV_CHECK(a_dev && b_dev && out_dev, mtgv::ERR_INVALID, "null argument");
    hipLaunchKernelGGL(mtgv::probiou_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a_dev, b_dev, out_dev,
                       (long)m);
    HIP_OK(hipGetLastError());
  });
}
MTGV_API int mtgv_nms(const float* pred_dev, int32_t n, int32_t nc, int32_t nm, int32_t na, float conf, float iou,
                      int32_t max_det, float max_wh, int32_t* n_det_dev, float* boxes_dev, float* conf_dev, int32_t* cls_dev,
                      int32_t* keep_idx_dev, int32_t* workspace_dev, size_t workspace_bytes, void* stream) {
  return mtgv::guarded([&] {
    MTGV_CHECK(pred_dev && n_det_dev && boxes_dev && conf_dev && cls_dev && keep_idx_dev, mtgv::ERR_INVALID, "null argument");
    mtgv::nms_launch(pred_dev, n, nc, nm, na, conf, iou, max_det, max_wh, n_det_dev, boxes_dev, conf_dev, cls_dev, keep_idx_dev,
                     nullptr, workspace_dev, workspace_bytes, (hipStream_t)stream);
  });
}
}
