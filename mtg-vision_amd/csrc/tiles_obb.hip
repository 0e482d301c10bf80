// Tiled detection, the rotated merge: what tiles.hip does for xyxy boxes, for the oriented quads of an OBB detector.  The
// candidates are the card slots mtgv_obb_cards filled per tile (the tiles as frames); the overlap of two of them is the exact
// area of intersection of two convex quads, and a kept card that nobody oriented takes its orientation from an oriented
// duplicate it dropped.  The rule is this library's; mtgv/tiles.py: merge_tiles_obb_host and quad_inter_host state it in
// numpy and the kernel is tested against them, every output bit for bit.  One workgroup of 1024 threads per frame, one
// candidate per thread, the mapping, the cut rule, the key, the sort and the greedy pass being tiles_merge.h's:
//
//   1. candidate c = tl * Kt + j: slot j of the frame's tl-th tile t, if state[t * Kt + j] is 1 or 2 and the tile has a j-th
//      detection of card_cls (obb_cards_kernel's scan); its four corners go to camera pixels into LDS.
//   2. cut rule on the bounds of the mapped corners; key, sort.
//   3. greedy suppression: in a round every live thread behind the kept candidate a intersects its own quad with a's
//      (quad_pair) and drops out if inter > ios_thr * min(area_a, area_b).  A ballot of "dropped in this round and state 2"
//      per wave and round stays in LDS: its first bit is the round's donor.
//   4. slot k < n_sel is the k-th kept candidate, turned by its donor where it had state 1; the others are pad boxes.
//
// No FMA contraction anywhere in this file, and float32 division is the correctly rounded one.
#include "common.h"
#include "mtgv.h"
#include "tiles_merge.h"

#pragma clang fp contract(off)

namespace mtgv {

struct Quad {
  float x[4], y[4];
};

__device__ __forceinline__ float min4_f(const float (&v)[4]) { return min_f(min_f(v[0], v[1]), min_f(v[2], v[3])); }
__device__ __forceinline__ float max4_f(const float (&v)[4]) { return max_f(max_f(v[0], v[1]), max_f(v[2], v[3])); }

// the doubled signed area
__device__ __forceinline__ float quad_shoelace(const Quad& q) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) & 3;
    s = s + (q.x[i] * q.y[j] - q.x[j] * q.y[i]);
  }
  return s;
}

// sum over P's edges of cross(p', q') of the part p' -> q' of the edge that lies inside Q's four half-planes (sq: the sign
// of Q's winding, same: the product of both signs).  CLOSED: a point on a boundary line is inside and an edge along an edge of
// Q counts iff the two run the same way; open: neither.  Fully unrolled, every index a constant: registers only.
template <bool CLOSED>
__device__ __forceinline__ float quad_edge_sum(const Quad& P, const Quad& Q, float sq, float same) {
  float ex[4], ey[4], d[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ex[k] = Q.x[(k + 1) & 3] - Q.x[k], ey[k] = Q.y[(k + 1) & 3] - Q.y[k];
#pragma unroll
    for (int i = 0; i < 4; ++i) d[k][i] = sq * (ex[k] * (P.y[i] - Q.y[k]) - ey[k] * (P.x[i] - Q.x[k]));
  }
  float tot = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int e1 = (e + 1) & 3;
    const float dx = P.x[e1] - P.x[e], dy = P.y[e1] - P.y[e];
    float t0 = 0.f, t1 = 1.f;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dp = d[k][e], dq = d[k][e1];
      const bool line = !(ex[k] == 0.f && ey[k] == 0.f);  // a zero-length edge of Q bounds nothing
      const bool along = dp == 0.f && dq == 0.f;
      const bool inp = CLOSED ? dp >= 0.f : dp > 0.f, inq = CLOSED ? dq >= 0.f : dq > 0.f;
      const bool along_out = CLOSED ? (along && !(same * (dx * ex[k] + dy * ey[k]) > 0.f)) : along;
      const bool rest = line && !along;
      ok = ok && !(line && along_out) && !(rest && !inp && !inq);
      const bool cross = rest && (inp != inq);
      const float t = dp / (dp - dq);
      t1 = (cross && inp && t < t1) ? t : t1;
      t0 = (cross && !inp && t > t0) ? t : t0;
    }
    const float x0 = P.x[e] + t0 * dx, y0 = P.y[e] + t0 * dy;
    const float x1 = P.x[e] + t1 * dx, y1 = P.y[e] + t1 * dy;
    tot = (ok && t0 < t1) ? tot + (x0 * y1 - x1 * y0) : tot;
  }
  return tot;
}

// the pair function (quad_inter_host): a, b in absolute pixels -> inter, area_a, area_b
__device__ __forceinline__ void quad_pair(const Quad& a, const Quad& b, float& inter, float& area_a, float& area_b) {
  const float iw = min_f(max4_f(a.x), max4_f(b.x)) - max_f(min4_f(a.x), min4_f(b.x));
  const float ih = min_f(max4_f(a.y), max4_f(b.y)) - max_f(min4_f(a.y), min4_f(b.y));
  Quad ra, rb;
#pragma unroll
  for (int i = 0; i < 4; ++i) ra.x[i] = a.x[i] - a.x[0], ra.y[i] = a.y[i] - a.y[0], rb.x[i] = b.x[i] - a.x[0], rb.y[i] = b.y[i] - a.y[0];
  const float sa = quad_shoelace(ra), sb = quad_shoelace(rb);
  area_a = fabsf(sa) * 0.5f, area_b = fabsf(sb) * 0.5f;
  inter = 0.f;
  if (iw > 0.f && ih > 0.f && !(sa == 0.f) && !(sb == 0.f)) {  // (the shortcut is part of the rule)
    const float sga = sa > 0.f ? 1.f : -1.f, sgb = sb > 0.f ? 1.f : -1.f, same = sga * sgb;
    const float s = (sga * quad_edge_sum<true>(ra, rb, sgb, same) + sgb * quad_edge_sum<false>(rb, ra, sga, same)) * 0.5f;
    inter = s > 0.f ? s : 0.f;
  }
}

__device__ __forceinline__ Quad quad_load(const float* p) {
  Quad q;
#pragma unroll
  for (int i = 0; i < 4; ++i) q.x[i] = p[i * 2], q.y[i] = p[i * 2 + 1];
  return q;
}

struct TilesMergeObbArgs {
  const int* n_det;     // (nt)
  const float* conf;    // (nt, max_det)
  const int* cls;       // (nt, max_det)
  const float* quads;   // (nt * kt, 4, 2), pixels of the tile's detector input
  const int* state;     // (nt * kt)
  const int* tiles;     // (nt, 5) frame, y0, x0, wh, ww
  const int* geo;       // (nt, 4) nh, nw, top, left
  const double* ratio;  // (nt)
  const int* tile_start;  // (frames + 1)
  const int* hw;          // (frames, 2)
  const float* pad_frac;  // (k, 4)
  int nt, max_det, kt, max_tiles, k, card_cls;
  float edge, ios_thr;
  float* sel_boxes;  // (frames * k, 4)
  float* quads_src;  // (frames * k, 4, 2)
  int* frame_idx;    // (frames * k)
  float* sel_conf;   // (frames * k)
  int* src_slot;     // (frames * k)
  int* n_sel;        // (frames)
  int* state_out;    // (frames * k)
  int* oriented_by;  // (frames * k)
};

__global__ __launch_bounds__(TILES_THREADS) void tiles_merge_obb_kernel(const TilesMergeObbArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned long long keys[TILES_THREADS];   // 8 KiB
  __shared__ __attribute__((aligned(16))) float quad[TILES_THREADS * 8];            // 32 KiB, by candidate index c
  __shared__ unsigned long long s_donor[TILES_MAX_K][TILES_WAVES];                 // 8 KiB: round, wave -> dropped and state 2
  __shared__ unsigned long long s_alive[2][TILES_WAVES];
  __shared__ int s_keep[TILES_MAX_K];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.k, Kt = a.kt;
  const int fh = a.hw[f * 2], fw = a.hw[f * 2 + 1];
  int ts, te;
  tiles_range(a.tile_start, f, a.nt, a.max_tiles, ts, te);
  const int ncand = (te - ts) * Kt;  // <= 1024: the launcher checked max_tiles * kt

  // 1., 2. this thread's candidate
  unsigned long long key = 0ull;
  if (tid < ncand) {
    const int tl = tid / Kt, j = tid - tl * Kt, t = ts + tl;
    const int st = a.state[t * Kt + j];
    if (st == 1 || st == 2) {
      // the j-th detection of the card class (obb_cards_kernel's scan)
      const int nd = min(max(a.n_det[t], 0), a.max_det);
      const int* cl = a.cls + (long)t * a.max_det;
      int d = 0, seen = 0;
      for (; d < nd; ++d)
        if (cl[d] == a.card_cls && seen++ == j) break;
      if (d < nd) {
        const int y0 = a.tiles[t * 5 + 1], x0 = a.tiles[t * 5 + 2], wh = a.tiles[t * 5 + 3], ww = a.tiles[t * 5 + 4];
        const double top = (double)a.geo[t * 4 + 2], left = (double)a.geo[t * 4 + 3], r = a.ratio[t];
        const float* s = a.quads + (long)(t * Kt + j) * 8;
        Quad q;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          q.x[i] = tile_to_src(s[i * 2], left, r, (double)x0, (double)ww);
          q.y[i] = tile_to_src(s[i * 2 + 1], top, r, (double)y0, (double)wh);
          quad[tid * 8 + i * 2] = q.x[i], quad[tid * 8 + i * 2 + 1] = q.y[i];
        }
        if (!tiles_cut(min4_f(q.x), min4_f(q.y), max4_f(q.x), max4_f(q.y), x0, y0, ww, wh, fw, fh, a.edge))
          key = tiles_key(a.conf[(long)t * a.max_det + d], tid);
      }
    }
  }
  const int n2 = tiles_sort(keys, key, ncand);

  // 3. greedy suppression: thread i owns the i-th candidate of the order
  const unsigned long long mykey = keys[tid];
  const bool alive = tid < n2 && mykey != 0ull;
  const int c = tiles_cand(mykey);
  Quad mine = {};
  int mstate = 0;
  if (alive) {
    mine = quad_load(quad + c * 8);
    mstate = a.state[(ts + c / Kt) * Kt + (c - (c / Kt) * Kt)];
  }
  const int nk = tiles_greedy(
      keys, s_alive, s_keep, alive, K < ncand ? K : ncand,  // a round keeps one quad or ends the pass
      [&](int pc) {
        const Quad kept = quad_load(quad + pc * 8);
        float inter, area_a, area_b;
        quad_pair(kept, mine, inter, area_a, area_b);
        return !(area_a == 0.f) && !(area_b == 0.f) && inter > a.ios_thr * min_f(area_a, area_b);
      },
      [&](int round, bool dropped) {
        const unsigned long long m = __ballot(dropped && mstate == 2);
        if (lane == 0) s_donor[round][wave] = m;
      });

  // 4. the frame's K slots
  if (tid == 0) a.n_sel[f] = nk;
  if (tid < K) {
    const long o = (long)f * K + tid;
    float q[8], x0, y0, x1, y1, cf = 0.f;
    int slot = -1, st = 0, by = -1;
    if (tid < nk) {
      const int cc = tiles_cand(keys[s_keep[tid]]);
      const int tl = cc / Kt, j = cc - tl * Kt, t = ts + tl;
      slot = t * Kt + j;
      st = a.state[slot];
      const Quad kq = quad_load(quad + cc * 8);
      x0 = min4_f(kq.x), y0 = min4_f(kq.y), x1 = max4_f(kq.x), y1 = max4_f(kq.y);
      // the confidence: the same scan again (one thread per slot)
      const int nd = min(max(a.n_det[t], 0), a.max_det);
      const int* cl = a.cls + (long)t * a.max_det;
      int d = 0, seen = 0;
      for (; d < nd; ++d)
        if (cl[d] == a.card_cls && seen++ == j) break;
      cf = a.conf[(long)t * a.max_det + (d < nd ? d : 0)];
      // the round's donor: the first candidate of the order that this one dropped and that has state 2
      int dp = -1;
#pragma unroll
      for (int w = TILES_WAVES - 1; w >= 0; --w) {
        const unsigned long long mw = s_donor[tid][w];
        if (mw != 0ull) dp = (w << 6) + __builtin_ctzll(mw);
      }
      bool roll = false;
      if (st == 1 && dp >= 0) {
        const int dc = tiles_cand(keys[dp]);
        const Quad dq = quad_load(quad + dc * 8);
        const float uax = (kq.x[0] + kq.x[1]) - (kq.x[2] + kq.x[3]), uay = (kq.y[0] + kq.y[1]) - (kq.y[2] + kq.y[3]);
        const float ubx = (dq.x[0] + dq.x[1]) - (dq.x[2] + dq.x[3]), uby = (dq.y[0] + dq.y[1]) - (dq.y[2] + dq.y[3]);
        const float dot = uax * ubx + uay * uby;
        if (dot != 0.f) st = 2, by = (ts + dc / Kt) * Kt + (dc - (dc / Kt) * Kt);
        roll = dot < 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int s = (i + 2) & 3;
        q[i * 2] = roll ? kq.x[s] : kq.x[i], q[i * 2 + 1] = roll ? kq.y[s] : kq.y[i];
      }
    } else {
      const float* pf = a.pad_frac + tid * 4;
      x0 = pf[0] * (float)fw, y0 = pf[1] * (float)fh, x1 = pf[2] * (float)fw, y1 = pf[3] * (float)fh;
      q[0] = x0, q[1] = y0, q[2] = x1, q[3] = y0, q[4] = x1, q[5] = y1, q[6] = x0, q[7] = y1;
    }
    a.sel_boxes[o * 4 + 0] = x0, a.sel_boxes[o * 4 + 1] = y0, a.sel_boxes[o * 4 + 2] = x1, a.sel_boxes[o * 4 + 3] = y1;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.quads_src[o * 8 + i] = q[i];
    a.frame_idx[o] = f;
    a.sel_conf[o] = cf;
    a.src_slot[o] = slot;
    a.state_out[o] = st;
    a.oriented_by[o] = by;
  }
}

__global__ __launch_bounds__(256) void quad_inter_kernel(const float* __restrict__ a, const float* __restrict__ b, long m, float* __restrict__ inter,
                                                        float* __restrict__ area_a, float* __restrict__ area_b) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  float it, aa, ab;
  quad_pair(quad_load(a + i * 8), quad_load(b + i * 8), it, aa, ab);
  inter[i] = it, area_a[i] = aa, area_b[i] = ab;
}

}  // namespace mtgv

using namespace mtgv;

extern "C" {
MTGV_API int mtgv_tiles_merge_obb(const int32_t* n_det_dev, const float* conf_dev, const int32_t* cls_dev, const float* quads_dev,
                                  const int32_t* state_dev, int32_t nt, int32_t max_det, int32_t kt, const int32_t* tiles_dev,
                                  const int32_t* geo_dev, const double* ratio_dev, const int32_t* tile_start_dev, const int32_t* hw_dev,
                                  int32_t frames, int32_t max_tiles_per_frame, const float* pad_frac_dev, int32_t k, float edge, float ios_thr,
                                  int32_t card_cls, float* sel_boxes_src_dev, float* quads_src_dev, int32_t* frame_idx_dev, float* sel_conf_dev,
                                  int32_t* src_slot_dev, int32_t* n_sel_dev, int32_t* state_out_dev, int32_t* oriented_by_dev, void* stream) {
  return guarded([&] {
    // the caps first, from the caller's numbers alone: no device is needed to be told that a step is too large
    MTGV_CHECK(k >= 1 && k <= TILES_MAX_K, ERR_INVALID, "tiles merge obb: %d cards per frame outside [1, %d]", k, TILES_MAX_K);
    MTGV_CHECK(max_det >= 1 && kt >= 1 && kt <= max_det, ERR_INVALID, "tiles merge obb: %d cards per tile outside [1, max_det = %d]", kt, max_det);
    MTGV_CHECK(frames >= 0 && frames <= 65535, ERR_INVALID, "tiles merge obb: %d frames outside [0, 65535]", frames);
    MTGV_CHECK(nt >= 0 && max_tiles_per_frame >= 0 && (long)max_tiles_per_frame * kt <= TILES_THREADS, ERR_INVALID,
               "tiles merge obb: %ld candidates per frame (%d tiles x %d cards per tile) exceed the cap of %d", (long)max_tiles_per_frame * kt,
               max_tiles_per_frame, kt, TILES_THREADS);
    if (frames == 0) return;
    MTGV_CHECK(tile_start_dev && hw_dev && pad_frac_dev && sel_boxes_src_dev && quads_src_dev && frame_idx_dev && sel_conf_dev && src_slot_dev &&
                   n_sel_dev && state_out_dev && oriented_by_dev,
               ERR_INVALID, "tiles merge obb: null argument");
    MTGV_CHECK(nt == 0 || (n_det_dev && conf_dev && cls_dev && quads_dev && state_dev && tiles_dev && geo_dev && ratio_dev), ERR_INVALID,
               "tiles merge obb: null argument");
    const TilesMergeObbArgs a{n_det_dev, conf_dev, cls_dev, quads_dev, state_dev, tiles_dev, geo_dev, ratio_dev, tile_start_dev, hw_dev, pad_frac_dev,
                              nt, max_det, kt, max_tiles_per_frame, k, card_cls, edge, ios_thr,
                              sel_boxes_src_dev, quads_src_dev, frame_idx_dev, sel_conf_dev, src_slot_dev, n_sel_dev, state_out_dev, oriented_by_dev};
    hipLaunchKernelGGL(tiles_merge_obb_kernel, dim3(frames), dim3(TILES_THREADS), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
  });
}

MTGV_API int mtgv_op_quad_inter(const float* a_dev, const float* b_dev, int64_t m, float* inter_dev, float* area_a_dev, float* area_b_dev,
                                void* stream) {
  return guarded([&] {
    MTGV_CHECK(m >= 0, ERR_INVALID, "quad_inter: m=%lld", (long long)m);
    if (m == 0) return;
    MTGV_CHECK(a_dev && b_dev && inter_dev && area_a_dev && area_b_dev, ERR_INVALID, "quad_inter: null argument");
    hipLaunchKernelGGL(quad_inter_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a_dev, b_dev, (long)m, inter_dev,
                       area_a_dev, area_b_dev);
    HIP_OK(hipGetLastError());
  });
}
}
