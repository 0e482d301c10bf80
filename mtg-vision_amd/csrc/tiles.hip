// Tiled detection, the merge: the detector ran on overlapping windows (tiles) of large source frames; this kernel maps the
// per-tile detections back into camera pixels, drops the cards a window cut, removes the duplicates the overlap produced
// and writes the K best cards of every frame for the crop stage (mtgv_warp_quads_src with an identity geometry).  The
// rule is this library's; mtgv/tiles.py: merge_tiles_host states it in numpy and the kernel is tested against that, every
// output bit for bit.  One workgroup of 1024 threads per frame, one candidate per thread:
//
//   1. candidate c = tl * Kt + j: detection j < min(n_det[t], Kt) of the frame's tl-th tile t.  Its box goes to camera
//      pixels in float64, x = (x_det - left) / ratio + x0 clipped to [x0, x0 + ww] (y likewise), rounded to float32, into LDS.
//   2. cut rule: a window side that is no side of the frame is an inner side; a box within `edge` of one is dropped.
//   3. key = conf as order-preserving bits << 32 | ~c; a dropped or missing candidate has key 0.  Bitonic sort in LDS,
//      descending: conf descending, tile ascending, j ascending; the keys are unique, so the order is deterministic.
//   4. greedy suppression in that order: the first candidate still alive is kept and knocks out every later one with
//      inter > ios_thr * min(area) (float32, no division, strict).  One ballot per wave and kept box; at most K rounds.
//   5. slot k < n_sel is the k-th kept candidate, the others are pad boxes.  No atomic decides a position.
//
// Every loop bound is known before its loop and every barrier is reached by all 1024 threads.  The mapping, the cut rule, the
// key, the sort and the greedy pass are tiles_merge.h's, shared with the rotated merge (tiles_obb.hip).
// No FMA contraction anywhere in this file: merge_tiles_host evaluates the same single operations.
#include "common.h"
#include "mtgv.h"
#include "tiles_merge.h"

#pragma clang fp contract(off)

namespace mtgv {

struct TilesMergeArgs {
  const int* n_det;     // (nt)
  const float* boxes;   // (nt, max_det, 4) xyxy, pixels of the tile's detector input
  const float* conf;    // (nt, max_det)
  const float* quads;   // (nt * kt, 4, 2) or null: the boxes' corners
  const int* tiles;     // (nt, 5) frame, y0, x0, wh, ww
  const int* geo;       // (nt, 4) nh, nw, top, left
  const double* ratio;  // (nt)
  const int* tile_start;  // (frames + 1)
  const int* hw;          // (frames, 2)
  const float* pad_frac;  // (k, 4)
  int nt, max_det, kt, max_tiles, k;
  float edge, ios_thr;
  float* sel_boxes;  // (frames * k, 4)
  float* quads_src;  // (frames * k, 4, 2)
  int* frame_idx;    // (frames * k)
  float* sel_conf;   // (frames * k)
  int* src_slot;     // (frames * k)
  int* n_sel;        // (frames)
};

__global__ __launch_bounds__(TILES_THREADS) void tiles_merge_kernel(const TilesMergeArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned long long keys[TILES_THREADS];  // 8 KiB
  __shared__ __attribute__((aligned(16))) float box[TILES_THREADS * 4];            // 16 KiB, by candidate index c
  __shared__ unsigned long long s_alive[2][TILES_WAVES];                          // the waves' ballots, double-buffered
  __shared__ int s_keep[TILES_MAX_K];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int K = a.k, Kt = a.kt;
  const int fh = a.hw[f * 2], fw = a.hw[f * 2 + 1];
  int ts, te;
  tiles_range(a.tile_start, f, a.nt, a.max_tiles, ts, te);
  const int ncand = (te - ts) * Kt;  // <= 1024: the launcher checked max_tiles * kt

  // 1. - 3. this thread's candidate
  unsigned long long key = 0ull;
  if (tid < ncand) {
    const int tl = tid / Kt, j = tid - tl * Kt, t = ts + tl;
    int nd = a.n_det[t];
    nd = nd < Kt ? nd : Kt;
    if (j < nd) {
      const int y0 = a.tiles[t * 5 + 1], x0 = a.tiles[t * 5 + 2], wh = a.tiles[t * 5 + 3], ww = a.tiles[t * 5 + 4];
      const double top = (double)a.geo[t * 4 + 2], left = (double)a.geo[t * 4 + 3], r = a.ratio[t];
      const float* b = a.boxes + ((long)t * a.max_det + j) * 4;
      const float bx0 = tile_to_src(b[0], left, r, (double)x0, (double)ww), by0 = tile_to_src(b[1], top, r, (double)y0, (double)wh);
      const float bx1 = tile_to_src(b[2], left, r, (double)x0, (double)ww), by1 = tile_to_src(b[3], top, r, (double)y0, (double)wh);
      box[tid * 4 + 0] = bx0, box[tid * 4 + 1] = by0, box[tid * 4 + 2] = bx1, box[tid * 4 + 3] = by1;
      if (!tiles_cut(bx0, by0, bx1, by1, x0, y0, ww, wh, fw, fh, a.edge)) key = tiles_key(a.conf[(long)t * a.max_det + j], tid);
    }
  }
  const int n2 = tiles_sort(keys, key, ncand);

  // 4. greedy suppression: thread i owns the i-th candidate of the order
  const unsigned long long mykey = keys[tid];
  const bool alive = tid < n2 && mykey != 0ull;
  const int c = tiles_cand(mykey);
  float mx0 = 0.f, my0 = 0.f, mx1 = 0.f, my1 = 0.f, marea = 0.f;
  if (alive) {
    mx0 = box[c * 4], my0 = box[c * 4 + 1], mx1 = box[c * 4 + 2], my1 = box[c * 4 + 3];
    marea = (mx1 - mx0) * (my1 - my0);
  }
  const int nk = tiles_greedy(
      keys, s_alive, s_keep, alive, K < ncand ? K : ncand,  // a round keeps one box or ends the pass
      [&](int pc) {
        const float ax0 = box[pc * 4], ay0 = box[pc * 4 + 1], ax1 = box[pc * 4 + 2], ay1 = box[pc * 4 + 3];
        const float aarea = (ax1 - ax0) * (ay1 - ay0);
        const float iw = max_f(0.f, min_f(ax1, mx1) - max_f(ax0, mx0)), ih = max_f(0.f, min_f(ay1, my1) - max_f(ay0, my0));
        const float inter = iw * ih;
        return inter > a.ios_thr * min_f(aarea, marea);
      },
      [](int, bool) {});

  // 5. the frame's K slots
  if (tid == 0) a.n_sel[f] = nk;
  if (tid < K) {
    const long o = (long)f * K + tid;
    float q[8], x0, y0, x1, y1, cf = 0.f;
    int slot = -1;
    if (tid < nk) {
      const int cc = tiles_cand(keys[s_keep[tid]]);
      const int tl = cc / Kt, j = cc - tl * Kt, t = ts + tl;
      x0 = box[cc * 4], y0 = box[cc * 4 + 1], x1 = box[cc * 4 + 2], y1 = box[cc * 4 + 3];
      cf = a.conf[(long)t * a.max_det + j];
      slot = t * Kt + j;
      if (a.quads != nullptr) {
        const int wy0 = a.tiles[t * 5 + 1], wx0 = a.tiles[t * 5 + 2], wh = a.tiles[t * 5 + 3], ww = a.tiles[t * 5 + 4];
        const double top = (double)a.geo[t * 4 + 2], left = (double)a.geo[t * 4 + 3], r = a.ratio[t];
        const float* s = a.quads + (long)slot * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          q[i * 2] = tile_to_src(s[i * 2], left, r, (double)wx0, (double)ww);
          q[i * 2 + 1] = tile_to_src(s[i * 2 + 1], top, r, (double)wy0, (double)wh);
        }
      } else {
        q[0] = x0, q[1] = y0, q[2] = x1, q[3] = y0, q[4] = x1, q[5] = y1, q[6] = x0, q[7] = y1;
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
  }
}

}  // namespace mtgv

using namespace mtgv;

extern "C" {
MTGV_API int mtgv_tiles_merge(const int32_t* n_det_dev, const float* boxes_dev, const float* conf_dev, const float* quads_dev, int32_t nt,
                              int32_t max_det, int32_t kt, const int32_t* tiles_dev, const int32_t* geo_dev, const double* ratio_dev,
                              const int32_t* tile_start_dev, const int32_t* hw_dev, int32_t frames, int32_t max_tiles_per_frame,
                              const float* pad_frac_dev, int32_t k, float edge, float ios_thr, float* sel_boxes_src_dev, float* quads_src_dev,
                              int32_t* frame_idx_dev, float* sel_conf_dev, int32_t* src_slot_dev, int32_t* n_sel_dev, void* stream) {
  return guarded([&] {
    // the caps first, from the caller's numbers alone: no device is needed to be told that a step is too large
    MTGV_CHECK(k >= 1 && k <= TILES_MAX_K, ERR_INVALID, "tiles merge: %d cards per frame outside [1, %d]", k, TILES_MAX_K);
    MTGV_CHECK(max_det >= 1 && kt >= 1 && kt <= max_det, ERR_INVALID, "tiles merge: %d cards per tile outside [1, max_det = %d]", kt, max_det);
    MTGV_CHECK(frames >= 0 && frames <= 65535, ERR_INVALID, "tiles merge: %d frames outside [0, 65535]", frames);
    MTGV_CHECK(nt >= 0 && max_tiles_per_frame >= 0 && (long)max_tiles_per_frame * kt <= TILES_THREADS, ERR_INVALID,
               "tiles merge: %ld candidates per frame (%d tiles x %d cards per tile) exceed the cap of %d", (long)max_tiles_per_frame * kt,
               max_tiles_per_frame, kt, TILES_THREADS);
    if (frames == 0) return;
    MTGV_CHECK(tile_start_dev && hw_dev && pad_frac_dev && sel_boxes_src_dev && quads_src_dev && frame_idx_dev && sel_conf_dev && src_slot_dev &&
                   n_sel_dev,
               ERR_INVALID, "tiles merge: null argument");
    MTGV_CHECK(nt == 0 || (n_det_dev && boxes_dev && conf_dev && tiles_dev && geo_dev && ratio_dev), ERR_INVALID, "tiles merge: null argument");
    const TilesMergeArgs a{n_det_dev, boxes_dev, conf_dev, quads_dev, tiles_dev, geo_dev, ratio_dev, tile_start_dev, hw_dev, pad_frac_dev,
                           nt, max_det, kt, max_tiles_per_frame, k, edge, ios_thr,
                           sel_boxes_src_dev, quads_src_dev, frame_idx_dev, sel_conf_dev, src_slot_dev, n_sel_dev};
    hipLaunchKernelGGL(tiles_merge_kernel, dim3(frames), dim3(TILES_THREADS), 0, (hipStream_t)stream, a);
    HIP_OK(hipGetLastError());
  });
}
}
