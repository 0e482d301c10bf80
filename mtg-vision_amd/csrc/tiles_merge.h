// What the two tile-merge kernels share (tiles.hip: mtgv_tiles_merge on xyxy boxes, tiles_obb.hip: mtgv_tiles_merge_obb on
// oriented quads): the mapping of a coordinate into camera pixels, the cut rule, the 64-bit order key, the bitonic sort and
// the greedy pass with one ballot per wave.  One workgroup of TILES_THREADS threads per frame, one candidate per thread.
// Every loop bound is known before its loop and every barrier is reached by all the threads.
// No FMA contraction: the host rules (mtgv/tiles.py) evaluate the same single operations.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace mtgv {

static constexpr int TILES_THREADS = 1024;  // = the cap on candidates per frame
static constexpr int TILES_WAVES = TILES_THREADS / 64;
static constexpr int TILES_MAX_K = 64;

// one coordinate of the detector's input -> camera pixels: float64, clipped to the window (comparisons, not fmin / fmax: a
// NaN stays one, as under np.where), rounded to float32
__device__ __forceinline__ float tile_to_src(float v, double pad, double ratio, double origin, double extent) {
  double s = ((double)v - pad) / ratio + origin;
  const double hi = origin + extent;
  s = s < origin ? origin : (s > hi ? hi : s);
  return (float)s;
}

__device__ __forceinline__ float min_f(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float max_f(float a, float b) { return a > b ? a : b; }

// the frame's tiles; tile_start is trusted no further than max_tiles: a longer, negative or outlying range has no candidates
__device__ __forceinline__ void tiles_range(const int* tile_start, int f, int nt, int max_tiles, int& ts, int& te) {
  ts = tile_start[f], te = tile_start[f + 1];
  if (ts < 0 || te < ts || te > nt || te - ts > max_tiles) te = ts = 0;
}

// the cut rule on a candidate's bounds: a window side that is no side of the frame is an inner side
__device__ __forceinline__ bool tiles_cut(float bx0, float by0, float bx1, float by1, int x0, int y0, int ww, int wh, int fw, int fh, float e) {
  return (x0 > 0 && bx0 < (float)x0 + e) || (x0 + ww < fw && bx1 > (float)(x0 + ww) - e) || (y0 > 0 && by0 < (float)y0 + e) ||
         (y0 + wh < fh && by1 > (float)(y0 + wh) - e);
}

// key = conf as order-preserving bits << 32 | ~c: descending keys are conf descending, candidate index ascending; 0 is no
// candidate (a finite conf >= 0 gives ord >= 2^31)
__device__ __forceinline__ unsigned long long tiles_key(float conf, int c) {
  const unsigned u = __float_as_uint(conf);
  const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)ord << 32) | (unsigned)(~(unsigned)c);
}
__device__ __forceinline__ int tiles_cand(unsigned long long key) { return (int)(~(unsigned)(key & 0xffffffffull)) & (TILES_THREADS - 1); }

// keys[tid] = key, then the bitonic sort of keys[0, n2), descending: the absent ones (0) end up behind the survivors.
// Returns n2, the power of two >= ncand (block-uniform, <= 1024).
__device__ __forceinline__ int tiles_sort(unsigned long long* keys, unsigned long long key, int ncand) {
  const int tid = threadIdx.x;
  keys[tid] = key;
  int n2 = 1;
  while (n2 < ncand) n2 <<= 1;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int l = tid ^ j;
      if (tid < n2 && l > tid) {
        const unsigned long long x = keys[tid], y = keys[l];
        const bool desc = (tid & k) == 0;
        if (desc ? (x < y) : (x > y)) keys[tid] = y, keys[l] = x;
      }
      __syncthreads();
    }
  }
  return n2;
}

// greedy suppression in the sorted order, thread i owning the i-th candidate: the first candidate still alive is kept
// (s_keep[round] = its position) and every later live thread asks drop(pc), pc being the kept one's candidate index.  One
// ballot per wave and round; at most `rounds` rounds.  done(round, dropped) is called by every thread of a round that kept
// one.  Returns the number kept (block-uniform); ends with a barrier, so s_keep is complete.
template <class Drop, class Done>
__device__ __forceinline__ int tiles_greedy(const unsigned long long* keys, unsigned long long (*s_alive)[TILES_WAVES], int* s_keep, bool alive,
                                            int rounds, Drop drop, Done done) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nk = 0;
  bool open = true;  // block-uniform
  for (int it = 0; it < rounds; ++it) {
    const unsigned long long m = __ballot(alive);
    if (lane == 0) s_alive[it & 1][wave] = m;
    __syncthreads();  // (the other buffer was last read one round ago, in front of this barrier's predecessor)
    int p = -1;
    if (open) {
#pragma unroll
      for (int w = TILES_WAVES - 1; w >= 0; --w) {
        const unsigned long long mw = s_alive[it & 1][w];
        if (mw != 0ull) p = (w << 6) + __builtin_ctzll(mw);
      }
    }
    if (p < 0) {
      open = false;  // nobody is alive: the remaining rounds only keep the barriers in step
    } else {
      const int pc = tiles_cand(keys[p]);
      if (tid == p) s_keep[nk] = p, alive = false;
      bool dropped = false;
      if (alive && tid > p) dropped = drop(pc);
      if (dropped) alive = false;
      done(nk, dropped);
      nk += 1;
    }
  }
  __syncthreads();
  return nk;
}

}  // namespace mtgv
