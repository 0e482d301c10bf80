// Detection mask -> ultralytics `masks.xy` contour points on the GPU.
//
// Replaces the host tracing of mtgv.adapters._mask_segments (ops.masks2segments behind mtgvision/od_export.py:152-153:
// cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) per mask; cv2 / ultralytics absent, parity unpinned).  The host
// function stays in the product as the specification and the fallback; this kernel reproduces it point for point:
//   1. foreground as a bit image in LDS with a zero border (mask != 0, or the logits' bilinear x`scale` interpolation > 0)
//   2. row runs in raster order; runs of adjacent rows that touch ([x0 - 1, x1 + 1] overlap: 8-connectivity) are merged by
//      a union-find on run indices whose links always point at the smaller index, so a blob's root is its first run in
//      raster order: roots in index order are scipy's label order (3 x 3 structure), and a root's x0 is the leftmost
//      pixel of the blob's top row, the trace's start
//   3. Moore trace of every blob from the bit image, one lane per blob: neighbours W NW N NE E SE S SW, scan from
//      `back` (0 at the start), after a move in direction d back = (d + 5) % 8; the walk ends when it steps on the start
//      pixel again (from any direction - which truncates some shapes, as on the host) or finds no neighbour
//   4. CHAIN_APPROX_SIMPLE on the closed chain: point i stays iff p[i] - p[i-1] != p[i+1] - p[i] (cyclic); the first
//      trace only counts the kept points (it knows the closing step, which point 0 needs, only at its end), a prefix
//      sum over the blobs gives every blob's offset ("largest": the first blob with the most points, at offset 0), the
//      second trace writes (blob 0 of "all" and a mask's only blob start at offset 0 whatever the counts are and are
//      written during the first trace).  No atomic decides an output position: the result is deterministic.
// Every loop is bounded before it starts: a trace by 8 x the mask's foreground pixels (it visits a (pixel, back) state
// once) and by the point capacity, union-find walks by the run count.  A mask over a cap (CT_MAX_RUNS runs, CT_MAX_BLOBS
// blobs, max_points points, or a bound hit) reports status 1 and the host path takes it.
#include "common.h"
#include "mtgv.h"

#pragma clang fp contract(off)

namespace mtgv {

constexpr int CT = 512;            // threads per block (one block per mask)
constexpr int CT_NW = CT / 64;     // waves
// Per-mask capacities.  tests/contours_common.py restates them (MAX_RUNS, MAX_BLOBS): keep the two in step.
constexpr int CT_MAX_RUNS = 4096;   // row runs of one mask (run table in LDS: 12 bytes each)
constexpr int CT_MAX_BLOBS = 1024;  // 8-connected blobs of one mask (blob table in the workspace: 16 bytes each)
constexpr size_t CT_LDS_LIMIT = 150 * 1024;

// words of one row of the bit image: a zero word on the left, pixel x at bit x + 32, at least one zero bit on the right
__host__ __device__ static inline int ct_wpr(int w) { return (w + 64) / 32; }
static inline size_t ct_lds_bytes(int h, int w) {
  return ((size_t)(h + 2) * ct_wpr(w) + 1) * 4 + (size_t)CT_MAX_RUNS * 12 + (size_t)2 * (h + 1) * 4;
}
static inline size_t ct_workspace_bytes(int n) { return (size_t)n * CT_MAX_BLOBS * 16; }

// exclusive prefix of `v` over the block's threads in thread order, and the block's total.  s_w: CT_NW ints of LDS.
__device__ __forceinline__ int ct_block_scan(int v, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  __syncthreads();  // s_w may still be read from the previous scan
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < CT_NW; ++k) {
    const int s = s_w[k];
    base += k < wave ? s : 0;
    tot += s;
  }
  total = tot;
  return base + incl - v;
}

// step of direction d (W NW N NE E SE S SW) as dx + 1 and dy + 1, two bits per direction
constexpr uint32_t CT_DX = 0u | 0u << 2 | 1u << 4 | 2u << 6 | 2u << 8 | 2u << 10 | 1u << 12 | 0u << 14;
constexpr uint32_t CT_DY = 1u | 0u << 2 | 0u << 4 | 0u << 6 | 1u << 8 | 2u << 10 | 2u << 12 | 2u << 14;
__device__ __forceinline__ int ct_dx(int d) { return (int)((CT_DX >> (2 * d)) & 3u) - 1; }
__device__ __forceinline__ int ct_dy(int d) { return (int)((CT_DY >> (2 * d)) & 3u) - 1; }

// the three pixels left of, at and right of bit column c in image row r (bit 0 = left)
__device__ __forceinline__ uint32_t ct_row3(const uint32_t* img, int wpr, int r, int c) {
  const int wi = (c - 1) >> 5, sh = (c - 1) & 31;
  const uint32_t lo = img[r * wpr + wi], hi = img[r * wpr + wi + 1];  // wi + 1 <= wpr: the next row's zero word or the pad word
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & 7u;
}

// One blob's trace from its start pixel (image row sr, bit column sc): returns the number of points CHAIN_APPROX_SIMPLE
// keeps, and in keep0 whether point 0 is among them (known only at the end: it needs the closing step).  WRITE = true
// also stores the kept points (x, y) at out[pos], out[pos + 1] ... while pos < cap, point 0 first if keep0_in says so;
// with stop_at_cap the walk ends once the slot is full (the returned count is then meaningless: the caller has it from the
// counting pass).  `bad` is set when the walk is still going after max_steps steps.
template <bool WRITE>
__device__ __forceinline__ int ct_trace(const uint32_t* img, int wpr, int sr, int sc, int max_steps, int keep0_in, bool stop_at_cap,
                                        int& keep0, int* out, int pos, int cap, bool& bad) {
  int cr = sr, cc = sc, back = 0, np = 1, fd = 0, pd = 0, cnt = 0;
  bool done = false;
  auto put = [&](int r, int c) {
    if (pos < cap) out[2 * pos] = c - 32, out[2 * pos + 1] = r - 1;
    ++pos;
  };
  if (WRITE && keep0_in) put(sr, sc);
  for (int step = 0; step < max_steps; ++step) {
    if (WRITE && stop_at_cap && pos >= cap) {  // the slot is full: the mask is over the cap, nothing more can be written
      done = true;
      break;
    }
    const uint32_t top = ct_row3(img, wpr, cr - 1, cc), mid = ct_row3(img, wpr, cr, cc), bot = ct_row3(img, wpr, cr + 1, cc);
    // bit d = neighbour d is set
    const uint32_t ring = (mid & 1u) | top << 1 | (mid >> 2) << 4 | (bot >> 2) << 5 | ((bot >> 1) & 1u) << 6 | (bot & 1u) << 7;
    const uint32_t rot = ((ring | ring << 8) >> back) & 0xffu;
    if (rot == 0u) {  // an isolated pixel
      done = true;
      break;
    }
    const int d = (back + __builtin_ctz(rot)) & 7;
    const int nr = cr + ct_dy(d), nc = cc + ct_dx(d);
    back = (d + 5) & 7;
    if (nr == sr && nc == sc) {  // on the start again: the chain is closed
      done = true;
      break;
    }
    // (nr, nc) is point np; the step into it is the out-step of point np - 1 = (cr, cc)
    if (np == 1) {
      fd = d;
    } else if (pd != d) {
      if (WRITE) put(cr, cc);
      ++cnt;
    }
    pd = d, cr = nr, cc = nc, ++np;
  }
  if (!done) bad = true;
  if (np == 1) {  // a single point is kept as it is
    keep0 = 1;
    return 1;
  }
  // the closing step, last point -> point 0 (not a unit step where the walk was cut short)
  const int qy = sr - cr, qx = sc - cc;
  const bool keep_last = ct_dy(pd) != qy || ct_dx(pd) != qx;
  if (WRITE && keep_last) put(cr, cc);
  keep0 = (ct_dy(fd) != qy || ct_dx(fd) != qx) ? 1 : 0;
  cnt += (keep_last ? 1 : 0) + keep0;
  if (cnt == 0) cnt = 1, keep0 = 1;  // nothing kept: the first point
  return cnt;
}

// LOGITS = false: `src` is the (n, H, W) uint8 mask.  LOGITS = true: `src` is the (n, H / scale, W / scale) float mask
// logits; foreground is the expression of mask_binarize_kernel (detector_kernel.h) and mask_quads_kernel<true>
// (quads.hip), in their order (tests/test_gpu_contours.py pins the equality).
template <bool LOGITS>
__global__ __launch_bounds__(CT) void mask_contours_kernel(const void* __restrict__ src, int H, int W, int scale, int strategy,
                                                          int max_points, int* __restrict__ points, int* __restrict__ n_points,
                                                          int* __restrict__ n_blobs, int* __restrict__ status, int4* ws) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sm_u[];
  const int wpr = ct_wpr(W);
  const int n_words = (H + 2) * wpr + 1;
  uint32_t* img = sm_u;                                        // [(H + 2) * wpr + 1]
  int* run_y = reinterpret_cast<int*>(img + n_words);           // [CT_MAX_RUNS]
  int* run_xx = run_y + CT_MAX_RUNS;                            // [CT_MAX_RUNS] x0 | x1 << 16
  int* parent = run_xx + CT_MAX_RUNS;                           // [CT_MAX_RUNS]
  int* rowoff = parent + CT_MAX_RUNS;                           // [H + 1] first run of every row
  int* lr_lo = rowoff;                                          // LOGITS, before rowoff is filled: first / last positive
  int* lr_hi = rowoff + (H + 1);                                // column of a logit row, [H / scale] each
  __shared__ int s_w[CT_NW];
  __shared__ int s_best[CT_NW][2];
  __shared__ int s_bad;

  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int4* blob = ws + (size_t)n * CT_MAX_BLOBS;  // x: first run, y: kept points, z: keep0, w: offset
  int* out = points + (size_t)n * max_points * 2;
  if (tid == 0) s_bad = 0;

  // ---- 1. the bit image: a thread per word ----
  if (LOGITS) {
    const int mh = H / scale, mw = W / scale;
    const float* Lg = reinterpret_cast<const float*>(src) + (size_t)n * mh * mw;
    for (int r = wave; r < mh; r += CT_NW) {  // which logit rows / columns are positive at all (as quads.hip)
      int lo = 0x7fffffff, hi = -1;
      for (int c = lane; c < mw; c += 64)
        if (Lg[r * mw + c] > 0.f) lo = c < lo ? c : lo, hi = c > hi ? c : hi;
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) {
        const int olo = __shfl_xor(lo, m), ohi = __shfl_xor(hi, m);
        lo = olo < lo ? olo : lo;
        hi = ohi > hi ? ohi : hi;
      }
      if (lane == 0) lr_lo[r] = lo, lr_hi[r] = hi;
    }
    __syncthreads();
    const float inv = 1.0f / (float)scale;
    for (int i = tid; i < n_words; i += CT) {
      const int r = i / wpr, j = i - r * wpr;
      uint32_t bits = 0u;
      if (r >= 1 && r <= H && j >= 1) {
        const int y = r - 1, xb0 = (j - 1) * 32;
        float sy = inv * ((float)y + 0.5f) - 0.5f;
        sy = sy < 0.f ? 0.f : sy;
        const int y0 = (int)sy;
        const int y1 = y0 + (y0 < mh - 1 ? 1 : 0);
        const float ly1 = sy - (float)y0;
        const float ly0 = 1.0f - ly1;
        const int clo = lr_lo[y0] < lr_lo[y1] ? lr_lo[y0] : lr_lo[y1];
        const int chi = lr_hi[y0] > lr_hi[y1] ? lr_hi[y0] : lr_hi[y1];
        // a pixel whose four taps are all <= 0 is background: only columns near positive logits are evaluated
        if (chi >= 0) {
          int xa = (clo - 1) * scale, xe = (chi + 2) * scale;
          xa = xa < xb0 ? xb0 : xa;
          xe = xe > W ? W : xe;
          xe = xe > xb0 + 32 ? xb0 + 32 : xe;
          int tx0 = -1;  // the four taps are reloaded only when the left tap column moves (every `scale` pixels)
          float t00 = 0.f, t01 = 0.f, t10 = 0.f, t11 = 0.f;
          for (int x = xa; x < xe; ++x) {
            float sxf = inv * ((float)x + 0.5f) - 0.5f;
            sxf = sxf < 0.f ? 0.f : sxf;
            const int x0 = (int)sxf;
            const int x1 = x0 + (x0 < mw - 1 ? 1 : 0);
            const float lx1 = sxf - (float)x0;
            const float lx0 = 1.0f - lx1;
            if (x0 != tx0) {
              t00 = Lg[y0 * mw + x0], t01 = Lg[y0 * mw + x1], t10 = Lg[y1 * mw + x0], t11 = Lg[y1 * mw + x1];
              tx0 = x0;
            }
            const float v = ly0 * (lx0 * t00 + lx1 * t01) + ly1 * (lx0 * t10 + lx1 * t11);
            if (v > 0.f) bits |= 1u << (x - xb0);
          }
        }
      }
      img[i] = bits;
    }
  } else {
    const uint8_t* m = reinterpret_cast<const uint8_t*>(src) + (size_t)n * H * W;
    const bool vec = (W % 16) == 0 && ((size_t)m % 16) == 0;
    for (int i = tid; i < n_words; i += CT) {
      const int r = i / wpr, j = i - r * wpr;
      uint32_t bits = 0u;
      if (r >= 1 && r <= H && j >= 1) {
        const uint8_t* row = m + (size_t)(r - 1) * W;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int xb = (j - 1) * 32 + half * 16;
          if (xb >= W) continue;
          uint8_t px[16];
          if (vec) {
            *reinterpret_cast<uint4*>(px) = *reinterpret_cast<const uint4*>(row + xb);
          } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) px[k] = xb + k < W ? row[xb + k] : 0;
          }
#pragma unroll
          for (int k = 0; k < 16; ++k) bits |= (px[k] != 0 ? 1u : 0u) << (half * 16 + k);
        }
      }
      img[i] = bits;
    }
  }
  __syncthreads();

  // ---- 2. row runs in raster order: a thread owns consecutive rows ----
  const int R = (H + CT - 1) / CT;
  const int y_begin = tid * R < H ? tid * R : H, y_end = y_begin + R < H ? y_begin + R : H;
  int c_local = 0, fg_local = 0;
  for (int y = y_begin; y < y_end; ++y) {
    const uint32_t* row = img + (y + 1) * wpr;
    int c = 0;
    for (int j = 1; j < wpr; ++j) {
      const uint32_t w = row[j];
      c += __popc(w & ~(w << 1 | row[j - 1] >> 31));  // bits whose left neighbour is clear: run starts
      fg_local += __popc(w);
    }
    rowoff[y] = c;  // (lr_lo / lr_hi are dead: the image is built)
    c_local += c;
  }
  int n_runs, fg;
  const int run_base = ct_block_scan(c_local, s_w, n_runs);
  ct_block_scan(fg_local, s_w, fg);
  if (n_runs > CT_MAX_RUNS || n_runs == 0) {  // block-uniform
    if (tid == 0) {
      n_points[n] = 0, status[n] = n_runs > CT_MAX_RUNS ? 1 : 0;
      if (n_blobs != nullptr) n_blobs[n] = 0;
    }
    return;
  }
  {
    int o = run_base;
    for (int y = y_begin; y < y_end; ++y) {
      const int c = rowoff[y];
      rowoff[y] = o;
      const uint32_t* row = img + (y + 1) * wpr;
      int k = o, x0 = 0;
      bool in_run = false;
      auto emit = [&](int x1) {
        if (k < CT_MAX_RUNS) run_y[k] = y, run_xx[k] = x0 | x1 << 16, parent[k] = k;
        ++k;
      };
      for (int j = 1; j < wpr; ++j) {
        uint32_t t = row[j];
        const int xb = (j - 1) * 32;
        if (in_run) {
          const int ones = __builtin_ctzll(~(uint64_t)t);  // 32 when the word is full
          if (ones == 32) continue;
          emit(xb + ones - 1);
          in_run = false;
          t &= ~((1u << ones) - 1u);
        }
        while (t != 0u) {  // at most 16 runs start in a word
          const int s = __builtin_ctz(t);
          const int ones = __builtin_ctzll(~(uint64_t)(t >> s));
          x0 = xb + s;
          if (s + ones >= 32) {  // runs on into the next word (the last word of a row ends in a zero bit)
            in_run = true;
            break;
          }
          emit(xb + s + ones - 1);
          t &= ~(((1u << ones) - 1u) << s);
        }
      }
      o += c;
    }
    if (tid == CT - 1) rowoff[H] = n_runs;
  }
  __syncthreads();

  // ---- 3. union-find: a thread per run links it to the touching runs of the row above ----
  // find: parents only ever point at smaller indices, so a walk ends within n_runs steps
  auto find = [&](int a) -> int {
    for (int it = 0; it < n_runs; ++it) {
      const int p = __hip_atomic_load(&parent[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (p == a) return a;
      a = p;
    }
    s_bad = 1;
    return a;
  };
  for (int i = tid; i < n_runs; i += CT) {
    const int y = run_y[i];
    if (y == 0) continue;
    const int x0 = run_xx[i] & 0xffff, x1 = run_xx[i] >> 16;
    for (int k = rowoff[y - 1]; k < rowoff[y]; ++k) {
      const int kx0 = run_xx[k] & 0xffff, kx1 = run_xx[k] >> 16;
      if (kx0 > x1 + 1) break;
      if (kx1 < x0 - 1) continue;
      // union(i, k): the larger root is linked under the smaller.  The larger of the pair shrinks with every retry
      // (a retry happens when another thread re-linked `a` first), so n_runs iterations always suffice.
      int a = i, b = k, it = 0;
      for (; it < n_runs; ++it) {
        a = find(a), b = find(b);
        if (a == b) break;
        if (a < b) {
          const int t = a;
          a = b, b = t;
        }
        const int old = atomicMin(&parent[a], b);
        if (old == a) break;
        a = old;
      }
      if (it == n_runs) s_bad = 1;
    }
  }
  __syncthreads();

  // ---- 4. blobs = roots in index order: a thread owns consecutive runs ----
  const int RR = (n_runs + CT - 1) / CT;
  const int r_begin = tid * RR < n_runs ? tid * RR : n_runs, r_end = r_begin + RR < n_runs ? r_begin + RR : n_runs;
  int b_local = 0;
  for (int i = r_begin; i < r_end; ++i) b_local += parent[i] == i ? 1 : 0;
  int nb;
  int b_pos = ct_block_scan(b_local, s_w, nb);
  if (nb > CT_MAX_BLOBS || s_bad != 0) {  // block-uniform (s_bad was last written before the barriers of the scan)
    if (tid == 0) {
      n_points[n] = 0, status[n] = 1;
      if (n_blobs != nullptr) n_blobs[n] = nb;
    }
    return;
  }
  for (int i = r_begin; i < r_end; ++i)
    if (parent[i] == i) blob[b_pos++].x = i;
  __syncthreads();

  // ---- 5. first trace: count.  Blob b is traced by lane b / 8 of wave b % 8, so that a few blobs sit on different waves.
  // A blob whose offset is known beforehand - blob 0 of "all", the only blob of a mask: the usual card - is written in
  // this walk already, with point 0 first: it is the leftmost pixel of the top row, so the walk leaves it to the E, SE, S
  // or SW and comes back from there, two different steps, and it is always kept (were it not, the mask reports status 1).
  const int max_steps = 8 * fg;
  const int BB = (nb + CT - 1) / CT;
  const bool direct0 = strategy == 0 || nb == 1;  // blob 0 needs no second walk
  bool bad = false;
  for (int q = 0; q < BB; ++q) {
    const int b = q * CT + lane * CT_NW + wave;
    if (b >= nb) continue;
    const int i = blob[b].x, sr = run_y[i] + 1, sc = (run_xx[i] & 0xffff) + 32;
    int keep0 = 0, cnt;
    if (b == 0 && direct0) {
      cnt = ct_trace<true>(img, wpr, sr, sc, max_steps, 1, false, keep0, out, 0, max_points, bad);
      if (keep0 != 1) bad = true;
    } else {
      cnt = ct_trace<false>(img, wpr, sr, sc, max_steps, 0, false, keep0, nullptr, 0, 0, bad);
    }
    blob[b].y = cnt, blob[b].z = keep0;
  }
  if (bad) s_bad = 1;
  __syncthreads();

  // ---- 6. offsets: a thread owns consecutive blobs ----
  const int k_begin = tid * BB < nb ? tid * BB : nb, k_end = k_begin + BB < nb ? k_begin + BB : nb;
  int total, best = -1;
  if (strategy == 0) {
    int p_local = 0;
    for (int b = k_begin; b < k_end; ++b) p_local += blob[b].y;
    int off = ct_block_scan(p_local, s_w, total);
    for (int b = k_begin; b < k_end; ++b) {
      blob[b].w = off;
      off += blob[b].y;
    }
  } else {  // the first blob with the most points
    int bc = -1, bi = 0x7fffffff;
    for (int b = k_begin; b < k_end; ++b)
      if (blob[b].y > bc) bc = blob[b].y, bi = b;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const int oc = __shfl_xor(bc, m), oi = __shfl_xor(bi, m);
      if (oc > bc || (oc == bc && oi < bi)) bc = oc, bi = oi;
    }
    if (lane == 0) s_best[wave][0] = bc, s_best[wave][1] = bi;
    __syncthreads();
    bc = -1, bi = 0x7fffffff;
    for (int k = 0; k < CT_NW; ++k)
      if (s_best[k][0] > bc || (s_best[k][0] == bc && s_best[k][1] < bi)) bc = s_best[k][0], bi = s_best[k][1];
    total = bc, best = bi;
  }
  __syncthreads();

  // ---- 7. second trace: write (the counting walk found the same chain within max_steps, or the mask has status 1) ----
  for (int q = 0; q < BB; ++q) {
    const int b = q * CT + lane * CT_NW + wave;
    if (b >= nb || (strategy != 0 && b != best) || (b == 0 && direct0)) continue;
    const int4 e = blob[b];
    int keep0;
    ct_trace<true>(img, wpr, run_y[e.x] + 1, (run_xx[e.x] & 0xffff) + 32, max_steps, e.z, true, keep0, out, strategy == 0 ? e.w : 0, max_points, bad);
  }
  if (tid == 0) {
    n_points[n] = total < max_points ? total : max_points;
    status[n] = (total > max_points || s_bad != 0) ? 1 : 0;
    if (n_blobs != nullptr) n_blobs[n] = nb;
  }
}

}  // namespace mtgv

using namespace mtgv;

namespace {
template <bool LOGITS>
void launch_contours(const void* src, int n, int h, int w, int scale, int strategy, int max_points, int* points, int* n_points,
                     int* n_blobs, int* status, void* ws, size_t ws_bytes, hipStream_t s) {
  // every argument check comes before the first HIP call
  MTGV_CHECK(n >= 1 && h >= 1 && w >= 1 && max_points >= 1, ERR_INVALID, "mask_contours: n=%d h=%d w=%d max_points=%d", n, h, w, max_points);
  MTGV_CHECK(scale >= 1, ERR_INVALID, "mask_contours: scale=%d", scale);
  MTGV_CHECK(strategy == 0 || strategy == 1, ERR_INVALID, "mask_contours: unknown strategy %d (0 all, 1 largest)", strategy);
  MTGV_CHECK(h <= 32767 && w <= 32767 && ct_lds_bytes(h, w) <= CT_LDS_LIMIT, ERR_INVALID,
             "mask_contours: a %d x %d mask exceeds the LDS capacity", h, w);
  MTGV_CHECK(ws_bytes >= ct_workspace_bytes(n), ERR_INVALID, "mask_contours: workspace of %zu bytes, %zu needed", ws_bytes,
             ct_workspace_bytes(n));
  MTGV_CHECK(src != nullptr && points != nullptr && n_points != nullptr && status != nullptr && ws != nullptr, ERR_INVALID,
             "mask_contours: null argument");
  const size_t lds = ct_lds_bytes(h, w);
  lds_opt_in<mask_contours_kernel<LOGITS>>(lds, (int)CT_LDS_LIMIT);
  hipLaunchKernelGGL((mask_contours_kernel<LOGITS>), dim3(n), dim3(CT), lds, s, src, h, w, scale, strategy, max_points, points, n_points,
                     n_blobs, status, reinterpret_cast<int4*>(ws));
  HIP_OK(hipGetLastError());
}
}  // namespace

extern "C" {

MTGV_API size_t mtgv_mask_contours_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t max_points) {
  (void)h, (void)w, (void)max_points;  // the blob table only; the rest of a mask's state is in LDS
  return n >= 1 ? ct_workspace_bytes(n) : 0;
}

MTGV_API int mtgv_mask_contours(const uint8_t* masks_dev, int32_t n, int32_t h, int32_t w, int32_t strategy, int32_t max_points,
                                int32_t* points_dev, int32_t* n_points_dev, int32_t* n_blobs_dev, int32_t* status_dev, void* workspace_dev,
                                size_t workspace_bytes, void* stream) {
  return guarded([&] {
    launch_contours<false>(masks_dev, n, h, w, 1, strategy, max_points, (int*)points_dev, (int*)n_points_dev, (int*)n_blobs_dev,
                           (int*)status_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
  });
}

MTGV_API int mtgv_mask_contours_logits(const float* logits_dev, int32_t n, int32_t mh, int32_t mw, int32_t scale, int32_t strategy,
                                       int32_t max_points, int32_t* points_dev, int32_t* n_points_dev, int32_t* n_blobs_dev,
                                       int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return guarded([&] {
    MTGV_CHECK(scale >= 1, ERR_INVALID, "mask_contours: scale=%d", scale);
    MTGV_CHECK(mh >= 1 && mw >= 1 && mh <= 32767 / scale && mw <= 32767 / scale, ERR_INVALID, "mask_contours: mh=%d mw=%d scale=%d", mh, mw,
               scale);
    launch_contours<true>(logits_dev, n, mh * scale, mw * scale, scale, strategy, max_points, (int*)points_dev, (int*)n_points_dev,
                          (int*)n_blobs_dev, (int*)status_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
  });
}
}
