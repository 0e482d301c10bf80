// Device-resident card tracker (track.h).  update: one wave64 workgroup per frame = stream, lane t owns track slot t with its
// filter state in registers, the frame's detections in LDS, the greedy association as at most K rounds of a wave-wide
// lexicographic minimum over (distance, birth, detection index).  A second, single-workgroup launch compacts the due slots in
// ascending order; on a handle with an embed budget that launch is track_select_kernel, which takes at most `budget` of them,
// the longest-waiting first.  The wide form (MTGV_TRACKER_WIDE: up to 256 slots, 64 detections) is a second update kernel with up to
// four waves per workgroup; the one-wave kernel is what a handle of mtgv_tracker_create launches.  What a track does on its
// own (Slot and the slot_* pieces) is written once for both.  Everything the host tracker computes in fp64 is computed here
// in fp64 with the same operations in the same order: this translation unit must not contract a * b + c into an FMA.
#include "track.h"

#include <math.h>
#include <limits.h>
#include <algorithm>
#include <set>

#pragma clang fp contract(off)

namespace mtgv {

namespace {

constexpr int FRAMES_PER_LAUNCH = 32;  // stream and clock of each frame travel as kernel arguments: no copy, no staging buffer
struct FrameArgs {
  int32_t stream[FRAMES_PER_LAUNCH];
  double now[FRAMES_PER_LAUNCH];
};

struct Params {
  int T, K, top_k, hmax, delay, period;
  double thr, wait;
};

struct State {
  double* kal;
  int32_t* ints;
  double* last_t;
  int64_t* m_ids;
  float* m_scores;
  int32_t* ctrs;
};

// _KalmanTrack's constants (mtgv/tracker.py): norfair's OptimizedKalmanFilter defaults
constexpr double KAL_R = 4.0, KAL_Q = 0.1, KAL_POS_VAR = 10.0, KAL_VEL_VAR = 1.0;

// ---- what both update kernels share: the frame's detection list and everything a track does on its own.  No piece holds a
// barrier or reads another thread's registers; what crosses a wave stays in the kernels.

// a frame in LDS: its detections (the valid slots in ascending k, as fp64) and what the step reports per slot k
template <int KM>
struct Dets {
  alignas(16) double det[KM][8];  // (16: a corner pair per LDS access, as a __shared__ array of its own has)
  int det_k[KM];
  int o_id[KM], o_slot[KM], o_due[KM];
};

// called by one whole wave (K <= 64: the list fits its ballot) -> the number of detections; the caller's barrier publishes it
template <int KM>
__device__ __forceinline__ int stage_detections(Dets<KM>& D, int lane, int f, int K, const float* __restrict__ quads,
                                                const int32_t* __restrict__ n_det, const int32_t* __restrict__ state) {
  bool valid = lane < K;
  if (valid && n_det != nullptr) valid = lane < min(n_det[f], K);
  if (valid && state != nullptr) valid = state[(size_t)f * K + lane] > 0;
  const unsigned long long vm = __ballot(valid);
  if (lane < KM) D.o_id[lane] = 0, D.o_slot[lane] = -1, D.o_due[lane] = 0;
  if (valid) {
    const int di = __popcll(vm & ((1ull << lane) - 1ull));
    D.det_k[di] = lane;
    const float* q = quads + ((size_t)f * K + lane) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) D.det[di][j] = (double)q[j];
  }
  return __popcll(vm);
}

template <int KM>
__device__ __forceinline__ void write_report(const Dets<KM>& D, int f, int K, int t, int32_t* __restrict__ track_id, int32_t* __restrict__ slot_of,
                                             int32_t* __restrict__ due_flag) {
  if (t < K) {
    const size_t o = (size_t)f * K + t;
    track_id[o] = D.o_id[t], slot_of[o] = D.o_slot[t], due_flag[o] = D.o_due[t];
  }
}

// mean corner distance of detection q to a track's predicted corners: the host's np.linalg.norm(..., axis=1).mean()
__device__ __forceinline__ double track_distance(const double* q, const double (&pos)[8]) {
  double sum = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double dx = q[2 * c] - pos[2 * c], dy = q[2 * c + 1] - pos[2 * c + 1];
    const double r = __dsqrt_rn(dx * dx + dy * dy);
    sum = c == 0 ? r : sum + r;
  }
  return sum / 4.0;
}

// track slot t of stream s in its thread's registers
struct Slot {
  int live = 0, hit = 0, init = 0, id = 0, birth = 0, has_z = 0;
  int mdi = -1;        // detection the track took in this frame
  bool fresh = false;  // created in this frame
  double last_t = 0.0;
  double pos[8] = {}, vel[8] = {}, pp[8] = {}, pv[8] = {}, vv[8] = {};
};

__device__ __forceinline__ Slot slot_load(const State& st, int s, int T, int t, bool own) {
  const int32_t* I = st.ints + (size_t)s * TRACK_INTS * T;
  const double* Kal = st.kal + (size_t)s * TRACK_KAL * T;
  Slot a;
  if (own) {
    a.live = I[0 * T + t], a.hit = I[1 * T + t], a.init = I[2 * T + t], a.id = I[3 * T + t], a.birth = I[4 * T + t];
    a.has_z = I[5 * T + t];
    a.last_t = st.last_t[(size_t)s * T + t];
  }
  if (a.live) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a.pos[j] = Kal[(0 + j) * T + t], a.vel[j] = Kal[(8 + j) * T + t], a.pp[j] = Kal[(16 + j) * T + t];
      a.pv[j] = Kal[(24 + j) * T + t], a.vv[j] = Kal[(32 + j) * T + t];
    }
  }
  return a;
}

// the slot back to memory; a track created in this frame starts without kept matches
__device__ __forceinline__ void slot_store(const State& st, const Slot& a, int s, int T, int t, bool own, int top_k) {
  if (!own) return;
  int32_t* I = st.ints + (size_t)s * TRACK_INTS * T;
  double* Kal = st.kal + (size_t)s * TRACK_KAL * T;
  I[0 * T + t] = a.live, I[1 * T + t] = a.hit, I[2 * T + t] = a.init, I[3 * T + t] = a.id, I[4 * T + t] = a.birth;
  I[5 * T + t] = a.has_z;
  st.last_t[(size_t)s * T + t] = a.last_t;
  if (a.live) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      Kal[(0 + j) * T + t] = a.pos[j], Kal[(8 + j) * T + t] = a.vel[j], Kal[(16 + j) * T + t] = a.pp[j];
      Kal[(24 + j) * T + t] = a.pv[j], Kal[(32 + j) * T + t] = a.vv[j];
    }
  }
  if (a.fresh) {
    for (int k = 0; k < top_k; ++k) {
      st.m_ids[((size_t)s * T + t) * top_k + k] = -1;
      st.m_scores[((size_t)s * T + t) * top_k + k] = -INFINITY;
    }
  }
}

// 1. drop, 2. age and predict
__device__ __forceinline__ void slot_age(Slot& a) {
  if (a.live && a.hit < 0) a.live = 0, a.id = 0;
  if (a.live) {
    a.hit -= 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) a.pos[j] = a.pos[j] + a.vel[j];
  }
}

// whether a match in this frame takes the track out of initialisation, which costs the stream an id
__device__ __forceinline__ int slot_gets_id(const Slot& a, const Params& p) { return (a.init && min(a.hit + 2 * p.period, p.hmax) > p.delay) ? 1 : 0; }

// the track takes detection di = z: hit counter, the id on leaving initialisation, _KalmanTrack.kalman_update -> slot_gets_id
__device__ __forceinline__ int slot_take(Slot& a, const Params& p, const double* z, int di, int next_id) {
  const int gets_id = slot_gets_id(a, p);
  a.mdi = di;
  a.hit = min(a.hit + 2 * p.period, p.hmax);
  if (gets_id) a.init = 0, a.id = next_id, a.has_z = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const double e = z[j] - a.pos[j];
    const double sv = a.pp[j] + 2.0 * a.pv[j] + a.vv[j] + KAL_Q + KAL_R;
    const double k0 = 1.0 - KAL_R / sv, k1 = (a.pv[j] + a.vv[j]) / sv;
    a.pos[j] = a.pos[j] + k0 * e;
    a.vel[j] = a.vel[j] + k1 * e;
    const double nvv = a.vv[j] + KAL_Q - k1 * k1 * sv;
    a.pp[j] = k0 * KAL_R, a.pv[j] = k1 * KAL_R, a.vv[j] = nvv;
  }
  return gets_id;
}

// a track that is born initialised takes its id at creation
__device__ __forceinline__ bool spawn_initialising(const Params& p) { return p.period <= p.delay; }

// a new track in this (free) slot from the unmatched detection di = z
__device__ __forceinline__ void slot_spawn(Slot& a, const Params& p, const double* z, int di, int next_id, int next_birth) {
  const bool new_init = spawn_initialising(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) a.pos[j] = z[j], a.vel[j] = 0.0, a.pp[j] = KAL_POS_VAR, a.pv[j] = 0.0, a.vv[j] = KAL_VEL_VAR;
  a.live = 1, a.hit = p.period, a.init = new_init ? 1 : 0, a.id = new_init ? 0 : next_id, a.birth = next_birth;
  a.has_z = 0, a.last_t = 0.0, a.mdi = di, a.fresh = true;
}

// 5. report and gate
// On a budget handle (BUDGET; defer: its (frames * K, 2) candidate records) a due track is a candidate only: its key, the time
// it has waited (+inf without an embedding), and the frame's clock go into the record of its flat slot f K + k, and
// track_select_kernel stamps the tracks it takes.  On any other handle the update stamps a due track itself.
template <bool BUDGET, int KM>
__device__ __forceinline__ void slot_report(Slot& a, const Params& p, double now, Dets<KM>& D, int f, int s, int T, int t, double* defer) {
  const bool rep = a.live && a.id > 0 && a.mdi >= 0 && a.hit >= 0;
  const bool due = rep && (!a.has_z || now - a.last_t > p.wait);
  if constexpr (BUDGET) {
    if (due) {
      double* rec = defer + 2 * ((size_t)f * p.K + D.det_k[a.mdi]);
      rec[0] = a.has_z ? now - a.last_t : INFINITY, rec[1] = now;
    }
  } else {
    if (due) a.last_t = now;
  }
  if (rep) {
    const int k = D.det_k[a.mdi];
    D.o_id[k] = a.id, D.o_slot[k] = s * T + t, D.o_due[k] = due ? 1 : 0;
  }
}

// Defer: nothing, or the one double* of a budget handle (its candidate records), whose kernel differs in slot_report alone.
// A trailing parameter pack, so that the kernel of every other handle keeps the argument list it had (the one-wave kernel
// then compiles to the same instruction stream as without the pack).
__device__ __forceinline__ double* defer_of() { return nullptr; }
__device__ __forceinline__ double* defer_of(double* d) { return d; }

template <class... Defer>
__global__ __launch_bounds__(64) void track_update_kernel(State st, Params p, FrameArgs fr, int f0, const float* __restrict__ quads,
                                                          const int32_t* __restrict__ n_det, const int32_t* __restrict__ state,
                                                          int32_t* __restrict__ track_id, int32_t* __restrict__ slot_of,
                                                          int32_t* __restrict__ due_flag, Defer... defer) {
  __shared__ Dets<TRACK_MAX_CARDS> D;
  const int lane = threadIdx.x;
  const int f = f0 + blockIdx.x, s = fr.stream[blockIdx.x];
  const double now = fr.now[blockIdx.x];
  const int T = p.T;

  const int nd = stage_detections(D, lane, f, p.K, quads, n_det, state);
  __syncthreads();

  const bool own = lane < T;
  Slot a = slot_load(st, s, T, lane, own);
  int32_t* C = st.ctrs + (size_t)s * TRACK_CTRS;
  int next_id = C[0], next_birth = C[1], overflow = C[2];
  slot_age(a);

  // 3. greedy association, closest pair first: the initialised tracks, then the initialising ones on what is left
  unsigned free_d = nd > 0 ? (0xffffffffu >> (32 - nd)) : 0u;
  for (int phase = 0; phase < 2; ++phase) {
    const bool cand = a.live && a.init == phase;
    double d[TRACK_MAX_CARDS];
#pragma unroll
    for (int di = 0; di < TRACK_MAX_CARDS; ++di) {
      d[di] = INFINITY;
      if (di < nd && cand && ((free_d >> di) & 1u)) {
        const double dist = track_distance(D.det[di], a.pos);
        if (dist < p.thr) d[di] = dist;  // a NaN never matches
      }
    }
    bool used = false;
    for (int round = 0; round < nd; ++round) {
      double best = INFINITY;
      int bdi = -1;
      if (cand && !used) {
#pragma unroll
        for (int di = 0; di < TRACK_MAX_CARDS; ++di)
          if (((free_d >> di) & 1u) && d[di] < best) best = d[di], bdi = di;  // strict: the lowest index wins a tie
      }
      double m = best;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off));
      if (!(m < INFINITY)) break;  // wave-uniform
      int b = best == m ? a.birth : INT_MAX;  // ties between tracks: creation order, as the host's list order
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) b = min(b, __shfl_xor(b, off));
      const bool win = best == m && a.birth == b;
      const int wl = __ffsll((unsigned long long)__ballot(win)) - 1;
      const int wdi = __shfl(bdi, wl);
      free_d &= ~(1u << wdi);
      int gets_id = 0;
      if (lane == wl) {
        used = true;
        gets_id = slot_take(a, p, D.det[wdi], wdi, next_id);
      }
      next_id += __shfl(gets_id, wl);
    }
  }

  // 4. unmatched detections, ascending, take the lowest free slot
  unsigned long long freem = __ballot(own && !a.live);
  for (int di = 0; di < nd; ++di) {
    if (!((free_d >> di) & 1u)) continue;
    if (freem == 0ull) {
      overflow += 1;
      continue;
    }
    const int sl = __ffsll(freem) - 1;
    freem &= freem - 1ull;
    if (lane == sl) slot_spawn(a, p, D.det[di], di, next_id, next_birth);
    if (!spawn_initialising(p)) next_id += 1;
    next_birth += 1;
  }

  slot_report<sizeof...(Defer) != 0>(a, p, now, D, f, s, T, lane, defer_of(defer...));
  slot_store(st, a, s, T, lane, own, p.top_k);
  if (lane == 0) C[0] = next_id, C[1] = next_birth, C[2] = overflow;
  __syncthreads();
  write_report(D, f, p.K, lane, track_id, slot_of, due_flag);
}

// The wide form (MTGV_TRACKER_WIDE): one workgroup of W = ceil(T / 64) waves per frame, thread t owns slot t, up to 64
// detections in LDS.  A track's own arithmetic is the one-wave kernel's, the same slot_* pieces; only what crosses a wave
// differs: the round's minimum is reduced per wave by shuffles and across waves through LDS, the free detections are a 64-bit
// mask, the free slots W ballots.  A lane keeps no distance row: it caches (best, index) over the free detections and rescans
// from LDS only when that detection was taken by another track (its minimum over the free set changes only then).
// Every __syncthreads() below is reached by every thread: the loop bounds (nd, two phases) and the early exit are values
// that all threads read from LDS after a barrier.
template <class... Defer>
__global__ __launch_bounds__(TRACK_WIDE_MAX_TRACKS) void track_update_wide_kernel(State st, Params p, FrameArgs fr, int f0,
                                                                                  const float* __restrict__ quads,
                                                                                  const int32_t* __restrict__ n_det,
                                                                                  const int32_t* __restrict__ state,
                                                                                  int32_t* __restrict__ track_id, int32_t* __restrict__ slot_of,
                                                                                  int32_t* __restrict__ due_flag, Defer... defer) {
  constexpr int WM = TRACK_WIDE_MAX_TRACKS / 64;
  __shared__ Dets<TRACK_WIDE_MAX_CARDS> D;
  __shared__ int s_nd;
  __shared__ double r_dist[WM];                                   // per wave: its minimum of the round ...
  __shared__ int r_birth[WM], r_thread[WM], r_di[WM], r_gets[WM];  // ... and whose it is
  __shared__ unsigned long long s_free[WM];                        // per wave: ballot of its free slots
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
  const int f = f0 + blockIdx.x, s = fr.stream[blockIdx.x];
  const double now = fr.now[blockIdx.x];
  const int T = p.T;

  if (wave == 0) {  // (K <= 64: the whole list in wave 0)
    const int n = stage_detections(D, lane, f, p.K, quads, n_det, state);
    if (lane == 0) s_nd = n;
  }
  __syncthreads();
  const int nd = s_nd;  // workgroup-uniform, 0..64

  const bool own = tid < T;
  Slot a = slot_load(st, s, T, tid, own);
  int32_t* C = st.ctrs + (size_t)s * TRACK_CTRS;
  int next_id = C[0], next_birth = C[1], overflow = C[2];  // (written by thread 0 behind the last barrier)
  slot_age(a);

  // 3. greedy association, closest pair first: the initialised tracks, then the initialising ones on what is left
  unsigned long long free_d = nd >= 64 ? ~0ull : ((1ull << nd) - 1ull);  // workgroup-uniform: changed only by values read from LDS
  for (int phase = 0; phase < 2; ++phase) {
    const bool cand = a.live && a.init == phase;
    bool used = false, rescan = true;
    double best = INFINITY;
    int bdi = -1;
    for (int round = 0; round < nd; ++round) {
      if (cand && !used && rescan) {  // (divergent, no barrier inside)
        best = INFINITY, bdi = -1;
        for (int di = 0; di < nd; ++di) {
          if (!((free_d >> di) & 1ull)) continue;
          const double dist = track_distance(D.det[di], a.pos);
          if (dist < p.thr && dist < best) best = dist, bdi = di;  // a NaN never matches; strict: the lowest index wins a tie
        }
        rescan = false;
      }
      const double mine = cand && !used ? best : INFINITY;
      double m = mine;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off));
      int b = mine == m ? a.birth : INT_MAX;  // ties between tracks: creation order, as the host's list order
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) b = min(b, __shfl_xor(b, off));
      const bool win = mine == m && a.birth == b;
      const int wl = max(__ffsll((unsigned long long)__ballot(win)) - 1, 0);
      if (lane == wl) {  // one lane per wave (the entry is not used when m is not finite)
        r_dist[wave] = m, r_birth[wave] = b, r_thread[wave] = tid, r_di[wave] = bdi;
        r_gets[wave] = slot_gets_id(a, p);
      }
      __syncthreads();
      double gm = INFINITY;
      int gb = INT_MAX, gt = -1, gdi = -1, gets_id = 0;
      for (int w = 0; w < W; ++w) {
        const double wm = r_dist[w];
        const int wb = r_birth[w];
        if (wm < gm || (wm == gm && wm < INFINITY && wb < gb)) gm = wm, gb = wb, gt = r_thread[w], gdi = r_di[w], gets_id = r_gets[w];
      }
      __syncthreads();  // all have read the entries before the next round (or phase) rewrites them
      if (!(gm < INFINITY)) break;  // workgroup-uniform: gm was read from LDS behind a barrier by every thread
      free_d &= ~(1ull << gdi);
      if (tid == gt) {
        used = true;
        slot_take(a, p, D.det[gdi], gdi, next_id);  // (-> gets_id, which every thread has from LDS)
      } else if (bdi == gdi) {
        rescan = true;  // the cached minimum was taken
      }
      next_id += gets_id;
    }
  }

  // 4. unmatched detections, ascending, take the lowest free slot of the whole workgroup
  {
    const unsigned long long fb = __ballot(own && !a.live);
    if (lane == 0) s_free[wave] = fb;
  }
  __syncthreads();
  unsigned long long freem[WM];
#pragma unroll
  for (int w = 0; w < WM; ++w) freem[w] = w < W ? s_free[w] : 0ull;
  for (int di = 0; di < nd; ++di) {  // workgroup-uniform: nd, free_d and freem are the same in every thread
    if (!((free_d >> di) & 1ull)) continue;
    int sl = -1;
#pragma unroll
    for (int w = 0; w < WM; ++w)
      if (sl < 0 && freem[w] != 0ull) sl = w * 64 + __ffsll(freem[w]) - 1, freem[w] &= freem[w] - 1ull;
    if (sl < 0) {
      overflow += 1;
      continue;
    }
    if (tid == sl) slot_spawn(a, p, D.det[di], di, next_id, next_birth);
    if (!spawn_initialising(p)) next_id += 1;
    next_birth += 1;
  }

  slot_report<sizeof...(Defer) != 0>(a, p, now, D, f, s, T, tid, defer_of(defer...));
  slot_store(st, a, s, T, tid, own, p.top_k);
  if (tid == 0) C[0] = next_id, C[1] = next_birth, C[2] = overflow;
  __syncthreads();
  write_report(D, f, p.K, tid, track_id, slot_of, due_flag);
}

// ordered compaction of the due slots: one wave walks the n = F * K flags in ascending order (no atomics, so the order of
// due_idx does not depend on which workgroup finished first); entries behind n_due are -1
__global__ __launch_bounds__(64) void track_compact_kernel(const int32_t* __restrict__ due_flag, int n, int32_t* __restrict__ due_idx,
                                                           int32_t* __restrict__ rank_of, int32_t* __restrict__ n_due) {
  const int lane = threadIdx.x;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool flag = i < n && due_flag[i] != 0;
    const unsigned long long m = __ballot(flag);
    if (i < n) {
      const int r = flag ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
      rank_of[i] = r;
      if (flag) due_idx[r] = i;
    }
    base += __popcll(m);
  }
  for (int i = base + lane; i < n; i += 64) due_idx[i] = -1;
  if (lane == 0) *n_due = base;
}

// ---- the embed budget: track_select_kernel in the place of track_compact_kernel (mtgv/tracker.py: select_due is the rule).
// Of the step's candidates (due_flag, or a key that is no NaN) it takes the min(budget, candidates) with the largest key, ties
// to the smaller flat index, and writes them as the compaction does: due_idx ascending with -1 behind, rank_of, n_due, and
// n_deferred = candidates - n_due.  One workgroup of 256 threads; thread t owns the `per` consecutive slots from t * per.
// The keys are staged once in LDS as order-preserving 64-bit integers (0: no candidate; no candidate's key maps to 0).
// When the budget binds, the budget-th largest key is found exactly by a radix select from the top byte down, eight passes
// of an LDS histogram of one byte over the keys that share the bytes found so far.  The histogram's atomics only count;
// the position of an output row comes from two ordered prefix counts over the threads (ties, then everything selected).
// Every loop bound (`per`, eight passes, four waves) is fixed before its loop, and every barrier is reached by every thread:
// the one branch around barriers, `binds`, is a value that all threads read from LDS behind a barrier.
constexpr int SELECT_THREADS = 256;
constexpr int SELECT_MAX_SLOTS = 8192;  // 64 KiB of staged keys (MI355X: 160 KiB of LDS per CU, one workgroup may ask for all)
constexpr int SELECT_WAVES = SELECT_THREADS / 64;

struct SelectShared {
  int hist[256];
  int wave_sum[SELECT_WAVES];
  int digit, rest;
};

__device__ __forceinline__ unsigned long long select_key(double waited) {  // a < b <=> key(a) < key(b); -0.0 counts as +0.0
  const unsigned long long u = (unsigned long long)__double_as_longlong(waited + 0.0);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// exclusive prefix sum of v over the workgroup's threads in thread order -> (prefix, total); two barriers, called by all
__device__ __forceinline__ int select_scan(int v, int* wave_sum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  __syncthreads();  // the last call's readers are done with wave_sum
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < SELECT_WAVES; ++w) {
    const int ws = wave_sum[w];
    before += w < wave ? ws : 0, all += ws;
  }
  total = all;
  return before + inc - v;
}

// waited: the key of slot i at waited[i * stride] (a budget handle's records: stride 2, the frame's clock behind the key).
// due_flag nullptr: a NaN key marks a slot that is no candidate.  last_t given: the taken tracks (slot_of) are stamped.
__global__ __launch_bounds__(SELECT_THREADS) void track_select_kernel(const double* __restrict__ waited, int stride,
                                                                      const int32_t* __restrict__ due_flag, int n, int budget,
                                                                      const int32_t* __restrict__ slot_of, double* __restrict__ last_t,
                                                                      int32_t* __restrict__ due_idx, int32_t* __restrict__ rank_of,
                                                                      int32_t* __restrict__ n_due, int32_t* __restrict__ n_deferred) {
  extern __shared__ unsigned long long s_key[];  // n keys, then SelectShared
  SelectShared& sh = *reinterpret_cast<SelectShared*>(s_key + n);
  const int tid = threadIdx.x;
  const int per = (n + SELECT_THREADS - 1) / SELECT_THREADS;
  const int lo = min(tid * per, n), hi = min(lo + per, n);

  int mine = 0;
  for (int i = lo; i < hi; ++i) {
    bool cand = due_flag != nullptr ? due_flag[i] != 0 : true;
    unsigned long long key = 0ull;
    if (cand) {
      const double w = waited[(size_t)i * stride];
      cand = w == w;
      if (cand) key = select_key(w);
    }
    s_key[i] = key;
    mine += cand ? 1 : 0;
  }
  int cands;
  (void)select_scan(mine, sh.wave_sum, cands);  // (its barriers publish s_key too)
  const bool binds = cands > budget;            // workgroup-uniform: a sum read from LDS behind a barrier

  // the threshold: the budget-th largest key, and how many of the keys equal to it are taken
  unsigned long long thr = 0ull;  // not binding: every candidate's key is above 0
  int take_eq = 0;
  if (binds) {
    int rest = budget;  // the rank of the wanted key among those that share the prefix
    for (int pass = 7; pass >= 0; --pass) {
      const unsigned long long above = pass == 7 ? 0ull : (~0ull << (8 * pass + 8));
      sh.hist[tid] = 0;
      __syncthreads();
      for (int i = lo; i < hi; ++i) {
        const unsigned long long key = s_key[i];
        if (key != 0ull && (key & above) == thr) atomicAdd(&sh.hist[(int)((key >> (8 * pass)) & 0xffull)], 1);
      }
      __syncthreads();
      // thread d: how many keys of the prefix have a byte above d; byte d holds the wanted key iff gt < rest <= gt + h
      const int h = sh.hist[tid];
      int total;
      const int lt = select_scan(h, sh.wave_sum, total);
      const int gt = total - lt - h;
      if (gt < rest && rest <= gt + h) sh.digit = tid, sh.rest = rest - gt;  // exactly one thread: rest is in 1..total
      __syncthreads();
      thr |= (unsigned long long)sh.digit << (8 * pass);
      rest = sh.rest;
      // (the next pass's barrier behind the clearing of hist orders these reads before the next writes of digit / rest)
    }
    take_eq = rest;
  }

  // ties in ascending flat index: an ordered prefix count of the keys equal to the threshold
  int eq = 0;
  for (int i = lo; i < hi; ++i) eq += (binds && s_key[i] == thr) ? 1 : 0;
  int eq_total;
  int eq_rank = select_scan(eq, sh.wave_sum, eq_total);
  int sel = 0;
  for (int i = lo; i < hi; ++i) {
    const unsigned long long key = s_key[i];
    bool take = key > thr;
    if (binds && key == thr) take = eq_rank < take_eq, eq_rank += 1;
    sel += take ? 1 : 0;
  }
  int n_sel;
  int r = select_scan(sel, sh.wave_sum, n_sel);
  eq_rank -= eq;  // back to the thread's first
  for (int i = lo; i < hi; ++i) {
    const unsigned long long key = s_key[i];
    bool take = key > thr;
    if (binds && key == thr) take = eq_rank < take_eq, eq_rank += 1;
    rank_of[i] = take ? r : -1;
    if (take) {
      due_idx[r] = i;
      if (last_t != nullptr && slot_of[i] >= 0) last_t[slot_of[i]] = waited[(size_t)i * stride + 1];
      r += 1;
    }
  }
  for (int i = n_sel + tid; i < n; i += SELECT_THREADS) due_idx[i] = -1;
  if (tid == 0) *n_due = n_sel, *n_deferred = cands - n_sel;
}

void select_launch(const double* waited, int stride, const int32_t* due_flag, int n, int budget, const int32_t* slot_of, double* last_t,
                   int32_t* due_idx, int32_t* rank_of, int32_t* n_due, int32_t* n_deferred, hipStream_t s) {
  const size_t lds = (size_t)n * sizeof(unsigned long long) + sizeof(SelectShared);
  lds_opt_in<track_select_kernel>(lds, (int)(SELECT_MAX_SLOTS * sizeof(unsigned long long) + sizeof(SelectShared)));
  hipLaunchKernelGGL(track_select_kernel, dim3(1), dim3(SELECT_THREADS), lds, s, waited, stride, due_flag, n, budget, slot_of, last_t, due_idx,
                     rank_of, n_due, n_deferred);
  HIP_OK(hipGetLastError());
}

// row r < n_due: avg = w z + (1 - w) avg in f32 (avg = z the first time, then the same formula), q[r] = avg;
// pad (a budget handle): q rows behind n_due are zeroed, so that the match never reads what nobody wrote
__global__ __launch_bounds__(128) void track_commit_kernel(const float* __restrict__ z, float* __restrict__ q, const int32_t* __restrict__ due_idx,
                                                           const int32_t* __restrict__ n_due, const int32_t* __restrict__ slot_of,
                                                           int32_t* __restrict__ ints, float* __restrict__ avg_z, int T, int dim, float w,
                                                           float omw, int pad) {
  const int r = blockIdx.x;  // (the grid is min(rows of z, F * K) blocks; with pad every row of z)
  if (r >= *n_due) {  // (the whole block)
    if (pad)
      for (int c = threadIdx.x; c < dim; c += 128) q[(size_t)r * dim + c] = 0.f;
    return;
  }
  const int slot = slot_of[due_idx[r]];
  if (slot < 0) return;  // (cannot happen: a due slot has a track)
  int32_t* has = ints + (size_t)(slot / T) * TRACK_INTS * T + 5 * T + slot % T;
  const bool had = *has != 0;
  __syncthreads();
  float* a = avg_z + (size_t)slot * dim;
  for (int c = threadIdx.x; c < dim; c += 128) {
    const float zc = z[(size_t)r * dim + c];
    const float prev = had ? a[c] : zc;
    const float v = w * zc + omw * prev;
    a[c] = v;
    q[(size_t)r * dim + c] = v;
  }
  if (threadIdx.x == 0) *has = 1;
}

// slot i of the step: a due track takes (and keeps) row rank_of[i] of the new matches, a track that was not due emits what
// it kept, a slot without a track -1 / -inf.  A track owns at most one slot of a step, so no two threads touch one track.
__global__ __launch_bounds__(256) void track_store_kernel(const int64_t* __restrict__ ids, const float* __restrict__ scores,
                                                          const int32_t* __restrict__ slot_of, const int32_t* __restrict__ rank_of,
                                                          int64_t* __restrict__ m_ids, float* __restrict__ m_scores, int64_t* __restrict__ out_ids,
                                                          float* __restrict__ out_scores, int n, int top_k, int rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int slot = slot_of[i];
  const int r = rank_of[i] < rows ? rank_of[i] : -1;  // never past the caller's rows
  for (int t = 0; t < top_k; ++t) {
    int64_t id = -1;
    float sc = -INFINITY;
    if (slot >= 0) {
      if (r >= 0) {
        id = ids[(size_t)r * top_k + t], sc = scores[(size_t)r * top_k + t];
        m_ids[(size_t)slot * top_k + t] = id, m_scores[(size_t)slot * top_k + t] = sc;
      } else {
        id = m_ids[(size_t)slot * top_k + t], sc = m_scores[(size_t)slot * top_k + t];
      }
    }
    out_ids[(size_t)i * top_k + t] = id, out_scores[(size_t)i * top_k + t] = sc;
  }
}

__global__ __launch_bounds__(256) void track_reset_kernel(State st, float* __restrict__ avg_z, int s0, int T, int dim, int top_k) {
  const int s = s0 + blockIdx.x;
  for (int i = threadIdx.x; i < TRACK_KAL * T; i += 256) st.kal[(size_t)s * TRACK_KAL * T + i] = 0.0;
  for (int i = threadIdx.x; i < TRACK_INTS * T; i += 256) st.ints[(size_t)s * TRACK_INTS * T + i] = 0;
  for (int i = threadIdx.x; i < T; i += 256) st.last_t[(size_t)s * T + i] = 0.0;
  for (int i = threadIdx.x; i < T * dim; i += 256) avg_z[(size_t)s * T * dim + i] = 0.f;
  for (int i = threadIdx.x; i < T * top_k; i += 256) st.m_ids[(size_t)s * T * top_k + i] = -1, st.m_scores[(size_t)s * T * top_k + i] = -INFINITY;
  if (threadIdx.x == 0) {
    int32_t* C = st.ctrs + (size_t)s * TRACK_CTRS;
    C[0] = 1, C[1] = 0, C[2] = 0, C[3] = 0;
  }
}

// dst row r = src row due_idx[r], r < min(n_due, max_rows); 16 bytes per thread where the rows allow it; pad: the rows
// behind n_due are zeroed
__global__ __launch_bounds__(256) void track_gather_u8_kernel(const uint8_t* __restrict__ src, long src_rows, long row_bytes,
                                                              const int32_t* __restrict__ due_idx, const int32_t* __restrict__ n_due,
                                                              uint8_t* __restrict__ dst, int vec, int pad) {
  const int r = blockIdx.x;
  uint8_t* b = dst + (long)r * row_bytes;
  if (r >= *n_due) {
    if (pad && vec) {
      uint4* b4 = (uint4*)b;
      for (long c = (long)blockIdx.y * 256 + threadIdx.x; c < row_bytes / 16; c += (long)gridDim.y * 256) b4[c] = make_uint4(0u, 0u, 0u, 0u);
    } else if (pad) {
      for (long c = (long)blockIdx.y * 256 + threadIdx.x; c < row_bytes; c += (long)gridDim.y * 256) b[c] = 0;
    }
    return;
  }
  const long i = due_idx[r];
  if (i < 0 || i >= src_rows) return;
  const uint8_t* a = src + i * row_bytes;
  if (vec) {
    const uint4* a4 = (const uint4*)a;
    uint4* b4 = (uint4*)b;
    for (long c = (long)blockIdx.y * 256 + threadIdx.x; c < row_bytes / 16; c += (long)gridDim.y * 256) b4[c] = a4[c];
  } else {
    for (long c = (long)blockIdx.y * 256 + threadIdx.x; c < row_bytes; c += (long)gridDim.y * 256) b[c] = a[c];
  }
}

template <class P>
void dev_alloc(P*& p, size_t count) {
  HIP_OK(hipMalloc((void**)&p, count * sizeof(P)));
}

}  // namespace

mtgv_tracker_cfg tracker_resolve_cfg(const mtgv_tracker_cfg& in, int32_t flags) {
  mtgv_tracker_cfg c = in;
  MTGV_CHECK((flags & ~MTGV_TRACKER_WIDE) == 0, ERR_INVALID, "tracker: unknown flags 0x%x", (unsigned)flags);
  const int max_t = (flags & MTGV_TRACKER_WIDE) ? TRACK_WIDE_MAX_TRACKS : TRACK_MAX_TRACKS;
  const int max_k = (flags & MTGV_TRACKER_WIDE) ? TRACK_WIDE_MAX_CARDS : TRACK_MAX_CARDS;
  MTGV_CHECK(c.streams >= 1 && c.streams <= 4096, ERR_INVALID, "tracker: streams %d outside 1..4096", c.streams);
  MTGV_CHECK(c.max_tracks >= 1 && c.max_tracks <= max_t, ERR_INVALID, "tracker: max_tracks %d outside 1..%d", c.max_tracks, max_t);
  MTGV_CHECK(c.cards_per_frame >= 1 && c.cards_per_frame <= max_k, ERR_INVALID, "tracker: cards_per_frame %d outside 1..%d", c.cards_per_frame,
             max_k);
  MTGV_CHECK(c.dim >= 1 && c.dim <= 65536, ERR_INVALID, "tracker: dim %d outside 1..65536", c.dim);
  MTGV_CHECK(c.top_k >= 1 && c.top_k <= TRACK_MAX_TOPK, ERR_INVALID, "tracker: top_k %d outside 1..%d", c.top_k, TRACK_MAX_TOPK);
  // zero: the reference's value (mtgvision/server.py:100-106, :41-43)
  if (c.distance_threshold == 0.0) c.distance_threshold = 300.0;
  if (c.hit_counter_max == 0) c.hit_counter_max = 5;
  if (c.initialization_delay == 0) c.initialization_delay = 2;
  if (c.period == 0) c.period = 1;
  if (c.update_wait_sec == 0.0) c.update_wait_sec = 0.5;
  if (c.ewma_weight == 0.0) c.ewma_weight = 0.1;
  MTGV_CHECK(c.distance_threshold > 0.0 && c.distance_threshold < INFINITY, ERR_INVALID, "tracker: distance_threshold %g must be positive and finite",
             c.distance_threshold);
  MTGV_CHECK(c.hit_counter_max >= 1 && c.hit_counter_max <= (1 << 20), ERR_INVALID, "tracker: hit_counter_max %d outside 1..2^20", c.hit_counter_max);
  MTGV_CHECK(c.period >= 1 && c.period <= (1 << 20), ERR_INVALID, "tracker: period %d outside 1..2^20", c.period);
  MTGV_CHECK(c.initialization_delay >= -1 && c.initialization_delay <= (1 << 20), ERR_INVALID, "tracker: initialization_delay %d outside -1..2^20",
             c.initialization_delay);
  MTGV_CHECK(c.update_wait_sec == c.update_wait_sec, ERR_INVALID, "tracker: update_wait_sec is NaN");
  MTGV_CHECK(c.ewma_weight > 0.0 && c.ewma_weight <= 1.0, ERR_INVALID, "tracker: ewma_weight %g outside (0, 1]", c.ewma_weight);
  return c;
}

int tracker_check_budget(int embed_budget) {
  MTGV_CHECK(embed_budget >= 1 && embed_budget <= 65535, ERR_INVALID, "tracker: embed_budget %d outside 1..65535", embed_budget);
  return embed_budget;
}

Tracker::Tracker(const mtgv_tracker_cfg& c, int32_t flags, int embed_budget)
    : c_(tracker_resolve_cfg(c, flags)), wide_((flags & MTGV_TRACKER_WIDE) != 0), budget_(embed_budget == 0 ? 0 : tracker_check_budget(embed_budget)) {
  const size_t S = c_.streams, T = c_.max_tracks, K = c_.cards_per_frame;
  if (budget_ > 0) {  // the candidate records of a step: never more slots than the selection takes
    dev_alloc(defer_, 2 * std::min<size_t>(S * K, SELECT_MAX_SLOTS));
    dev_alloc(n_deferred_, 1);
  }
  dev_alloc(kal_, S * TRACK_KAL * T);
  dev_alloc(ints_, S * TRACK_INTS * T);
  dev_alloc(last_t_, S * T);
  dev_alloc(avg_z_, S * T * c_.dim);
  dev_alloc(m_ids_, S * T * c_.top_k);
  dev_alloc(m_scores_, S * T * c_.top_k);
  dev_alloc(ctrs_, S * TRACK_CTRS);
  dev_alloc(slot_of_, S * K);
  dev_alloc(due_flag_, S * K);
  dev_alloc(rank_of_, S * K);
  reset(-1, nullptr);
  HIP_OK(hipStreamSynchronize(nullptr));
}

Tracker::~Tracker() {
  for (void* p : {(void*)kal_, (void*)ints_, (void*)last_t_, (void*)avg_z_, (void*)m_ids_, (void*)m_scores_, (void*)ctrs_, (void*)slot_of_,
                  (void*)due_flag_, (void*)rank_of_, (void*)defer_, (void*)n_deferred_})
    if (p != nullptr) (void)hipFree(p);
}

void Tracker::reset(int stream_or_all, hipStream_t s) {
  MTGV_CHECK(stream_or_all >= -1 && stream_or_all < c_.streams, ERR_INVALID, "tracker: stream %d outside [-1, %d)", stream_or_all, c_.streams);
  const State st{kal_, ints_, last_t_, m_ids_, m_scores_, ctrs_};
  const int s0 = stream_or_all < 0 ? 0 : stream_or_all, n = stream_or_all < 0 ? c_.streams : 1;
  hipLaunchKernelGGL(track_reset_kernel, dim3(n), dim3(256), 0, s, st, avg_z_, s0, c_.max_tracks, c_.dim, c_.top_k);
  HIP_OK(hipGetLastError());
  frames_ = 0;  // the step's slot table refers to the tracks that were
}

void Tracker::update(const float* quads, const int32_t* n_det, const int32_t* state, int frames, const int32_t* stream_of_frame, const double* now,
                     int32_t* track_id, int32_t* due_idx, int32_t* n_due, int32_t* n_deferred, hipStream_t s) {
  MTGV_CHECK(quads && stream_of_frame && now && track_id && due_idx && n_due, ERR_INVALID, "tracker: null argument");
  MTGV_CHECK(n_det != nullptr || state != nullptr, ERR_INVALID, "tracker: one of n_det and state must be given");
  MTGV_CHECK(frames >= 1 && frames <= c_.streams, ERR_INVALID, "tracker: %d frames for %d streams", frames, c_.streams);
  MTGV_CHECK(budget_ > 0 || n_deferred == nullptr, ERR_INVALID, "tracker: n_deferred on a handle without an embed budget");
  MTGV_CHECK(budget_ == 0 || (long)frames * c_.cards_per_frame <= SELECT_MAX_SLOTS, ERR_INVALID,
             "tracker: a step of %d x %d slots on a budget handle (at most %d)", frames, c_.cards_per_frame, SELECT_MAX_SLOTS);
  std::set<int32_t> seen;
  for (int f = 0; f < frames; ++f) {
    MTGV_CHECK(stream_of_frame[f] >= 0 && stream_of_frame[f] < c_.streams, ERR_INVALID, "tracker: frame %d names stream %d outside [0, %d)", f,
               stream_of_frame[f], c_.streams);
    MTGV_CHECK(seen.insert(stream_of_frame[f]).second, ERR_INVALID, "tracker: stream %d appears twice in one step", stream_of_frame[f]);
    MTGV_CHECK(now[f] == now[f], ERR_INVALID, "tracker: the clock of frame %d is NaN", f);
  }
  const State st{kal_, ints_, last_t_, m_ids_, m_scores_, ctrs_};
  const Params p{c_.max_tracks, c_.cards_per_frame, c_.top_k, c_.hit_counter_max, c_.initialization_delay, c_.period,
                 c_.distance_threshold, c_.update_wait_sec};
  for (int f0 = 0; f0 < frames; f0 += FRAMES_PER_LAUNCH) {
    const int n = std::min(FRAMES_PER_LAUNCH, frames - f0);
    FrameArgs fr = {};
    for (int i = 0; i < n; ++i) fr.stream[i] = stream_of_frame[f0 + i], fr.now[i] = now[f0 + i];
    const dim3 wide_block(64 * ceil_div(c_.max_tracks, 64));
    if (wide_ && budget_ > 0)
      hipLaunchKernelGGL(track_update_wide_kernel<double*>, dim3(n), wide_block, 0, s, st, p, fr, f0, quads, n_det, state, track_id, slot_of_, due_flag_,
                         defer_);
    else if (wide_)
      hipLaunchKernelGGL(track_update_wide_kernel<>, dim3(n), wide_block, 0, s, st, p, fr, f0, quads, n_det, state, track_id, slot_of_, due_flag_);
    else if (budget_ > 0)
      hipLaunchKernelGGL(track_update_kernel<double*>, dim3(n), dim3(64), 0, s, st, p, fr, f0, quads, n_det, state, track_id, slot_of_, due_flag_,
                         defer_);
    else
      hipLaunchKernelGGL(track_update_kernel<>, dim3(n), dim3(64), 0, s, st, p, fr, f0, quads, n_det, state, track_id, slot_of_, due_flag_);
  }
  if (budget_ > 0)
    select_launch(defer_, 2, due_flag_, frames * c_.cards_per_frame, budget_, slot_of_, last_t_, due_idx, rank_of_, n_due,
                  n_deferred != nullptr ? n_deferred : n_deferred_, s);
  else
    hipLaunchKernelGGL(track_compact_kernel, dim3(1), dim3(64), 0, s, due_flag_, frames * c_.cards_per_frame, due_idx, rank_of_, n_due);
  HIP_OK(hipGetLastError());
  frames_ = frames, due_idx_ = due_idx, n_due_ = n_due;
}

void Tracker::commit(const float* z, float* q, int rows, hipStream_t s) {
  MTGV_CHECK(z && q && rows >= 1, ERR_INVALID, "tracker: null argument or no rows");
  MTGV_CHECK(frames_ > 0, ERR_INVALID, "tracker: commit without an update");
  const double w = c_.ewma_weight;
  const int pad = budget_ > 0 ? 1 : 0;  // a budget handle's q is matched whole: every row is written, one block each
  MTGV_CHECK(!pad || rows <= 65535, ERR_INVALID, "tracker: commit of %d rows on a budget handle (at most 65535)", rows);
  hipLaunchKernelGGL(track_commit_kernel, dim3(pad ? rows : std::min(rows, frames_ * c_.cards_per_frame)), dim3(128), 0, s, z, q, due_idx_, n_due_,
                     slot_of_, ints_, avg_z_, c_.max_tracks, c_.dim, (float)w, (float)(1.0 - w), pad);
  HIP_OK(hipGetLastError());
}

void Tracker::store(const int64_t* ids, const float* scores, int rows, int64_t* out_ids, float* out_scores, hipStream_t s) {
  MTGV_CHECK(out_ids && out_scores && rows >= 0 && (rows == 0 || (ids && scores)), ERR_INVALID, "tracker: null argument");
  MTGV_CHECK(frames_ > 0, ERR_INVALID, "tracker: store without an update");
  const int n = frames_ * c_.cards_per_frame;
  // rows == 0 (nothing was due): ids / scores are never read
  hipLaunchKernelGGL(track_store_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, ids, scores, slot_of_, rank_of_, m_ids_, m_scores_, out_ids,
                     out_scores, n, c_.top_k, rows);
  HIP_OK(hipGetLastError());
}

void Tracker::get_state(int stream, double* kal, int32_t* ints, double* last_t, float* avg_z, int64_t* m_ids, float* m_scores, int32_t* ctrs,
                        hipStream_t s) {
  MTGV_CHECK(stream >= 0 && stream < c_.streams, ERR_INVALID, "tracker: stream %d outside [0, %d)", stream, c_.streams);
  const size_t T = c_.max_tracks, i = stream;
  HIP_OK(hipStreamSynchronize(s));
  auto get = [&](void* dst, const void* src, size_t bytes) {
    if (dst != nullptr) HIP_OK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  };
  get(kal, kal_ + i * TRACK_KAL * T, TRACK_KAL * T * sizeof(double));
  get(ints, ints_ + i * TRACK_INTS * T, TRACK_INTS * T * sizeof(int32_t));
  get(last_t, last_t_ + i * T, T * sizeof(double));
  get(avg_z, avg_z_ + i * T * c_.dim, T * c_.dim * sizeof(float));
  get(m_ids, m_ids_ + i * T * c_.top_k, T * c_.top_k * sizeof(int64_t));
  get(m_scores, m_scores_ + i * T * c_.top_k, T * c_.top_k * sizeof(float));
  get(ctrs, ctrs_ + i * TRACK_CTRS, TRACK_CTRS * sizeof(int32_t));
}

void tracker_select_launch(const double* waited, int n, int budget, int32_t* due_idx, int32_t* rank_of, int32_t* n_due, int32_t* n_deferred,
                           hipStream_t s) {
  MTGV_CHECK(waited && due_idx && rank_of && n_due && n_deferred, ERR_INVALID, "track_select: null argument");
  MTGV_CHECK(n >= 1 && n <= SELECT_MAX_SLOTS, ERR_INVALID, "track_select: n %d outside 1..%d", n, SELECT_MAX_SLOTS);
  (void)tracker_check_budget(budget);
  select_launch(waited, 1, nullptr, n, budget, nullptr, nullptr, due_idx, rank_of, n_due, n_deferred, s);
}

void tracker_gather_u8_launch(const uint8_t* src, int64_t src_rows, int64_t row_bytes, const int32_t* due_idx, const int32_t* n_due, int max_rows,
                              uint8_t* dst, bool pad, hipStream_t s) {
  MTGV_CHECK(src && due_idx && n_due && dst, ERR_INVALID, "tracker_gather: null argument");
  MTGV_CHECK(src_rows >= 0 && row_bytes > 0 && max_rows >= 0 && max_rows <= 65535, ERR_INVALID, "tracker_gather: bad shape");
  if (max_rows == 0) return;
  const int vec = row_bytes % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
  const long units = vec ? row_bytes / 16 : row_bytes;
  const int gy = (int)std::min<long>(std::max<long>(1, units / 1024), 32);
  hipLaunchKernelGGL(track_gather_u8_kernel, dim3(max_rows, gy), dim3(256), 0, s, src, (long)src_rows, (long)row_bytes, due_idx, n_due, dst, vec, pad ? 1 : 0);
  HIP_OK(hipGetLastError());
}

}  // namespace mtgv
