// Device-resident card tracker: mtgv/tracker.py's KalmanPointTracker + TrackerCtx gating for S independent streams,
// one workgroup (one wave; up to four in the wide form) per stream, all state on the GPU (include/mtgv.h: mtgv_tracker_*).
#pragma once
#include "common.h"
#include "mtgv.h"

namespace mtgv {

constexpr int TRACK_MAX_TRACKS = 64;   // one lane of the wave per slot
constexpr int TRACK_MAX_CARDS = 16;    // detections of a frame held in LDS
constexpr int TRACK_WIDE_MAX_TRACKS = 256;  // MTGV_TRACKER_WIDE: one thread of a workgroup of up to four waves per slot
constexpr int TRACK_WIDE_MAX_CARDS = 64;
constexpr int TRACK_MAX_TOPK = 8;
constexpr int TRACK_KAL = 40;          // doubles per slot: pos, vel, pp, pv, vv of the 8 corner coordinates
constexpr int TRACK_INTS = 6;          // live, hit_counter, is_initializing, id, birth, has_z
constexpr int TRACK_CTRS = 4;          // per stream: next_id, next_birth, overflow, (unused)

// Policy with the zero fields replaced by the reference's values; throws ERR_INVALID on anything out of range.
// No HIP call: works on a machine without a GPU.  flags: 0 or MTGV_TRACKER_WIDE (the caps of the wide form).
mtgv_tracker_cfg tracker_resolve_cfg(const mtgv_tracker_cfg& c, int32_t flags = 0);
// embed_budget in 1..65535, else ERR_INVALID; no HIP call
int tracker_check_budget(int embed_budget);

class Tracker {
 public:
  // embed_budget 0: none.  1..65535: update selects at most that many due tracks per step (the longest-waiting first, the
  // rest stay due), commit writes every row of q, and a step has at most 8192 slots (mtgv_tracker_create_budget)
  explicit Tracker(const mtgv_tracker_cfg& c, int32_t flags = 0, int embed_budget = 0);
  ~Tracker();
  Tracker(const Tracker&) = delete;
  Tracker& operator=(const Tracker&) = delete;

  void reset(int stream_or_all, hipStream_t s);
  void update(const float* quads, const int32_t* n_det, const int32_t* state, int frames, const int32_t* stream_of_frame, const double* now,
              int32_t* track_id, int32_t* due_idx, int32_t* n_due, int32_t* n_deferred, hipStream_t s);
  void commit(const float* z, float* q, int rows, hipStream_t s);
  void store(const int64_t* ids, const float* scores, int rows, int64_t* out_ids, float* out_scores, hipStream_t s);
  void get_state(int stream, double* kal, int32_t* ints, double* last_t, float* avg_z, int64_t* m_ids, float* m_scores, int32_t* ctrs,
                 hipStream_t s);

 private:
  mtgv_tracker_cfg c_;
  bool wide_;  // the multi-wave update kernel, at every size
  int budget_;  // embeds per step, 0 none
  int frames_ = 0;  // of the last update: commit / store run over frames_ * K rows
  // state, per (stream, slot); lane-major so that the wave's loads coalesce
  double* kal_ = nullptr;       // (S, TRACK_KAL, T)
  int32_t* ints_ = nullptr;     // (S, TRACK_INTS, T)
  double* last_t_ = nullptr;    // (S, T)
  float* avg_z_ = nullptr;      // (S, T, dim)
  int64_t* m_ids_ = nullptr;    // (S, T, top_k)
  float* m_scores_ = nullptr;   // (S, T, top_k)
  int32_t* ctrs_ = nullptr;     // (S, TRACK_CTRS)
  // per step, per frame slot f * K + k
  int32_t* slot_of_ = nullptr;  // s * T + slot of the reported track, -1 none
  int32_t* due_flag_ = nullptr;
  int32_t* rank_of_ = nullptr;  // position in due_idx, -1 not due
  double* defer_ = nullptr;     // budget: per flat slot (key = time waited, the frame's clock) of a candidate
  int32_t* n_deferred_ = nullptr;  // budget: where the count goes when the caller does not ask for it
  const int32_t* due_idx_ = nullptr;  // the caller's buffers of the last update (read by commit / store)
  const int32_t* n_due_ = nullptr;
};

// pad: rows [n_due, max_rows) of dst are zeroed
void tracker_gather_u8_launch(const uint8_t* src, int64_t src_rows, int64_t row_bytes, const int32_t* due_idx, const int32_t* n_due,
                              int max_rows, uint8_t* dst, bool pad, hipStream_t s);
// the selection kernel of a budget handle alone: waited (n) fp64, NaN = no candidate (mtgv_op_track_select)
void tracker_select_launch(const double* waited, int n, int budget, int32_t* due_idx, int32_t* rank_of, int32_t* n_due, int32_t* n_deferred,
                           hipStream_t s);

}  // namespace mtgv
