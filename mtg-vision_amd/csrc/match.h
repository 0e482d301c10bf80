// Card bank: device-resident L2-normalised vectors + exact cosine top-k.
#pragma once
#include "common.h"
#include "gemm_f32.h"

namespace mtgv {

class Bank {
 public:
  Bank(int dim, int64_t capacity);
  ~Bank();
  int dim() const { return dim_; }
  int64_t size() const { return size_; }
  int64_t capacity() const { return cap_; }
  void clear();  // labels go back to their defaults
  void append(const float* v, int64_t n, bool is_device, hipStream_t s);
  void set_row(int64_t row, const float* v_host, hipStream_t s);
  void get_rows(int64_t row, int64_t n, float* out_host) const;
  // thr: results scoring below it are dropped (id -1, score -inf); -INFINITY keeps everything.
  // scores == nullptr: ids receives [b][k][2] int64 = (id, float32 bits of the score) - the sharded match's exchange format
  void topk(const float* q, int b, int k, int64_t id_base, float thr, int64_t* ids, float* scores, hipStream_t s);
  // Row labels: tags (uint64 bit set, default 0) and group (int32, default -1 = the row is its own group).  Allocated on
  // first use; append gives new rows the defaults, set_row keeps a row's labels, clear resets them.  A null host pointer
  // leaves that label as it is (set) or is not written (get).
  void set_labels(int64_t row0, int64_t n, const uint64_t* tags_host, const int32_t* groups_host, hipStream_t s);
  void get_labels(int64_t row0, int64_t n, uint64_t* tags_host, int32_t* groups_host) const;
  // topk over the rows whose tags pass the query's masks[b][3] = (all_of, any_of, none_of) (device; null: no filter);
  // distinct: a group >= 0 is represented by its best row only.  Same order, threshold and pad rules as topk.
  void topk_labelled(const float* q, int b, int k, int64_t id_base, float thr, const uint64_t* masks, bool distinct, int64_t* ids,
                     float* scores, hipStream_t s);
  // topk_labelled over this bank as one row shard, in the labelled exchange format: packed[b][k][2] int64 = (id, the row's
  // group as uint32 << 32 | float32 bits of the score); pads are (-1, group -1, -inf).  No threshold (the merge applies
  // it); an empty bank writes pads.
  void topk_packed_labelled(const float* q, int b, int k, int64_t id_base, const uint64_t* masks, bool distinct, int64_t* packed,
                            hipStream_t s);
  // queries of two-pass matches so far whose answer the first pass could not prove and that were scanned exactly
  // (synchronises the device)
  int64_t prepass_fallbacks() const;
  // Test surface of the two-pass match's first pass: the candidates it hands the re-rank, cand_s / cand_i as
  // [b][slots][per_range] in the caller's device buffers; range w covers columns [w * range_cols, (w + 1) * range_cols).
  // prepass_layout sizes the buffers for the bank's current size; prepass_candidates throws (ERR_INVALID) before writing
  // anything when topk would not run the first pass on this bank and batch.
  void prepass_layout(int* slots, int* range_cols, int* per_range) const;
  void prepass_candidates(const float* q, int b, float* cand_s, int* cand_i, int* slots, int* range_cols, hipStream_t s);

 private:
  // two-pass match (match.hip): approximate fp16 scores over a hi-only copy of the bank, exact re-rank of the candidates
  bool prepass_ok(int b, int k) const;
  void topk_prepass(const float* q, int b, int k, int64_t id_base, float thr, int64_t* ids, float* scores, hipStream_t s);
  void refresh_hi(int64_t row0, int64_t rows, hipStream_t s);
  void ensure_labels();
  void topk_one_pass(const float* q, int b, int k, int64_t id_base, float thr, bool labelled, const uint64_t* masks, bool distinct,
                     int64_t* ids, float* scores, hipStream_t s);

  int dim_;
  int64_t cap_, size_ = 0;
  DevBuf vecs_, qn_, cand_s_, cand_i_;
  DevBuf tags_, groups_;     // row labels, capacity rows each (uint64 / int32); null until a label is set or a labelled match runs
  DevBuf hi_, qhi_, stat_;   // fp16 hi halves of the (row-scaled) bank rows / of the normalised queries, 2 bytes per element
};

// merge of all-gathered per-shard candidates in the exchange format (gathered[R][b_total][k][2]: id, score bits) for
// the queries [row0, row0 + b).  distinct: the candidates are in the labelled exchange format, and there is one result per
// group >= 0: picking a candidate retires every other candidate of its group
void topk_merge_gathered_launch(const int64_t* gathered, int R, int b_total, int k, int row0, int b, float thr, bool distinct, int64_t* ids,
                                float* scores, hipStream_t s);
void topk_merge_launch_i64(float* cs, const int64_t* ci, int b, int ncand, int k, float thr, int64_t* ids, float* scores,
                           hipStream_t s);

}  // namespace mtgv
