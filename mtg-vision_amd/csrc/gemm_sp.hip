// LDS-DMA split-precision GEMM: activation packing, tile selection, launch.
#include "gemm_sp.h"

#include <limits.h>
#include <array>
#include <mutex>
#include <utility>
#include <vector>

#include "gemm_sp_kernel.h"
#include "operand_registry.h"

namespace mtgv {

// ---- SP8 packing of activations (the registry packs constant operands, operand_registry.hip) ----
__global__ __launch_bounds__(256) void sp8_pack_plain_kernel(const float* __restrict__ in, sp_h8* __restrict__ out, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  sp_h8 hi, lo;
  sp8_split8(*reinterpret_cast<const sp_f4*>(in + i * 8), *reinterpret_cast<const sp_f4*>(in + i * 8 + 4), hi, lo);
  out[2 * i] = hi;
  out[2 * i + 1] = lo;
}

void sp8_pack_plain_launch(const float* in, void* out, long rows, int K, hipStream_t s) {
  MTGV_CHECK(K % 8 == 0, ERR_INVALID, "sp8: K=%d must be a multiple of 8", K);
  const long n8 = rows * (K / 8);
  if (n8 <= 0) return;
  hipLaunchKernelGGL(sp8_pack_plain_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, in, (sp_h8*)out, n8);
  HIP_OK(hipGetLastError());
}

const char* sp_zero_page() {
  static char* zero[MTGV_MAX_DEVICES] = {};  // one zero page per device: a handle may live on any GPU of the process (mtgv.h)
  static std::mutex mu;
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(mu);
  if (zero[dev] == nullptr) {
    HIP_OK(hipMalloc((void**)&zero[dev], 256));
    HIP_OK(hipMemset(zero[dev], 0, 256));
  }
  return zero[dev];
}

// ---- tile configurations (one translation unit each: gemm_sp_c<id>.hip) ----
template <int ID>
void gemm_sp_launch_cfg(const SpDev& g, int amode, hipStream_t s);  // gemm_sp_inst.h, instantiated by gemm_sp_c<ID>.hip
void gemm_sp_topk_labels_launch(const SpDev& g, hipStream_t s);     // gemm_sp_topk_labels.hip

namespace {
typedef void (*SpLaunchFn)(const SpDev&, int, hipStream_t);
template <int... ID>
constexpr std::array<SpLaunchFn, sizeof...(ID)> sp_launchers(std::integer_sequence<int, ID...>) {
  return {{&gemm_sp_launch_cfg<ID>...}};
}
const auto kLaunch = sp_launchers(std::make_integer_sequence<int, kSpNumCfg>{});

// relative efficiency of each tile's main loop (fitted to tools/gemm_sp_sweep.py); 0: chosen by name below, not searched
const double kEff[kSpNumCfg] = {0.93, 1.00, 0.88, 0.80, 0.62, 0.00, 0.00, 0.00};

SpPlan plan_of(int cfg, int M, int N) {
  const SpTile& k = kSpTile[cfg];
  SpPlan pl;
  pl.cfg = cfg, pl.bm = k.bm(), pl.bn = k.bn(), pl.unit_rows = k.wave_rows();
  pl.tiles_m = ceil_div(M, k.bm()), pl.tiles_n = ceil_div(N, k.bn());
  return pl;
}
}  // namespace

bool window_conv_on() {
  static const bool on = env_int("MTGV_SP_WINDOW", 1) != 0;
  return on;
}

// the window conv (SP_A_WINDOW) takes this launch on the plan's tile
bool window_conv_fits(const GemmArgs& a, const SpPlan& pl) {
  const SpTile& k = kSpTile[pl.cfg];
  if (!(window_conv_on() && a.KH == 3 && a.KW == 3 && a.stride == 1 && conv_pad_h(a) == 1 && conv_pad_w(a) == 1 && a.stride_w <= 0 && a.Cin % k.kps() == 0 &&
        a.OH == a.H && a.OW == a.Wd))
    return false;
  return sp_window_fits(k, a.Wd);
}

// SP_CFG_N160 has one instance: a SiLU window conv from SP8 to SP8 without residual, GRN sums or output remap
static bool n160_instance(const GemmArgs& a) {
  SpPlan p;
  p.cfg = SP_CFG_N160;
  return is_conv(a) && a.a_fmt == 1 && a.W2 == nullptr && a.act == ACT_SILU && a.out_fmt == 1 && a.res == nullptr && a.grn_part == nullptr &&
         !is_remap(a) && a.topk == 0 && window_conv_fits(a, p);
}

bool gemm_sp_active() { return gemm_precision() == GEMM_PREC_F16X3; }

bool gemm_sp_takes_sp8(const float* W, int M, int N, int K, int lda, int c_off) {
  if (!gemm_sp_active()) return false;
  if (K % 8 != 0 || N % 4 != 0 || lda % 8 != 0 || c_off % 8 != 0 || M <= 0) return false;
  return operand_sp8(W, K, nullptr, nullptr);
}

// chained 1x1: SP8 conv input (SP_A_CONV / SP_A_WINDOW: the only ones with SP_EPI_CHAIN instances, gemm_sp_inst.h), SiLU
// between the layers, the whole output row in one tile of a configuration that chains (sp_chain_cfg), plain epilogue
// otherwise.  Phase form (bias_tab, SP_EPI_CHAIN_PHASE: instances on the tap gather only): Out2's rows scattered to
// phase (oy, ox) of the os-times larger grid, no bias vector.
static int chain_cfg(const GemmArgs& a) {
  if (a.W2 == nullptr || a.Out2 == nullptr || !is_conv(a)) return -1;
  if (!(gemm_sp_active() && a.a_fmt == 1 && a.act == ACT_SILU && a.res == nullptr && a.grn_part == nullptr && a.topk == 0 && a.batch == 1 &&
        a.os_nq == 0 && a.a_scale == nullptr && a.ln_w == nullptr))
    return -1;
  if (a.bias_tab == nullptr) {
    if (!(a.os == 1 && a.OH2 == a.OH && a.OW2 == a.OW)) return -1;
  } else {
    if (!(a.bias == nullptr && a.os >= 1 && a.oy >= 0 && a.oy < a.os && a.ox >= 0 && a.ox < a.os && a.OH2 == a.OH * a.os && a.OW2 == a.OW * a.os &&
          ((uintptr_t)a.bias_tab & 15) == 0))
      return -1;
    SpPlan p;
    p.cfg = sp_chain_cfg(a.N);
    if (p.cfg < 0 || window_conv_fits(a, p)) return -1;  // (a 3x3 / pad 1 conv would take the window: no phase instance there)
  }
  if (sp_chain_cfg(a.N) < 0 || a.N2 <= 0 || a.N2 % 32 != 0 || a.N2 > a.N) return -1;
  if (a.K % 8 != 0 || a.c_total % 8 != 0 || a.c_off % 8 != 0 || a.ldo2 % 4 != 0 || a.o_off2 % 4 != 0 || ((uintptr_t)a.Out2 & 15) != 0) return -1;
  if (a.out_fmt2 == 1 && (a.ldo2 % 8 != 0 || a.o_off2 % 8 != 0)) return -1;
  if (a.stride_w > 0 || a.Cin % 8 != 0) return -1;
  if (!operand_sp8(a.W, a.K, nullptr, nullptr) || !operand_sp8(a.W2, a.N, nullptr, nullptr)) return -1;
  return sp_chain_cfg(a.N);
}
bool gemm_sp_chain_ok(const GemmArgs& a) { return chain_cfg(a) >= 0; }

SpPlan gemm_sp_plan(const GemmArgs& a) {
  SpPlan pl;
  if (a.W2 != nullptr) {
    const int c = chain_cfg(a);
    MTGV_CHECK(c >= 0, ERR_INVALID, "gemm: this launch cannot chain its second layer (M=%d N=%d K=%d N2=%d): ask gemm_sp_chain_ok first", a.M,
               a.N, a.K, a.N2);
    return plan_of(c, a.M, a.N);  // (N == bn: one column tile)
  }
  const bool sp8_in = a.a_fmt == 1;
  auto none = [&]() -> SpPlan {
    MTGV_CHECK(!sp8_in && a.out_fmt == 0 && a.res_fmt == 0, ERR_INVALID,
               "gemm: SP8 tensors handed to a launch the SP kernel cannot run (M=%d N=%d K=%d)", a.M, a.N, a.K);
    return pl;
  };
  if (!gemm_sp_active()) return none();
  const bool conv = is_conv(a);
  const bool remap = is_remap(a);
  if (a.batch != 1 || a.crop_boxes != nullptr || a.m_count != nullptr || a.ln_w != nullptr) return none();
  if (a.topk > 0) {  // match path: SP_CFG_TOPK tiles, f32 queries by DMA (SP_A_F32), fused top-k (gemm_sp_kernel.h, SP_EPI_TOPK)
    const SpTile& k1 = kSpTile[SP_CFG_TOPK];
    // A labelled match keeps this kernel however few rows the bank has (one ragged tile: rows past N are clamped on load and
    // score -inf): a row shard of a small bank then runs the kernel the whole bank runs, and the sharded labelled match
    // returns the single bank's score bits (mtgv_bank_topk_packed_ex).  Unlabelled launches keep their rule.
    const bool narrow = a.N < k1.bn() && !topk_labelled(a);
    if (sp8_in || conv || a.K % 8 != 0 || a.c_total % 8 != 0 || a.c_off % 8 != 0 || ((uintptr_t)a.A & 15) != 0 || a.a_scale != nullptr ||
        a.a_mul != 1.0f || a.res != nullptr || a.act != ACT_NONE || a.M < k1.bm() || narrow || !operand_sp8(a.W, a.K, nullptr, nullptr))
      return none();
    return plan_of(SP_CFG_TOPK, a.M, a.N);
  }
  if (conv && (!sp8_in || a.stride_w > 0 || a.Cin % 8 != 0)) return none();  // the gather is a DMA-path feature
  if (remap && !sp8_in) return none();
  if (a.K % 8 != 0 || a.c_total % 8 != 0 || a.c_off % 8 != 0 || a.ldo % 4 != 0 || a.o_off % 4 != 0 ||
      (a.res != nullptr && a.ldr % 4 != 0))
    return none();
  // a ragged last column quad is stored element by element: plain f32 outputs only
  if (a.N % 4 != 0 && (a.out_fmt != 0 || a.res != nullptr || a.grn_part != nullptr || remap)) return none();
  if (a.out_fmt == 1 && (a.N % 8 != 0 || a.ldo % 8 != 0 || a.o_off % 8 != 0 || a.grn_part != nullptr)) return none();
  if (a.res != nullptr && a.res_fmt == 1 && (a.ldr % 8 != 0 || a.N % 8 != 0)) return none();
  if (((uintptr_t)a.Out % 16) != 0 || (a.res != nullptr && ((uintptr_t)a.res % 16) != 0)) return none();
  if (sp8_in && a.a_scale != nullptr) return none();
  if (!operand_sp8(a.W, a.K, nullptr, nullptr)) return none();
  if (!sp8_in && (a.N < 64 || a.M < 128)) return none();  // tiny problems: the convert-on-load kernel's narrow tiles fit better

  int best = -1;
  double best_cost = 0;
  const int force = env_int("MTGV_SP_CFG", INT_MIN);  // tools/sp_cfg_sweep.py; read per plan
  const bool forced = force != INT_MIN;
  if (forced && force >= 0 && force < kSpNumCfg && kSpTile[force].ks == 2 && (force != SP_CFG_N160 || n160_instance(a))) best = force;
  if (best < 0) {
    for (int c = 0; c < kSpNumCfg; ++c) {
      const SpTile& k = kSpTile[c];
      if (kEff[c] <= 0.0) continue;  // not part of the search
      // the 1 KB-per-stage multiplier image of the f32-by-DMA A path does not fit beside the 128 x 192 ring twice per CU
      if (!sp8_in && a.a_scale != nullptr && sp_ring(k, SP_A_F32_MUL, kSpRing) > kSpTwoPerCu) continue;
      const long tiles = (long)ceil_div(a.M, k.bm()) * ceil_div(a.N, k.bn());
      // two blocks per CU: a "round" is up to kSpRoundTiles tiles, each CU working on two at half speed
      const double rounds = (double)((tiles + kSpRoundTiles - 1) / kSpRoundTiles);
      const double per_cu = rounds * 2.0 * k.bm() * k.bn();
      const double cost = per_cu / kEff[c];
      if (best < 0 || cost < best_cost) best = c, best_cost = cost;
    }
  }
  // the whole-ConvTranspose launch (os_nq column groups of 64): one group per 128 x 64 tile measured 9 % faster than 128 x 128
  if (a.os_nq == kSpTile[SP_CFG_OS_NQ].bn() && !forced) best = SP_CFG_OS_NQ;
  {  // 3x3 / stride-1 convs with 16-channel slices (Cin % 32 != 0): the window conv in 16-k stages instead of nine tap gathers
    SpPlan p16;
    p16.cfg = SP_CFG_WIN16;
    if (!forced && conv && sp8_in && a.Cin % kSpTile[best].kps() != 0 && a.N <= kSpTile[SP_CFG_WIN16].bn() && window_conv_fits(a, p16))
      best = SP_CFG_WIN16;
  }
  // the detector heads' stacked first 3x3 convs (64 box + 64 class + 32 coefficient columns): one 160-column tile instead
  // of two 96-column ones - no MFMAs on columns that do not exist, one window fill per slice instead of two.  Only for
  // launches of several rounds of these tiles (P3 of a batch of 640 x 640 frames: 1600), which are bound by what the tiles
  // do.  A launch of one round is bound by how long one tile takes, and there narrower tiles win: P4 (400 row tiles) took
  // 105.5 / 78.2 / 80.4 / 71.2 / 67.0 us on the 128-, 192-, 96-, 64- and 32-column tiles (profiles/r04_sp_cfg_sweep.txt,
  // launch 46), and P5 has 100 row tiles.  Both keep the search's tile.
  // The rule goes by the launch's shape, not by its caller: any SiLU 3x3 / stride-1 SP8 conv of 160 columns and more than
  // a round of row tiles takes it, mtgv_op_conv2d_ex's included (that is how tests/test_gpu_sp8_tile160.py reaches it), and
  // so the detector's switch MTGV_DET_HEAD_DIRECT=0, which restores the head's earlier launches, is read here and puts
  // every such launch back on the search's tile.  Results do not depend on the tile.
  if (!forced && a.N == kSpTile[SP_CFG_N160].bn() && n160_instance(a) && ceil_div(a.M, kSpTile[SP_CFG_N160].bm()) > kSpRoundTiles &&
      env_int("MTGV_DET_HEAD_DIRECT", 1) != 0)
    best = SP_CFG_N160;
  // eight-wave twin of the 128 x 192 tile (four waves per SIMD) for pwconv1-shaped launches: SP8 rows in, activation
  // + GRN sums out; measured -3..-4 % on the stage 2-3 layers, nothing on the others (not below 12288 rows: 6144 x
  // 3072 x 768, the stage-3 pwconv1, is 8 % faster on the four-wave tile - tools/sp_cfg_sweep.py,
  // profiles/r04_sp_cfg_sweep.txt)
  if (best == SP_CFG_TOPK && !conv && sp8_in && a.grn_part != nullptr && a.topk == 0 && a.K >= 256 && a.M >= 12288) best = SP_CFG_PW1_8W;
  return plan_of(best, a.M, a.N);
}

// Tuning aid: with MTGV_SP_STAMPS=1 every launch made while the launch profiler is on leaves per-tile clock stamps
// (gemm_sp_kernel.h); gemm_sp_stamps_dump writes them next to the per-launch table (tools/sp_stamps.py reads them).
namespace {
struct StampRec { int M, N, K, cfg, amode, act, tiles; long* buf; };
std::vector<StampRec> g_stamps;
bool stamps_on() {
  static const bool on = env_int("MTGV_SP_STAMPS", 0) != 0;
  return on;
}
}  // namespace

// top-k candidate layout of a launch the SP kernel would take: groups of `cols` columns, `slots` groups per row
bool gemm_sp_topk_layout(const GemmArgs& a, int* slots, int* cols) {
  const SpPlan pl = gemm_sp_plan(a);
  if (pl.cfg < 0) return false;
  const SpTile& k = kSpTile[pl.cfg];
  *slots = pl.tiles_n * k.wn;
  *cols = k.wave_cols();
  return true;
}

double gemm_sp_fill_bytes(const GemmArgs& a, const SpPlan& pl) {
  const SpTile& k = kSpTile[pl.cfg];
  const double tiles = (double)pl.tiles_m * pl.tiles_n;
  const double b_tile = (double)k.bn() * a.K * 4.0;
  double a_tile = (double)k.bm() * a.K * 4.0;  // dense rows, or one gather per tap
  if (a.a_fmt == 1 && is_conv(a) && window_conv_fits(a, pl)) a_tile = (double)sp_window_bytes(k, a.Wd) * (a.Cin / k.kps());
  if (a.a_scale != nullptr) a_tile += (double)(a.K / k.kps()) * sp_stage_mul(SP_A_F32_MUL);
  return tiles * (a_tile + b_tile);
}

void gemm_sp_stamps_dump(const char* path) {
  if (g_stamps.empty()) return;
  HIP_OK(hipDeviceSynchronize());
  FILE* f = fopen(path, "wb");
  MTGV_CHECK(f != nullptr, ERR_RUNTIME, "cannot open %s", path);
  std::vector<long> host;
  for (const StampRec& r : g_stamps) {
    const int hdr[8] = {r.M, r.N, r.K, r.cfg, r.amode, r.act, r.tiles, 0};
    fwrite(hdr, sizeof(int), 8, f);
    host.resize((size_t)r.tiles * 8);
    HIP_OK(hipMemcpy(host.data(), r.buf, host.size() * sizeof(long), hipMemcpyDeviceToHost));
    fwrite(host.data(), sizeof(long), host.size(), f);
    HIP_OK(hipFree(r.buf));
  }
  fclose(f);
  g_stamps.clear();
}

int gemm_sp_topk_hi16_range_cols() { return kSpTile[SP_CFG_TOPK].wave_cols(); }
int gemm_sp_topk_hi16_slots(int N) { return ceil_div(N, kSpTile[SP_CFG_TOPK].bn()) * kSpTile[SP_CFG_TOPK].wn; }

void gemm_sp_topk_hi16_launch(const void* q_hi, const void* bank_hi, const float* wscale, int b, int N, int K, int kp, float* cand_s,
                              int* cand_i, int* slots, hipStream_t s) {
  const SpTile& k1 = kSpTile[SP_CFG_TOPK];
  MTGV_CHECK(b >= k1.bm() && N >= k1.bn() && K % 64 == 0 && kp >= 1 && kp <= k1.wave_cols(), ERR_INVALID, "topk_hi16: b=%d N=%d K=%d kp=%d", b, N, K, kp);
  MTGV_CHECK(((uintptr_t)q_hi & 15) == 0 && ((uintptr_t)bank_hi & 15) == 0, ERR_INVALID, "topk_hi16: operands must be 16-byte aligned");
  SpDev g;
  g.A = reinterpret_cast<const char*>(q_hi);
  g.a_rowb = (long)K * 2;
  g.W = reinterpret_cast<const char*>(bank_hi);
  g.wscale = wscale;
  g.M = b, g.N = N, g.K = K;
  g.zero = sp_zero_page();
  g.off32 = ((double)N * K * 2.0 < 4294967296.0 - 65536.0) ? 1 : 0;
  g.tiles_m = ceil_div(b, k1.bm()), g.tiles_n = ceil_div(N, k1.bn());
  g.cand_s = cand_s, g.cand_i = cand_i, g.topk = kp;
  g.d_hw = make_fastdiv(1), g.d_ohw = make_fastdiv(1), g.d_ow = make_fastdiv(1), g.d_cin = make_fastdiv(1), g.d_kw = make_fastdiv(1);
  if (slots) *slots = g.tiles_n * k1.wn;
  kLaunch[SP_CFG_TOPK](g, SP_A_HI16, s);
  HIP_OK(hipGetLastError());
}

// How A reaches LDS.  f32 A: by DMA and split at the fragment read when the rows are 16-byte aligned, need no range
// multiplier and a tile's rows span at most 8 images of the per-image multipliers; through registers otherwise
static int sp_amode_of(const GemmArgs& a, const SpPlan& pl) {
  if (a.a_fmt == 1) return !is_conv(a) ? SP_A_SP8 : window_conv_fits(a, pl) ? SP_A_WINDOW : SP_A_CONV;
  if (a.a_mul == 1.0f && ((uintptr_t)a.A & 15) == 0) {
    if (a.a_scale == nullptr) return SP_A_F32;
    if (((uintptr_t)a.a_scale & 15) == 0 && (kSpTile[pl.cfg].bm() - 1) / (a.hw > 0 ? a.hw : 1) + 2 <= 8) return SP_A_F32_MUL;
  }
  return SP_A_REG;
}

// the kernel arguments of launch `a` on plan `pl`
static SpDev sp_dev_of(const GemmArgs& a, const SpPlan& pl) {
  MTGV_CHECK(pl.cfg >= 0 && pl.cfg < kSpNumCfg, ERR_INVALID, "gemm_sp: no plan");
  SpDev g;
  g.A = reinterpret_cast<const char*>(a.A);
  g.a_rowb = (long)a.c_total * 4;
  g.a_offb = (long)a.c_off * 4;
  MTGV_CHECK(operand_sp8(a.W, a.K, &g.W, &g.wscale), ERR_RUNTIME, "gemm_sp: weights lost their SP8 copy");
  g.bias = a.bias;
  g.res = a.res;
  g.ldr = a.ldr;
  g.res_fmt = a.res_fmt;
  g.Out = a.Out;
  g.ldo = a.ldo;
  g.o_off = a.o_off;
  g.out_fmt = a.out_fmt;
  g.M = a.M, g.N = a.N, g.K = a.K;
  g.grn_part = a.grn_part;
  g.hw = a.hw > 0 ? a.hw : 1;
  g.segmax = a.segmax;
  g.d_hw = make_fastdiv((uint32_t)g.hw);
  g.a_scale = a.a_scale;
  g.a_mul = a.a_fmt == 1 ? 1.0f : a.a_mul;
  g.a_unmul = a.a_fmt == 1 ? 1.0f : a.a_unmul;
  g.zero = sp_zero_page();
  {  // byte extents of the operands as the DMA addresses them
    const double lim = 4294967296.0 - 65536.0;
    g.off32 = ((double)a.M * g.a_rowb + (double)g.a_offb < lim && (double)a.N * a.K * 4.0 < lim) ? 1 : 0;
  }
  g.tiles_m = pl.tiles_m, g.tiles_n = pl.tiles_n;
  g.cand_s = a.cand_s, g.cand_i = a.cand_i, g.topk = a.topk;
  if (topk_labelled(a)) {
    g.col_tags = reinterpret_cast<const unsigned long*>(a.col_tags), g.col_groups = a.col_groups;
    g.row_masks = reinterpret_cast<const unsigned long*>(a.row_masks), g.distinct = a.topk_distinct;
  }
  g.act = a.act;
  g.H = a.H, g.Wd = a.Wd, g.Cin = a.Cin, g.KW = a.KW, g.stride = a.stride, g.pad = conv_pad_h(a), g.pad_w = conv_pad_w(a), g.OH = a.OH, g.OW = a.OW;
  g.d_ohw = make_fastdiv((uint32_t)(a.OH * a.OW));
  g.d_ow = make_fastdiv((uint32_t)a.OW);
  g.d_cin = make_fastdiv((uint32_t)(a.Cin > 0 ? a.Cin : 1));
  g.d_kw = make_fastdiv((uint32_t)a.KW);
  g.remap = is_remap(a);
  g.os = a.os, g.oy = a.oy, g.ox = a.ox, g.OH2 = a.OH2, g.OW2 = a.OW2;
  if (a.W2 != nullptr) {
    MTGV_CHECK(operand_sp8(a.W2, a.N, &g.W2, &g.wscale2), ERR_RUNTIME, "gemm_sp: second-layer weights lost their SP8 copy");
    g.bias2 = a.bias2, g.Out2 = a.Out2, g.ldo2 = a.ldo2, g.o_off2 = a.o_off2, g.out_fmt2 = a.out_fmt2;
    g.act2 = a.act2, g.N2 = a.N2;
    g.bias_tab = a.bias_tab;
  }
  g.nq = a.os_nq;
  g.d_nq = make_fastdiv((uint32_t)(a.os_nq > 0 ? a.os_nq : 1)), g.d_os = make_fastdiv((uint32_t)(a.os > 0 ? a.os : 1));
  if (a.os_nq > 0)
    MTGV_CHECK(g.remap && a.os_nq % 8 == 0 && a.N == a.os * a.os * a.os_nq && a.oy == 0 && a.ox == 0 && a.res == nullptr &&
                   a.grn_part == nullptr,
               ERR_INVALID, "gemm_sp: os_nq=%d does not describe a %dx%d scatter of N=%d columns", a.os_nq, a.os, a.os, a.N);
  return g;
}

SpPath gemm_sp_path(const GemmArgs& a, const SpPlan& pl) {
  SpPath p;
  p.cfg = pl.cfg, p.amode = sp_amode_of(a, pl), p.epi = sp_epi_of(sp_dev_of(a, pl));
  p.ring = p.amode == SP_A_WINDOW ? sp_window_ring(kSpTile[pl.cfg], a.Wd, (long)pl.tiles_m * pl.tiles_n) : kSpRing;
  return p;
}

void gemm_sp_launch(const GemmArgs& a, const SpPlan& pl, hipStream_t s) {
  SpDev g = sp_dev_of(a, pl);
  const int amode = sp_amode_of(a, pl);
  if (stamps_on() && gemm_profile_enabled()) {
    const int tiles = pl.tiles_m * pl.tiles_n;
    long* buf = nullptr;
    HIP_OK(hipMalloc(&buf, (size_t)tiles * 8 * sizeof(long)));
    HIP_OK(hipMemsetAsync(buf, 0, (size_t)tiles * 8 * sizeof(long), s));
    g.stamps = buf;
    g_stamps.push_back({a.M, a.N, a.K, pl.cfg, amode, a.act, tiles, buf});
  }
  if (topk_labelled(a)) {
    MTGV_CHECK(pl.cfg == SP_CFG_TOPK && amode == SP_A_F32, ERR_RUNTIME, "gemm_sp: labelled top-k planned on configuration %d, A mode %d", pl.cfg, amode);
    gemm_sp_topk_labels_launch(g, s);
  } else {
    kLaunch[pl.cfg](g, amode, s);
  }
  HIP_OK(hipGetLastError());
}

}  // namespace mtgv
