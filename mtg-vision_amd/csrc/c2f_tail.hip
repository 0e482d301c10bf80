// Fused C2f tail: launch side (kernels in c2f_tail_kernel.h).
#include "c2f_tail.h"

#include "c2f_tail_kernel.h"
#include "gemm_sp.h"
#include "operand_registry.h"

namespace mtgv {

namespace {
// tile geometry of the instance that takes slices of ch channels
struct TailGeom { int th, tw, win_bytes, lds; };
template <class G>
constexpr TailGeom geom_of() { return {G::TH, G::TW, G::WIN_PX * G::RB, G::LDS}; }
bool tail_geom(int ch, TailGeom* t) {
  if (ch == C2fTail16::CH) *t = geom_of<C2fTail16>();
  else if (ch == C2fTail32::CH) *t = geom_of<C2fTail32>();
  else return false;
  return true;
}

template <auto Kern>
void launch(const C2fTailDev& g, long tiles, int lds, hipStream_t s) {
  lds_opt_in<Kern>((size_t)lds, lds);
  hipLaunchKernelGGL(Kern, dim3((unsigned)tiles), dim3(256), (size_t)lds, s, g);
}
}  // namespace

bool c2f_tail_ok(const C2fTailArgs& a) {
  TailGeom t;
  if (!gemm_sp_active() || !tail_geom(a.ch, &t)) return false;
  if (a.cout != 2 * a.ch || !(a.ch == C2fTail16::CH ? a.nb == 1 : (a.nb == 1 || a.nb == 2))) return false;
  if (a.n_img <= 0 || a.H < 80 || a.W < 80 || a.H % t.th != 0 || a.W % t.tw != 0) return false;
  if (a.cat_ct % 8 != 0 || a.cat_co % 8 != 0 || a.out_ct % 8 != 0 || a.out_co % 8 != 0) return false;
  if (a.cat_ct < a.cat_co + (1 + a.nb) * a.ch || a.out_ct < a.out_co + a.cout) return false;
  if (((uintptr_t)a.cat & 15) != 0 || ((uintptr_t)a.out & 15) != 0) return false;
  if (a.b1 == nullptr || a.b2 == nullptr || a.b3 == nullptr) return false;
  if (((uintptr_t)a.b1 & 15) != 0 || ((uintptr_t)a.b2 & 15) != 0 || ((uintptr_t)a.b3 & 15) != 0) return false;
  if ((long)a.n_img * (a.H / t.th) * (a.W / t.tw) > 0x7fffffffL) return false;
  // the kernels read the row scales four at a time (a weight at a row offset inside a stacked operand may not be aligned)
  const char* w8 = nullptr;
  const float *ws1 = nullptr, *ws2 = nullptr, *ws3 = nullptr;
  if (!(operand_sp8(a.w1, 9 * a.ch, &w8, &ws1) && operand_sp8(a.w2, 9 * a.ch, &w8, &ws2) && operand_sp8(a.w3, (2 + a.nb) * a.ch, &w8, &ws3)))
    return false;
  return (((uintptr_t)ws1 | (uintptr_t)ws2 | (uintptr_t)ws3) & 15) == 0;
}

void c2f_tail_launch(const C2fTailArgs& a, hipStream_t s) {
  MTGV_CHECK(c2f_tail_ok(a), ERR_INVALID, "c2f_tail: no kernel for ch=%d n=%d cout=%d on %dx%d: ask c2f_tail_ok first", a.ch, a.nb, a.cout,
             a.H, a.W);
  TailGeom t;
  tail_geom(a.ch, &t);
  const int k3 = (2 + a.nb) * a.ch;
  C2fTailDev g;
  g.cat = reinterpret_cast<const char*>(a.cat);
  g.rowb = (long)a.cat_ct * 4;
  g.e_offb = a.cat_co * 4;
  g.y_offb = (a.cat_co + a.nb * a.ch) * 4;
  g.H = a.H, g.W = a.W;
  g.tiles_x = a.W / t.tw, g.tiles_per_img = g.tiles_x * (a.H / t.th);
  g.d_tpi = make_fastdiv((uint32_t)g.tiles_per_img), g.d_tx = make_fastdiv((uint32_t)g.tiles_x);
  MTGV_CHECK(operand_sp8(a.w1, 9 * a.ch, &g.W1, &g.ws1) && operand_sp8(a.w2, 9 * a.ch, &g.W2, &g.ws2) && operand_sp8(a.w3, k3, &g.W3, &g.ws3),
             ERR_RUNTIME, "c2f_tail: weights lost their SP8 copy");
  g.b1 = a.b1, g.b2 = a.b2, g.b3 = a.b3;
  g.out = a.out, g.ldo = a.out_ct, g.o_off = a.out_co;
  g.shortcut = a.shortcut ? 1 : 0;
  g.zero = sp_zero_page();
  const long tiles = (long)a.n_img * g.tiles_per_img;

  // Recorded as the first 3x3 layer (KH = 3: the launch belongs with the detector's 3x3 convs), the other two layers'
  // algorithmic FLOPs beside it; compulsory bytes: the slices of cat in front of y_new once, the output once, the weights.
  // LDS fill: per tile the window, the slice in front of y_last where it is staged (ch = 16) and every weight matrix.
  const double M = (double)a.n_img * a.H * a.W;
  GemmArgs rec;
  rec.M = (int)M, rec.N = a.ch, rec.K = 9 * a.ch, rec.KH = 3, rec.KW = 3, rec.pad = 1, rec.Cin = a.ch, rec.act = ACT_SILU;
  rec.H = rec.OH = a.H, rec.Wd = rec.OW = a.W;
  const double xflops = 2.0 * M * a.ch * 9 * a.ch + 2.0 * M * a.cout * k3;
  const double wfloats = 2.0 * a.ch * 9 * a.ch + (double)a.cout * k3;
  const double early = a.ch == C2fTail16::CH ? (double)t.th * t.tw * a.ch * 4.0 : 0.0;  // (ch = 32: straight to registers)
  gemm_profile_begin(rec, s, 1, (double)tiles * (t.win_bytes + early + wfloats * 4.0), 4.0 * (M * (k3 - a.ch) + M * a.cout + wfloats), xflops);
  if (a.ch == C2fTail16::CH) launch<c2f_tail_kernel>(g, tiles, t.lds, s);
  else if (a.nb == 1) launch<c2f_tail32_kernel<1>>(g, tiles, t.lds, s);
  else launch<c2f_tail32_kernel<2>>(g, tiles, t.lds, s);
  HIP_OK(hipGetLastError());
  gemm_profile_end(s);
}

}  // namespace mtgv
