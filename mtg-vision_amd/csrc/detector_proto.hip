// The detector's prototype branch: Conv3 -> ConvTranspose2d(k2, s2) -> Conv3 -> Conv1, and the ConvTranspose folded
// into the second conv (detector.h), with its two test entry points.
#include "detector.h"
#include "gemm_sp.h"
#include "gemm_sp_cfg.h"
#include "operand_registry.h"

namespace mtgv {

void proto_fold_compose(const float* wt, const float* bt, const float* w2, const float* b2, int c, int mid, int cout, float* we,
                        float* bias9) {
  // S(a, d): the (t, k) pairs of phase a that read low-resolution offset d
  struct Pair { int t, k; };
  auto taps = [](int a, int d, Pair* out) {
    int cnt = 0;
    for (int t = 0; t < 3; ++t) {
      const int r = a + t - 1;
      const int fl = r >= 0 ? r / 2 : -((-r + 1) / 2);  // floor(r / 2)
      if (fl - (a - 1) == d) out[cnt++] = {t, r - 2 * fl};
    }
    return cnt;
  };
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
          Pair py[3], px[3];
          const int ny = taps(a, dy, py), nx = taps(b, dx, px);
          for (int o = 0; o < cout; ++o)
            for (int i = 0; i < c; ++i) {
              double sum = 0.0;
              for (int u = 0; u < ny; ++u)
                for (int v = 0; v < nx; ++v) {
                  const float* const r2 = w2 + (((size_t)o * 3 + py[u].t) * 3 + px[v].t) * mid;
                  const float* const rt = wt + ((size_t)i * mid * 2 + py[u].k) * 2 + px[v].k;  // + m * 4
                  for (int m = 0; m < mid; ++m) sum += (double)r2[m] * (double)rt[(size_t)m * 4];
                }
              we[(((((size_t)(a * 2 + b) * cout + o) * 2 + dy) * 2 + dx) * c) + i] = (float)sum;
            }
        }
  for (int rc = 0; rc < 3; ++rc)
    for (int cc = 0; cc < 3; ++cc)
      for (int o = 0; o < cout; ++o) {
        double sum = (double)b2[o];
        for (int ty = (rc == 0 ? 1 : 0); ty < (rc == 2 ? 2 : 3); ++ty)
          for (int tx = (cc == 0 ? 1 : 0); tx < (cc == 2 ? 2 : 3); ++tx) {
            const float* const r2 = w2 + (((size_t)o * 3 + ty) * 3 + tx) * mid;
            for (int m = 0; m < mid; ++m) sum += (double)r2[m] * (double)bt[m];
          }
        bias9[(size_t)(rc * 3 + cc) * cout + o] = (float)sum;
      }
}

ProtoTailW proto_tail_weights(const float* wt, const float* bt, int c, int mid, const ConvW& cv2, const ConvW& cv3,
                              std::vector<float*>& allocs) {
  MTGV_CHECK(cv2.k == 3 && cv2.cin == mid && cv3.k == 1 && cv3.cin == cv2.cout, ERR_RUNTIME, "detector: unexpected Proto geometry");
  ProtoTailW p;
  p.cv2 = cv2, p.cv3 = cv3;
  // ConvTranspose2d(k2,s2): weight (in, out, kh, kw) -> four [out][in] matrices, and all four stacked as one [4 mid][c]
  // operand, rows (kh, kw, o), the bias repeated per phase: one launch reads the input once
  float* const bias = upload_operand(std::vector<float>(bt, bt + mid), 0, allocs);
  std::vector<float> all, ball;
  for (int kh = 0; kh < 2; ++kh)
    for (int kw = 0; kw < 2; ++kw) {
      std::vector<float> m((size_t)mid * c);
      for (int o = 0; o < mid; ++o)
        for (int i = 0; i < c; ++i) m[(size_t)o * c + i] = wt[(((size_t)i * mid + o) * 2 + kh) * 2 + kw];
      ConvW q;
      q.w = upload_operand(m, c, allocs), q.b = bias, q.cout = mid, q.cin = c, q.k = 1;
      p.up[kh * 2 + kw] = q;
      all.insert(all.end(), m.begin(), m.end());
      ball.insert(ball.end(), bt, bt + mid);
    }
  p.up_all.w = upload_operand(all, c, allocs), p.up_all.b = upload_operand(ball, 0, allocs);
  p.up_all.cout = 4 * mid, p.up_all.cin = c, p.up_all.k = 1;
  // the fold: where the phase launches exist (gemm_sp.hip, chain_cfg)
  const int co = cv2.cout;
  if (c == mid && co == mid && c % 32 == 0 && sp_chain_cfg(co) >= 0 && cv3.cout % 32 == 0 && cv3.cout <= co) {
    std::vector<float> w2((size_t)co * 9 * mid), b2(co), we((size_t)4 * co * 4 * c), b9((size_t)9 * co);
    HIP_OK(hipMemcpy(w2.data(), cv2.w, w2.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(b2.data(), cv2.b, b2.size() * sizeof(float), hipMemcpyDeviceToHost));
    proto_fold_compose(wt, bt, w2.data(), b2.data(), c, mid, co, we.data(), b9.data());
    const size_t per = (size_t)co * 4 * c;
    for (int q = 0; q < 4; ++q) {
      ConvW f;
      f.w = upload_operand(std::vector<float>(we.begin() + q * per, we.begin() + (q + 1) * per), 4 * c, allocs);
      f.cout = co, f.cin = c, f.k = 2;
      p.fold[q] = f;
    }
    p.fold_bias = upload_operand(b9, 0, allocs);
  }
  return p;
}

// one phase of the folded form: a 2x2 conv over pr1 with pad (1 - a, 1 - b), cv3 chained, rows scattered to phase (a, b)
static GemmArgs proto_phase_args(const ProtoTailW& w, int q, const View& pr1, const View& protos, int n) {
  const int a = q >> 1, b = q & 1;
  const ConvW& f = w.fold[q];
  GemmArgs g = conv_args({pr1.p, n, pr1.H, pr1.W, pr1.ct, pr1.co, pr1.C, pr1.fmt}, f.w, nullptr, f.cout, 2, 2, 1, 0,
                         {nullptr, pr1.H, pr1.W, f.cout, 0, 1}, ACT_SILU);
  g.pad_h = 1 - a, g.pad_w = 1 - b;
  g.os = 2, g.oy = a, g.ox = b, g.OH2 = protos.H, g.OW2 = protos.W;
  g.bias_tab = w.fold_bias;
  g.W2 = w.cv3.w, g.bias2 = w.cv3.b, g.Out2 = protos.p, g.N2 = w.cv3.cout, g.ldo2 = protos.ct, g.o_off2 = protos.co;
  g.out_fmt2 = protos.fmt, g.act2 = ACT_SILU;
  // the profiler's algorithmic FLOPs stay those of the layers replaced: a quarter of ConvTranspose + cv2 per launch
  // (cv3's are the chained layer's own)
  g.xflops = 2.0 * g.M * w.up_all.cout * w.up_all.cin / 4.0 + 2.0 * g.M * w.cv2.cout * (9.0 * w.cv2.cin) - 2.0 * g.M * g.N * g.K;
  return g;
}

bool proto_tail_launch(const ProtoTailW& w, const View& pr1, const View& pr2, const View& pr3, const View& protos, int n, bool fold,
                       hipStream_t s) {
  MTGV_CHECK(protos.H == 2 * pr1.H && protos.W == 2 * pr1.W && pr2.H == protos.H && pr2.W == protos.W && pr1.C == w.up_all.cin &&
                 protos.C == w.cv3.cout,
             ERR_RUNTIME, "detector: Proto views do not match its weights");
  if (fold && w.fold[0].w != nullptr && pr1.fmt == 1 && gemm_sp_chain_ok(proto_phase_args(w, 0, pr1, protos, n))) {
    for (int q = 0; q < 4; ++q) gemm_launch(proto_phase_args(w, q, pr1, protos, n), s);
    return true;
  }
  {
    // SP8 activations (LDS-DMA kernel): one launch with N = 4 * 64 columns whose epilogue scatters column group q to
    // output phase (q / 2, q % 2) - the input is read once instead of four times (round 3: 4 x 27 us at 3.9 TB/s, bound
    // by that re-read).  Same products in the same order per output element: bit-identical to the four launches.
    const bool one_launch = env_int("MTGV_PROTO_UP1", 1) != 0;  // read per call (A/B in one process); 0: the four-launch form
    const bool single = one_launch && pr1.fmt == 1 && w.up[0].cout % 8 == 0;
    View grid = pr2;  // a 1x1 conv over the input grid whose rows scatter to the 2x grid of pr2
    grid.H = pr1.H, grid.W = pr1.W;
    for (int q = 0; q < (single ? 1 : 4); ++q) {
      GemmArgs g = conv_desc(single ? w.up_all : w.up[q], pr1, grid, 1, ACT_NONE, n);
      g.os = 2, g.OH2 = pr2.H, g.OW2 = pr2.W;
      if (single) g.os_nq = w.up[0].cout;
      else g.oy = q >> 1, g.ox = q & 1;
      gemm_launch(g, s);
    }
  }
  conv_pair_launch(w.cv2, pr2, pr3, 1, w.cv3, protos, ACT_SILU, n, s);
  return false;
}

void Detector::proto(const std::string& H, const View& p3, int n, hipStream_t s) {
  conv(cw_.at(H + ".proto.cv1"), p3, view("pr1"), 1, ACT_SILU, nullptr, n, s);
  const View pr1 = view("pr1"), pr2 = view("pr2"), pr3 = view("pr3"), protos = view("protos");
  if (count_flops_) {  // the layers as the model defines them
    flops_ += 2.0 * ((double)n * pr1.H * pr1.W) * proto_w_.up_all.cout * proto_w_.up_all.cin;
    conv(proto_w_.cv2, pr2, pr3, 1, ACT_SILU, nullptr, n, s);
    conv(proto_w_.cv3, pr3, protos, 1, ACT_SILU, nullptr, n, s);
    return;
  }
  const bool fold = env_int("MTGV_PROTO_FOLD", 1) != 0;  // read per call (A/B in one process); 0: ConvTranspose, then cv2 + cv3
  proto_tail_launch(proto_w_, pr1, pr2, pr3, protos, n, fold, s);
}

}  // namespace mtgv

using namespace mtgv;

extern "C" {
MTGV_API int mtgv_op_proto_fold_compose(const float* wt_host, const float* bt_host, const float* w2_host, const float* b2_host, int32_t c,
                                        int32_t mid, int32_t cout, float* we_host, float* bias9_host) {
  return guarded([&] {
    MTGV_CHECK(wt_host && bt_host && w2_host && b2_host && we_host && bias9_host && c > 0 && mid > 0 && cout > 0, ERR_INVALID,
               "proto_fold_compose: bad argument");
    proto_fold_compose(wt_host, bt_host, w2_host, b2_host, c, mid, cout, we_host, bias9_host);
  });
}
MTGV_API int mtgv_op_proto_tail(const mtgv_proto_tail* d, int32_t* folded, void* stream) {
  return guarded([&] {
    MTGV_CHECK(d && d->pr1 && d->wt && d->bt && d->w2 && d->b2 && d->w3 && d->b3 && d->protos, ERR_INVALID, "proto_tail: null argument");
    MTGV_CHECK(d->n > 0 && d->h > 0 && d->w > 0 && d->c > 0 && d->c % 8 == 0 && d->nm > 0 && d->pr1_ct % 8 == 0 && d->pr1_co % 8 == 0 &&
                   d->pr1_co + d->c <= d->pr1_ct && d->protos_ct % 4 == 0 && d->protos_co % 4 == 0 && d->protos_co + d->nm <= d->protos_ct,
               ERR_INVALID, "proto_tail: bad geometry");
    MTGV_CHECK(gemm_sp_active(), ERR_INVALID, "proto_tail: the f16x3 operand mode only (SP8 activations)");
    hipStream_t s = (hipStream_t)stream;
    const int c = d->c;
    std::vector<float*> allocs;
    struct Cleanup {
      std::vector<float*>& a;
      hipStream_t s;
      ~Cleanup() {
        (void)hipStreamSynchronize(s);
        for (float* p : a) operand_unregister(p), (void)hipFree(p);
      }
    } cleanup{allocs, s};
    ConvW cv2, cv3;
    cv2.w = upload_operand(std::vector<float>(d->w2, d->w2 + (size_t)c * 9 * c), 9 * c, allocs);
    cv2.b = upload_operand(std::vector<float>(d->b2, d->b2 + c), 0, allocs), cv2.cout = c, cv2.cin = c, cv2.k = 3;
    cv3.w = upload_operand(std::vector<float>(d->w3, d->w3 + (size_t)d->nm * c), c, allocs);
    cv3.b = upload_operand(std::vector<float>(d->b3, d->b3 + d->nm), 0, allocs), cv3.cout = d->nm, cv3.cin = c, cv3.k = 1;
    const ProtoTailW w = proto_tail_weights(d->wt, d->bt, c, c, cv2, cv3, allocs);
    const size_t mid_floats = (size_t)d->n * 4 * d->h * d->w * c;
    View pr1, pr2, pr3, protos;
    pr1.p = (float*)d->pr1, pr1.H = d->h, pr1.W = d->w, pr1.ct = d->pr1_ct, pr1.co = d->pr1_co, pr1.C = c, pr1.fmt = 1;
    pr2.H = 2 * d->h, pr2.W = 2 * d->w, pr2.ct = c, pr2.C = c, pr2.fmt = 1;
    pr3 = pr2;
    for (View* v : {&pr2, &pr3}) {
      HIP_OK(hipMalloc((void**)&v->p, mid_floats * sizeof(float)));
      allocs.push_back(v->p);
    }
    protos.p = (float*)d->protos, protos.H = 2 * d->h, protos.W = 2 * d->w, protos.ct = d->protos_ct, protos.co = d->protos_co, protos.C = d->nm;
    const bool ran = proto_tail_launch(w, pr1, pr2, pr3, protos, d->n, d->fold != 0, s);
    if (folded) *folded = ran ? 1 : 0;
  });
}
}
