// Host side of the fused C2f tail (c2f_tail_kernel.h): the block's last bottleneck and its closing 1x1 conv as one
// launch on SP8 activations.
#pragma once
#include "common.h"

namespace mtgv {

struct C2fTailArgs {
  const float* cat = nullptr;  // SP8 NHWC concat buffer: slices of ch channels from channel cat_co on, cat_ct floats per pixel
  int cat_ct = 0, cat_co = 0;
  int n_img = 0, H = 0, W = 0;
  int ch = 0;                  // channels of a slice
  int nb = 0;                  // bottlenecks of the block: the last one reads slice nb and the 1x1 reads (2 + nb) slices
  bool shortcut = false;
  const float *w1 = nullptr, *b1 = nullptr;  // bottleneck cv1 [ch][3][3][ch] (registered operands, operand_registry.h)
  const float *w2 = nullptr, *b2 = nullptr;  // bottleneck cv2 [ch][3][3][ch]
  const float *w3 = nullptr, *b3 = nullptr;  // the block's cv2 [cout][(2 + nb) ch]
  int cout = 0;
  float* out = nullptr;        // SP8 NHWC, out_ct floats per pixel, first channel out_co
  int out_ct = 0, out_co = 0;
};

// Is there a kernel for this block?  f16x3 mode, maps of at least 80 x 80 in whole tiles - the launches that fill the
// chip - and either ch = 16 with one bottleneck (8 x 32 tiles) or ch = 32 with one or two (8 x 16 tiles); cout = 2 ch,
// weights registered with SP8 copies, 16-byte aligned vectors.  False: the caller runs the three launches.
bool c2f_tail_ok(const C2fTailArgs& a);
void c2f_tail_launch(const C2fTailArgs& a, hipStream_t s);

}  // namespace mtgv
