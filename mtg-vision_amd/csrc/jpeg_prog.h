// The progressive part of a JPEG decode batch (jpeg_prog.hip), as jpeg.hip launches it between its own `dc` and `idct`.
#pragma once

#include <hip/hip_runtime.h>

#include "jpeg_host.h"

namespace mtgv {
namespace jpeg {

struct ProgArgs {
  const ImgDesc* d;
  const HuffTab* tabs;
  const ScanDesc* scans;     // sorted by level
  const int64_t* item_base;  // nscans + 1: prefix of the scans' restart segments
  const uint32_t* seg_off;
  const uint8_t* ecs;        // staged entropy-coded bytes
  const int64_t* blk_base;   // n + 1
  int16_t* coef;
  int32_t* err;              // per image, zero on entry
  int32_t* ok;
  int32_t* status;
  int32_t n, nscans;
};

// zero the coefficient blocks of the progressive images, decode their scans level by level (one launch per level over
// every (scan, restart segment) of the batch), then set ok / status of those images: 2 + plan.levels() launches
void launch_progressive(const ProgArgs& a, const DecodePlan& plan, hipStream_t s);

}  // namespace jpeg
}  // namespace mtgv
