// Progressive JPEG (SOF2, Huffman, 8-bit): the coefficient assembly over several scans, for the images of a batch that
// the baseline path (jpeg.hip) cannot take.  It fills the same int16 coefficient blocks, in MCU order, that idct_kernel
// reads, so dequantisation, IDCT, upsampling and colour conversion run unchanged over the whole batch.
//
//   prog_zero      the blocks of the progressive images := 0 (a scan only writes the coefficients it codes)
//   prog_scan      once per dependency level.  A scan depends on an earlier scan of the same image if they share a
//                  component and their bands [Ss, Se] overlap; level = 1 + the highest level it depends on (the host
//                  plans this, jpeg_host.cpp).  Scans of one level touch disjoint coefficients, so one launch decodes
//                  every (scan, restart segment) of that level in the batch: a restart segment starts at a known block
//                  with EOBRUN = 0 and the predictors reset.  One work item per 64-thread workgroup: all lanes copy the
//                  item's Huffman tables into LDS, then lane 0 runs the serial decode of jpeg_prog_decode.h (the text
//                  the host check runs under a sanitizer).  The 0xFF00 stuffing is undone inline by the bit reader; the
//                  host has already found the RSTn markers, so the segment's byte range is known.
//   prog_finish    ok / status of the progressive images from their error words
//
// A work item that does not decode sets its image's error word; later levels, idct and color skip that image, and the
// decode routine checks every block slot against the image's block count, so nothing is written outside its slots.
#include "jpeg_prog.h"

#include "common.h"
#include "jpeg_common.h"
#include "jpeg_prog_decode.h"

namespace mtgv {
namespace jpeg {

namespace {

// eight threads per block: one int4 (eight coefficients) each
__global__ __launch_bounds__(256) void prog_zero_kernel(ProgArgs A, int64_t nblk) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t blk = g >> 3;
  if (blk >= nblk) return;
  const int i = find_base(A.blk_base, A.n, blk);
  if (!A.d[i].prog) return;
  ((int4*)A.coef)[g] = make_int4(0, 0, 0, 0);
}

__global__ __launch_bounds__(64) void prog_scan_kernel(ProgArgs A, int64_t item0) {
  __shared__ HuffTab s_tab[3];
  __shared__ __attribute__((aligned(16))) int16_t s_work[64];
  __shared__ uint8_t s_zz[64];  // the zig-zag order beside the tables: one LDS read per coefficient written
  const int64_t item = item0 + blockIdx.x;
  const int k = find_base(A.item_base, A.nscans, item);
  const ScanDesc& S = A.scans[k];
  const int i = S.img;
  if (A.err[i] != 0) return;  // an earlier level failed (or, harmlessly, an item of this one); one wave, one load: uniform
  const int seg = (int)(item - A.item_base[k]);
  const int ntab = S.ss > 0 ? 1 : S.ah == 0 ? S.ncomp : 0;
  for (int j = 0; j < ntab && j < 3; ++j) {
    const uint32_t* src = (const uint32_t*)(A.tabs + S.tab[j]);
    uint32_t* dst = (uint32_t*)&s_tab[j];
    for (int w = threadIdx.x; w < (int)(sizeof(HuffTab) / 4); w += 64) dst[w] = src[w];
  }
  s_zz[threadIdx.x] = k_natural[threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  const HuffTab* tab[3];  // (filled at run time: an initialiser list of LDS addresses becomes a static initialiser)
  for (int j = 0; j < 3; ++j) tab[j] = s_tab + j;
  const uint32_t b0 = A.seg_off[S.seg0 + seg], b1 = A.seg_off[S.seg0 + seg + 1];
  int r = 1;
  if (b0 <= b1 && (int64_t)b1 <= S.ecs_len) r = prog_decode_segment(A.d[i], S, tab, s_zz, A.ecs + S.ecs + b0, b1 - b0, seg, A.coef + A.d[i].blk0 * 64, s_work);
  if (r) atomicOr(&A.err[i], 1);
}

__global__ __launch_bounds__(64) void prog_finish_kernel(ProgArgs A) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n || !A.d[i].prog) return;
  const int ok = A.err[i] == 0;
  A.ok[i] = ok;
  A.status[i] = ok ? 0 : 1;
}

}  // namespace

void launch_progressive(const ProgArgs& a, const DecodePlan& plan, hipStream_t s) {
  const int64_t nblk = plan.bb()[plan.n];
  hipLaunchKernelGGL(prog_zero_kernel, dim3((unsigned)ceil_div64(nblk * 8, 256)), dim3(256), 0, s, a, nblk);
  for (int l = 0; l < plan.levels(); ++l) {
    const int64_t i0 = plan.item_base[plan.level_scan[l]], i1 = plan.item_base[plan.level_scan[l + 1]];
    if (i1 > i0) hipLaunchKernelGGL(prog_scan_kernel, dim3((unsigned)(i1 - i0)), dim3(64), 0, s, a, i0);
  }
  hipLaunchKernelGGL(prog_finish_kernel, dim3(ceil_div(plan.n, 64)), dim3(64), 0, s, a);
}

}  // namespace jpeg
}  // namespace mtgv
