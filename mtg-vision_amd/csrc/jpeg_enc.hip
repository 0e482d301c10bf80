// Baseline JPEG encode on the GPU (SOF0, Huffman, 8-bit YCbCr 4:2:0 or 4:4:4, the standard tables of Annex K).
//
// The output is byte for byte what libjpeg-turbo writes with its defaults (Pillow's `save(f, "JPEG", quality=q)`, and
// cv2.imencode at the same quality): a JFIF header, fixed-point RGB -> YCbCr (jccolor), edge replication to whole
// blocks / MCU rows (jcprepct, jcsample), h2v2 downsampling with the 1, 2, 1, 2 bias, the islow integer forward DCT
// (jfdctint), rounding quantisation with the scaled Annex K tables clamped to 255 (force_baseline), dummy blocks where
// a 4:2:0 MCU runs past the luma plane (jccoefct), the standard Huffman tables (jchuff), 1-padding and 0xFF stuffing.
//
// One call = n images of one geometry, in seven launches (integer arithmetic only, no workgroup waits for another):
//   fdct     colour + downsample + forward DCT + quantise: 8 threads per block, int16 coefficients in zig-zag order,
//            blocks in scan order (MCU by MCU: Y Y Y Y Cb Cr or Y Cb Cr)
//   count    one wave per block, a lane per coefficient: the bits each lane emits (DC difference, ZRLs + run/size code
//            + value bits, EOB) summed over the wave -> bits per block
//   scan     one workgroup per image: exclusive scan of the block bits -> bit offset of every block, bits per image
//   write    one wave per block: the lanes' codes assembled in LDS, then stored at the block's bit offset (words the
//            block shares with its neighbours are ORed in with atomics, the rest stored plainly)
//   ff       4 KiB tiles of every image's byte stream (the last byte padded with 1-bits): 0xFF bytes per tile
//   offsets  one workgroup: file size of every image (header + stuffed bytes + EOI), their exclusive scan ->
//            out_offsets, and the output position of every tile
//   scatter  header, stuffed bytes and EOI to the output; the bit-stream words are cleared behind the read
// The bit stream must be zero where `write` ORs into it.  It is cleared once when the handle is created and `scatter`
// clears every word a call wrote, so no call needs a clearing launch.  Workspaces are sized at creation; per-call
// parameters (geometry, the two scaled quantisation tables, the header bytes) travel as kernel arguments.
//
// The host arithmetic behind those parameters (geometry, bounds, scaled tables, header) is in jpeg_host.h /
// jpeg_host.cpp, their records in jpeg_desc.h and the Annex K tables in jpeg_tables.h, all without HIP; this file
// keeps the kernels, the handle and the C ABI.
#include <string.h>

#include <algorithm>

#include "common.h"
#include "jpeg_common.h"
#include "jpeg_host.h"
#include "jpeg_tables.h"
#include "mtgv.h"

using namespace mtgv;
using jpeg::HDR_BYTES;
using jpeg::MAX_BLOCK_BITS;
using jpeg::TILE;

namespace {

constexpr int MAX_TILE_WG = 2048;  // workgroups of the ff / scatter launches (they stride over the tiles)

// the Annex K Huffman tables (jpeg_tables.h) as codes
struct HuffEnc {
  uint32_t dc[2][12];   // (code << 8) | length, by category; [0] luma, [1] chroma
  uint32_t ac[2][256];  // by run/size symbol; 0 where the table has no code
};

constexpr HuffEnc make_huff() {
  HuffEnc t{};
  for (int c = 0; c < 2; ++c) {
    for (int ac = 0; ac < 2; ++ac) {
      const uint8_t* bits = jpeg::k_bits[2 * c + ac];
      uint32_t code = 0;
      int k = 0;
      for (int l = 1; l <= 16; ++l) {
        for (int j = 0; j < bits[l]; ++j, ++code, ++k) {
          if (ac) t.ac[c][jpeg::k_val_ac[c][k]] = code << 8 | (uint32_t)l;
          else t.dc[c][jpeg::k_val_dc[k]] = code << 8 | (uint32_t)l;
        }
        code <<= 1;
      }
    }
  }
  return t;
}

__constant__ HuffEnc k_huff = make_huff();

// per-call parameters (kernel arguments): the records of jpeg_desc.h under this file's own names, which the kernels'
// symbols carry
struct Geo : jpeg::Geo {};
struct QTab : jpeg::QTab {};
struct Hdr : jpeg::Hdr {};

struct Work {
  int16_t* coef;      // 64 per block, zig-zag order
  uint32_t* bits;     // bits per block
  uint64_t* boff;     // bit offset of each block in its image's stream
  uint64_t* nbits;    // bits per image
  uint32_t* stream;   // per image `words` words, MSB first
  int32_t* tile_ff;   // 0xFF bytes per tile
  int64_t* tile_out;  // output position of each tile's first byte
};


// ---------------------------------------------------------------------------------------------------------------------
// fdct

// jccolor.c rgb_ycc_convert: FIX(x) = round(x * 2^16); Cb and Cr round with 0.5 - epsilon
__device__ inline int ycc(int comp, const uint8_t* p) {
  const int r = p[0], g = p[1], b = p[2];
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// one 1-D pass of jfdctint.c (islow): PASS 1 leaves the result scaled up by 2^PASS1_BITS, pass 2 removes it
template <int PASS>
__device__ inline void fdct8(const int* d, int* o) {
  constexpr int CB = 13, P1 = 2, SH = PASS == 1 ? CB - P1 : CB + P1;
  auto descale = [](int x, int n) { return (x + (1 << (n - 1))) >> n; };
  int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7];
  int tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5];
  int tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  if (PASS == 1) {
    o[0] = (t10 + t11) * (1 << P1);
    o[4] = (t10 - t11) * (1 << P1);
  } else {
    o[0] = descale(t10 + t11, P1);
    o[4] = descale(t10 - t11, P1);
  }
  int z1 = (t12 + t13) * 4433;
  o[2] = descale(z1 + t13 * 6270, SH);
  o[6] = descale(z1 - t12 * 15137, SH);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  tmp4 *= 2446;
  tmp5 *= 16819;
  tmp6 *= 25172;
  tmp7 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o[7] = descale(tmp4 + z1 + z3, SH);
  o[5] = descale(tmp5 + z2 + z4, SH);
  o[3] = descale(tmp6 + z2 + z3, SH);
  o[1] = descale(tmp7 + z1 + z4, SH);
}

// 8 threads per block: a row each for the samples and pass 1, a column each for pass 2 and the quantisation, eight
// zig-zag coefficients each for the store.  A dummy block (4:2:0 luma past the plane) is transformed from the block
// whose DC it repeats - the previous block of the MCU, or that block's own source - and keeps only that DC.
__global__ __launch_bounds__(256) void fdct_kernel(Geo g, QTab qt, const uint8_t* __restrict__ src, int16_t* __restrict__ coef,
                                                   int64_t nblk) {
  __shared__ int ws[32][8][9];
  __shared__ int qz[32][64];
  const int lb = threadIdx.x >> 3, lane = threadIdx.x & 7;
  const int64_t b = (int64_t)blockIdx.x * 32 + lb;
  const bool valid = b < nblk;
  int comp = 0;
  bool dummy = false;
  if (valid) {
    const int64_t i = b / g.bpi, l = b - i * g.bpi;
    const int64_t m = l / g.bpm;
    const int slot = (int)(l - m * g.bpm);
    const int mx = (int)(m % g.mcux), my = (int)(m / g.mcux);
    const uint8_t* img = src + i * g.h * (int64_t)g.w * 3;
    int bx = mx, by = my;
    comp = g.s420 ? (slot < 4 ? 0 : slot - 3) : slot;
    if (g.s420 && comp == 0) {
      auto past = [&](int s) { return 2 * mx + (s & 1) >= g.wb || 2 * my + (s >> 1) >= g.hb; };
      dummy = past(slot);
      int s = slot;
      while (s > 0 && past(s)) --s;  // slot 0 always lies inside the plane
      bx = 2 * mx + (s & 1);
      by = 2 * my + (s >> 1);
    }
    int d[8], o[8];
    if (g.s420 && comp) {  // h2v2_downsample of the edge-extended full-resolution plane
      const int cy = min(by * 8 + lane, ((g.h + 1) >> 1) - 1);
      const uint8_t* r0 = img + (int64_t)(2 * cy) * g.w * 3;
      const uint8_t* r1 = img + (int64_t)min(2 * cy + 1, g.h - 1) * g.w * 3;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int cx = bx * 8 + c;
        const int x0 = min(2 * cx, g.w - 1) * 3, x1 = min(2 * cx + 1, g.w - 1) * 3;
        d[c] = ((ycc(comp, r0 + x0) + ycc(comp, r0 + x1) + ycc(comp, r1 + x0) + ycc(comp, r1 + x1) + 1 + (c & 1)) >> 2) - 128;
      }
    } else {
      const uint8_t* row = img + (int64_t)min(by * 8 + lane, g.h - 1) * g.w * 3;
#pragma unroll
      for (int c = 0; c < 8; ++c) d[c] = ycc(comp, row + min(bx * 8 + c, g.w - 1) * 3) - 128;
    }
    fdct8<1>(d, o);
#pragma unroll
    for (int c = 0; c < 8; ++c) ws[lb][lane][c] = o[c];
  }
  __syncthreads();
  if (valid) {  // pass 2 on column `lane`, quantise: sign(c) * floor((|c| + 4Q) / 8Q) (jcdctmgr.c, islow divisors 8Q)
    int d[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = ws[lb][r][lane];
    fdct8<2>(d, o);
    const uint8_t* q = qt.q[comp ? 1 : 0];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t Q = q[r * 8 + lane];
      const uint32_t a = (uint32_t)abs(o[r]);
      const int v = (int)((a + 4 * Q) / (8 * Q));
      qz[lb][r * 8 + lane] = o[r] < 0 ? -v : v;
    }
  }
  __syncthreads();
  if (!valid) return;
  int16_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = lane * 8 + j;
    v[j] = (int16_t)(dummy && k ? 0 : qz[lb][k_natural[k]]);
  }
  int4 pk;
  pk.x = (uint16_t)v[0] | (uint32_t)(uint16_t)v[1] << 16;
  pk.y = (uint16_t)v[2] | (uint32_t)(uint16_t)v[3] << 16;
  pk.z = (uint16_t)v[4] | (uint32_t)(uint16_t)v[5] << 16;
  pk.w = (uint16_t)v[6] | (uint32_t)(uint16_t)v[7] << 16;
  *(int4*)(coef + b * 64 + lane * 8) = pk;
}

// ---------------------------------------------------------------------------------------------------------------------
// Huffman: a wave per block, lane k = zig-zag coefficient k.  The lane emits `nzrl` ZRL codes and then `len` bits of
// `code` (its Huffman code followed by its value bits): lane 0 the DC difference, a non-zero AC coefficient its run
// (from the previous non-zero one, found with a ballot) and size, lane 63 the EOB when the block ends in zeros.  Lane
// order is bit order.

struct Piece {
  uint32_t code;
  int len, nzrl;
  uint32_t zrl;  // (code << 8) | length of the table's ZRL
};

__device__ inline Piece lane_piece(const Geo& g, const int16_t* __restrict__ coef, int64_t b, int lane) {
  const int64_t i = b / g.bpi, l = b - i * g.bpi;
  const int64_t m = l / g.bpm;
  const int slot = (int)(l - m * g.bpm);
  const int t = g.s420 ? slot >= 4 : slot > 0;  // table: 0 luma, 1 chroma
  const int v = coef[b * 64 + lane];
  const uint64_t nz = __ballot(v != 0);
  Piece p{0, 0, 0, k_huff.ac[t][0xF0]};
  if (lane == 0) {
    // DC predictor: the previous block of the same component in scan order (0 at the start of the image)
    int64_t pb = -1;
    if (g.s420 && slot >= 1 && slot <= 3) pb = b - 1;
    else if (m > 0) pb = b - g.bpm + (g.s420 && slot == 0 ? 3 : 0);
    const int diff = v - (pb >= 0 ? (int)coef[pb * 64] : 0);
    const int a = abs(diff), s = a ? 32 - __clz(a) : 0;
    const uint32_t e = k_huff.dc[t][s];
    p.code = (e >> 8) << s | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1));
    p.len = (int)(e & 255) + s;
  } else if (v != 0) {
    const uint64_t before = nz & ((1ull << lane) - 1) & ~1ull;  // non-zero AC coefficients ahead of this one
    const int r = lane - (before ? 63 - __clzll(before) : 0) - 1;
    const int a = abs(v), s = 32 - __clz(a);
    const uint32_t e = k_huff.ac[t][(r & 15) << 4 | s];
    p.code = (e >> 8) << s | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1));
    p.len = (int)(e & 255) + s;
    p.nzrl = r >> 4;
  } else if (lane == 63) {
    const uint32_t e = k_huff.ac[t][0x00];  // EOB
    p.code = e >> 8;
    p.len = (int)(e & 255);
  }
  return p;
}

__device__ inline int piece_bits(const Piece& p) { return p.nzrl * (int)(p.zrl & 255) + p.len; }

__global__ __launch_bounds__(256) void count_kernel(Geo g, const int16_t* __restrict__ coef, uint32_t* __restrict__ bits, int64_t nblk) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nblk) return;  // whole waves
  const int lane = threadIdx.x & 63;
  const int tot = wave_incl(piece_bits(lane_piece(g, coef, b, lane)));
  if (lane == 63) bits[b] = (uint32_t)tot;
}

// exclusive scan over a 256-thread workgroup of 64-bit values; `total` gets the sum.  s: 4 words of LDS.
__device__ inline uint64_t block_excl64(uint64_t v, uint64_t* s, uint64_t& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint64_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(x, o, 64);
    if (lane >= o) x += t;
  }
  __syncthreads();
  if (lane == 63) s[wv] = x;
  __syncthreads();
  uint64_t before = 0;
  for (int k = 0; k < wv; ++k) before += s[k];
  total = s[0] + s[1] + s[2] + s[3];
  __syncthreads();  // s may be reused by the caller's next scan
  return before + x - v;
}

// one workgroup per image; thread t scans a contiguous run of the image's blocks
__global__ __launch_bounds__(256) void scan_kernel(Geo g, const uint32_t* __restrict__ bits, uint64_t* __restrict__ boff,
                                                   uint64_t* __restrict__ nbits) {
  __shared__ uint64_t s[4];
  const int64_t b0 = (int64_t)blockIdx.x * g.bpi;
  const int64_t per = (g.bpi + 255) / 256;
  const int64_t lo = b0 + min((int64_t)threadIdx.x * per, g.bpi), hi = b0 + min((int64_t)(threadIdx.x + 1) * per, g.bpi);
  uint64_t sum = 0;
  for (int64_t b = lo; b < hi; ++b) sum += bits[b];
  uint64_t total;
  uint64_t run = block_excl64(sum, s, total);
  for (int64_t b = lo; b < hi; ++b) {
    boff[b] = run;
    run += bits[b];
  }
  if (threadIdx.x == 0) nbits[blockIdx.x] = total;
}

// ORs `len` (<= 32 - 6) bits of `code`, most significant first, into the MSB-first bit string w at bit `pos`
__device__ inline void put_bits(uint32_t* w, int pos, uint32_t code, int len) {
  const uint64_t x = (uint64_t)code << (64 - len - (pos & 31));
  atomicOr(&w[pos >> 5], (uint32_t)(x >> 32));
  if ((uint32_t)x) atomicOr(&w[(pos >> 5) + 1], (uint32_t)x);
}

__global__ __launch_bounds__(256) void write_kernel(Geo g, const int16_t* __restrict__ coef, const uint64_t* __restrict__ boff,
                                                    uint32_t* __restrict__ stream, int64_t nblk) {
  constexpr int W = (31 + MAX_BLOCK_BITS + 31) / 32 + 1;  // words a block can touch (+1: put_bits' second word)
  __shared__ uint32_t buf[4][W];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + wv;
  const bool valid = b < nblk;  // whole waves
  if (lane < W) buf[wv][lane] = 0;
  __syncthreads();
  uint64_t pos0 = 0;
  int total = 0;
  if (valid) {
    const Piece p = lane_piece(g, coef, b, lane);
    const int mine = piece_bits(p);
    const int incl = wave_incl(mine);
    total = __shfl(incl, 63, 64);
    pos0 = boff[b];
    int pos = (int)(pos0 & 31) + incl - mine;
    const int zl = (int)(p.zrl & 255);
    for (int z = 0; z < p.nzrl; ++z, pos += zl) put_bits(buf[wv], pos, p.zrl >> 8, zl);
    if (p.len) put_bits(buf[wv], pos, p.code, p.len);
  }
  __syncthreads();
  if (!valid) return;
  const int nw = ((int)(pos0 & 31) + total + 31) >> 5;
  if (lane < nw) {
    uint32_t* dst = stream + (b / g.bpi) * g.words + (pos0 >> 5);
    const uint32_t v = buf[wv][lane];
    if (lane == 0 || lane == nw - 1) {  // shared with the neighbouring blocks
      if (v) atomicOr(dst + lane, v);
    } else {
      dst[lane] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// bytes: 0xFF stuffing, header, EOI

// thread's 16 bytes of tile t of image i's byte stream (nb bytes, the last one padded with 1-bits); returns how many
// of them exist
__device__ inline int tile_bytes(const Geo& g, const uint32_t* stream, int i, int t, uint64_t nbits, uint8_t* by) {
  const int64_t nb = (int64_t)((nbits + 7) >> 3);
  const int64_t p0 = (int64_t)t * TILE + threadIdx.x * 16;
  const int cnt = (int)max((int64_t)0, min((int64_t)16, nb - p0));
  if (cnt == 0) return 0;
  const uint4 w = *(const uint4*)(stream + i * g.words + (p0 >> 2));
  const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 16; ++k) by[k] = (uint8_t)(ws[k >> 2] >> (24 - 8 * (k & 3)));
  if (p0 + cnt == nb && (nbits & 7)) by[cnt - 1] |= (uint8_t)(0xFF >> (nbits & 7));
  return cnt;
}

__device__ inline int tiles_of(uint64_t nbits) { return (int)((((nbits + 7) >> 3) + TILE - 1) / TILE); }

__global__ __launch_bounds__(256) void ff_kernel(Geo g, const uint32_t* __restrict__ stream, const uint64_t* __restrict__ nbits,
                                                 int32_t* __restrict__ tile_ff) {
  __shared__ int s[4];
  const int64_t nt = (int64_t)g.n * g.tpi;
  for (int64_t f = blockIdx.x; f < nt; f += gridDim.x) {
    const int i = (int)(f / g.tpi), t = (int)(f % g.tpi);
    const uint64_t nb = nbits[i];
    if (t >= tiles_of(nb)) continue;  // uniform over the workgroup
    uint8_t by[16];
    const int cnt = tile_bytes(g, stream, i, t, nb, by);
    int ff = 0;
    for (int k = 0; k < cnt; ++k) ff += by[k] == 0xFF;
    int tot;
    block_incl(ff, s, tot);
    if (threadIdx.x == 0) tile_ff[f] = tot;
    __syncthreads();
  }
}

// one workgroup: file sizes -> out_offsets (n + 1) and the output position of every live tile
__global__ __launch_bounds__(256) void offsets_kernel(Geo g, const uint64_t* __restrict__ nbits, const int32_t* __restrict__ tile_ff,
                                                      int64_t* __restrict__ tile_out, int64_t* __restrict__ out_offsets) {
  __shared__ uint64_t s[4];
  uint64_t carry = 0;
  for (int i0 = 0; i0 < g.n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    uint64_t size = 0;
    int nt = 0;
    if (i < g.n) {
      nt = tiles_of(nbits[i]);
      size = g.hlen + ((nbits[i] + 7) >> 3) + 2;
      for (int t = 0; t < nt; ++t) size += tile_ff[(int64_t)i * g.tpi + t];
    }
    uint64_t total;
    const uint64_t off = carry + block_excl64(size, s, total);
    if (i < g.n) {
      out_offsets[i] = (int64_t)off;
      const int64_t nb = (int64_t)((nbits[i] + 7) >> 3);
      int64_t pos = (int64_t)off + g.hlen;
      for (int t = 0; t < nt; ++t) {
        const int64_t f = (int64_t)i * g.tpi + t;
        tile_out[f] = pos;
        pos += min((int64_t)TILE, nb - (int64_t)t * TILE) + tile_ff[f];
      }
    }
    carry += total;
  }
  if (threadIdx.x == 0) out_offsets[g.n] = (int64_t)carry;
}

__global__ __launch_bounds__(256) void scatter_kernel(Geo g, Hdr hdr, uint32_t* __restrict__ stream, const uint64_t* __restrict__ nbits,
                                                      const int64_t* __restrict__ tile_out, const int64_t* __restrict__ out_offsets,
                                                      uint8_t* __restrict__ out) {
  __shared__ int s[4];
  const int64_t nt = (int64_t)g.n * g.tpi;
  for (int64_t f = blockIdx.x; f < nt; f += gridDim.x) {
    const int i = (int)(f / g.tpi), t = (int)(f % g.tpi);
    const uint64_t nb = nbits[i];
    const int ntiles = tiles_of(nb);
    if (t >= ntiles) continue;  // uniform over the workgroup
    uint8_t by[16];
    const int cnt = tile_bytes(g, stream, i, t, nb, by);
    int ff = 0;
    for (int k = 0; k < cnt; ++k) ff += by[k] == 0xFF;
    int tot;
    int64_t o = tile_out[f] + block_incl(cnt + ff, s, tot) - (cnt + ff);
    for (int k = 0; k < cnt; ++k) {
      out[o++] = by[k];
      if (by[k] == 0xFF) out[o++] = 0;
    }
    if (cnt) {  // the words this thread read are not read again: leave them zero for the next call
      const int64_t p0 = (int64_t)t * TILE + threadIdx.x * 16;
      uint32_t* w = stream + i * g.words + (p0 >> 2);
      for (int k = 0; k < (cnt + 3) >> 2; ++k) w[k] = 0;
    }
    if (t == 0)
      for (int k = threadIdx.x; k < g.hlen; k += 256) out[out_offsets[i] + k] = hdr.b[k];
    if (t == ntiles - 1 && threadIdx.x == 0) {
      const int64_t e = out_offsets[i + 1] - 2;
      out[e] = 0xFF;
      out[e + 1] = 0xD9;
    }
    __syncthreads();
  }
}

}  // namespace

struct mtgv_jpeg_encoder {
  int max_images;
  int64_t max_pixels;
  int64_t cap_blocks, cap_stream_words, cap_tiles;
  Work work = {};
};

namespace {
void destroy_enc(mtgv_jpeg_encoder* h) {
  if (!h) return;
  const Work& w = h->work;
  void* dev[] = {w.coef, w.bits, w.boff, w.nbits, w.stream, w.tile_ff, w.tile_out};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  delete h;
}
}  // namespace

MTGV_API int mtgv_jpeg_encode_bound(int32_t h, int32_t w, int32_t sampling, int64_t* nbytes) {
  return guarded([&] {
    MTGV_CHECK(nbytes != nullptr, ERR_INVALID, "null nbytes");
    jpeg::check_geometry(h, w, sampling);
    *nbytes = jpeg::bound_of(jpeg::geometry(h, w, sampling));
  });
}

MTGV_API int mtgv_jpeg_encode_header(int32_t h, int32_t w, int32_t quality, int32_t sampling, uint8_t* out_host, int64_t capacity,
                                     int64_t* nbytes) {
  return guarded([&] {
    MTGV_CHECK(out_host != nullptr && nbytes != nullptr, ERR_INVALID, "null argument");
    jpeg::check_geometry(h, w, sampling);
    jpeg::check_quality(quality);
    MTGV_CHECK(capacity >= HDR_BYTES, ERR_INVALID, "jpeg: header needs %d bytes, capacity %lld", HDR_BYTES, (long long)capacity);
    jpeg::build_header(h, w, quality, sampling, out_host);
    *nbytes = HDR_BYTES;
  });
}

MTGV_API int mtgv_jpeg_encoder_create(int32_t max_images, int64_t max_pixels, mtgv_jpeg_encoder** out) {
  return guarded([&] {
    MTGV_CHECK(out != nullptr, ERR_INVALID, "null out");
    *out = nullptr;
    MTGV_CHECK(max_images >= 1 && max_pixels >= 1, ERR_INVALID, "jpeg: limits must be positive: %d images, %lld pixels", max_images,
               (long long)max_pixels);
    MTGV_CHECK(max_pixels < (1ll << 34), ERR_INVALID, "jpeg: limits too large");
    auto* h = new mtgv_jpeg_encoder();
    h->max_images = max_images;
    h->max_pixels = max_pixels;
    // 4:4:4 has the most blocks per padded pixel (3 per 64); every image's stream region is its worst case rounded up
    // to whole tiles
    h->cap_blocks = 3 * ceil_div64(max_pixels, 64);
    h->cap_tiles = ceil_div64(ceil_div64(h->cap_blocks * MAX_BLOCK_BITS, 8), TILE) + max_images;
    h->cap_stream_words = h->cap_tiles * (TILE / 4);
    Work& w = h->work;
    try {
      HIP_OK(hipMalloc((void**)&w.coef, h->cap_blocks * 64 * sizeof(int16_t)));
      HIP_OK(hipMalloc((void**)&w.bits, h->cap_blocks * sizeof(uint32_t)));
      HIP_OK(hipMalloc((void**)&w.boff, h->cap_blocks * sizeof(uint64_t)));
      HIP_OK(hipMalloc((void**)&w.nbits, max_images * sizeof(uint64_t)));
      HIP_OK(hipMalloc((void**)&w.stream, h->cap_stream_words * sizeof(uint32_t)));
      HIP_OK(hipMalloc((void**)&w.tile_ff, h->cap_tiles * sizeof(int32_t)));
      HIP_OK(hipMalloc((void**)&w.tile_out, h->cap_tiles * sizeof(int64_t)));
      HIP_OK(hipMemset(w.stream, 0, h->cap_stream_words * sizeof(uint32_t)));  // kept zero between calls (scatter)
      HIP_OK(hipDeviceSynchronize());
    } catch (...) {
      destroy_enc(h);
      throw;
    }
    *out = h;
  });
}

MTGV_API void mtgv_jpeg_encoder_destroy(mtgv_jpeg_encoder* h) { destroy_enc(h); }

MTGV_API int mtgv_jpeg_encode(mtgv_jpeg_encoder* h, const uint8_t* src_dev, int32_t n, int32_t height, int32_t width, int32_t quality,
                              int32_t sampling, uint8_t* out_dev, int64_t out_capacity, int64_t* out_offsets_dev, void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null encoder");
    MTGV_CHECK(n >= 0 && n <= h->max_images, ERR_INVALID, "jpeg: %d images, the encoder holds at most %d", n, h->max_images);
    jpeg::check_geometry(height, width, sampling);
    jpeg::check_quality(quality);
    MTGV_CHECK(out_offsets_dev != nullptr, ERR_INVALID, "null out_offsets");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
      HIP_OK(hipMemsetAsync(out_offsets_dev, 0, sizeof(int64_t), s));
      return;
    }
    MTGV_CHECK(src_dev != nullptr && out_dev != nullptr, ERR_INVALID, "null argument");
    Geo g{jpeg::geometry(height, width, sampling)};
    g.n = n;
    const int64_t pix = n * jpeg::padded_pixels(g);
    MTGV_CHECK(pix <= h->max_pixels, ERR_INVALID, "jpeg: batch needs %lld pixels padded to whole MCUs, the encoder holds %lld",
               (long long)pix, (long long)h->max_pixels);
    const int64_t nblk = n * g.bpi, ntiles = (int64_t)n * g.tpi;
    MTGV_CHECK(nblk <= h->cap_blocks && ntiles <= h->cap_tiles, ERR_INVALID, "jpeg: batch exceeds the encoder's workspace");
    const int64_t bound = jpeg::bound_of(g);
    MTGV_CHECK(out_capacity >= n * bound, ERR_INVALID, "jpeg: output capacity %lld < %d images x %lld bytes (mtgv_jpeg_encode_bound)",
               (long long)out_capacity, n, (long long)bound);
    QTab qt;
    jpeg::scaled_tables(quality, qt.q);
    Hdr hdr;
    jpeg::build_header(height, width, quality, sampling, hdr.b);
    const Work& W = h->work;
    const unsigned tile_wg = (unsigned)std::min<int64_t>(ntiles, MAX_TILE_WG);
    hipLaunchKernelGGL(fdct_kernel, dim3((unsigned)ceil_div64(nblk, 32)), dim3(256), 0, s, g, qt, src_dev, W.coef, nblk);
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)ceil_div64(nblk, 4)), dim3(256), 0, s, g, W.coef, W.bits, nblk);
    hipLaunchKernelGGL(scan_kernel, dim3(n), dim3(256), 0, s, g, W.bits, W.boff, W.nbits);
    hipLaunchKernelGGL(write_kernel, dim3((unsigned)ceil_div64(nblk, 4)), dim3(256), 0, s, g, W.coef, W.boff, W.stream, nblk);
    hipLaunchKernelGGL(ff_kernel, dim3(tile_wg), dim3(256), 0, s, g, W.stream, W.nbits, W.tile_ff);
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(256), 0, s, g, W.nbits, W.tile_ff, W.tile_out, out_offsets_dev);
    hipLaunchKernelGGL(scatter_kernel, dim3(tile_wg), dim3(256), 0, s, g, hdr, W.stream, W.nbits, W.tile_out, out_offsets_dev, out_dev);
    HIP_OK(hipGetLastError());
  });
}
