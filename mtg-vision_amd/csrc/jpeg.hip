// Baseline JPEG decode on the GPU (SOF0 / SOF1, Huffman, 8-bit; 1 component or YCbCr 4:4:4 / 4:2:2 / 4:2:0).
//
// Host (jpeg_host.h / jpeg_host.cpp, no HIP; the records it writes for the kernels are in jpeg_desc.h): walk the markers
// of every image, build descriptors (geometry, quantisation tables, Huffman lookup tables, restart interval,
// entropy-coded segment) and lay out the staging image.  This file keeps the kernels, the handle and the C ABI:
// mtgv_jpeg_decode plans the batch, waits for the previous upload, stages descriptors and entropy-coded bytes into the
// handle's pinned buffer, copies it in one transfer and launches.  Anything outside the supported subset is refused
// before any launch.
//
// Device, one batch in eleven launches (all integer arithmetic):
//   unstuff_count / unstuff_scan / unstuff_scatter  drop the 0x00 after each 0xFF and the RSTn markers (prefix-sum
//                              compaction per 4 KiB tile) -> one bit stream per image + the start byte of every
//                              restart segment
//   sync / sync_fix            self-synchronising parallel Huffman decode (Weissenberger & Schmidt, ICPP 2018): the
//                              stream is cut into 64-byte chunks, each decoded from a guessed state (chunk start, block
//                              0 of the MCU, zig-zag 0) to the first symbol boundary past its end; the exit state
//                              (bit position, block in MCU, zig-zag index) must equal the next chunk's start state.
//                              Within a workgroup, chunks re-decode from their predecessor's exit until nothing
//                              changes (at most 256 rounds); sync_fix then walks every image's workgroup seams in
//                              order, re-decoding chunk after chunk until the states agree again.  Chunk 0 and every
//                              restart segment start from a known state, so once start[c] == exit[c - 1] holds for
//                              every chunk each start is proven; the worst case is a sequential walk.
//   count / verify             blocks per chunk -> per-image exclusive scan; totals per image and per restart segment
//                              checked against the frame geometry -> status word
//   write                      decode again from the proven states, int16 coefficients into their block slots
//   dc                         per-component prefix sum of the DC differences, reset at every restart segment
//   idct                       dequantise + islow integer IDCT (the IJG / libjpeg-turbo jidctint algorithm) -> planes
//   color                      fancy h2v1 / h2v2 upsampling (libjpeg-turbo jdsample rules) + fixed-point YCbCr -> RGB
//                              (jdcolor tables) -> RGB uint8 at the caller's offset / pitch
// Every decode loop is bounded by the stream length.  A stream that does not decode sets its image's status word; the
// write, dc, idct and color launches then skip that image, so nothing is written outside its workspace and slot.
//
// Progressive files (SOF2) are taken by a handle created with MTGV_JPEG_PROGRESSIVE only.  Such an image has no stream of
// its own in the launches above (ImgDesc.prog: no tiles, chunks or restart segments); its coefficient blocks are
// assembled scan by scan by jpeg_prog.hip, launched between dc and idct, and idct / color then run over the whole batch.
// A batch without progressive files runs exactly the eleven launches above, on either kind of handle.
#include <string.h>

#include <algorithm>
#include <string>

#include "common.h"
#include "jpeg_common.h"
#include "jpeg_host.h"
#include "jpeg_prog.h"
#include "mtgv.h"

using namespace mtgv;
using namespace mtgv::jpeg;

namespace {

constexpr int SYNC_WG = 256;  // chunks per workgroup of the in-workgroup synchronisation
constexpr uint32_t POS_END = 0xFFFFFFFFu, POS_ERR = 0xFFFFFFFEu;

struct Staged {  // what one call uploads: pointers into the device copy of the staging image
  const ImgDesc* d;
  const HuffTab* tabs;
  const int64_t* chunk_base;  // n + 1 prefix arrays for the ragged launches
  const int64_t* blk_base;
  const int64_t* seg_base;
  const int64_t* tile_base;
  const int64_t* pix_base;
  const uint8_t* ecs;  // staged entropy-coded bytes
  int n;
};

struct Work {  // the handle's workspaces, allocated at creation
  uint8_t* cs;          // compacted bit streams
  int32_t* tile_cnt;    // per tile: kept bytes, markers, offset, marker offset
  uint32_t* slen;       // stream bytes per image
  int32_t* err;         // per image: 1 entropy decode error, 2 restart marker error
  int32_t* ok;          // per image: decoded so far
  uint32_t* seg_start;  // start byte of each restart segment in the bit stream
  uint32_t* seg_cnt;    // blocks decoded in each segment
  uint64_t* cstart;     // chunk start / exit states
  uint64_t* cexit;
  uint32_t* ccnt;       // blocks started in each chunk, then their exclusive scan
  int16_t* coef;        // 64 per block, natural order
  uint8_t* plane;
};

struct Params : Staged, Work {
  uint8_t* dst;
  int32_t* status;
};

// ---------------------------------------------------------------------------------------------------------------------
// unstuffing

// byte p of an entropy-coded segment d[0, len): kept in the bit stream?  *marker: an RSTn marker starts here
__device__ inline bool keep_byte(const uint8_t* d, int64_t len, int64_t p, int* marker) {
  const uint8_t b = d[p];
  *marker = -1;
  if (b == 0xFF) {
    const uint8_t nx = p + 1 < len ? d[p + 1] : 0xFF;
    if (nx >= 0xD0 && nx <= 0xD7) *marker = nx - 0xD0;
    return nx == 0x00;  // stuffed 0xFF; otherwise a fill byte or the first byte of a marker
  }
  if (p > 0 && d[p - 1] == 0xFF && (b == 0x00 || (b >= 0xD0 && b <= 0xD7))) return false;
  return true;
}

__global__ __launch_bounds__(256) void unstuff_count_kernel(Params P) {
  __shared__ int s[8];
  const int t = blockIdx.x;
  const int i = find_base(P.tile_base, P.n, t);
  const ImgDesc& D = P.d[i];
  const uint8_t* d = P.ecs + D.ecs;
  const int64_t p0 = (int64_t)(t - P.tile_base[i]) * TILE_BYTES + threadIdx.x * 16;
  int kept = 0, mk = 0;
  for (int k = 0; k < 16; ++k) {
    const int64_t p = p0 + k;
    if (p >= D.ecs_len) break;
    int m;
    kept += keep_byte(d, D.ecs_len, p, &m);
    mk += m >= 0;
  }
  int tk, tm;
  block_incl(kept, s, tk);
  block_incl(mk, s + 4, tm);
  if (threadIdx.x == 0) {
    P.tile_cnt[t * 4 + 0] = tk;
    P.tile_cnt[t * 4 + 1] = tm;
  }
}

// one thread per image: tile offsets, stream length, marker count
__global__ __launch_bounds__(64) void unstuff_scan_kernel(Params P) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= P.n) return;
  const ImgDesc& D = P.d[i];
  if (D.prog) return;  // no stream of its own: jpeg_prog.hip
  int off = 0, moff = 0;
  for (int64_t t = P.tile_base[i]; t < P.tile_base[i + 1]; ++t) {
    P.tile_cnt[t * 4 + 2] = off;
    P.tile_cnt[t * 4 + 3] = moff;
    off += P.tile_cnt[t * 4 + 0];
    moff += P.tile_cnt[t * 4 + 1];
  }
  P.slen[i] = (uint32_t)off;
  P.seg_start[D.seg0] = 0;
  if (moff != D.nseg - 1) atomicOr(&P.err[i], 2);
}

__global__ __launch_bounds__(256) void unstuff_scatter_kernel(Params P) {
  __shared__ int s[8];
  const int t = blockIdx.x;
  const int i = find_base(P.tile_base, P.n, t);
  const ImgDesc& D = P.d[i];
  const uint8_t* d = P.ecs + D.ecs;
  const int64_t p0 = (int64_t)(t - P.tile_base[i]) * TILE_BYTES + threadIdx.x * 16;
  uint32_t keepm = 0;
  int kept = 0, mk = 0, mnum[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int64_t p = p0 + k;
    mnum[k] = -1;
    if (p >= D.ecs_len) continue;
    if (keep_byte(d, D.ecs_len, p, &mnum[k])) keepm |= 1u << k, ++kept;
    mk += mnum[k] >= 0;
  }
  int tk, tm;
  int ko = block_incl(kept, s, tk) - kept + P.tile_cnt[t * 4 + 2];
  int mo = block_incl(mk, s + 4, tm) - mk + P.tile_cnt[t * 4 + 3];
  uint8_t* out = P.cs + D.ecs;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (mnum[k] >= 0) {
      // marker number mo starts segment mo + 1 at the next kept byte
      if (mo + 1 < D.nseg) P.seg_start[D.seg0 + mo + 1] = (uint32_t)ko;
      if (mnum[k] != (mo & 7)) atomicOr(&P.err[i], 2);
      ++mo;
    }
    if (keepm >> k & 1) out[ko++] = d[p0 + k];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Huffman decode from a state.  State word: bit position | block in MCU << 32 | zig-zag index << 40.

__device__ inline uint64_t pack_st(uint32_t pos, int b, int z) { return (uint64_t)pos | (uint64_t)b << 32 | (uint64_t)z << 40; }

__device__ inline uint32_t peek32(const uint8_t* s, uint32_t pos) {
  const uint32_t* w = (const uint32_t*)s + (pos >> 5);
  const uint64_t x = (uint64_t)__builtin_bswap32(w[0]) << 32 | __builtin_bswap32(w[1]);
  return (uint32_t)(x >> (32 - (pos & 31)));
}

enum { RUN_SYNC = 0, RUN_COUNT = 1, RUN_WRITE = 2 };

struct RunOut {
  uint32_t blocks;
  bool error;
};

// Decode image i's stream from state `st` until the first symbol boundary at or past bit `stop` (RUN_WRITE: the first
// block boundary).  Returns the state there, POS_END past the last segment, POS_ERR on an invalid code or a segment
// that does not end on an MCU boundary.  RUN_COUNT adds the blocks started before `stop` to seg_cnt; RUN_WRITE writes
// them from block `blk` on (a block already started at `st` is decoded, not written).
template <int MODE>
__device__ uint64_t run(const Params& P, int i, uint64_t st, uint32_t stop, int64_t blk, RunOut& ro) {
  ro.blocks = 0;
  ro.error = false;
  uint32_t pos = (uint32_t)st;
  if (pos == POS_END) return st;
  if (pos == POS_ERR) {
    ro.error = true;
    return st;
  }
  const ImgDesc& D = P.d[i];
  const uint8_t* s = P.cs + D.ecs;
  const uint32_t nbits = P.slen[i] * 8u;
  const uint32_t* segst = P.seg_start + D.seg0;
  int b = (int)(st >> 32) & 0xff, z = (int)(st >> 40) & 0xff;
  if (b >= D.bpm || z > 63) {
    ro.error = true;
    return pack_st(POS_ERR, 0, 0);
  }
  int seg;
  {  // segment of pos: largest s with segst[s] * 8 <= pos
    int lo = 0, hi = D.nseg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((uint64_t)segst[mid] * 8 <= pos) lo = mid;
      else hi = mid - 1;
    }
    seg = lo;
  }
  // (segment starts the unstuffing did not write - fewer markers than restart intervals, an image already marked
  // corrupt - are clamped to the stream so that no read leaves it)
  auto seg_end_of = [&](int sg) { return sg + 1 < D.nseg ? (uint32_t)min((uint64_t)segst[sg + 1] * 8, (uint64_t)nbits) : nbits; };
  uint32_t seg_end = seg_end_of(seg);
  if (pos > nbits) pos = nbits;
  uint32_t seg_blocks = 0;
  const int64_t blk_end = D.blk0 + D.nblocks;
  bool skip = MODE == RUN_WRITE && z != 0;
  int16_t* out = nullptr;
  int comp = D.bcomp[b];
  const HuffTab* tdc = P.tabs + D.c[comp].dc;
  const HuffTab* tac = P.tabs + D.c[comp].ac;
  uint64_t res;
  const uint32_t budget = nbits + (uint32_t)D.nseg + 2;
  for (uint32_t it = 0;; ++it) {
    if (it > budget) {
      res = pack_st(POS_ERR, 0, 0);
      ro.error = true;
      break;
    }
    if (pos >= stop && (MODE != RUN_WRITE || z == 0)) {
      res = pack_st(pos, b, z);
      break;
    }
    bool past = pos >= seg_end;
    int len = 0, sym = 0;
    uint32_t w = 0;
    if (!past) {
      w = peek32(s, pos);
      const HuffTab* t = z == 0 ? tdc : tac;
      const uint32_t e = t->lut[w >> 23];
      if (e) {
        len = (int)(e >> 8);
        sym = (int)(e & 0xff);
      } else {
        len = 10;
        while (len <= 16 && (int32_t)(w >> (32 - len)) > t->maxcode[len]) ++len;
        if (len > 16) {
          // no code matches: corrupt data (or an unsynchronised guess) if all 16 bits lie inside the segment; otherwise
          // these are the segment's 1-bit padding, which no code may consist of
          if (pos + 16 <= seg_end) {
            res = pack_st(POS_ERR, 0, 0);
            ro.error = true;
            break;
          }
          len = 17;  // past the end
        } else {
          sym = t->val[(w >> (32 - len)) + t->valoff[len]];
        }
      }
      const int sb = z == 0 ? sym : (sym & 15);
      past = pos + (uint32_t)len + (uint32_t)sb > seg_end;
      if (!past) {
        int v = 0;
        if (sb) {
          const uint32_t bits = (w << len) >> (32 - sb);
          v = bits < (1u << (sb - 1)) ? (int)bits - (1 << sb) + 1 : (int)bits;
        }
        pos += (uint32_t)(len + sb);
        if (z == 0) {  // DC difference: a block starts
          ++ro.blocks;
          ++seg_blocks;
          if (MODE == RUN_WRITE && blk >= blk_end) skip = true;  // cannot happen once verified; kept as a bound
          if (MODE == RUN_WRITE && !skip) {
            out = P.coef + (blk++) * 64;
            int4* o4 = (int4*)out;
#pragma unroll
            for (int k = 0; k < 8; ++k) o4[k] = make_int4(0, 0, 0, 0);
            out[0] = (int16_t)v;
          }
          z = 1;
        } else {
          const int r = sym >> 4;
          if (sb) {
            z += r;
            if (MODE == RUN_WRITE && !skip) out[k_natural[z > 63 ? 63 : z]] = (int16_t)v;
            ++z;
          } else if (r == 15) {
            z += 16;  // ZRL
          } else {
            z = 64;  // EOB
          }
        }
        if (z >= 64) {
          z = 0;
          if (++b == D.bpm) b = 0;
          skip = false;
          comp = D.bcomp[b];
          tdc = P.tabs + D.c[comp].dc;
          tac = P.tabs + D.c[comp].ac;
        }
        continue;
      }
    }
    // the next symbol would run past the end of the restart segment: the segment is complete
    if (b != 0 || z != 0) {
      res = pack_st(POS_ERR, 0, 0);
      ro.error = true;
      break;
    }
    if (MODE == RUN_COUNT && seg_blocks) atomicAdd(&P.seg_cnt[D.seg0 + seg], seg_blocks);
    seg_blocks = 0;
    if (seg + 1 >= D.nseg) {
      res = pack_st(POS_END, 0, 0);
      break;
    }
    ++seg;
    pos = seg_end;
    seg_end = seg_end_of(seg);
    if (pos > seg_end) pos = seg_end;
  }
  if (MODE == RUN_COUNT && seg_blocks) atomicAdd(&P.seg_cnt[D.seg0 + seg], seg_blocks);
  return res;
}

__device__ inline uint64_t guess_state(const Params& P, int i, int64_t k) {
  const uint64_t pos = (uint64_t)k * CHUNK_BYTES * 8;
  return pos >= (uint64_t)P.slen[i] * 8 ? pack_st(k == 0 ? 0 : POS_END, 0, 0) : pack_st((uint32_t)pos, 0, 0);
}

__global__ __launch_bounds__(SYNC_WG) void sync_kernel(Params P, int64_t nchunks) {
  __shared__ uint64_t s_exit[SYNC_WG];
  __shared__ int s_changed[2];
  const int64_t c = (int64_t)blockIdx.x * SYNC_WG + threadIdx.x;
  const bool valid = c < nchunks;
  const int i = valid ? find_base(P.chunk_base, P.n, c) : 0;
  const int64_t k = valid ? c - P.chunk_base[i] : 0;
  const bool linked = valid && k > 0 && threadIdx.x > 0;
  const uint32_t stop = (uint32_t)((k + 1) * CHUNK_BYTES * 8);
  RunOut ro;
  uint64_t start = valid ? guess_state(P, i, k) : 0;
  uint64_t ex = valid ? run<RUN_SYNC>(P, i, start, stop, 0, ro) : 0;
  for (int round = 0; round < SYNC_WG; ++round) {
    s_exit[threadIdx.x] = ex;
    if (threadIdx.x == 0) s_changed[round & 1] = 0;
    __syncthreads();
    if (linked) {
      const uint64_t ns = s_exit[threadIdx.x - 1];
      if (ns != start) {
        start = ns;
        ex = run<RUN_SYNC>(P, i, start, stop, 0, ro);
        s_changed[round & 1] = 1;
      }
    }
    __syncthreads();
    if (!s_changed[round & 1]) break;
  }
  if (valid) {
    P.cstart[c] = start;
    P.cexit[c] = ex;
  }
}

// one thread per image: the workgroup seams, in stream order
__global__ __launch_bounds__(64) void sync_fix_kernel(Params P) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= P.n) return;
  const int64_t cb = P.chunk_base[i], ce = P.chunk_base[i + 1];
  RunOut ro;
  for (int64_t c = (cb / SYNC_WG + 1) * SYNC_WG; c < ce;) {
    uint64_t e = P.cexit[c - 1];
    int64_t j = c;
    while (j < ce && P.cstart[j] != e) {
      P.cstart[j] = e;
      e = run<RUN_SYNC>(P, i, e, (uint32_t)((j - cb + 1) * CHUNK_BYTES * 8), 0, ro);
      P.cexit[j] = e;
      ++j;
    }
    c = (j / SYNC_WG + 1) * SYNC_WG;
  }
}

__global__ __launch_bounds__(256) void count_kernel(Params P, int64_t nchunks) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= nchunks) return;
  const int i = find_base(P.chunk_base, P.n, c);
  const int64_t k = c - P.chunk_base[i];
  RunOut ro;
  run<RUN_COUNT>(P, i, P.cstart[c], (uint32_t)((k + 1) * CHUNK_BYTES * 8), 0, ro);
  P.ccnt[c] = ro.blocks;
  if (ro.error) atomicOr(&P.err[i], 1);
}

// one wave per image: exclusive scan of the chunk counts, totals checked against the geometry -> status
__global__ __launch_bounds__(64) void verify_kernel(Params P) {
  const int i = blockIdx.x;
  const ImgDesc& D = P.d[i];
  if (D.prog) return;  // prog_finish_kernel sets its ok / status
  const int lane = threadIdx.x;
  const int64_t cb = P.chunk_base[i], ce = P.chunk_base[i + 1];
  int64_t run_total = 0;
  for (int64_t c0 = cb; c0 < ce; c0 += 64) {
    const int64_t c = c0 + lane;
    const int v = c < ce ? (int)P.ccnt[c] : 0;
    const int inc = wave_incl(v);
    if (c < ce) P.ccnt[c] = (uint32_t)(run_total + inc - v);
    run_total += __shfl(inc, 63, 64);
  }
  bool bad = run_total != D.nblocks;
  const int64_t nmcu = (int64_t)D.mcux * D.mcuy;
  for (int s = lane; s < D.nseg; s += 64) {
    const int64_t left = nmcu - (int64_t)s * D.ri;
    const int64_t want = (left < D.ri ? left : D.ri) * D.bpm;
    bad |= P.seg_cnt[D.seg0 + s] != want;
  }
  bad = __any(bad);
  if (lane == 0) {
    const int ok = !bad && P.err[i] == 0;
    P.ok[i] = ok;
    P.status[i] = ok ? 0 : 1;
  }
}

__global__ __launch_bounds__(256) void write_kernel(Params P, int64_t nchunks) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= nchunks) return;
  const int i = find_base(P.chunk_base, P.n, c);
  if (!P.ok[i]) return;
  const int64_t k = c - P.chunk_base[i];
  RunOut ro;
  run<RUN_WRITE>(P, i, P.cstart[c], (uint32_t)((k + 1) * CHUNK_BYTES * 8), P.d[i].blk0 + P.ccnt[c], ro);
}

// one workgroup per restart segment: DC = running sum of the differences, per component
__global__ __launch_bounds__(256) void dc_kernel(Params P) {
  __shared__ int s[12];
  const int64_t g = blockIdx.x;
  const int i = find_base(P.seg_base, P.n, g);
  if (!P.ok[i]) return;  // uniform over the workgroup
  const ImgDesc& D = P.d[i];
  const int64_t sg = g - P.seg_base[i];
  const int64_t nmcu = (int64_t)D.mcux * D.mcuy;
  const int64_t b0 = sg * D.ri * D.bpm, b1 = ((sg + 1) * D.ri < nmcu ? (sg + 1) * D.ri : nmcu) * D.bpm;
  int carry[3] = {0, 0, 0};
  for (int64_t t0 = b0; t0 < b1; t0 += 256) {
    const int64_t bi = t0 + threadIdx.x;
    const bool in = bi < b1;
    int16_t* cf = P.coef + (D.blk0 + bi) * 64;
    const int v = in ? cf[0] : 0;
    const int comp = in ? D.bcomp[bi % D.bpm] : -1;
    int mine = 0;
    for (int q = 0; q < D.ncomp; ++q) {
      int tot;
      const int inc = block_incl(comp == q ? v : 0, s + 4 * q, tot);
      if (comp == q) mine = carry[q] + inc;
      carry[q] += tot;
    }
    if (in) cf[0] = (int16_t)mine;
  }
}

__device__ inline uint8_t idct_limit(int x) {  // libjpeg's post-IDCT range-limit table, indexed with x & 1023
  const int i = x & 1023;
  return (uint8_t)(i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896);
}

// 8 threads per block: a column each in pass 1, a row each in pass 2
__global__ __launch_bounds__(256) void idct_kernel(Params P, int64_t nblocks) {
  __shared__ int ws[32][8][9];
  const int lb = threadIdx.x >> 3, lane = threadIdx.x & 7;
  const int64_t blk = (int64_t)blockIdx.x * 32 + lb;
  const bool valid = blk < nblocks;
  const int i = valid ? find_base(P.blk_base, P.n, blk) : 0;
  const bool live = valid && P.ok[i];
  const ImgDesc& D = P.d[i];
  const int64_t L = blk - D.blk0;
  const int slot = live ? (int)(L % D.bpm) : 0;
  const CompDesc& C = D.c[live ? D.bcomp[slot] : 0];
  constexpr int CB = 13, P1 = 2;
  auto mul = [](int a, int f) { return a * f; };
  if (live) {  // pass 1: column `lane`
    const int16_t* in = P.coef + blk * 64 + lane;
    const uint16_t* q = C.q + lane;
    int z2 = in[16] * q[16], z3 = in[48] * q[48];
    int z1 = mul(z2 + z3, 4433);
    int tmp2 = z1 + mul(z3, -15137), tmp3 = z1 + mul(z2, 6270);
    z2 = in[0] * q[0];
    z3 = in[32] * q[32];
    int tmp0 = (z2 + z3) << CB, tmp1 = (z2 - z3) << CB;
    const int t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
    tmp0 = in[56] * q[56];
    tmp1 = in[40] * q[40];
    tmp2 = in[24] * q[24];
    tmp3 = in[8] * q[8];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = mul(z3 + z4, 9633);
    tmp0 = mul(tmp0, 2446);
    tmp1 = mul(tmp1, 16819);
    tmp2 = mul(tmp2, 25172);
    tmp3 = mul(tmp3, 12299);
    z1 = mul(z1, -7373);
    z2 = mul(z2, -20995);
    z3 = mul(z3, -16069) + z5;
    z4 = mul(z4, -3196) + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr int sh = CB - P1, rd = 1 << (sh - 1);
    int(*w)[9] = ws[lb];
    w[0][lane] = (t10 + tmp3 + rd) >> sh;
    w[7][lane] = (t10 - tmp3 + rd) >> sh;
    w[1][lane] = (t11 + tmp2 + rd) >> sh;
    w[6][lane] = (t11 - tmp2 + rd) >> sh;
    w[2][lane] = (t12 + tmp1 + rd) >> sh;
    w[5][lane] = (t12 - tmp1 + rd) >> sh;
    w[3][lane] = (t13 + tmp0 + rd) >> sh;
    w[4][lane] = (t13 - tmp0 + rd) >> sh;
  }
  __syncthreads();
  if (!live) return;
  const int* r = ws[lb][lane];
  int z2 = r[2], z3 = r[6];
  int z1 = mul(z2 + z3, 4433);
  int tmp2 = z1 + mul(z3, -15137), tmp3 = z1 + mul(z2, 6270);
  int tmp0 = (r[0] + r[4]) << CB, tmp1 = (r[0] - r[4]) << CB;
  const int t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  tmp0 = r[7];
  tmp1 = r[5];
  tmp2 = r[3];
  tmp3 = r[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = mul(z3 + z4, 9633);
  tmp0 = mul(tmp0, 2446);
  tmp1 = mul(tmp1, 16819);
  tmp2 = mul(tmp2, 25172);
  tmp3 = mul(tmp3, 12299);
  z1 = mul(z1, -7373);
  z2 = mul(z2, -20995);
  z3 = mul(z3, -16069) + z5;
  z4 = mul(z4, -3196) + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  constexpr int sh = CB + P1 + 3, rd = 1 << (sh - 1);
  uint8_t o[8];
  o[0] = idct_limit((t10 + tmp3 + rd) >> sh);
  o[7] = idct_limit((t10 - tmp3 + rd) >> sh);
  o[1] = idct_limit((t11 + tmp2 + rd) >> sh);
  o[6] = idct_limit((t11 - tmp2 + rd) >> sh);
  o[2] = idct_limit((t12 + tmp1 + rd) >> sh);
  o[5] = idct_limit((t12 - tmp1 + rd) >> sh);
  o[3] = idct_limit((t13 + tmp0 + rd) >> sh);
  o[4] = idct_limit((t13 - tmp0 + rd) >> sh);
  int64_t by, bx;
  if (D.ncomp == 1) {
    by = L / C.bw;
    bx = L % C.bw;
  } else {
    const int64_t m = L / D.bpm;
    by = (m / D.mcux) * C.v + D.bdy[slot];
    bx = (m % D.mcux) * C.h + D.bdx[slot];
  }
  uint8_t* dst = P.plane + C.plane + (by * 8 + lane) * (int64_t)(C.bw * 8) + bx * 8;
  uint2 pk;
  pk.x = o[0] | o[1] << 8 | o[2] << 16 | (uint32_t)o[3] << 24;
  pk.y = o[4] | o[5] << 8 | o[6] << 16 | (uint32_t)o[7] << 24;
  *(uint2*)dst = pk;
}

// libjpeg jdcolor.c tables, evaluated: FIX(x) = round(x * 2^16), ONE_HALF = 2^15
__device__ inline void ycc_rgb(int y, int cb, int cr, uint8_t* o) {
  cb -= 128;
  cr -= 128;
  const int r = y + ((91881 * cr + 32768) >> 16);
  const int g = y + ((-22554 * cb + 32768 + -46802 * cr) >> 16);
  const int b = y + ((116130 * cb + 32768) >> 16);
  o[0] = (uint8_t)min(max(r, 0), 255);
  o[1] = (uint8_t)min(max(g, 0), 255);
  o[2] = (uint8_t)min(max(b, 0), 255);
}

// chroma sample of output pixel (y, x): libjpeg-turbo h2v1 / h2v2 fancy upsampling (box replication when the
// downsampled width is 2 or less, as jinit_upsampler selects)
__device__ inline int chroma(const uint8_t* p, int stride, int mode, int y, int x, int cw, int ch) {
  if (mode == 1) return p[(int64_t)y * stride + x];
  const int xi = x >> 1;
  if (mode == 2) {
    const uint8_t* r = p + (int64_t)y * stride;
    if (cw <= 2) return r[xi];
    if ((x & 1) == 0) return xi == 0 ? r[0] : (3 * r[xi] + r[xi - 1] + 1) >> 2;
    return xi == cw - 1 ? r[xi] : (3 * r[xi] + r[xi + 1] + 2) >> 2;
  }
  const int yi = y >> 1;
  if (cw <= 2) return p[(int64_t)yi * stride + xi];
  const int yn = min(max((y & 1) ? yi + 1 : yi - 1, 0), ch - 1);
  const uint8_t* r0 = p + (int64_t)yi * stride;
  const uint8_t* r1 = p + (int64_t)yn * stride;
  auto col = [&](int c) { return 3 * r0[c] + r1[c]; };
  const int t = col(xi);
  if ((x & 1) == 0) return xi == 0 ? (4 * t + 8) >> 4 : (3 * t + col(xi - 1) + 8) >> 4;
  return xi == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + col(xi + 1) + 7) >> 4;
}

__global__ __launch_bounds__(256) void color_kernel(Params P, int64_t npix) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= npix) return;
  const int i = find_base(P.pix_base, P.n, g);
  if (!P.ok[i]) return;
  const ImgDesc& D = P.d[i];
  const int64_t l = g - P.pix_base[i];
  const int y = (int)(l / D.w), x = (int)(l % D.w);
  const int ys = D.c[0].bw * 8;
  const int Y = P.plane[D.c[0].plane + (int64_t)y * ys + x];
  uint8_t* o = P.dst + D.dst_off + (int64_t)y * D.pitch + (int64_t)x * 3;
  if (D.ncomp == 1) {
    o[0] = o[1] = o[2] = (uint8_t)Y;
    return;
  }
  const int cs = D.c[1].bw * 8, cw = (D.w + 1) >> 1, ch = (D.h + 1) >> 1;
  const int cb = chroma(P.plane + D.c[1].plane, cs, D.mode, y, x, cw, ch);
  const int cr = chroma(P.plane + D.c[2].plane, cs, D.mode, y, x, cw, ch);
  uint8_t rgb[3];
  ycc_rgb(Y, cb, cr, rgb);
  o[0] = rgb[0];
  o[1] = rgb[1];
  o[2] = rgb[2];
}

}  // namespace

struct mtgv_jpeg_decoder {
  DecoderCaps caps;
  uint8_t* h_stage = nullptr;
  uint8_t* d_stage = nullptr;
  Work work = {};
  hipEvent_t staged = nullptr;  // the last upload from h_stage
  bool pending = false;
  int device = 0;
};

namespace {

void destroy(mtgv_jpeg_decoder* h) {
  if (!h) return;
  if (h->pending) (void)hipEventSynchronize(h->staged);
  if (h->staged) (void)hipEventDestroy(h->staged);
  if (h->h_stage) (void)hipHostFree(h->h_stage);
  const Work& w = h->work;
  void* dev[] = {h->d_stage, w.cs, w.tile_cnt, w.slen, w.err, w.ok, w.seg_start, w.seg_cnt, w.cstart, w.cexit, w.ccnt, w.coef, w.plane};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  delete h;
}

}  // namespace

MTGV_API int mtgv_jpeg_info(const uint8_t* data, int64_t nbytes, int32_t* info) {
  return guarded([&] {
    MTGV_CHECK(info != nullptr, ERR_INVALID, "null info");
    Parsed p;
    parse(data, nbytes, p);
    info[0] = p.h;
    info[1] = p.w;
    info[2] = p.ncomp;
    info[3] = p.sampling;
    info[4] = p.ri;
    info[5] = p.supported;
    set_last_error(p.supported ? std::string() : "jpeg: unsupported: " + p.why);
  });
}

MTGV_API int mtgv_jpeg_info_ex(const uint8_t* data, int64_t nbytes, int32_t flags, int32_t* info) {
  return guarded([&] {
    MTGV_CHECK(info != nullptr, ERR_INVALID, "null info");
    MTGV_CHECK((flags & ~MTGV_JPEG_PROGRESSIVE) == 0, ERR_INVALID, "jpeg: unknown flags 0x%x", flags);
    Parsed p;
    parse(data, nbytes, p);
    info[0] = p.h;
    info[1] = p.w;
    info[2] = p.ncomp;
    info[3] = p.sampling;
    info[4] = p.ri;
    info[5] = p.supported;
    info[6] = 0;
    info[7] = 1;
    std::string why = p.why;
    if (!p.supported && (flags & MTGV_JPEG_PROGRESSIVE)) {
      ProgParsed pp;
      parse_progressive(data, nbytes, pp);
      if (pp.progressive) {
        info[0] = pp.h;
        info[1] = pp.w;
        info[2] = pp.ncomp;
        info[3] = pp.sampling;
        info[4] = pp.ri;
        info[5] = pp.supported;
        info[6] = 1;
        info[7] = (int32_t)pp.scans.size();
        why = pp.why;
      }
    }
    set_last_error(info[5] ? std::string() : "jpeg: unsupported: " + why);
  });
}

MTGV_API int mtgv_jpeg_decoder_create(int32_t max_images, int64_t max_bytes, int64_t max_pixels, mtgv_jpeg_decoder** out) {
  return mtgv_jpeg_decoder_create_ex(max_images, max_bytes, max_pixels, 0, 0, out);
}

MTGV_API int mtgv_jpeg_decoder_create_ex(int32_t max_images, int64_t max_bytes, int64_t max_pixels, int32_t flags, int64_t max_scans,
                                         mtgv_jpeg_decoder** out) {
  return guarded([&] {
    MTGV_CHECK(out != nullptr, ERR_INVALID, "null out");
    *out = nullptr;
    MTGV_CHECK((flags & ~MTGV_JPEG_PROGRESSIVE) == 0, ERR_INVALID, "jpeg: unknown flags 0x%x", flags);
    const bool prog = (flags & MTGV_JPEG_PROGRESSIVE) != 0;
    MTGV_CHECK(max_scans >= 0 && max_scans <= (1 << 24) && (prog || max_scans == 0), ERR_INVALID,
               "jpeg: max_scans %lld (0 .. 2^24, and 0 without MTGV_JPEG_PROGRESSIVE)", (long long)max_scans);
    MTGV_CHECK(max_images >= 1 && max_bytes >= 1 && max_pixels >= 1, ERR_INVALID, "limits must be positive: %d images, %lld bytes, %lld pixels",
               max_images, (long long)max_bytes, (long long)max_pixels);
    MTGV_CHECK(max_bytes < (1ll << 31) && max_pixels < (1ll << 34), ERR_INVALID, "limits too large");
    auto* h = new mtgv_jpeg_decoder();
    const DecoderCaps& c = h->caps = !prog ? decoder_caps(max_images, max_bytes, max_pixels)
                                           : decoder_caps(max_images, max_bytes, max_pixels, max_scans ? max_scans : 16ll * max_images);
    const int64_t n = max_images;
    Work& w = h->work;
    try {
      HIP_OK(hipGetDevice(&h->device));
      HIP_OK(hipHostMalloc((void**)&h->h_stage, c.stage, hipHostMallocDefault));
      HIP_OK(hipMalloc((void**)&h->d_stage, c.stage));
      HIP_OK(hipMalloc((void**)&w.cs, c.ecs + 256));
      HIP_OK(hipMalloc((void**)&w.tile_cnt, c.tiles * 4 * sizeof(int32_t)));
      HIP_OK(hipMalloc((void**)&w.slen, n * sizeof(uint32_t)));
      HIP_OK(hipMalloc((void**)&w.err, n * sizeof(int32_t)));
      HIP_OK(hipMalloc((void**)&w.ok, n * sizeof(int32_t)));
      HIP_OK(hipMalloc((void**)&w.seg_start, c.segs * sizeof(uint32_t)));
      HIP_OK(hipMalloc((void**)&w.seg_cnt, c.segs * sizeof(uint32_t)));
      HIP_OK(hipMalloc((void**)&w.cstart, c.chunks * sizeof(uint64_t)));
      HIP_OK(hipMalloc((void**)&w.cexit, c.chunks * sizeof(uint64_t)));
      HIP_OK(hipMalloc((void**)&w.ccnt, c.chunks * sizeof(uint32_t)));
      HIP_OK(hipMalloc((void**)&w.coef, c.blocks * 64 * sizeof(int16_t)));
      HIP_OK(hipMalloc((void**)&w.plane, c.plane));
      HIP_OK(hipEventCreateWithFlags(&h->staged, hipEventDisableTiming));
    } catch (...) {
      destroy(h);
      throw;
    }
    *out = h;
  });
}

MTGV_API void mtgv_jpeg_decoder_destroy(mtgv_jpeg_decoder* h) { destroy(h); }

MTGV_API int mtgv_jpeg_decode(mtgv_jpeg_decoder* h, const uint8_t* data_host, const int64_t* offsets, const int64_t* sizes, int32_t n,
                              uint8_t* dst_dev, const int64_t* dst_offset, const int64_t* dst_pitch, int32_t* status_dev,
                              void* stream) {
  return guarded([&] {
    MTGV_CHECK(h != nullptr, ERR_INVALID, "null decoder");
    MTGV_CHECK(n >= 0 && n <= h->caps.max_images, ERR_INVALID, "jpeg: %d images, the decoder holds at most %d", n, h->caps.max_images);
    if (n == 0) return;
    MTGV_CHECK(data_host && offsets && sizes && dst_dev && dst_offset && dst_pitch && status_dev, ERR_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    // ---- plan: every image parsed and the whole batch checked before the staging buffer is touched or anything launched
    const DecodePlan plan = plan_decode(h->caps, data_host, offsets, sizes, n, dst_offset, dst_pitch);
    // ---- the previous upload has left the pinned buffer
    if (h->pending) HIP_OK(hipEventSynchronize(h->staged));
    h->pending = false;
    // ---- stage, copy
    stage(plan, data_host, offsets, h->h_stage);
    HIP_OK(hipMemcpyAsync(h->d_stage, h->h_stage, plan.total, hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(h->staged, s));
    h->pending = true;
    const int64_t nch = plan.cb()[n], nblk = plan.bb()[n], nseg = plan.sb()[n], ntile = plan.tb()[n], npix = plan.pb()[n];
    HIP_OK(hipMemsetAsync(h->work.err, 0, n * sizeof(int32_t), s));
    if (nseg) HIP_OK(hipMemsetAsync(h->work.seg_cnt, 0, nseg * sizeof(uint32_t), s));
    // ---- launch
    Params P;
    const int64_t* db = (const int64_t*)(h->d_stage + plan.o_base);
    static_cast<Staged&>(P) = {(const ImgDesc*)h->d_stage,
                               (const HuffTab*)(h->d_stage + plan.o_tab),
                               db,
                               db + (n + 1),
                               db + 2 * (n + 1),
                               db + 3 * (n + 1),
                               db + 4 * (n + 1),
                               h->d_stage + plan.o_ecs,
                               n};
    static_cast<Work&>(P) = h->work;
    P.dst = dst_dev;
    P.status = status_dev;
    if (plan.nprog < n) {  // the baseline images (always, on a handle without MTGV_JPEG_PROGRESSIVE)
      hipLaunchKernelGGL(unstuff_count_kernel, dim3((unsigned)ntile), dim3(256), 0, s, P);
      hipLaunchKernelGGL(unstuff_scan_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, s, P);
      hipLaunchKernelGGL(unstuff_scatter_kernel, dim3((unsigned)ntile), dim3(256), 0, s, P);
      hipLaunchKernelGGL(sync_kernel, dim3((unsigned)ceil_div64(nch, SYNC_WG)), dim3(SYNC_WG), 0, s, P, nch);
      hipLaunchKernelGGL(sync_fix_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, s, P);
      hipLaunchKernelGGL(count_kernel, dim3((unsigned)ceil_div64(nch, 256)), dim3(256), 0, s, P, nch);
      hipLaunchKernelGGL(verify_kernel, dim3(n), dim3(64), 0, s, P);
      hipLaunchKernelGGL(write_kernel, dim3((unsigned)ceil_div64(nch, 256)), dim3(256), 0, s, P, nch);
      hipLaunchKernelGGL(dc_kernel, dim3((unsigned)nseg), dim3(256), 0, s, P);
    }
    if (plan.nprog > 0) {  // the progressive ones: their coefficients assembled scan by scan (jpeg_prog.hip)
      ProgArgs A;
      A.d = P.d;
      A.tabs = P.tabs;
      A.scans = (const ScanDesc*)(h->d_stage + plan.o_scan);
      A.item_base = (const int64_t*)(h->d_stage + plan.o_item);
      A.seg_off = (const uint32_t*)(h->d_stage + plan.o_seg);
      A.ecs = P.ecs;
      A.blk_base = P.blk_base;
      A.coef = P.coef;
      A.err = P.err;
      A.ok = P.ok;
      A.status = P.status;
      A.n = n;
      A.nscans = (int32_t)plan.scans.size();
      launch_progressive(A, plan, s);
    }
    hipLaunchKernelGGL(idct_kernel, dim3((unsigned)ceil_div64(nblk, 32)), dim3(256), 0, s, P, nblk);
    hipLaunchKernelGGL(color_kernel, dim3((unsigned)ceil_div64(npix, 256)), dim3(256), 0, s, P, npix);
    HIP_OK(hipGetLastError());
  });
}
