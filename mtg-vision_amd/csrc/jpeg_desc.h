// The records that the JPEG codecs' host side (jpeg_host.cpp) writes and their kernels (jpeg.hip, jpeg_prog.hip,
// jpeg_enc.hip) read, with the constants both sides size them by.  No HIP header and fixed-width types only: the library
// compiles this with hipcc (host and device pass), the stand-alone host checks with g++, and the static_asserts hold
// all of them to one layout.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mtgv {
namespace jpeg {

// ---- decoder
constexpr int CHUNK_BYTES = 64;   // self-synchronising decode: bytes of stream per thread
constexpr int TILE_BYTES = 4096;  // unstuffing: 256 threads x 16 bytes

struct HuffTab {
  uint16_t lut[512];    // 9-bit lookahead: (length << 8) | symbol; 0: the code is longer than 9 bits
  int32_t maxcode[17];  // largest code of each length, -1 if none
  int32_t valoff[17];   // symbol index = code + valoff[length]
  uint8_t val[256];
};

struct CompDesc {
  uint16_t q[64];  // natural order
  int32_t dc, ac;  // Huffman table index within the batch
  int32_t h, v;    // sampling factors (1 x 1 for a single-component scan)
  int32_t bw, bh;  // plane size in blocks
  int64_t plane;   // byte offset of the plane in the plane workspace
};

struct ImgDesc {
  int32_t h, w, ncomp, mode;  // mode: 0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0
  int32_t mcux, mcuy, bpm, ri, nseg, nchunks, ntiles;
  int32_t prog;  // 1: progressive (SOF2): no chunks, tiles or segments of its own; its scans are ScanDesc records
  int8_t bcomp[8], bdx[8], bdy[8];  // MCU slot -> component, block offset inside the MCU
  int64_t ecs;                      // byte offset of the entropy-coded data (staging) and of the bit stream (workspace)
  int64_t ecs_len;
  int64_t chunk0, seg0, tile0, blk0, pix0, nblocks;
  int64_t dst_off, pitch;
  CompDesc c[3];
};

static_assert(sizeof(HuffTab) == 1416 && alignof(HuffTab) == 4, "HuffTab layout");
static_assert(sizeof(CompDesc) == 160 && offsetof(CompDesc, plane) == 152, "CompDesc layout");
static_assert(sizeof(ImgDesc) == 632 && offsetof(ImgDesc, ecs) == 72 && offsetof(ImgDesc, ecs_len) == 80 &&
                  offsetof(ImgDesc, chunk0) == 88 && offsetof(ImgDesc, seg0) == 96 && offsetof(ImgDesc, tile0) == 104 &&
                  offsetof(ImgDesc, blk0) == 112 && offsetof(ImgDesc, pix0) == 120 && offsetof(ImgDesc, nblocks) == 128 &&
                  offsetof(ImgDesc, dst_off) == 136 && offsetof(ImgDesc, pitch) == 144 && offsetof(ImgDesc, c) == 152,
              "ImgDesc layout");

// ---- progressive decoder (jpeg_prog.hip, jpeg_prog_decode.h): one record per scan, sorted by dependency level
constexpr int PROG_MAX_LEVELS = 64;  // launches of the scan decode a batch may need; a longer chain is refused

struct ScanDesc {
  int32_t img;       // image of the batch
  int32_t ncomp;     // components in the scan: 1..3 (more than one: an interleaved DC scan)
  int8_t comp[4];    // frame component of each
  int8_t slot0[4];   // its first slot in the MCU
  int32_t tab[4];    // Huffman table within the batch: of each component (DC first scan) or tab[0] (AC scans)
  int32_t ss, se, ah, al;
  int32_t ri, nseg;  // units per restart segment (>= 1), segments
  int32_t uw, uh;    // the grid the scan walks: MCUs (interleaved) or the component's own blocks, ceil(w_c / 8) x ceil(h_c / 8)
  int32_t level;     // 1 + the highest level among the earlier scans of a shared component with an overlapping band
  int32_t bad;       // 1: the restart markers do not match the restart interval -> status 1
  int64_t ecs;       // entropy-coded bytes, stuffing and RSTn markers included: offset in the staged region, length
  int64_t ecs_len;
  int64_t seg0;      // seg_off[seg0 + s] .. seg_off[seg0 + s + 1]: bytes of restart segment s within the scan (nseg + 1 entries)
};

static_assert(sizeof(ScanDesc) == 96 && offsetof(ScanDesc, tab) == 16 && offsetof(ScanDesc, ss) == 32 && offsetof(ScanDesc, ri) == 48 &&
                  offsetof(ScanDesc, level) == 64 && offsetof(ScanDesc, ecs) == 72 && offsetof(ScanDesc, ecs_len) == 80 &&
                  offsetof(ScanDesc, seg0) == 88,
              "ScanDesc layout");

// ---- encoder
constexpr int MAX_BLOCK_BITS = 1660;  // DC: 11-bit chroma code + 11 bits; 63 AC: 16-bit code + 10 bits each
constexpr int TILE = 4096;            // bytes of the byte stage per workgroup: 256 threads x 16
constexpr int HDR_BYTES = 623;        // SOI .. SOS with two DQT and four DHT markers (same for both samplings)

// per-call parameters (kernel arguments)
struct Geo {
  int32_t n, h, w, s420;  // s420: 1 for 4:2:0, 0 for 4:4:4
  int32_t bpm, mcux;      // blocks per MCU, MCUs across
  int32_t wb, hb;         // luma plane in blocks (4:2:0 luma blocks past it are dummy blocks)
  int32_t tpi, hlen;      // byte tiles per image (worst case), header bytes
  int64_t bpi;            // blocks per image
  int64_t words;          // bit-stream words per image (tpi * TILE / 4)
};

struct QTab {
  uint8_t q[2][64];  // scaled quantisation tables, natural order: [0] luma, [1] chroma
};

struct Hdr {
  uint8_t b[HDR_BYTES];
};

static_assert(sizeof(Geo) == 56 && offsetof(Geo, bpi) == 40 && offsetof(Geo, words) == 48, "Geo layout");
static_assert(sizeof(QTab) == 128 && sizeof(Hdr) == 623, "QTab / Hdr layout");

}  // namespace jpeg
}  // namespace mtgv
