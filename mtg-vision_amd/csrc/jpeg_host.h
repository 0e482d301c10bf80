// Host side of the JPEG codecs (jpeg_host.cpp): everything between the caller's bytes and the kernels' arguments that
// never calls HIP.  Decoder: the marker walk over untrusted input, the capacities of a handle, the plan of one batch
// (descriptors, Huffman tables, ragged bases, staging layout) and the staging image itself.  Encoder: geometry, bounds,
// the scaled quantisation tables and the file header.  Includes status.h, the record / table headers and the standard
// library only, so it also builds with a plain host compiler under a sanitizer (tests/host/jpeg_host_check.cpp).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "jpeg_desc.h"
#include "status.h"

namespace mtgv {
namespace jpeg {

// ---------------------------------------------------------------------------------------------------------------------
// decoder

struct Parsed {
  int h = 0, w = 0, ncomp = 0, sampling = 0, ri = 0, supported = 0;
  std::string why;  // first unsupported feature
  struct Comp {
    int id, h, v, tq, td, ta;
  } comp[4];
  uint16_t qt[4][64];
  bool qdef[4] = {false, false, false, false};
  uint8_t hbits[2][4][17];
  uint8_t hval[2][4][256];
  bool hdef[2][4] = {{false, false, false, false}, {false, false, false, false}};
  int64_t ecs = 0, ecs_len = 0;
};

// walks the markers of one file; throws ERR_INVALID on malformed input, sets p.why on unsupported input
void parse(const uint8_t* d, int64_t n, Parsed& p);

// canonical codes of a DHT table; false if a code does not fit its length (libjpeg: no all-ones code)
bool huff_codes(const uint8_t* bits, int* maxcode, int* valoff, uint16_t* lut, const uint8_t* val);

// One scan of a progressive file (SOF2), as parse_progressive() reads it
struct ProgScan {
  int ns = 0;                // components in the scan
  int comp[4] = {0, 0, 0, 0};  // index of each in the frame
  int ss = 0, se = 0, ah = 0, al = 0;
  int ri = 0;                // restart interval in force at this SOS (0: none)
  int64_t ecs = 0, ecs_len = 0;  // entropy-coded bytes, stuffing and RSTn markers included
  std::vector<uint32_t> rst;     // for each RSTn marker: the byte after it, relative to ecs
  bool rst_in_order = true;      // the markers count 0..7 cyclically
  // the Huffman tables the scan decodes with, as defined when its SOS was read: tab[j] of component j for a DC first
  // scan, tab[0] for an AC scan, none for a DC refinement scan
  struct Tab {
    uint8_t bits[17];
    uint8_t val[256];
  };
  std::vector<Tab> tab;
};

struct ProgParsed {
  bool progressive = false;  // false: the frame is not SOF2 and nothing else below is set; parse() has the verdict
  int h = 0, w = 0, ncomp = 0, sampling = 0, ri = 0, supported = 0;  // ri: the first scan's restart interval
  std::string why;
  Parsed::Comp comp[4];
  uint16_t qt[4][64];  // by table index, natural order, as defined when the first SOS was read
  std::vector<ProgScan> scans;
};

// The second walk, for progressive files: frame header, then every scan with its components, Ss / Se / Ah / Al, restart
// interval, table snapshot and entropy-coded byte range.  Throws ERR_INVALID (naming the marker) on malformed input and
// on a scan script T.81 Annex G does not allow; sets p.why on a well-formed file outside the subset, among them an
// incomplete progression (some coefficient of some component is never brought to Al = 0).  Never reads past d[n - 1].
void parse_progressive(const uint8_t* d, int64_t n, ProgParsed& p);

// what a decoder handle holds: the caller's limits and the element counts of the workspaces sized from them
struct DecoderCaps {
  int max_images;
  int64_t max_bytes, max_pixels;
  int64_t stage;   // bytes of the staging buffer
  int64_t ecs;     // bytes of entropy-coded data, each image padded to 8 bytes + 8 (the bit-stream workspace adds 256)
  int64_t chunks, tiles, segs, blocks;
  int64_t plane;   // bytes of the plane workspace
  // progressive handles (0 otherwise): scans per batch, restart segments of all scans (+ one entry per scan)
  int64_t max_scans, prog_segs;
};

DecoderCaps decoder_caps(int max_images, int64_t max_bytes, int64_t max_pixels);
// a handle that also takes progressive files; max_scans: scans per batch over all its progressive images
DecoderCaps decoder_caps(int max_images, int64_t max_bytes, int64_t max_pixels, int64_t max_scans);

// one batch, checked against the capacities: everything the launches trust
struct DecodePlan {
  int n = 0;
  std::vector<Parsed> ps;
  std::vector<ImgDesc> ds;
  std::vector<HuffTab> tabs;   // deduplicated over the batch
  std::vector<int64_t> bases;  // five n + 1 prefix arrays, in the order of the accessors below
  int64_t o_tab = 0, o_base = 0, o_ecs = 0, total = 0;  // staging layout: descriptors | tables | bases | entropy-coded bytes
  const int64_t* cb() const { return bases.data(); }  // chunks
  const int64_t* bb() const { return bases.data() + (n + 1); }  // blocks
  const int64_t* sb() const { return bases.data() + 2 * (n + 1); }  // restart segments
  const int64_t* tb() const { return bases.data() + 3 * (n + 1); }  // unstuffing tiles
  const int64_t* pb() const { return bases.data() + 4 * (n + 1); }  // pixels
  // progressive images (caps.max_scans > 0 only; all empty / zero for a batch without one).  Such an image has
  // ds[i].prog = 1 and no chunks, tiles or restart segments in the arrays above; its scans are records of their own,
  // sorted by dependency level, staged between the bases and the entropy-coded bytes.
  int nprog = 0;
  std::vector<ProgParsed> pps;      // n entries; progressive == false for a baseline image
  std::vector<ScanDesc> scans;      // level 1 first
  std::vector<int64_t> item_base;   // scans.size() + 1: prefix of nseg, the work items (scan, restart segment)
  std::vector<uint32_t> seg_off;    // per scan nseg + 1 byte offsets within its entropy-coded bytes
  std::vector<int32_t> level_scan;  // levels + 1: scans [level_scan[l], level_scan[l + 1]) have level l + 1
  std::vector<int64_t> scan_src;    // per scan: byte offset of its entropy-coded bytes in the caller's data
  int64_t o_scan = 0, o_item = 0, o_seg = 0;
  int levels() const { return level_scan.empty() ? 0 : (int)level_scan.size() - 1; }
};

// parses every image (n >= 1) and lays the batch out; throws before anything is written if an image is malformed or
// unsupported or the batch does not fit `caps`.  Progressive files are accepted when caps.max_scans > 0.
DecodePlan plan_decode(const DecoderCaps& caps, const uint8_t* data_host, const int64_t* offsets, const int64_t* sizes, int n,
                       const int64_t* dst_offset, const int64_t* dst_pitch);

// writes the staging image of a plan into dst[0, plan.total)
void stage(const DecodePlan& plan, const uint8_t* data_host, const int64_t* offsets, uint8_t* dst);

// ---------------------------------------------------------------------------------------------------------------------
// encoder

void check_geometry(int32_t h, int32_t w, int32_t sampling);
void check_quality(int32_t quality);
Geo geometry(int32_t h, int32_t w, int32_t sampling);  // of one image; the caller sets n
int64_t padded_pixels(const Geo& g);                   // pixels of one image once padded to whole MCUs
int64_t bound_of(const Geo& g);                        // bytes of one encoded image, at most
void scaled_tables(int quality, uint8_t q[2][64]);     // jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)
// jcmarker.c with libjpeg's defaults: SOI, JFIF APP0, DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, SOS -> o[0, HDR_BYTES)
void build_header(int32_t h, int32_t w, int32_t quality, int32_t sampling, uint8_t* o);

}  // namespace jpeg
}  // namespace mtgv
