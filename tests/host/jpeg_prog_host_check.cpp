// Stand-alone check of the progressive JPEG path's host side (csrc/jpeg_host.cpp: parse_progressive, the plan and the
// staging image of a progressive handle) and of the scan decode the kernels run (csrc/jpeg_prog_decode.h, the same text
// compiled for the host), meant to be built with a host sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mtg-vision_amd/csrc
//       tests/host/jpeg_prog_host_check.cpp mtg-vision_amd/csrc/jpeg_host.cpp -o jpeg_prog_host_check   (one command line)
//   ./jpeg_prog_host_check out_dir a.jpg b.jpg ...
//
// No HIP, no Python.  Every file and every mutant of it (truncations, bytes overwritten in the headers and in the
// entropy-coded data) is parsed from an exact-size heap copy, planned under exact limits, staged into an exact-size
// buffer and decoded, level by level as the launches do, into an exact-size coefficient buffer, each restart segment
// from an exact-size copy of its bytes: an access one element outside any of them is a sanitizer report.  A refusal
// must be an Error or a non-zero status.  Mutants are made of the files whose name starts with m_.  The coefficients
// of every intact progressive file are written to out_dir/<name>.coef (int16, MCU order, 64 per block in natural
// order) for the caller to compare.  Prints the counts; exit status 0 and nothing on stderr means clean.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "jpeg_host.h"
#include "jpeg_prog_decode.h"
#include "jpeg_tables.h"

using namespace mtgv;
using namespace mtgv::jpeg;

namespace {

typedef std::vector<uint8_t> Bytes;

long n_progressive = 0, n_other = 0, n_unsupported = 0, n_invalid = 0, n_plans = 0, n_refused = 0, n_decoded = 0, n_status1 = 0;

#define REQUIRE(cond, ...)                                     \
  do {                                                         \
    if (!(cond)) {                                             \
      fprintf(stderr, "jpeg_prog_host_check: [%s] ", #cond);   \
      fprintf(stderr, __VA_ARGS__);                            \
      fprintf(stderr, " at line %d\n", __LINE__);              \
      exit(1);                                                 \
    }                                                          \
  } while (0)

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

template <class T>
std::unique_ptr<T[]> exact_copy(const T* d, size_t n) {
  std::unique_ptr<T[]> c(new T[n]);
  if (n) memcpy(c.get(), d, n * sizeof(T));
  return c;
}

struct Batch {
  Bytes data;
  std::vector<int64_t> offsets, sizes, dst_offset, dst_pitch;
  int64_t bytes = 0, pixels = 0, scans = 0;
  int n() const { return (int)sizes.size(); }
  void add(const Bytes& f, int h, int w, int ncomp, int hm, int vm, int nscans) {
    offsets.push_back((int64_t)data.size());
    sizes.push_back((int64_t)f.size());
    data.insert(data.end(), f.begin(), f.end());
    dst_offset.push_back(n() == 1 ? 0 : dst_offset.back() + dst_pitch.back() * 65535);
    dst_pitch.push_back(3ll * w);
    bytes += (int64_t)f.size();
    if (ncomp == 1) hm = vm = 1;
    pixels += (int64_t)ceil_div(w, 8 * hm) * 8 * hm * ceil_div(h, 8 * vm) * 8 * vm;
    scans += nscans;
  }
};

// what the launches of a progressive handle trust, beyond what jpeg_host_check verifies for baseline images
void check_plan(const DecoderCaps& caps, const DecodePlan& plan) {
  const int n = plan.n;
  const int64_t nscans = (int64_t)plan.scans.size();
  REQUIRE(nscans <= caps.max_scans && (int64_t)plan.seg_off.size() <= caps.prog_segs, "scan capacity");
  REQUIRE(plan.item_base.size() == (size_t)(nscans ? nscans + 1 : 0) && plan.scan_src.size() == (size_t)nscans, "scan arrays");
  REQUIRE(plan.levels() <= PROG_MAX_LEVELS && (nscans == 0 || plan.level_scan.back() == nscans), "levels");
  REQUIRE((int64_t)plan.tabs.size() <= 4ll * n + 2 * caps.max_scans, "%zu tables", plan.tabs.size());
  REQUIRE(plan.o_scan % 256 == 0 && plan.o_item % 256 == 0 && plan.o_seg % 256 == 0 && plan.o_ecs % 256 == 0, "staging alignment");
  REQUIRE(plan.o_base + (int64_t)plan.bases.size() * 8 <= plan.o_scan && plan.o_scan + nscans * (int64_t)sizeof(ScanDesc) <= plan.o_item &&
              plan.o_item + (int64_t)plan.item_base.size() * 8 <= plan.o_seg && plan.o_seg + (int64_t)plan.seg_off.size() * 4 <= plan.o_ecs &&
              plan.total <= caps.stage,
          "staging layout");
  const int64_t ecs_region = plan.total - plan.o_ecs;
  REQUIRE(ecs_region <= caps.ecs, "entropy-coded region %lld, capacity %lld", (long long)ecs_region, (long long)caps.ecs);
  int nprog = 0;
  for (int i = 0; i < n; ++i) {
    const ImgDesc& D = plan.ds[i];
    nprog += D.prog;
    if (D.prog) REQUIRE(D.nchunks == 0 && D.ntiles == 0 && D.nseg == 0 && D.ecs_len == 0, "image %d: progressive with a stream of its own", i);
    REQUIRE(D.blk0 == plan.bb()[i] && D.nblocks >= 1 && D.blk0 + D.nblocks <= caps.blocks, "image %d: blocks", i);
  }
  REQUIRE(nprog == plan.nprog, "progressive images");
  for (int64_t k = 0; k < nscans; ++k) {
    const ScanDesc& S = plan.scans[k];
    REQUIRE(S.img >= 0 && S.img < n && plan.ds[S.img].prog, "scan %lld: image %d", (long long)k, S.img);
    REQUIRE(k == 0 || plan.scans[k - 1].level <= S.level, "scan %lld: not sorted by level", (long long)k);
    REQUIRE(S.level >= 1 && k >= plan.level_scan[S.level - 1] && k < plan.level_scan[S.level], "scan %lld: level %d", (long long)k, S.level);
    REQUIRE(S.ncomp >= 1 && S.ncomp <= 3 && S.nseg >= 1 && S.ri >= 1 && S.uw >= 1 && S.uh >= 1, "scan %lld: geometry", (long long)k);
    REQUIRE(plan.item_base[k + 1] - plan.item_base[k] == S.nseg, "scan %lld: items", (long long)k);
    REQUIRE(S.ecs >= 0 && S.ecs_len >= 0 && S.ecs + align_up(S.ecs_len, 8) + 8 <= ecs_region, "scan %lld: bytes", (long long)k);
    REQUIRE(S.seg0 >= 0 && S.seg0 + S.nseg + 1 <= (int64_t)plan.seg_off.size(), "scan %lld: segment offsets", (long long)k);
    for (int sg = 0; sg < S.nseg; ++sg)
      REQUIRE(plan.seg_off[S.seg0 + sg] <= plan.seg_off[S.seg0 + sg + 1] && (int64_t)plan.seg_off[S.seg0 + sg + 1] <= S.ecs_len,
              "scan %lld: segment %d", (long long)k, sg);
    const int ntab = S.ss > 0 ? 1 : S.ah == 0 ? S.ncomp : 0;
    for (int j = 0; j < ntab; ++j) REQUIRE(S.tab[j] >= 0 && S.tab[j] < (int)plan.tabs.size(), "scan %lld: table", (long long)k);
    for (int j = 0; j < S.ncomp; ++j)
      REQUIRE(S.comp[j] >= 0 && S.comp[j] < plan.ds[S.img].ncomp && S.slot0[j] >= 0 && S.slot0[j] < plan.ds[S.img].bpm, "scan %lld: component", (long long)k);
  }
}

struct Decoded {
  std::vector<int32_t> status;         // per image; baseline images stay 0 (they are not decoded here)
  std::unique_ptr<int16_t[]> coef;     // exact size
  int64_t nblk = 0;
};

// what prog_zero / prog_scan / prog_finish do, from the staging image alone
Decoded decode_staged(const DecodePlan& plan, const uint8_t* st) {
  const int n = plan.n;
  Decoded o;
  o.status.assign(n, 0);
  o.nblk = plan.bb()[n];
  o.coef.reset(new int16_t[o.nblk * 64]);
  const ImgDesc* ds = (const ImgDesc*)st;
  const HuffTab* tabs = (const HuffTab*)(st + plan.o_tab);
  const ScanDesc* scans = (const ScanDesc*)(st + plan.o_scan);
  const int64_t* item_base = (const int64_t*)(st + plan.o_item);
  const uint32_t* seg_off = (const uint32_t*)(st + plan.o_seg);
  const uint8_t* ecs = st + plan.o_ecs;
  for (int i = 0; i < n; ++i)  // a canary over the baseline images' blocks
    for (int64_t k = 0; k < ds[i].nblocks * 64; ++k) o.coef[ds[i].blk0 * 64 + k] = ds[i].prog ? 0 : 0x7157;
  for (int l = 0; l < plan.levels(); ++l)
    for (int64_t item = plan.item_base[plan.level_scan[l]]; item < plan.item_base[plan.level_scan[l + 1]]; ++item) {
      int64_t k = plan.level_scan[l];
      while (item_base[k + 1] <= item) ++k;
      const ScanDesc& S = scans[k];
      if (o.status[S.img]) continue;
      const int seg = (int)(item - item_base[k]);
      const ImgDesc& D = ds[S.img];
      const HuffTab* tab[3] = {tabs + S.tab[0], tabs + S.tab[1], tabs + S.tab[2]};
      const uint32_t b0 = seg_off[S.seg0 + seg], b1 = seg_off[S.seg0 + seg + 1];
      const auto bytes = exact_copy(ecs + S.ecs + b0, b1 - b0);
      // the image's blocks alone, exact size: a slot outside them is a report
      const auto blocks = exact_copy(o.coef.get() + D.blk0 * 64, (size_t)D.nblocks * 64);
      const std::unique_ptr<int16_t[]> work(new int16_t[64]);
      if (prog_decode_segment(D, S, tab, h_natural, bytes.get(), b1 - b0, seg, blocks.get(), work.get())) o.status[S.img] = 1;
      memcpy(o.coef.get() + D.blk0 * 64, blocks.get(), (size_t)D.nblocks * 64 * sizeof(int16_t));
    }
  for (int i = 0; i < n; ++i)
    if (!ds[i].prog)
      for (int64_t k = 0; k < ds[i].nblocks * 64; ++k) REQUIRE(o.coef[ds[i].blk0 * 64 + k] == 0x7157, "baseline image %d: block data touched", i);
  return o;
}

// plan + stage + decode under the given limits; false if the plan was refused
bool run_batch(const Batch& b, int64_t max_bytes, int64_t max_pixels, int64_t max_scans, Decoded* out = nullptr) {
  const auto data = exact_copy(b.data.data(), b.data.size());
  const DecoderCaps caps = decoder_caps(b.n(), std::max<int64_t>(max_bytes, 1), std::max<int64_t>(max_pixels, 1), std::max<int64_t>(max_scans, 1));
  DecodePlan plan;
  try {
    plan = plan_decode(caps, data.get(), b.offsets.data(), b.sizes.data(), b.n(), b.dst_offset.data(), b.dst_pitch.data());
  } catch (const Error&) {
    ++n_refused;
    return false;
  }
  ++n_plans;
  check_plan(caps, plan);
  std::unique_ptr<uint8_t[]> st(new uint8_t[plan.total]);
  stage(plan, data.get(), b.offsets.data(), st.get());
  for (size_t k = 0; k < plan.scans.size(); ++k)
    REQUIRE(memcmp(st.get() + plan.o_ecs + plan.scans[k].ecs, data.get() + plan.scan_src[k], plan.scans[k].ecs_len) == 0, "scan %zu: staged bytes", k);
  Decoded d = decode_staged(plan, st.get());
  for (int s : d.status) ++(s ? n_status1 : n_decoded);
  if (out) *out = std::move(d);
  return true;
}

// 1 progressive and supported, 0 not progressive, -1 unsupported, -2 invalid
int parse_exact(const Bytes& f, ProgParsed& pp) {
  const auto c = exact_copy(f.data(), f.size());
  try {
    parse_progressive(c.get(), (int64_t)f.size(), pp);
  } catch (const Error&) {
    ++n_invalid;
    return -2;
  }
  if (!pp.progressive) {
    ++n_other;
    return 0;
  }
  REQUIRE(pp.supported == (pp.why.empty() ? 1 : 0), "supported %d, why '%s'", pp.supported, pp.why.c_str());
  ++(pp.supported ? n_progressive : n_unsupported);
  return pp.supported ? 1 : -1;
}

void add_to(Batch& b, const Bytes& f) {  // a supported file of either kind
  ProgParsed pp;
  if (parse_exact(f, pp) == 1) {
    b.add(f, pp.h, pp.w, pp.ncomp, pp.comp[0].h, pp.comp[0].v, (int)pp.scans.size());
    return;
  }
  Parsed p;
  parse(f.data(), (int64_t)f.size(), p);
  REQUIRE(p.supported, "a file that is neither progressive nor baseline: %s", p.why.c_str());
  b.add(f, p.h, p.w, p.ncomp, p.comp[0].h, p.comp[0].v, 0);
}

void one_mutant(const Bytes& m) {
  ProgParsed pp;
  if (parse_exact(m, pp) != 1) return;
  Batch b;
  b.add(m, pp.h, pp.w, pp.ncomp, pp.comp[0].h, pp.comp[0].v, (int)pp.scans.size());
  REQUIRE(run_batch(b, b.bytes, b.pixels, b.scans), "a parsed mutant does not fit its own size");
}

void mutants(const Bytes& f) {
  const size_t lim = std::min<size_t>(f.size(), 700);
  for (size_t cut = 0; cut < f.size(); cut += cut < lim + 8 ? 1 : 41) one_mutant(Bytes(f.begin(), f.begin() + cut));
  static const uint8_t vals[8] = {0x00, 0x01, 0x11, 0x7f, 0xff, 0xc4, 0xda, 0xd9};
  Bytes m = f;
  for (size_t k = 0; k < f.size(); k += k < lim ? 1 : 7) {  // headers densely, then the scans (entropy-coded data, SOS and DHT between them)
    for (size_t v = 0; v < (k < lim ? 8u : 3u); ++v) {
      const uint8_t x = k < lim ? vals[v] : (uint8_t)(v == 0 ? 0x00 : v == 1 ? 0xff : f[k] ^ 0x5a);
      if (f[k] == x) continue;
      m[k] = x;
      one_mutant(m);
    }
    m[k] = f[k];
  }
}

Bytes read_file(const char* name) {
  FILE* f = fopen(name, "rb");
  REQUIRE(f != nullptr, "cannot open %s", name);
  Bytes b;
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + k);
  fclose(f);
  return b;
}

}  // namespace

int main(int argc, char** argv) {
  REQUIRE(argc >= 3, "usage: %s out_dir file.jpg ...", argv[0]);
  const std::string out_dir = argv[1];
  try {
    std::vector<Bytes> files;
    for (int i = 2; i < argc; ++i) files.push_back(read_file(argv[i]));
    Batch all;
    for (int i = 2; i < argc; ++i) {
      const Bytes& f = files[i - 2];
      ProgParsed pp;
      const int kind = parse_exact(f, pp);
      add_to(all, f);
      if (kind != 1) continue;
      Batch b;
      b.add(f, pp.h, pp.w, pp.ncomp, pp.comp[0].h, pp.comp[0].v, (int)pp.scans.size());
      Decoded d;
      REQUIRE(run_batch(b, b.bytes, b.pixels, b.scans, &d) && d.status[0] == 0, "%s: an intact progressive file was refused or did not decode", argv[i]);
      // limits a few bytes, a few pixels or one scan short
      REQUIRE(!run_batch(b, b.bytes - 3, b.pixels, b.scans) && !run_batch(b, b.bytes, b.pixels - 5, b.scans) && !run_batch(b, b.bytes, b.pixels, b.scans - 1),
              "%s: a short limit was accepted", argv[i]);
      const char* base = strrchr(argv[i], '/');
      const std::string name = out_dir + "/" + (base ? base + 1 : argv[i]) + ".coef";
      FILE* o = fopen(name.c_str(), "wb");
      REQUIRE(o != nullptr, "cannot write %s", name.c_str());
      REQUIRE(fwrite(d.coef.get(), sizeof(int16_t), (size_t)d.nblk * 64, o) == (size_t)d.nblk * 64, "short write");
      fclose(o);
    }
    // all files in one ragged batch (baseline ones between them), then the same batch twice over
    Decoded d;
    REQUIRE(run_batch(all, all.bytes, all.pixels, all.scans, &d), "the mixed batch was refused");
    for (int s : d.status) REQUIRE(s == 0, "an image of the mixed batch did not decode");
    for (int i = 2; i < argc; ++i) {  // the mutants of the files named m_*
      const char* base = strrchr(argv[i], '/');
      if (strncmp(base ? base + 1 : argv[i], "m_", 2) == 0) mutants(files[i - 2]);
    }
  } catch (const std::exception& e) {  // every expected refusal is caught where it is provoked
    fprintf(stderr, "jpeg_prog_host_check: unexpected exception: %s\n", e.what());
    return 1;
  }
  REQUIRE(n_plans > 0 && n_refused > 0 && n_status1 > 0, "%ld plans, %ld refused, %ld images with status 1", n_plans, n_refused, n_status1);
  printf("progressive %ld other %ld unsupported %ld invalid %ld (plans %ld, refused %ld, images decoded %ld, status 1 %ld)\n", n_progressive, n_other,
         n_unsupported, n_invalid, n_plans, n_refused, n_decoded, n_status1);
  return 0;
}
