// Stand-alone check of the JPEG codecs' host side (csrc/jpeg_host.cpp), meant to be built with a host sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mtg-vision_amd/csrc
//       tests/host/jpeg_host_check.cpp mtg-vision_amd/csrc/jpeg_host.cpp -o jpeg_host_check   (one command line)
//   ./jpeg_host_check a.jpg b.jpg ...
//
// No HIP, no Python.  Every input and every mutant of it (truncations, single bytes overwritten) is parsed from an
// exact-size heap copy, so a read one byte past the end is seen.  Files the parser supports are planned and staged,
// alone and in batches, into an exact-size heap buffer, under roomy limits and under limits a few bytes / pixels
// short; every plan that is not refused must satisfy the invariants the eleven launches rely on.  A refusal must be
// an Error.  The encoder's header must parse back to what was asked for.  Prints the three parse counts; exit
// status 0 and nothing on stderr means clean.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "jpeg_host.h"
#include "jpeg_tables.h"

using namespace mtgv;
using namespace mtgv::jpeg;

namespace {

typedef std::vector<uint8_t> Bytes;

long n_supported = 0, n_unsupported = 0, n_invalid = 0, n_plans = 0, n_refused = 0;

#define REQUIRE(cond, ...)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      fprintf(stderr, "jpeg_host_check: [%s] ", #cond);      \
      fprintf(stderr, __VA_ARGS__);                          \
      fprintf(stderr, " at line %d\n", __LINE__);            \
      exit(1);                                               \
    }                                                        \
  } while (0)

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

std::unique_ptr<uint8_t[]> exact_copy(const uint8_t* d, size_t n) {
  std::unique_ptr<uint8_t[]> c(new uint8_t[n]);
  if (n) memcpy(c.get(), d, n);
  return c;
}

// 1 supported, 0 unsupported, -1 invalid
int parse_exact(const uint8_t* d, size_t n, Parsed& p) {
  const auto c = exact_copy(d, n);
  try {
    parse(c.get(), (int64_t)n, p);
  } catch (const Error&) {
    ++n_invalid;
    return -1;
  }
  REQUIRE(p.supported == (p.why.empty() ? 1 : 0), "supported %d, why '%s'", p.supported, p.why.c_str());
  ++(p.supported ? n_supported : n_unsupported);
  return p.supported;
}

// pixels of a supported image once padded to whole MCUs
int64_t padded_pixels_of(const Parsed& p) {
  const int hm = p.ncomp == 1 ? 1 : p.comp[0].h, vm = p.ncomp == 1 ? 1 : p.comp[0].v;
  return (int64_t)ceil_div(p.w, 8 * hm) * 8 * hm * ceil_div(p.h, 8 * vm) * 8 * vm;
}

void check_bases(const char* what, const int64_t* b, int n, int64_t cap) {
  REQUIRE(b[0] == 0, "%s base starts at %lld", what, (long long)b[0]);
  for (int i = 0; i < n; ++i) REQUIRE(b[i + 1] >= b[i], "%s base decreases at %d", what, i);
  REQUIRE(b[n] <= cap, "%s base ends at %lld, capacity %lld", what, (long long)b[n], (long long)cap);
}

void check_plan(const DecoderCaps& caps, const DecodePlan& plan, int n) {
  REQUIRE(plan.n == n && (int)plan.ps.size() == n && (int)plan.ds.size() == n && plan.bases.size() == 5 * (size_t)(n + 1), "plan sizes");
  check_bases("chunk", plan.cb(), n, caps.chunks);
  check_bases("block", plan.bb(), n, caps.blocks);
  check_bases("segment", plan.sb(), n, caps.segs);
  check_bases("tile", plan.tb(), n, caps.tiles);
  check_bases("pixel", plan.pb(), n, caps.max_pixels);
  const int64_t ecs_region = plan.total - plan.o_ecs;
  for (int i = 0; i < n; ++i) {
    const ImgDesc& D = plan.ds[i];
    REQUIRE(D.ecs >= 0 && D.ecs_len >= 0 && D.ecs + align_up(D.ecs_len, 8) + 8 <= ecs_region && ecs_region <= caps.ecs,
            "image %d: ecs %lld + %lld outside %lld (capacity %lld)", i, (long long)D.ecs, (long long)D.ecs_len, (long long)ecs_region,
            (long long)caps.ecs);
    REQUIRE(D.ncomp == 1 || D.ncomp == 3, "image %d: %d components", i, D.ncomp);
    int bpm = 0;
    for (int c = 0; c < D.ncomp; ++c) {
      const CompDesc& C = D.c[c];
      REQUIRE(C.plane >= 0 && C.bw >= 1 && C.bh >= 1 && C.plane + 64 * (int64_t)C.bw * C.bh <= caps.plane, "image %d comp %d: plane", i, c);
      REQUIRE(C.dc >= 0 && C.dc < (int)plan.tabs.size() && C.ac >= 0 && C.ac < (int)plan.tabs.size(), "image %d comp %d: table index", i, c);
      bpm += C.h * C.v;
    }
    REQUIRE(bpm == D.bpm && D.bpm >= 1 && D.bpm <= 8, "image %d: %d blocks per MCU, components give %d", i, D.bpm, bpm);
    for (int k = 0; k < D.bpm; ++k) REQUIRE(D.bcomp[k] >= 0 && D.bcomp[k] < D.ncomp, "image %d: MCU slot %d", i, k);
    REQUIRE(D.blk0 == plan.bb()[i] && D.nblocks >= 1 && D.blk0 + D.nblocks <= caps.blocks, "image %d: blocks", i);
    REQUIRE(D.ri >= 1 && D.nseg >= 1 && D.nchunks >= 1 && D.ntiles >= 1, "image %d: ri %d nseg %d nchunks %d ntiles %d", i, D.ri, D.nseg,
            D.nchunks, D.ntiles);
    REQUIRE(D.chunk0 == plan.cb()[i] && D.seg0 == plan.sb()[i] && D.tile0 == plan.tb()[i] && D.pix0 == plan.pb()[i], "image %d: bases", i);
  }
  // staging layout: four regions, 256-aligned, disjoint, inside total <= the staging capacity
  REQUIRE(plan.o_tab % 256 == 0 && plan.o_base % 256 == 0 && plan.o_ecs % 256 == 0, "staging alignment");
  REQUIRE((int64_t)(n * sizeof(ImgDesc)) <= plan.o_tab && plan.o_tab + (int64_t)(plan.tabs.size() * sizeof(HuffTab)) <= plan.o_base &&
              plan.o_base + (int64_t)(plan.bases.size() * 8) <= plan.o_ecs && plan.o_ecs <= plan.total && plan.total <= caps.stage,
          "staging layout %lld %lld %lld %lld, capacity %lld", (long long)plan.o_tab, (long long)plan.o_base, (long long)plan.o_ecs,
          (long long)plan.total, (long long)caps.stage);
}

struct Batch {
  Bytes data;
  std::vector<int64_t> offsets, sizes, dst_offset, dst_pitch;
  int64_t bytes = 0, pixels = 0;
  int n() const { return (int)sizes.size(); }
  void add(const Bytes& f, const Parsed& p) {
    offsets.push_back((int64_t)data.size());
    sizes.push_back((int64_t)f.size());
    data.insert(data.end(), f.begin(), f.end());
    dst_offset.push_back(n() == 1 ? 0 : dst_offset.back() + dst_pitch.back() * 65535);
    dst_pitch.push_back(3ll * p.w);
    bytes += (int64_t)f.size();
    pixels += padded_pixels_of(p);
  }
};

// plan + stage under the given limits, `data` an exact-size copy of b.data; -1 if the plan was refused, else the number
// of Huffman tables
int plan_and_stage(const Batch& b, const uint8_t* data, int64_t max_bytes, int64_t max_pixels) {
  const int64_t mb = std::min<int64_t>(std::max<int64_t>(max_bytes, 1), (1ll << 31) - 1);  // what a handle accepts
  const int64_t mp = std::min<int64_t>(std::max<int64_t>(max_pixels, 1), (1ll << 34) - 1);
  const DecoderCaps caps = decoder_caps(b.n(), mb, mp);
  DecodePlan plan;
  try {
    plan = plan_decode(caps, data, b.offsets.data(), b.sizes.data(), b.n(), b.dst_offset.data(), b.dst_pitch.data());
  } catch (const Error&) {
    ++n_refused;
    return -1;
  }
  ++n_plans;
  check_plan(caps, plan, b.n());
  std::unique_ptr<uint8_t[]> st(new uint8_t[plan.total]);
  stage(plan, data, b.offsets.data(), st.get());
  REQUIRE(memcmp(st.get(), plan.ds.data(), b.n() * sizeof(ImgDesc)) == 0, "staged descriptors");
  for (int i = 0; i < b.n(); ++i) {
    const uint8_t* e = st.get() + plan.o_ecs + plan.ds[i].ecs;
    const int64_t len = plan.ds[i].ecs_len;
    REQUIRE(memcmp(e, data + b.offsets[i] + plan.ps[i].ecs, len) == 0, "image %d: staged entropy-coded bytes", i);
    for (int64_t k = len; k < align_up(len, 8) + 8; ++k) REQUIRE(e[k] == 0, "image %d: staged tail byte %lld", i, (long long)k);
  }
  return (int)plan.tabs.size();
}

int plan_and_stage(const Batch& b, int64_t max_bytes, int64_t max_pixels) {
  return plan_and_stage(b, exact_copy(b.data.data(), b.data.size()).get(), max_bytes, max_pixels);
}

// roomy limits, then limits a few bytes or a few pixels short: each refusal path on its own, `both` or taking turns
int under_limits(const Batch& b, bool both = true) {
  static unsigned turn = 0;
  const auto copy = exact_copy(b.data.data(), b.data.size());
  const uint8_t* d = copy.get();
  const int tabs = plan_and_stage(b, d, b.bytes + 4096, b.pixels + 4096);
  const bool pixels_short = ++turn & 1 && b.pixels < (1ll << 34);
  if (both || !pixels_short)
    REQUIRE(plan_and_stage(b, d, b.bytes - 3, b.pixels + 4096) < 0, "a batch of %lld bytes fits %lld", (long long)b.bytes, (long long)b.bytes - 3);
  if (b.pixels < (1ll << 34) && (both || pixels_short))
    REQUIRE(plan_and_stage(b, d, b.bytes + 4096, b.pixels - 5) < 0, "a batch of %lld pixels fits %lld", (long long)b.pixels, (long long)b.pixels - 5);
  return tabs;
}

void one_mutant(const Bytes& m) {
  Parsed p;
  if (parse_exact(m.data(), m.size(), p) != 1) return;
  Batch b;
  b.add(m, p);
  under_limits(b, false);
}

void mutants(const Bytes& f) {
  const size_t lim = std::min<size_t>(f.size(), 700);
  // every truncation up to 8 bytes past byte 700, then every 97th
  for (size_t cut = 0; cut < f.size(); cut += cut < lim + 8 ? 1 : 97) one_mutant(Bytes(f.begin(), f.begin() + cut));
  // every byte below 700 set to each of these
  static const uint8_t vals[8] = {0x00, 0x01, 0x11, 0x7f, 0xff, 0xc4, 0xda, 0xd9};
  Bytes m = f;
  for (size_t k = 0; k < lim; ++k) {
    for (uint8_t v : vals) {
      if (f[k] == v) continue;
      m[k] = v;
      one_mutant(m);
    }
    m[k] = f[k];
  }
}

void decoder_checks(const std::vector<Bytes>& files) {
  std::vector<int> good;  // indices of supported files
  std::vector<Parsed> ps(files.size());
  for (size_t i = 0; i < files.size(); ++i)
    if (parse_exact(files[i].data(), files[i].size(), ps[i]) == 1) good.push_back((int)i);
  // batches of 1, 2 and 3 files, and the same file three times: as many tables as once
  const int g = (int)good.size();
  for (int k = 0; k < g; ++k) {
    Batch one, two, three, same;
    for (int j = 0; j < 3; ++j) {
      const int a = good[(k + j) % g];
      if (j < 1) one.add(files[a], ps[a]);
      if (j < 2) two.add(files[a], ps[a]);
      three.add(files[a], ps[a]);
      same.add(files[good[k]], ps[good[k]]);
    }
    const int t1 = under_limits(one);
    REQUIRE(t1 >= 2 && t1 <= 4, "an intact supported file was refused or has %d tables", t1);
    const int t2 = under_limits(two), t3 = under_limits(three);
    REQUIRE(t2 >= t1 && t3 >= t2 && t3 <= 12, "tables per batch: %d, %d, %d", t1, t2, t3);
    REQUIRE(under_limits(same) == t1, "the same file three times: tables are not shared");
    // exact limits hold the batch; a pitch one byte short is refused
    REQUIRE(plan_and_stage(three, three.bytes, three.pixels) == t3, "a batch does not fit its own size");
    three.dst_pitch[1] -= 1;
    REQUIRE(plan_and_stage(three, three.bytes + 4096, three.pixels + 4096) < 0, "a short pitch was accepted");
  }
  for (const Bytes& f : files) mutants(f);
}

template <class F>
bool refuses(F&& f) {
  try {
    f();
  } catch (const Error&) {
    return true;
  }
  return false;
}

void encoder_checks() {
  static const int dims[7] = {1, 7, 8, 9, 16, 17, 65535};
  static const int quals[3] = {1, 50, 100};
  static const int samplings[2] = {420, 444};
  for (int h : dims)
    for (int w : dims)
      for (int q : quals)
        for (int s : samplings) {
          check_geometry(h, w, s);
          check_quality(q);
          // HDR_BYTES + EOI in an exact-size buffer: a header one byte longer would be seen
          std::unique_ptr<uint8_t[]> f(new uint8_t[HDR_BYTES + 2]);
          memset(f.get(), 0xAA, HDR_BYTES + 2);
          build_header(h, w, q, s, f.get());
          REQUIRE(f[HDR_BYTES - 2] == 63 && f[HDR_BYTES - 1] == 0 && f[HDR_BYTES] == 0xAA && f[HDR_BYTES + 1] == 0xAA,
                  "header is not %d bytes", HDR_BYTES);
          f[HDR_BYTES] = 0xFF;
          f[HDR_BYTES + 1] = 0xD9;
          Parsed p;
          parse(f.get(), HDR_BYTES + 2, p);
          REQUIRE(p.supported && p.h == h && p.w == w && p.sampling == s && p.ncomp == 3 && p.ecs == HDR_BYTES && p.ecs_len == 0,
                  "header of %dx%d q%d %d parses as %dx%d %d, %d components (%s)", h, w, q, s, p.h, p.w, p.sampling, p.ncomp, p.why.c_str());
          uint8_t qt[2][64];
          scaled_tables(q, qt);
          for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 64; ++k)
              REQUIRE(p.qt[p.comp[c].tq][k] == qt[c ? 1 : 0][k], "quality %d: component %d table entry %d", q, c, k);
          const Geo g = geometry(h, w, s);
          REQUIRE(g.hlen == HDR_BYTES && bound_of(g) >= HDR_BYTES + 2 && padded_pixels(g) >= (int64_t)h * w, "geometry of %dx%d %d", h, w, s);
        }
  REQUIRE(refuses([] { check_geometry(0, 8, 420); }) && refuses([] { check_geometry(8, 65536, 444); }) &&
              refuses([] { check_geometry(8, 8, 422); }) && refuses([] { check_quality(0); }) && refuses([] { check_quality(101); }),
          "an encoder argument outside its range was accepted");
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
  REQUIRE(argc >= 2, "usage: %s file.jpg ...", argv[0]);
  std::vector<Bytes> files;
  for (int i = 1; i < argc; ++i) files.push_back(read_file(argv[i]));
  try {
    decoder_checks(files);
    encoder_checks();
  } catch (const std::exception& e) {  // every expected refusal is caught where it is provoked
    fprintf(stderr, "jpeg_host_check: unexpected exception: %s\n", e.what());
    return 1;
  }
  REQUIRE(n_plans > 0 && n_refused > 0, "%ld plans checked, %ld refused", n_plans, n_refused);
  printf("supported %ld unsupported %ld invalid %ld (plans checked %ld, refused %ld)\n", n_supported, n_unsupported, n_invalid, n_plans, n_refused);
  return 0;
}
