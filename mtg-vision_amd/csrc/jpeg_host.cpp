// Host side of the JPEG codecs: see jpeg_host.h.  Nothing here calls HIP or reports through set_last_error(): failures
// are thrown as Error and the C-ABI wrappers in jpeg.hip / jpeg_enc.hip turn them into a status.
#include "jpeg_host.h"

#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <map>

#include "jpeg_tables.h"

namespace mtgv {
namespace jpeg {

namespace {

[[noreturn]] void bad(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void bad(const char* fmt, ...) {
  char b[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof(b), fmt, ap);
  va_end(ap);
  throw Error(ERR_INVALID, std::string("jpeg: ") + b);
}

void unsupported(Parsed& p, const std::string& why) {
  if (p.why.empty()) p.why = why;
}

inline int be16(const uint8_t* d) { return d[0] << 8 | d[1]; }

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// decoder: marker walk

// canonical codes of a DHT table; false if a code does not fit its length (libjpeg: no all-ones code)
bool huff_codes(const uint8_t* bits, int* maxcode, int* valoff, uint16_t* lut, const uint8_t* val) {
  int code = 0, k = 0;
  if (lut) memset(lut, 0, 512 * sizeof(uint16_t));
  for (int l = 1; l <= 16; ++l) {
    const int first = code, firstk = k;
    for (int j = 0; j < bits[l]; ++j, ++code, ++k) {
      if (lut && l <= 9) {
        const int sh = 9 - l;
        for (int e = 0; e < (1 << sh); ++e) lut[(code << sh) | e] = (uint16_t)(l << 8 | val[k]);
      }
    }
    if (code >= (1 << l)) return false;
    if (maxcode) {
      maxcode[l] = bits[l] ? code - 1 : -1;
      valoff[l] = firstk - first;
    }
    code <<= 1;
  }
  return true;
}

namespace {

// SOF segment s[0, sl) of marker m -> frame fields of p; the first feature outside the subset goes to p.why
// (progressive_ok: SOF2 is not one)
void read_sof(int m, const uint8_t* s, int sl, Parsed& p, bool& sof, bool progressive_ok) {
  if (sof) bad("second SOF marker 0x%02X", m);
  sof = true;
  if (sl < 6) bad("SOF segment too short");
  const int prec = s[0];
  p.h = be16(s + 1);
  p.w = be16(s + 3);
  p.ncomp = s[5];
  if (sl < 6 + 3 * p.ncomp) bad("SOF segment too short for %d components", p.ncomp);
  if (p.w == 0) bad("image width 0");
  for (int c = 0; c < std::min(p.ncomp, 4); ++c) {
    p.comp[c].id = s[6 + 3 * c];
    p.comp[c].h = s[7 + 3 * c] >> 4;
    p.comp[c].v = s[7 + 3 * c] & 15;
    p.comp[c].tq = s[8 + 3 * c];
    if (p.comp[c].h < 1 || p.comp[c].h > 4 || p.comp[c].v < 1 || p.comp[c].v > 4) bad("invalid sampling factors of component %d", c);
    if (p.comp[c].tq > 3) bad("invalid quantisation table index %d", p.comp[c].tq);
  }
  if (m == 0xC2 && progressive_ok) (void)0;
  else if (m == 0xC2 || m == 0xC6) unsupported(p, "progressive JPEG (SOF" + std::to_string(m - 0xC0) + ")");
  else if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) unsupported(p, "lossless JPEG (SOF" + std::to_string(m - 0xC0) + ")");
  else if (m >= 0xC9) unsupported(p, "arithmetic coding (SOF" + std::to_string(m - 0xC0) + ")");
  else if (m == 0xC5) unsupported(p, "hierarchical JPEG (SOF5)");
  if (prec != 8) unsupported(p, std::to_string(prec) + "-bit samples");
  if (p.h == 0) unsupported(p, "height given by a DNL marker");
  if (p.ncomp == 4) unsupported(p, "4 components (CMYK / YCCK)");
  else if (p.ncomp != 1 && p.ncomp != 3) unsupported(p, std::to_string(p.ncomp) + " components");
  if (p.ncomp == 3) {
    const auto& c = p.comp;
    if (c[1].h != 1 || c[1].v != 1 || c[2].h != 1 || c[2].v != 1) unsupported(p, "chroma sampling factors other than 1x1");
    else if (c[0].h == 1 && c[0].v == 1) p.sampling = 444;
    else if (c[0].h == 2 && c[0].v == 1) p.sampling = 422;
    else if (c[0].h == 2 && c[0].v == 2) p.sampling = 420;
    else unsupported(p, "luma sampling " + std::to_string(c[0].h) + "x" + std::to_string(c[0].v));
  } else if (p.ncomp == 1) {
    p.sampling = 400;
  }
}

void read_dqt(const uint8_t* s, int sl, Parsed& p) {
  int o = 0;
  while (o < sl) {
    const int pq = s[o] >> 4, tq = s[o] & 15;
    ++o;
    if (pq > 1 || tq > 3) bad("invalid DQT table %d precision %d", tq, pq);
    if (o + 64 * (pq + 1) > sl) bad("truncated DQT segment");
    for (int k = 0; k < 64; ++k) p.qt[tq][h_natural[k]] = pq ? (uint16_t)be16(s + o + 2 * k) : s[o + k];
    o += 64 * (pq + 1);
    p.qdef[tq] = true;
  }
}

void read_dht(const uint8_t* s, int sl, Parsed& p) {
  int o = 0;
  while (o < sl) {
    if (o + 17 > sl) bad("truncated DHT segment");
    const int tc = s[o] >> 4, th = s[o] & 15;
    if (tc > 1 || th > 3) bad("invalid DHT class %d / index %d", tc, th);
    int total = 0;
    uint8_t bits[17] = {0};
    for (int l = 1; l <= 16; ++l) total += bits[l] = s[o + l];
    if (total > 256) bad("DHT table with %d codes (more than 256)", total);
    if (o + 17 + total > sl) bad("truncated DHT segment");
    if (!huff_codes(bits, nullptr, nullptr, nullptr, nullptr)) bad("bad Huffman table (class %d, index %d): codes do not fit their lengths", tc, th);
    memcpy(p.hbits[tc][th], bits, 17);
    memset(p.hval[tc][th], 0, 256);
    memcpy(p.hval[tc][th], s + o + 17, total);
    if (tc == 0)
      for (int k = 0; k < total; ++k)
        if (p.hval[tc][th][k] > 15) bad("DC Huffman table %d has a symbol %d > 15", th, p.hval[tc][th][k]);
    p.hdef[tc][th] = true;
    o += 17 + total;
  }
}

}  // namespace

// walks the markers of one file; throws ERR_INVALID on malformed input, sets p.why on unsupported input
void parse(const uint8_t* d, int64_t n, Parsed& p) {
  if (d == nullptr || n <= 0) bad("empty input (%lld bytes)", (long long)n);
  if (n < 2 || d[0] != 0xFF || d[1] != 0xD8) bad("no SOI marker at the start");
  int64_t q = 2;
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = -1;
  for (;;) {
    if (q >= n) bad("truncated before SOS (byte %lld)", (long long)q);
    if (d[q] != 0xFF) bad("expected a marker at byte %lld, found 0x%02X", (long long)q, d[q]);
    while (q < n && d[q] == 0xFF) ++q;
    if (q >= n) bad("truncated before SOS");
    const int m = d[q++];
    if (m == 0xD8) bad("second SOI marker at byte %lld", (long long)q - 2);
    if (m == 0xD9) bad("EOI before any SOS: no image data");
    if ((m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
    if (q + 2 > n) bad("truncated marker 0x%02X", m);
    const int len = be16(d + q);
    if (len < 2 || q + len > n) bad("truncated marker segment 0x%02X (length %d, %lld bytes left)", m, len, (long long)(n - q));
    const uint8_t* s = d + q + 2;
    const int sl = len - 2;
    q += len;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      read_sof(m, s, sl, p, sof, false);
    } else if (m == 0xDB) {  // DQT
      read_dqt(s, sl, p);
    } else if (m == 0xC4) {  // DHT
      read_dht(s, sl, p);
    } else if (m == 0xDD) {  // DRI
      if (sl != 2) bad("DRI segment of length %d", len);
      p.ri = be16(s);
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) adobe = true, adobe_transform = s[11];
    } else if (m == 0xDC) {
      unsupported(p, "DNL marker");
    } else if (m == 0xDA) {  // SOS
      if (!sof) bad("SOS before SOF");
      if (sl < 1) bad("SOS segment too short");
      const int ns = s[0];
      if (sl != 4 + 2 * ns || ns < 1 || ns > 4) bad("malformed SOS segment");
      if (ns != p.ncomp) unsupported(p, "non-interleaved scans (" + std::to_string(ns) + " of " + std::to_string(p.ncomp) + " components)");
      for (int j = 0; j < ns && j < p.ncomp && p.ncomp <= 4; ++j) {
        int c = 0;
        while (c < p.ncomp && p.comp[c].id != s[1 + 2 * j]) ++c;
        if (c == p.ncomp) bad("SOS names component %d, absent from SOF", s[1 + 2 * j]);
        if (c != j) unsupported(p, "scan component order differs from the frame's");
        p.comp[c].td = s[2 + 2 * j] >> 4;
        p.comp[c].ta = s[2 + 2 * j] & 15;
        if (p.comp[c].td > 3 || p.comp[c].ta > 3) bad("invalid Huffman table index in SOS");
      }
      const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ah = s[3 + 2 * ns] >> 4, al = s[3 + 2 * ns] & 15;
      if (ss != 0 || se != 63 || ah != 0 || al != 0) unsupported(p, "spectral selection / successive approximation in the scan");
      p.ecs = q;
      break;
    }
    // APPn, COM and every other segment: skipped
  }
  if (p.ncomp == 3 && !jfif && ((adobe && adobe_transform == 0) || (!adobe && p.comp[0].id == 'R' && p.comp[1].id == 'G' && p.comp[2].id == 'B')))
    unsupported(p, "RGB colour space (no YCbCr transform)");
  // end of the entropy-coded segment: the first marker other than RSTn
  int64_t e = p.ecs;
  for (;;) {
    const void* f = memchr(d + e, 0xFF, (size_t)(n - e));
    if (f == nullptr) bad("truncated entropy-coded data (no EOI marker)");
    e = (const uint8_t*)f - d;
    int64_t k = e + 1;
    while (k < n && d[k] == 0xFF) ++k;
    if (k >= n) bad("truncated entropy-coded data (no EOI marker)");
    if (d[k] == 0x00 || (d[k] >= 0xD0 && d[k] <= 0xD7)) {
      e = k + 1;
      continue;
    }
    break;
  }
  p.ecs_len = e - p.ecs;
  // what follows: EOI, or segments after which another scan would be unsupported
  int64_t q2 = e;
  for (;;) {
    while (q2 < n && d[q2] == 0xFF) ++q2;
    if (q2 >= n) bad("truncated after the scan (no EOI marker)");
    const int m = d[q2++];
    if (m == 0xD9) break;
    if (m == 0xDA) {
      unsupported(p, "more than one scan");
      break;
    }
    if (m == 0xDC) unsupported(p, "DNL marker");
    if (q2 + 2 > n) bad("truncated marker 0x%02X after the scan", m);
    const int len = be16(d + q2);
    if (len < 2 || q2 + len > n) bad("truncated marker segment 0x%02X after the scan", m);
    q2 += len;
    if (q2 < n && d[q2] != 0xFF) bad("expected a marker at byte %lld after the scan", (long long)q2);
  }
  if (p.why.empty()) {
    for (int c = 0; c < p.ncomp; ++c) {
      if (!p.qdef[p.comp[c].tq]) bad("component %d uses undefined quantisation table %d", c, p.comp[c].tq);
      if (!p.hdef[0][p.comp[c].td]) bad("component %d uses undefined DC Huffman table %d", c, p.comp[c].td);
      if (!p.hdef[1][p.comp[c].ta]) bad("component %d uses undefined AC Huffman table %d", c, p.comp[c].ta);
    }
    p.supported = 1;
  }
}

// The walk over a progressive file: see jpeg_host.h.  Legality follows T.81 Annex G.1.1.1: a DC scan has Ss = Se = 0 and
// may interleave components, an AC scan has one component and 1 <= Ss <= Se <= 63 and comes after that component's first
// DC scan; the first scan over a coefficient has Ah = 0, every later one Ah = the Al before it and Al = Ah - 1.
void parse_progressive(const uint8_t* d, int64_t n, ProgParsed& pp) {
  pp = ProgParsed();
  if (d == nullptr || n <= 0) bad("empty input (%lld bytes)", (long long)n);
  if (n < 2 || d[0] != 0xFF || d[1] != 0xD8) bad("no SOI marker at the start");
  if (n > 0x7fffffff) bad("file of %lld bytes (2 GiB or more)", (long long)n);
  Parsed st;  // the frame and the tables in force
  int ri = 0;
  bool sof = false, jfif = false, adobe = false;
  int adobe_transform = -1;
  int coef_al[4][64];  // Al of the last scan over each coefficient, -1: none yet
  for (auto& c : coef_al)
    for (int& v : c) v = -1;
  auto finish = [&] {
    pp.h = st.h;
    pp.w = st.w;
    pp.ncomp = st.ncomp;
    pp.sampling = st.sampling;
    for (int c = 0; c < 4; ++c) pp.comp[c] = st.comp[c];
    pp.ri = pp.scans.empty() ? ri : pp.scans[0].ri;
    pp.why = st.why;
    pp.supported = st.why.empty() ? 1 : 0;
  };
  for (int c = 0; c < 4; ++c) st.comp[c] = Parsed::Comp{0, 0, 0, 0, 0, 0};
  int64_t q = 2;
  for (;;) {
    if (q >= n) bad("truncated before EOI (byte %lld)", (long long)q);
    if (d[q] != 0xFF) bad("expected a marker at byte %lld, found 0x%02X", (long long)q, d[q]);
    while (q < n && d[q] == 0xFF) ++q;
    if (q >= n) bad("truncated before EOI");
    const int m = d[q++];
    if (m == 0xD8) bad("second SOI marker at byte %lld", (long long)q - 2);
    if (m == 0xD9) {
      if (pp.scans.empty()) bad("EOI before any SOS: no image data");
      break;
    }
    if ((m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
    if (q + 2 > n) bad("truncated marker 0x%02X", m);
    const int len = be16(d + q);
    if (len < 2 || q + len > n) bad("truncated marker segment 0x%02X (length %d, %lld bytes left)", m, len, (long long)(n - q));
    const uint8_t* s = d + q + 2;
    const int sl = len - 2;
    q += len;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      read_sof(m, s, sl, st, sof, true);
      if (m != 0xC2) return;  // not progressive: parse() has the verdict
      pp.progressive = true;
    } else if (m == 0xDB) {  // DQT
      if (!pp.scans.empty()) unsupported(st, "DQT marker between scans");
      read_dqt(s, sl, st);
    } else if (m == 0xC4) {  // DHT
      read_dht(s, sl, st);
    } else if (m == 0xDD) {  // DRI
      if (sl != 2) bad("DRI segment of length %d", len);
      ri = be16(s);
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) adobe = true, adobe_transform = s[11];
    } else if (m == 0xDC) {
      unsupported(st, "DNL marker");
    } else if (m == 0xDA) {  // SOS
      if (!sof) bad("SOS before SOF");
      if (!st.why.empty()) {  // a frame outside the subset: its scans are not walked
        finish();
        return;
      }
      const int k = (int)pp.scans.size();  // number of this scan
      if (sl < 1) bad("SOS segment too short");
      const int ns = s[0];
      if (sl != 4 + 2 * ns || ns < 1 || ns > 4) bad("malformed SOS segment");
      ProgScan sc;
      sc.ns = ns;
      int td[4] = {0, 0, 0, 0}, ta[4] = {0, 0, 0, 0};
      for (int j = 0; j < ns; ++j) {
        int c = 0;
        while (c < st.ncomp && st.comp[c].id != s[1 + 2 * j]) ++c;
        if (c == st.ncomp) bad("SOS names component %d, absent from SOF", s[1 + 2 * j]);
        if (j > 0 && c <= sc.comp[j - 1]) bad("SOS of scan %d: components not in the frame's order", k);
        sc.comp[j] = c;
        td[j] = s[2 + 2 * j] >> 4;
        ta[j] = s[2 + 2 * j] & 15;
        if (td[j] > 3 || ta[j] > 3) bad("invalid Huffman table index in SOS");
      }
      sc.ss = s[1 + 2 * ns];
      sc.se = s[2 + 2 * ns];
      sc.ah = s[3 + 2 * ns] >> 4;
      sc.al = s[3 + 2 * ns] & 15;
      sc.ri = ri;
      if (sc.ss > sc.se || sc.se > 63 || (sc.ss == 0 && sc.se != 0))
        bad("SOS of scan %d: illegal spectral selection Ss %d Se %d", k, sc.ss, sc.se);
      if (sc.ss > 0 && ns != 1) bad("SOS of scan %d: an AC scan (Ss %d) with %d components", k, sc.ss, ns);
      if (sc.al > 13 || sc.ah > 13 || (sc.ah != 0 && sc.al != sc.ah - 1))
        bad("SOS of scan %d: illegal successive approximation Ah %d Al %d", k, sc.ah, sc.al);
      for (int j = 0; j < ns; ++j) {
        int* ca = coef_al[sc.comp[j]];
        if (sc.ss > 0 && ca[0] < 0) bad("SOS of scan %d: AC scan of component %d before its first DC scan", k, sc.comp[j]);
        for (int z = sc.ss; z <= sc.se; ++z) {
          if (sc.ah == 0 ? ca[z] != -1 : ca[z] != sc.ah)
            bad("SOS of scan %d: illegal scan script: Ah %d over coefficient %d of component %d, which the scans before left at Al %d", k,
                sc.ah, z, sc.comp[j], ca[z]);
          ca[z] = sc.al;
        }
      }
      if (pp.scans.empty()) {
        for (int c = 0; c < st.ncomp; ++c)
          if (!st.qdef[st.comp[c].tq]) bad("component %d uses undefined quantisation table %d", c, st.comp[c].tq);
        memcpy(pp.qt, st.qt, sizeof(pp.qt));
      }
      if (sc.ah == 0 || sc.ss > 0) {  // a DC refinement scan carries raw bits only
        const int tc = sc.ss > 0 ? 1 : 0;
        for (int j = 0; j < ns; ++j) {
          const int th = tc ? ta[j] : td[j];
          if (!st.hdef[tc][th]) bad("SOS of scan %d: undefined %s Huffman table %d", k, tc ? "AC" : "DC", th);
          ProgScan::Tab t;
          memcpy(t.bits, st.hbits[tc][th], 17);
          memcpy(t.val, st.hval[tc][th], 256);
          sc.tab.push_back(t);
        }
      }
      // the entropy-coded bytes: up to the first marker other than RSTn
      sc.ecs = q;
      int64_t e = q;
      int nrst = 0;
      for (;;) {
        const void* f = memchr(d + e, 0xFF, (size_t)(n - e));
        if (f == nullptr) bad("truncated entropy-coded data of scan %d (no EOI marker)", k);
        e = (const uint8_t*)f - d;
        int64_t x = e + 1;
        while (x < n && d[x] == 0xFF) ++x;
        if (x >= n) bad("truncated entropy-coded data of scan %d (no EOI marker)", k);
        if (d[x] == 0x00) {
          e = x + 1;
          continue;
        }
        if (d[x] >= 0xD0 && d[x] <= 0xD7) {
          if (d[x] - 0xD0 != (nrst & 7)) sc.rst_in_order = false;
          ++nrst;
          e = x + 1;
          sc.rst.push_back((uint32_t)(e - sc.ecs));
          continue;
        }
        break;
      }
      sc.ecs_len = e - sc.ecs;
      q = e;
      pp.scans.push_back(std::move(sc));
    }
    // APPn, COM and every other segment: skipped
  }
  if (!sof) bad("EOI before SOF");
  for (int c = 0; c < st.ncomp && c < 4 && st.why.empty(); ++c)
    for (int z = 0; z < 64; ++z)
      if (coef_al[c][z] != 0) {
        unsupported(st, "incomplete progression: coefficient " + std::to_string(z) + " of component " + std::to_string(c) +
                            (coef_al[c][z] < 0 ? " is in no scan" : " is left at Al " + std::to_string(coef_al[c][z])));
        break;
      }
  if (st.ncomp == 3 && !jfif && ((adobe && adobe_transform == 0) || (!adobe && st.comp[0].id == 'R' && st.comp[1].id == 'G' && st.comp[2].id == 'B')))
    unsupported(st, "RGB colour space (no YCbCr transform)");
  finish();
}

// ---------------------------------------------------------------------------------------------------------------------
// decoder: capacities, the plan of one batch, the staging image

DecoderCaps decoder_caps(int max_images, int64_t max_bytes, int64_t max_pixels) {
  DecoderCaps c{};
  c.max_images = max_images;
  c.max_bytes = max_bytes;
  c.max_pixels = max_pixels;
  const int64_t n = max_images;
  c.chunks = max_bytes / CHUNK_BYTES + n;
  c.tiles = max_bytes / TILE_BYTES + n;
  c.segs = max_bytes / 2 + n;
  c.blocks = 3 * ceil_div64(max_pixels, 64);
  c.plane = 3 * max_pixels;
  c.ecs = max_bytes + 16 * n;
  // four Huffman tables per image: a frame that names six distinct ones can overflow this, and plan_decode refuses it
  c.stage = align_up(n * (int64_t)sizeof(ImgDesc), 256) + align_up(4 * n * (int64_t)sizeof(HuffTab), 256) +
            align_up(5 * (n + 1) * 8, 256) + c.ecs + 256;
  return c;
}

DecoderCaps decoder_caps(int max_images, int64_t max_bytes, int64_t max_pixels, int64_t max_scans) {
  DecoderCaps c = decoder_caps(max_images, max_bytes, max_pixels);
  const int64_t n = max_images;
  c.max_scans = max_scans;
  // a restart segment is at least its two marker bytes; one closing entry per scan
  c.prog_segs = max_bytes / 2 + 2 * max_scans;
  c.ecs += 16 * max_scans;
  // two more Huffman tables per scan (Pillow's ten-scan script uses eight per image)
  c.stage = align_up(n * (int64_t)sizeof(ImgDesc), 256) + align_up((4 * n + 2 * max_scans) * (int64_t)sizeof(HuffTab), 256) +
            align_up(5 * (n + 1) * 8, 256) + align_up(max_scans * (int64_t)sizeof(ScanDesc), 256) + align_up((max_scans + 1) * 8, 256) +
            align_up(c.prog_segs * 4, 256) + c.ecs + 256;
  return c;
}

DecodePlan plan_decode(const DecoderCaps& caps, const uint8_t* data_host, const int64_t* offsets, const int64_t* sizes, int n,
                       const int64_t* dst_offset, const int64_t* dst_pitch) {
  DecodePlan plan;
  plan.n = n;
  // ---- parse every image before anything is laid out
  std::vector<Parsed>& ps = plan.ps = std::vector<Parsed>(n);
  int64_t in_bytes = 0, pix = 0, nscans = 0;
  for (int i = 0; i < n; ++i) {
    MTGV_CHECK(sizes[i] >= 0 && offsets[i] >= 0, ERR_INVALID, "jpeg: image %d: negative offset or size", i);
    try {
      parse(data_host + offsets[i], sizes[i], ps[i]);
    } catch (const Error& e) {
      throw Error(e.code, std::string(e.what()) + " (image " + std::to_string(i) + ")");
    }
    if (!ps[i].supported && caps.max_scans > 0) {  // a handle that takes progressive files: the second walk
      if (plan.pps.empty()) plan.pps = std::vector<ProgParsed>(n);
      ProgParsed& pp = plan.pps[i];
      try {
        parse_progressive(data_host + offsets[i], sizes[i], pp);
      } catch (const Error& e) {
        throw Error(e.code, std::string(e.what()) + " (image " + std::to_string(i) + ")");
      }
      if (pp.progressive) {
        MTGV_CHECK(pp.supported, ERR_INVALID, "jpeg: image %d unsupported: %s", i, pp.why.c_str());
        ++plan.nprog;
        nscans += (int64_t)pp.scans.size();
      }
    }
    const bool prog_i = plan.nprog > 0 && plan.pps[i].progressive;
    MTGV_CHECK(ps[i].supported || prog_i, ERR_INVALID, "jpeg: image %d unsupported: %s", i, ps[i].why.c_str());
    in_bytes += sizes[i];
    MTGV_CHECK(dst_pitch[i] >= 3ll * ps[i].w && dst_offset[i] >= 0, ERR_INVALID, "jpeg: image %d: pitch %lld < 3 * width %d", i,
               (long long)dst_pitch[i], ps[i].w);
  }
  MTGV_CHECK(in_bytes <= caps.max_bytes, ERR_INVALID, "jpeg: batch of %lld bytes, the decoder holds at most %lld", (long long)in_bytes,
             (long long)caps.max_bytes);
  MTGV_CHECK(nscans <= caps.max_scans, ERR_INVALID, "jpeg: batch of %lld progressive scans, the decoder was created for %lld", (long long)nscans,
             (long long)caps.max_scans);
  // ---- descriptors, Huffman tables (deduplicated), ragged bases
  std::vector<ImgDesc>& ds = plan.ds = std::vector<ImgDesc>(n);
  std::vector<HuffTab>& tabs = plan.tabs;
  std::map<std::string, int> tab_ix;
  plan.bases = std::vector<int64_t>(5 * (size_t)(n + 1), 0);
  int64_t* cb = plan.bases.data();
  int64_t* bb = cb + (n + 1);
  int64_t* sb = bb + (n + 1);
  int64_t* tb = sb + (n + 1);
  int64_t* pb = tb + (n + 1);
  int64_t ecs_off = 0, plane_off = 0;
  auto table = [&](const uint8_t* bits, const uint8_t* val) {
    std::string key((const char*)bits, 17);
    key.append((const char*)val, 256);
    auto it = tab_ix.find(key);
    if (it != tab_ix.end()) return it->second;
    HuffTab t;
    memset(&t, 0, sizeof(t));
    memcpy(t.val, val, 256);
    huff_codes(bits, t.maxcode, t.valoff, t.lut, val);
    t.maxcode[0] = -1;
    tabs.push_back(t);
    return tab_ix[key] = (int)tabs.size() - 1;
  };
  for (int i = 0; i < n; ++i) {
    const Parsed& p = ps[i];
    ImgDesc& D = ds[i];
    memset(&D, 0, sizeof(D));
    D.h = p.h;
    D.w = p.w;
    D.ncomp = p.ncomp;
    D.mode = p.ncomp == 1 ? 0 : p.sampling == 444 ? 1 : p.sampling == 422 ? 2 : 3;
    const int hm = p.ncomp == 1 ? 1 : p.comp[0].h, vm = p.ncomp == 1 ? 1 : p.comp[0].v;
    D.mcux = ceil_div(p.w, 8 * hm);
    D.mcuy = ceil_div(p.h, 8 * vm);
    const int64_t nmcu = (int64_t)D.mcux * D.mcuy;
    const bool prog = plan.nprog > 0 && plan.pps[i].progressive;
    D.prog = prog ? 1 : 0;
    D.ri = p.ri && !prog ? p.ri : (int)std::min<int64_t>(nmcu, 1 << 30);
    D.nseg = prog ? 0 : (int)ceil_div64(nmcu, D.ri);
    MTGV_CHECK(prog || 2 * (int64_t)(D.nseg - 1) <= p.ecs_len, ERR_INVALID,
               "jpeg: image %d: %d restart intervals cannot fit in %lld bytes of entropy-coded data", i, D.nseg, (long long)p.ecs_len);
    D.bpm = 0;
    for (int c = 0; c < p.ncomp; ++c) {
      const int ch = p.ncomp == 1 ? 1 : p.comp[c].h, cv = p.ncomp == 1 ? 1 : p.comp[c].v;
      CompDesc& C = D.c[c];
      memcpy(C.q, p.qt[p.comp[c].tq], sizeof(C.q));
      C.dc = prog ? 0 : table(p.hbits[0][p.comp[c].td], p.hval[0][p.comp[c].td]);  // a progressive scan names its own
      C.ac = prog ? 0 : table(p.hbits[1][p.comp[c].ta], p.hval[1][p.comp[c].ta]);
      C.h = ch;
      C.v = cv;
      C.bw = D.mcux * ch;
      C.bh = D.mcuy * cv;
      C.plane = plane_off;
      plane_off += (int64_t)C.bw * 8 * C.bh * 8;
      for (int y = 0; y < cv; ++y)
        for (int x = 0; x < ch; ++x, ++D.bpm) {
          D.bcomp[D.bpm] = (int8_t)c;
          D.bdx[D.bpm] = (int8_t)x;
          D.bdy[D.bpm] = (int8_t)y;
        }
    }
    D.nblocks = nmcu * D.bpm;
    D.ecs = ecs_off;
    D.ecs_len = prog ? 0 : p.ecs_len;
    if (!prog) ecs_off += align_up(p.ecs_len, 8) + 8;
    D.nchunks = prog ? 0 : (int)std::max<int64_t>(1, ceil_div64(p.ecs_len, CHUNK_BYTES));
    D.ntiles = prog ? 0 : (int)std::max<int64_t>(1, ceil_div64(p.ecs_len, TILE_BYTES));
    D.chunk0 = cb[i];
    D.seg0 = sb[i];
    D.tile0 = tb[i];
    D.blk0 = bb[i];
    D.pix0 = pb[i];
    D.dst_off = dst_offset[i];
    D.pitch = dst_pitch[i];
    cb[i + 1] = cb[i] + D.nchunks;
    bb[i + 1] = bb[i] + D.nblocks;
    sb[i + 1] = sb[i] + D.nseg;
    tb[i + 1] = tb[i] + D.ntiles;
    pb[i + 1] = pb[i] + (int64_t)p.h * p.w;
    pix += (int64_t)D.mcux * 8 * hm * D.mcuy * 8 * vm;
  }
  MTGV_CHECK(pix <= caps.max_pixels, ERR_INVALID, "jpeg: batch needs %lld pixels padded to whole MCUs, the decoder holds %lld",
             (long long)pix, (long long)caps.max_pixels);
  // ---- progressive images: one record per scan, its restart segments, its level
  struct Rec {
    ScanDesc s;
    int64_t src;
  };
  std::vector<Rec> recs;
  int levels = 0;
  for (int i = 0; i < n && plan.nprog > 0; ++i) {
    const ProgParsed& pp = plan.pps[i];
    if (!pp.progressive) continue;
    const ImgDesc& D = ds[i];
    const int hmax = pp.ncomp == 1 ? 1 : pp.comp[0].h, vmax = pp.ncomp == 1 ? 1 : pp.comp[0].v;
    const size_t first = recs.size();
    for (const ProgScan& sc : pp.scans) {
      Rec r;
      ScanDesc& S = r.s;
      memset(&S, 0, sizeof(S));
      S.img = i;
      S.ncomp = sc.ns;
      MTGV_CHECK(sc.ns >= 1 && sc.ns <= 3, ERR_INVALID, "jpeg: image %d: a scan of %d components", i, sc.ns);
      for (int j = 0; j < sc.ns; ++j) {
        S.comp[j] = (int8_t)sc.comp[j];
        int slot = 0;
        while (slot < D.bpm && D.bcomp[slot] != sc.comp[j]) ++slot;
        S.slot0[j] = (int8_t)slot;
      }
      for (size_t j = 0; j < sc.tab.size() && j < 4; ++j) S.tab[j] = table(sc.tab[j].bits, sc.tab[j].val);
      S.ss = sc.ss;
      S.se = sc.se;
      S.ah = sc.ah;
      S.al = sc.al;
      if (sc.ns > 1) {  // interleaved: MCUs
        S.uw = D.mcux;
        S.uh = D.mcuy;
      } else {  // the component's own grid
        const int ch = pp.ncomp == 1 ? 1 : pp.comp[sc.comp[0]].h, cv = pp.ncomp == 1 ? 1 : pp.comp[sc.comp[0]].v;
        S.uw = ceil_div(ceil_div(pp.w * ch, hmax), 8);
        S.uh = ceil_div(ceil_div(pp.h * cv, vmax), 8);
      }
      const int64_t units = (int64_t)S.uw * S.uh;
      S.ri = (int)(sc.ri && sc.ri < units ? sc.ri : std::min<int64_t>(units, 1 << 30));
      S.nseg = (int)ceil_div64(units, S.ri);
      S.bad = (int64_t)sc.rst.size() != S.nseg - 1 || !sc.rst_in_order;
      if (S.bad) S.nseg = 1;
      S.ecs = ecs_off;
      S.ecs_len = sc.ecs_len;
      ecs_off += align_up(sc.ecs_len, 8) + 8;
      S.seg0 = (int64_t)plan.seg_off.size();
      plan.seg_off.push_back(0);
      if (!S.bad) plan.seg_off.insert(plan.seg_off.end(), sc.rst.begin(), sc.rst.end());
      plan.seg_off.push_back((uint32_t)sc.ecs_len);
      // the level: after every earlier scan that shares a component and overlaps the band
      S.level = 1;
      for (size_t a = first; a < recs.size(); ++a) {
        const ScanDesc& A = recs[a].s;
        bool shares = false;
        for (int x = 0; x < A.ncomp; ++x)
          for (int y = 0; y < S.ncomp; ++y) shares |= A.comp[x] == S.comp[y];
        if (shares && A.ss <= S.se && S.ss <= A.se) S.level = std::max(S.level, A.level + 1);
      }
      levels = std::max(levels, S.level);
      r.src = offsets[i] + sc.ecs;
      recs.push_back(r);
    }
  }
  MTGV_CHECK(levels <= PROG_MAX_LEVELS, ERR_INVALID, "jpeg: a chain of %d dependent scans, at most %d are decoded", levels, PROG_MAX_LEVELS);
  if (!recs.empty()) {
    std::stable_sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.s.level < b.s.level; });
    plan.item_base.push_back(0);
    plan.level_scan.assign((size_t)levels + 1, 0);
    for (const Rec& r : recs) {
      plan.scans.push_back(r.s);
      plan.scan_src.push_back(r.src);
      plan.item_base.push_back(plan.item_base.back() + r.s.nseg);
      plan.level_scan[r.s.level] = (int32_t)plan.scans.size();
    }
    for (int l = 1; l <= levels; ++l) plan.level_scan[l] = std::max(plan.level_scan[l], plan.level_scan[l - 1]);
  }
  MTGV_CHECK((int64_t)plan.seg_off.size() <= caps.prog_segs && (int64_t)tabs.size() <= 4 * (int64_t)n + 2 * caps.max_scans, ERR_INVALID,
             "jpeg: batch exceeds the decoder's workspace");
  MTGV_CHECK(bb[n] <= caps.blocks && plane_off <= caps.plane && cb[n] <= caps.chunks && tb[n] <= caps.tiles && sb[n] <= caps.segs &&
                 ecs_off <= caps.ecs,
             ERR_INVALID, "jpeg: batch exceeds the decoder's workspace");
  // ---- staging layout: descriptors | tables | bases | entropy-coded bytes
  plan.o_tab = align_up((int64_t)n * sizeof(ImgDesc), 256);
  plan.o_base = plan.o_tab + align_up((int64_t)tabs.size() * sizeof(HuffTab), 256);
  plan.o_scan = plan.o_base + align_up((int64_t)plan.bases.size() * 8, 256);
  plan.o_item = plan.o_scan + align_up((int64_t)plan.scans.size() * sizeof(ScanDesc), 256);
  plan.o_seg = plan.o_item + align_up((int64_t)plan.item_base.size() * 8, 256);
  plan.o_ecs = plan.o_seg + align_up((int64_t)plan.seg_off.size() * 4, 256);
  plan.total = plan.o_ecs + ecs_off;
  MTGV_CHECK(plan.total <= caps.stage, ERR_RUNTIME, "jpeg: staging overflow (%lld > %lld)", (long long)plan.total, (long long)caps.stage);
  return plan;
}

void stage(const DecodePlan& plan, const uint8_t* data_host, const int64_t* offsets, uint8_t* dst) {
  const std::vector<ImgDesc>& ds = plan.ds;
  memcpy(dst, ds.data(), ds.size() * sizeof(ImgDesc));
  memcpy(dst + plan.o_tab, plan.tabs.data(), plan.tabs.size() * sizeof(HuffTab));
  memcpy(dst + plan.o_base, plan.bases.data(), plan.bases.size() * 8);
  if (!plan.scans.empty()) {
    memcpy(dst + plan.o_scan, plan.scans.data(), plan.scans.size() * sizeof(ScanDesc));
    memcpy(dst + plan.o_item, plan.item_base.data(), plan.item_base.size() * 8);
    memcpy(dst + plan.o_seg, plan.seg_off.data(), plan.seg_off.size() * 4);
    for (size_t k = 0; k < plan.scans.size(); ++k) {
      const ScanDesc& S = plan.scans[k];
      uint8_t* e = dst + plan.o_ecs + S.ecs;
      memcpy(e, data_host + plan.scan_src[k], S.ecs_len);
      memset(e + S.ecs_len, 0, align_up(S.ecs_len, 8) + 8 - S.ecs_len);
    }
  }
  for (int i = 0; i < plan.n; ++i) {
    if (ds[i].prog) continue;
    const Parsed& p = plan.ps[i];
    uint8_t* e = dst + plan.o_ecs + ds[i].ecs;
    memcpy(e, data_host + offsets[i] + p.ecs, p.ecs_len);
    memset(e + p.ecs_len, 0, align_up(p.ecs_len, 8) + 8 - p.ecs_len);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// encoder

void check_geometry(int32_t h, int32_t w, int32_t sampling) {
  MTGV_CHECK(h >= 1 && w >= 1 && h <= 65535 && w <= 65535, ERR_INVALID, "jpeg: image size %dx%d outside 1..65535", h, w);
  MTGV_CHECK(sampling == 420 || sampling == 444, ERR_INVALID, "jpeg: sampling %d not supported (420 or 444)", sampling);
}

void check_quality(int32_t quality) { MTGV_CHECK(quality >= 1 && quality <= 100, ERR_INVALID, "jpeg: quality %d outside 1..100", quality); }

Geo geometry(int32_t h, int32_t w, int32_t sampling) {
  Geo g{};
  g.h = h;
  g.w = w;
  g.s420 = sampling == 420;
  g.bpm = g.s420 ? 6 : 3;
  const int mcu = g.s420 ? 16 : 8;
  g.mcux = ceil_div(w, mcu);
  const int mcuy = ceil_div(h, mcu);
  g.wb = ceil_div(w, 8);
  g.hb = ceil_div(h, 8);
  g.bpi = (int64_t)g.mcux * mcuy * g.bpm;
  const int64_t ebytes = ceil_div64(g.bpi * MAX_BLOCK_BITS, 8);  // entropy-coded bytes before stuffing, at most
  g.tpi = (int)ceil_div64(ebytes, TILE);
  g.words = (int64_t)g.tpi * (TILE / 4);
  g.hlen = HDR_BYTES;
  return g;
}

// pixels of one image once padded to whole MCUs
int64_t padded_pixels(const Geo& g) { return g.bpi / g.bpm * (g.s420 ? 256 : 64); }

int64_t bound_of(const Geo& g) { return HDR_BYTES + 2 * ceil_div64(g.bpi * MAX_BLOCK_BITS, 8) + 2; }

void scaled_tables(int quality, uint8_t q[2][64]) {  // jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) q[t][k] = (uint8_t)std::min(std::max((k_basic_q[t][k] * scale + 50) / 100, 1), 255);
}

// jcmarker.c with libjpeg's defaults: SOI, JFIF APP0, DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, SOS
void build_header(int32_t h, int32_t w, int32_t quality, int32_t sampling, uint8_t* o) {
  uint8_t q[2][64];
  scaled_tables(quality, q);
  int p = 0;
  auto b1 = [&](int v) { o[p++] = (uint8_t)v; };
  auto b2 = [&](int v) {
    b1(v >> 8);
    b1(v & 255);
  };
  b2(0xFFD8);
  b2(0xFFE0);
  b2(16);
  for (char c : {'J', 'F', 'I', 'F', '\0'}) b1(c);
  b1(1), b1(1), b1(0), b2(1), b2(1), b1(0), b1(0);  // version 1.01, units 0, density 1 x 1, no thumbnail
  for (int t = 0; t < 2; ++t) {
    b2(0xFFDB);
    b2(67);
    b1(t);
    for (int k = 0; k < 64; ++k) b1(q[t][h_natural[k]]);
  }
  b2(0xFFC0);
  b2(17);
  b1(8), b2(h), b2(w), b1(3);
  b1(1), b1(sampling == 420 ? 0x22 : 0x11), b1(0);
  b1(2), b1(0x11), b1(1);
  b1(3), b1(0x11), b1(1);
  for (int t = 0; t < 4; ++t) {  // DC0, AC0, DC1, AC1
    const int c = t >> 1, ac = t & 1, nv = ac ? 162 : 12;
    b2(0xFFC4);
    b2(2 + 17 + nv);
    b1(ac << 4 | c);
    for (int l = 1; l <= 16; ++l) b1(k_bits[t][l]);
    for (int k = 0; k < nv; ++k) b1(ac ? k_val_ac[c][k] : k_val_dc[k]);
  }
  b2(0xFFDA);
  b2(12);
  b1(3);
  b1(1), b1(0x00), b1(2), b1(0x11), b1(3), b1(0x11);
  b1(0), b1(63), b1(0);
  if (p != HDR_BYTES) throw Error(ERR_RUNTIME, "jpeg: header of " + std::to_string(p) + " bytes");
}

}  // namespace jpeg
}  // namespace mtgv
