// Entropy decode of one restart segment of one scan of a progressive JPEG (T.81 Annex G, the semantics of libjpeg's
// jdphuff.c): DC first / DC refinement / AC first / AC refinement, into int16 coefficient blocks in MCU order.
//
// One definition for both sides: jpeg_prog.hip runs it on the device (one decoding lane per work item), the
// stand-alone host check (tests/host/jpeg_prog_host_check.cpp) runs the same text under a host sanitizer.  No HIP
// header: MTGV_HD is `__host__ __device__` under hipcc and empty under a plain host compiler.
//
// Bounds the caller can rely on.  The reader never loads a byte outside data[0, len).  The block loop runs over the
// segment's own units, the coefficient loops over [Ss, Se]; every block slot is checked against the image's block
// count and every table index against the table before it is used.  A code that is not in the table, a run past Se,
// a segment whose bits end before its blocks are covered and an EOB run that outlives the segment return 1; nothing
// is written outside the image's own blocks.
#pragma once

#include <stdint.h>

#include "jpeg_desc.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define MTGV_HD __host__ __device__
#else
#define MTGV_HD
#endif
#if defined(__clang__)
#define MTGV_UNROLL _Pragma("unroll")
#else
#define MTGV_UNROLL
#endif

namespace mtgv {
namespace jpeg {

// Bit reader over entropy-coded bytes with the stuffing still in place: 0xFF 0x00 is the byte 0xFF, 0xFF followed by
// anything else (an RSTn marker: the end of the segment) or the end of the data feeds zero bits from there on, counted
// in `fake`.  Zero bits looked at are harmless; once one has been consumed, overrun() holds.
struct ProgBits {
  const uint8_t* p;
  uint32_t pos, len;
  uint64_t acc;  // the low `cnt` bits are unread, most significant first
  int cnt, fake;
};

MTGV_HD inline void prog_bits_init(ProgBits& b, const uint8_t* p, uint32_t len) {
  b.p = p;
  b.pos = 0;
  b.len = len;
  b.acc = 0;
  b.cnt = 0;
  b.fake = 0;
}

MTGV_HD inline void prog_bits_fill(ProgBits& b) {
  if (b.cnt <= 32 && b.pos + 4 <= b.len) {  // four bytes in one load, if none of them is 0xFF
    uint32_t v;
    __builtin_memcpy(&v, b.p + b.pos, 4);
    if ((((v ^ 0xFFFFFFFFu) - 0x01010101u) & ~(v ^ 0xFFFFFFFFu) & 0x80808080u) == 0) {
      b.acc = b.acc << 32 | __builtin_bswap32(v);
      b.cnt += 32;
      b.pos += 4;
      return;
    }
  }
  while (b.cnt <= 56) {
    uint32_t v = 0;
    bool real = false;
    if (b.pos < b.len) {
      v = b.p[b.pos];
      if (v != 0xFF) {
        ++b.pos;
        real = true;
      } else if (b.pos + 1 < b.len && b.p[b.pos + 1] == 0x00) {
        b.pos += 2;
        real = true;
      } else {
        b.pos = b.len;  // a marker, or a lone 0xFF at the end: no more data
        v = 0;
      }
    }
    if (!real && b.fake < (1 << 20)) b.fake += 8;
    b.acc = b.acc << 8 | v;
    b.cnt += 8;
  }
}

MTGV_HD inline bool prog_bits_overrun(const ProgBits& b) { return b.cnt < b.fake; }

MTGV_HD inline uint32_t prog_get_bits(ProgBits& b, int n) {  // n in 0..16
  if (b.cnt < n) prog_bits_fill(b);
  b.cnt -= n;
  return (uint32_t)(b.acc >> b.cnt) & ((1u << n) - 1u);
}

// next Huffman symbol, -1 if no code of the table matches
MTGV_HD inline int prog_huff(ProgBits& b, const HuffTab* t) {
  if (b.cnt < 16) prog_bits_fill(b);
  const uint32_t look = (uint32_t)(b.acc >> (b.cnt - 16)) & 0xFFFFu;
  const uint32_t e = t->lut[look >> 7];
  if (e) {
    b.cnt -= (int)(e >> 8);
    return (int)(e & 0xFF);
  }
  int len = 10;
  while (len <= 16 && (int32_t)(look >> (16 - len)) > t->maxcode[len]) ++len;
  if (len > 16) return -1;
  const int32_t ix = (int32_t)(look >> (16 - len)) + t->valoff[len];
  if (ix < 0 || ix > 255) return -1;
  b.cnt -= len;
  return t->val[ix];
}

MTGV_HD inline int prog_extend(uint32_t bits, int s) {  // T.81 F.2.2.1 EXTEND, s in 1..15
  return bits < (1u << (s - 1)) ? (int)bits - (1 << s) + 1 : (int)bits;
}

// Slot of the block (by, bx) of component grid coordinates within the image's MCU-ordered blocks; -1 outside them.
// h x v: the component's sampling factors, slot0: its first slot in the MCU.
MTGV_HD inline int64_t prog_block_slot(const ImgDesc& D, int h, int v, int slot0, int by, int bx) {
  if (h < 1 || v < 1 || by < 0 || bx < 0 || bx / h >= D.mcux || by / v >= D.mcuy) return -1;
  const int64_t m = (int64_t)(by / v) * D.mcux + bx / h;
  const int64_t L = m * D.bpm + slot0 + (by % v) * h + bx % h;
  return L >= 0 && L < D.nblocks ? L : -1;
}

// AC refinement of one block (jdphuff.c decode_mcu_AC_refine).  The walk over the band asks of every coefficient whether
// it has a history; answering that from memory costs a load per coefficient, so the block is read once (sixteen
// independent 8-byte loads), copied into `work` (64 entries, natural order: LDS on the device) and reduced to a 64-bit
// mask in zig-zag order, and the walk runs on the mask.  Only the coefficients this scan changes are stored back,
// because scans of the same level write other coefficients of the same block at the same time.  Returns 1 on a bad
// code or a run past Se.
MTGV_HD inline int prog_refine_block(ProgBits& b, const HuffTab* t, int16_t* blk, int16_t* work, const uint8_t* zz, int ss, int se, int al,
                                     int64_t& eobrun) {
  static constexpr uint8_t kzz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  const int p1 = 1 << al, m1 = -(1 << al);
  uint64_t raw[16];
  MTGV_UNROLL
  for (int j = 0; j < 16; ++j) __builtin_memcpy(&raw[j], blk + 4 * j, 8);
  uint64_t nat = 0;  // natural order: coefficient n is not zero
  MTGV_UNROLL
  for (int j = 0; j < 16; ++j) {
    __builtin_memcpy(work + 4 * j, &raw[j], 8);
  MTGV_UNROLL
    for (int q = 0; q < 4; ++q) nat |= (uint64_t)(((raw[j] >> (16 * q)) & 0xFFFF) != 0) << (4 * j + q);
  }
  uint64_t nz = 0, dirty = 0;  // by zig-zag index: has a history / changed here
  MTGV_UNROLL
  for (int z = 0; z < 64; ++z) nz |= ((nat >> kzz[z]) & 1) << z;
  nz &= (~(uint64_t)0 >> (63 - se)) & (~(uint64_t)0 << ss);
  int k = ss;
  if (eobrun == 0) {
    for (; k <= se; ++k) {
      const int rs = prog_huff(b, t);
      if (rs < 0) return 1;
      int r = rs >> 4, s = rs & 15;
      if (s) {
        if (s != 1) return 1;
        s = prog_get_bits(b, 1) ? p1 : m1;
      } else if (r != 15) {
        eobrun = ((int64_t)1 << r) + (r ? prog_get_bits(b, r) : 0);
        break;
      }
      // pass the coefficients with a history (a correction bit each) and r without one
      do {
        if (nz >> k & 1) {
          if (prog_get_bits(b, 1)) {
            int16_t* c = work + zz[k];
            if ((*c & p1) == 0) {
              *c = (int16_t)(*c + (*c >= 0 ? p1 : m1));
              dirty |= (uint64_t)1 << k;
            }
          }
        } else if (--r < 0) {
          break;
        }
        ++k;
      } while (k <= se);
      if (s) {
        if (k > se) return 1;
        work[zz[k]] = (int16_t)s;
        dirty |= (uint64_t)1 << k;
      }
    }
  }
  if (eobrun > 0) {
    // the rest of the band: correction bits only (a block without history - a flat region - has none)
    for (uint64_t m = k <= se ? nz & (~(uint64_t)0 << k) : 0; m; m &= m - 1) {
      if (!prog_get_bits(b, 1)) continue;
      const int z = __builtin_ctzll(m);
      int16_t* c = work + zz[z];
      if ((*c & p1) == 0) {
        *c = (int16_t)(*c + (*c >= 0 ? p1 : m1));
        dirty |= (uint64_t)1 << z;
      }
    }
    --eobrun;
  }
  for (; dirty; dirty &= dirty - 1) {
    const int n = zz[__builtin_ctzll(dirty)];
    blk[n] = work[n];
  }
  return 0;
}

// Restart segment `seg` of scan S of image D: data[0, len) are its bytes, tab[j] the Huffman table of the scan's
// component j (DC first scan) or tab[0] the AC table, zz the zig-zag -> natural order table (64 entries), coef the
// image's first block, work 64 entries of fast scratch (8-byte aligned).  Returns 0, or 1 if the segment does not decode.
MTGV_HD inline int prog_decode_segment(const ImgDesc& D, const ScanDesc& S, const HuffTab* const* tab, const uint8_t* zz, const uint8_t* data,
                                       uint32_t len, int seg, int16_t* coef, int16_t* work) {
  const int64_t units = (int64_t)S.uw * S.uh;
  if (S.bad || S.ri < 1 || seg < 0 || seg >= S.nseg || S.ncomp < 1 || S.ncomp > 3 || S.uw < 1 || S.uh < 1) return 1;
  if (S.ss < 0 || S.se > 63 || S.ss > S.se || S.al < 0 || S.al > 13) return 1;
  const int64_t u0 = (int64_t)seg * S.ri;
  const int64_t u1 = u0 + S.ri < units ? u0 + S.ri : units;
  if (u0 >= u1) return 1;
  for (int j = 0; j < S.ncomp; ++j)
    if (S.comp[j] < 0 || S.comp[j] >= D.ncomp || S.comp[j] > 2) return 1;
  ProgBits b;
  prog_bits_init(b, data, len);
  const int al = S.al;

  if (S.ss == 0) {  // ---- DC scans: interleaved over MCUs, or one component over its own grid
    uint32_t pred[3] = {0, 0, 0};  // modular, as the int16 store is
    for (int64_t u = u0; u < u1; ++u) {
      const int uy = (int)(u / S.uw), ux = (int)(u % S.uw);
      for (int j = 0; j < S.ncomp; ++j) {
        const CompDesc& C = D.c[S.comp[j]];
        const int nby = S.ncomp == 1 ? 1 : C.v, nbx = S.ncomp == 1 ? 1 : C.h;
        for (int y = 0; y < nby; ++y)
          for (int x = 0; x < nbx; ++x) {
            const int by = S.ncomp == 1 ? uy : uy * C.v + y, bx = S.ncomp == 1 ? ux : ux * C.h + x;
            const int64_t L = prog_block_slot(D, C.h, C.v, S.slot0[j], by, bx);
            if (L < 0) return 1;
            int16_t* blk = coef + L * 64;
            if (S.ah == 0) {
              const int s = prog_huff(b, tab[j]);
              if (s < 0 || s > 15) return 1;
              if (s) pred[j] += (uint32_t)prog_extend(prog_get_bits(b, s), s);
              blk[0] = (int16_t)(pred[j] << al);
            } else if (prog_get_bits(b, 1)) {
              blk[0] = (int16_t)(blk[0] | (1 << al));
            }
          }
      }
      if (prog_bits_overrun(b)) return 1;
    }
    return 0;
  }

  // ---- AC scans: one component, its own grid
  if (S.ncomp != 1) return 1;
  const CompDesc& C = D.c[S.comp[0]];
  const HuffTab* t = tab[0];
  int64_t eobrun = 0;
  for (int64_t u = u0; u < u1; ++u) {
    if (eobrun > 0 && S.ah == 0) {  // first scan: the blocks of an EOB run stay as they are
      const int64_t skip = eobrun < u1 - u ? eobrun : u1 - u;
      eobrun -= skip;
      u += skip - 1;
      continue;
    }
    const int64_t L = prog_block_slot(D, C.h, C.v, S.slot0[0], (int)(u / S.uw), (int)(u % S.uw));
    if (L < 0) return 1;
    int16_t* blk = coef + L * 64;
    int k = S.ss;
    if (S.ah == 0) {
      for (; k <= S.se; ++k) {
        const int rs = prog_huff(b, t);
        if (rs < 0) return 1;
        const int r = rs >> 4, s = rs & 15;
        if (s) {
          k += r;
          if (k > S.se) return 1;
          blk[zz[k]] = (int16_t)((uint32_t)prog_extend(prog_get_bits(b, s), s) << al);
        } else if (r == 15) {
          k += 15;
          if (k > S.se) return 1;
        } else {
          eobrun = ((int64_t)1 << r) + (r ? prog_get_bits(b, r) : 0) - 1;
          break;
        }
      }
    } else if (prog_refine_block(b, t, blk, work, zz, S.ss, S.se, al, eobrun)) {
      return 1;
    }
    if (prog_bits_overrun(b)) return 1;
  }
  return eobrun > 0 || prog_bits_overrun(b) ? 1 : 0;
}

}  // namespace jpeg
}  // namespace mtgv
