// Progressive JPEG decoding, the entropy walk of one scan: plain C++ beside jpeg_core.h that the device code (jpeg_prog.hip)
// and the host check (tools/jpeg_prog_hostcheck.cpp, host compiler and sanitizers) both compile.  A progressive file
// differs from a baseline one only in how the coefficients get into the workspace: jdphuff.c's four scan kinds (DC
// first, DC refinement, AC first, AC refinement) restated over the bit reader and lookup tables of jpeg_core.h;
// everything behind the coefficients (jpg_idct, jpg_pixel) is the baseline code.  tests/jpeg_prog_cases.py restates
// the same in Python.
//
// Bounds: every read of the stream lies in the scan's [begin, end), every coefficient index in the scan's [Ss, Se]
// (both at most 63), every block index in the component's own blocks, and every loop runs over blocks or over 64
// indices: an end-of-band run only counts down over the blocks the scan visits anyway.  A hostile stream ends in one
// of the statuses 1-5, never in an access outside those ranges.  Coefficients are int16 with wrapping arithmetic.
#ifndef MSML_JPEG_PROG_CORE_H
#define MSML_JPEG_PROG_CORE_H
#include "jpeg_core.h"

// ---- two more descriptor words, and the scan table: JPG_SCAN_WORDS int32 per scan, in file order -------------------
#define JD_NSCAN 22   // scans of a progressive image; 0 = a baseline image (one scan, described by the descriptor)
#define JD_SCAN0 23   // its first record in the scan table
#define JPG_SCAN_WORDS 16
#define JS_BEGIN 0    // byte range of the scan's entropy-coded segment, relative to the stream
#define JS_END 1
#define JS_NCOMP 2    // components in the scan: 1 (its own blocks) or more (interleaved over MCUs, DC only)
#define JS_COMP 3     // [3] frame index of each, ascending
#define JS_TAB 6      // [3] Huffman table of each (index into the deduplicated tables): DC for Ss = 0, else AC
#define JS_SS 9
#define JS_SE 10
#define JS_AH 11
#define JS_AL 12
#define JS_RI 13      // restart interval at this scan: MCUs, which are blocks for a one-component scan
#define JPG_MAX_SCANS 4096
#define JPG_MAX_AL 13

// The checks msml_jpeg_decode_scans makes on the host copy of the table before it launches (also the host check's).
// d: the image's descriptor, already through jpg_desc_ok; scans: the whole table of nscan records.
inline bool jpg_scans_ok(const int* d, const int* scans, long nscan, int nh) {
  const int ns = d[JD_NSCAN], s0 = d[JD_SCAN0];
  if (d[JD_STATUS] != 0 || ns == 0) return ns == 0 || d[JD_STATUS] != 0;
  if (ns < 0 || ns > JPG_MAX_SCANS || s0 < 0 || (long)s0 + ns > nscan) return false;
  int at = 0;
  for (int i = 0; i < ns; ++i) {
    const int* s = scans + (long)(s0 + i) * JPG_SCAN_WORDS;
    if (s[JS_BEGIN] < at || s[JS_BEGIN] > s[JS_END] || s[JS_END] > d[JD_END]) return false;   // forward only
    at = s[JS_END];
    if (s[JS_NCOMP] < 1 || s[JS_NCOMP] > d[JD_NCOMP]) return false;
    for (int c = 0; c < s[JS_NCOMP]; ++c) {
      if (s[JS_COMP + c] < (c ? s[JS_COMP + c - 1] + 1 : 0) || s[JS_COMP + c] >= d[JD_NCOMP]) return false;
      if (s[JS_TAB + c] < 0 || s[JS_TAB + c] >= nh) return false;
    }
    if (s[JS_SS] < 0 || s[JS_SS] > s[JS_SE] || s[JS_SE] > 63) return false;
    if (s[JS_SS] == 0 ? s[JS_SE] != 0 : s[JS_NCOMP] != 1) return false;
    if (s[JS_AH] < 0 || s[JS_AH] > JPG_MAX_AL || s[JS_AL] < 0 || s[JS_AL] > JPG_MAX_AL || s[JS_RI] < 0) return false;
  }
  return true;
}

// v << al as int16, defined for every v
IMG_HD inline int jpg_shl16(int v, int al) { return (int)(int16_t)(uint16_t)((uint32_t)v << al); }

IMG_HD inline uint64_t jpg_band(int a, int b) {              // bits a..b, 0 <= a, b <= 63; empty when a > b
  if (a > b) return 0;
  return (~0ull >> (63 - (b - a))) << a;
}

// The correction bits of the coefficients in `m` (a set of nonzero-history zigzag indices): one bit each in index
// order, received up to 16 at a time; Blk::correct hands each coefficient the bit of its rank.
template <class Src, class Blk>
IMG_HD inline void jpg_prog_correct(JpgBits<Src>& b, Blk& blk, uint64_t m, int p1) {
#if defined(__HIP_DEVICE_COMPILE__)
  int left = __popcll(m);
#else
  int left = __builtin_popcountll(m);
#endif
  for (int base = 0; left > 0; base += 16, left -= 16) {     // at most 4 rounds
    const int cnt = left < 16 ? left : 16;
    const int bits = jpg_receive(b, cnt);
    blk.correct(m, base, bits, cnt, p1);
  }
}

// One scan of a progressive image.  d: the descriptor; L: its layout; s: the scan's record; src: the stream (d[JD_BASE]
// applied), handed back so that a window it keeps lives on; tab[c]: the lookup table of the scan's c-th component.
// Blk: the current block, coefficient k in ZIGZAG order --
//   dc_store(block, v), dc_or(block, bit)                      coefficient 0 of a block in the workspace
//   clear(); put(k, v); store(block, ss, se)                   a block of zeros, set k, write the band [ss, se]
//   load(block); nonzero(ss, se) -> 64-bit mask; correct(m, base, bits, cnt, p1)
//     correct: the coefficient of rank r in m, base <= r < base + cnt, takes bit (cnt - 1 - (r - base)) of `bits`; a
//     set bit moves it away from zero by p1 unless it has that bit already (jdphuff.c decode_mcu_AC_refine).
template <class Src, class Blk>
IMG_HD inline int jpg_prog_scan(const int* d, const JpgLayout& L, const int* s, Src& src, const int* const tab[3],
                                Blk& blk) {
  JpgBits<Src> b;
  b.src = src;
  b.pos = s[JS_BEGIN];
  b.end = s[JS_END];
  b.acc = 0;
  b.n = 0;
  b.pad = 0;
  b.marker = false;
  const int ns = s[JS_NCOMP], ss = s[JS_SS], se = s[JS_SE], ah = s[JS_AH], al = s[JS_AL], ri = s[JS_RI];
  const int p1 = 1 << al;
  int st = JPG_OK;
  int left = ri, rst = 0;
  if (ns > 1 || ss == 0) {
    // ---- DC scans: interleaved over the MCUs, or one component over its own blocks
    int pred[3] = {0, 0, 0};
    int c0 = 0, ownw = d[JD_MCUX], ownh = d[JD_MCUY];
    if (ns == 1) {
      c0 = s[JS_COMP];
      const int ch = c0 == 0 ? L.ch[0] : 1, cv = c0 == 0 ? L.cv[0] : 1;
      ownw = ((d[JD_W] * ch + d[JD_HMAX] - 1) / d[JD_HMAX] + 7) / 8;
      ownh = ((d[JD_H] * cv + d[JD_VMAX] - 1) / d[JD_VMAX] + 7) / 8;
    }
    for (int my = 0; my < ownh && st == JPG_OK; ++my) {
      for (int mx = 0; mx < ownw && st == JPG_OK; ++mx) {
        if (ri) {
          if (left == 0) {
            st = jpg_restart(b, rst++);
            if (st) break;
            pred[0] = pred[1] = pred[2] = 0;
            left = ri;
          }
          --left;
        }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 3; ++i) {                        // unrolled: pred[i] and tab[i] stay in registers
          if (i >= ns || st != JPG_OK) break;
          const int c = ns == 1 ? c0 : s[JS_COMP + i];
          const int ch = ns == 1 || c != 0 ? 1 : L.ch[0], cv = ns == 1 || c != 0 ? 1 : L.cv[0];
          const long cbase = c == 2 ? L.cbase[2] : (c == 1 ? L.cbase[1] : L.cbase[0]);
          const int bw = c == 2 ? L.bw[2] : (c == 1 ? L.bw[1] : L.bw[0]);
          for (int v = 0; v < cv && st == JPG_OK; ++v) {
            for (int h = 0; h < ch; ++h) {
              const long blkno = cbase + (long)(my * cv + v) * bw + (mx * ch + h);
              if (ah == 0) {
                const int sy = jpg_symbol(b, tab[i]);
                if (sy < 0) { st = JPG_ERR_CODE; break; }
                if (sy > 11) { st = JPG_ERR_CATEGORY; break; }
                if (sy) pred[i] = (int)(int16_t)(pred[i] + jpg_extend(jpg_receive(b, sy), sy));
                blk.dc_store(blkno, jpg_shl16(pred[i], al));
              } else if (jpg_receive(b, 1)) {
                blk.dc_or(blkno, p1);
              }
            }
          }
        }
        if (st == JPG_OK && b.n < b.pad) st = JPG_ERR_TRUNCATED;
      }
    }
  } else {
    // ---- AC scans: one component, its own blocks
    const int c = s[JS_COMP];
    const int ch = c == 0 ? L.ch[0] : 1, cv = c == 0 ? L.cv[0] : 1;
    const int ownw = ((d[JD_W] * ch + d[JD_HMAX] - 1) / d[JD_HMAX] + 7) / 8;
    const int ownh = ((d[JD_H] * cv + d[JD_VMAX] - 1) / d[JD_VMAX] + 7) / 8;
    const long cbase = c == 2 ? L.cbase[2] : (c == 1 ? L.cbase[1] : L.cbase[0]);
    const int bw = c == 2 ? L.bw[2] : (c == 1 ? L.bw[1] : L.bw[0]);
    const int* t = tab[0];
    int eobrun = 0;
    for (int by = 0; by < ownh && st == JPG_OK; ++by) {
      for (int bx = 0; bx < ownw && st == JPG_OK; ++bx) {
        if (ri) {
          if (left == 0) {
            st = jpg_restart(b, rst++);
            if (st) break;
            eobrun = 0;
            left = ri;
          }
          --left;
        }
        const long blkno = cbase + (long)by * bw + bx;
        if (ah == 0) {
          // first pass: run / size symbols, EOBn with n extra bits; a block inside a run stays zero
          if (eobrun > 0) {
            --eobrun;
            continue;
          }
          blk.clear();
          for (int k = ss; k <= se;) {
            const int sy = jpg_symbol(b, t);
            if (sy < 0) { st = JPG_ERR_CODE; break; }
            const int r = sy >> 4, sz = sy & 15;
            if (sz == 0) {
              if (r != 15) {
                eobrun = (1 << r) - 1;                       // this block ends the count's first unit
                if (r) eobrun += jpg_receive(b, r);
                break;
              }
              k += 16;
              if (k > se + 1) { st = JPG_ERR_INDEX; break; }
              continue;
            }
            if (sz > 10) { st = JPG_ERR_CATEGORY; break; }
            k += r;
            if (k > se) { st = JPG_ERR_INDEX; break; }
            blk.put(k, jpg_shl16(jpg_extend(jpg_receive(b, sz), sz), al));
            ++k;
          }
          if (st == JPG_OK) blk.store(blkno, ss, se);
        } else {
          // refinement: the run counts zero-history coefficients only; every nonzero-history one passed takes a bit
          blk.load(blkno);
          const uint64_t nz = blk.nonzero(ss, se);
          int k = ss;
          if (eobrun == 0) {
            while (k <= se) {
              const int sy = jpg_symbol(b, t);
              if (sy < 0) { st = JPG_ERR_CODE; break; }
              int r = sy >> 4;
              const int sz = sy & 15;
              int val = 0;
              if (sz == 0) {
                if (r != 15) {
                  eobrun = 1 << r;
                  if (r) eobrun += jpg_receive(b, r);
                  break;
                }
              } else {
                if (sz != 1) { st = JPG_ERR_CATEGORY; break; }
                val = jpg_receive(b, 1) ? p1 : -p1;
              }
              // the (r + 1)-th zero-history coefficient from k on, or se + 1
              uint64_t z = ~nz & jpg_band(k, se);
              for (; r > 0 && z; --r) z &= z - 1;            // r <= 15
              int target = se + 1;
              if (z) {
#if defined(__HIP_DEVICE_COMPILE__)
                target = __ffsll((unsigned long long)z) - 1;
#else
                target = __builtin_ctzll(z);
#endif
              }
              jpg_prog_correct(b, blk, nz & jpg_band(k, target - 1), p1);
              if (sz) {
                if (target > se) { st = JPG_ERR_INDEX; break; }
                blk.put(target, val);
              }
              k = target + 1;
            }
          }
          if (st == JPG_OK && eobrun > 0) {
            jpg_prog_correct(b, blk, nz & jpg_band(k, se), p1);
            --eobrun;
          }
          if (st == JPG_OK) blk.store(blkno, ss, se);
        }
        if (st == JPG_OK && b.n < b.pad) st = JPG_ERR_TRUNCATED;
      }
    }
  }
  src = b.src;
  return st;
}
#endif
