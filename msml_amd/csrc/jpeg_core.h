// Baseline JPEG decoding, the per-image arithmetic: plain C++ that the device code (jpeg.hip) and the host check
// (tools/jpeg_hostcheck.cpp, built with the host compiler and the sanitizers) both compile.  No intrinsics, no
// allocation.  libjpeg's defaults restated: Huffman decoding with restart handling, JDCT_ISLOW (jidctint.c), fancy
// upsampling (jdsample.c, with its plain replication for planes of width <= 2) and the 16-bit fixed-point YCbCr
// conversion (jdcolor.c).  tests/jpeg_cases.py restates the same in numpy.
//
// Every read of the entropy-coded bytes is bounded by the descriptor's [begin, end), every table index by the table's
// size, every coefficient index by 63: a hostile byte string ends in a status, never in an access outside those ranges.
#ifndef MSML_JPEG_CORE_H
#define MSML_JPEG_CORE_H
#include <stdint.h>

#include "packed_image.h"

// ---- the descriptor: JPG_DESC_WORDS int32 per image (msml_amd/jpeg.py writes it, msml_jpeg_decode checks it) ----------
#define JPG_DESC_WORDS 32
#define JD_BASE 0     // offset of the stream in the packed buffer, in dwords
#define JD_BEGIN 1    // first entropy-coded byte, relative to the stream
#define JD_END 2      // length of the stream in bytes (the entropy-coded segment runs to here, or to its EOI)
#define JD_H 3
#define JD_W 4
#define JD_NCOMP 5    // 1 or 3
#define JD_HMAX 6     // sampling factors of component 0 (the others are 1 x 1): 1 or 2
#define JD_VMAX 7
#define JD_QT 8       // [3] quantisation table of each component (index into the deduplicated tables)
#define JD_DC 11      // [3] DC Huffman table
#define JD_AC 14      // [3] AC Huffman table
#define JD_RI 17      // restart interval in MCUs, 0 = none
#define JD_STATUS 18  // the parser's verdict: 0, or a JPG_UNSUPPORTED_* the device copies into status[n]
#define JD_MCUX 19
#define JD_MCUY 20
#define JD_WS 21      // offset of the image's workspace, in units of JPG_WS_ALIGN bytes (msml_jpeg_workspace writes it)
#define JPG_WS_ALIGN 256

// ---- statuses ------------------------------------------------------------------------------------------------------
#define JPG_OK 0
#define JPG_ERR_CODE 1      // a code that is in no table
#define JPG_ERR_INDEX 2     // a coefficient index past 63
#define JPG_ERR_CATEGORY 3  // DC category > 11 or AC category > 10
#define JPG_ERR_RESTART 4   // restart marker missing or out of sequence
#define JPG_ERR_TRUNCATED 5 // data ends before the last MCU
#define JPG_ERR_OUTPUT 6    // meta_out does not describe an H x W rectangle inside dst
// 16.. : the parser's reasons (msml_amd/jpeg.py UNSUPPORTED)

// ---- Huffman table in lookup form: JPG_HUFF_WORDS int32 -------------------------------------------------------------
//   [0, 512)    9-bit lookahead: (length << 8) | symbol, 0 = the code is longer than 9 bits (or none)
//   [512, 530)  maxcode[l], l = 0..17: largest code of length l, -1 = none
//   [530, 547)  valoff[l] = index of the first symbol of length l minus its code
//   [547, 803)  huffval[256]
#define JPG_HUFF_WORDS 832
#define JPG_HUFF_LOOK 9
#define JPG_HUFF_MAXCODE 512
#define JPG_HUFF_VALOFF 530
#define JPG_HUFF_VAL 547

struct JpgLayout {
  int ncomp;
  int ch[3], cv[3];    // sampling factors
  int bw[3], bh[3];    // blocks per row / column of each component plane (padded to whole MCUs)
  long cbase[3];       // first block of the component among the image's coefficient blocks
  long nblk;           // blocks in all
  long pbase[3];       // byte offset of the component plane in the image's workspace
  long bytes;          // workspace bytes of the image, a multiple of JPG_WS_ALIGN
};

// Workspace of one image: coefficients int16 [nblk][64] (natural order), then the component planes uint8
// [bh * 8][bw * 8].
IMG_HD inline void jpg_layout(const int* d, JpgLayout& L) {
  L.ncomp = d[JD_NCOMP];
  long blk = 0;
  for (int c = 0; c < 3; ++c) {
    L.ch[c] = c == 0 ? d[JD_HMAX] : 1;
    L.cv[c] = c == 0 ? d[JD_VMAX] : 1;
    L.bw[c] = c < L.ncomp ? d[JD_MCUX] * L.ch[c] : 0;
    L.bh[c] = c < L.ncomp ? d[JD_MCUY] * L.cv[c] : 0;
    L.cbase[c] = blk;
    blk += (long)L.bw[c] * L.bh[c];
  }
  L.nblk = blk;
  for (int c = 0; c < 3; ++c) L.pbase[c] = blk * 128 + L.cbase[c] * 64;
  L.bytes = (blk * 192 + (JPG_WS_ALIGN - 1)) / JPG_WS_ALIGN * JPG_WS_ALIGN;
}

// ---- bit reader -----------------------------------------------------------------------------------------------------
// acc holds n valid bits at its top.  Past the end of the data, or at a marker, zero bytes are fed and counted in
// `pad`: the decoder has consumed bits that were never there exactly when n < pad.
// Src: where the bytes come from -- byte(i) for i in [begin, end) only.  The host reads the stream itself (JpgPtrSrc);
// the device stages it through LDS (jpeg.hip).
struct JpgPtrSrc {
  const unsigned char* p;
  IMG_HD int byte(int i) { return p[i]; }
};

template <class Src>
struct JpgBits {
  Src src;
  int pos, end;
  uint32_t acc;
  int n, pad;
  bool marker;
};

template <class Src>
IMG_HD inline void jpg_fill(JpgBits<Src>& b) {
  while (b.n <= 24) {
    uint32_t c = 0;
    if (!b.marker && b.pos < b.end) {
      c = (uint32_t)b.src.byte(b.pos);
      if (c == 0xFF) {
        int q = b.pos + 1;
        while (q < b.end && b.src.byte(q) == 0xFF) ++q;     // fill bytes
        if (q < b.end && b.src.byte(q) == 0) b.pos = q + 1; // FF 00: a data byte FF
        else b.marker = true;                               // a marker (pos stays on its FF), or the end
      } else {
        b.pos++;
      }
    } else {
      b.marker = true;
    }
    if (b.marker) { c = 0; b.pad += 8; }
    b.acc |= c << (24 - b.n);
    b.n += 8;
  }
}

template <class Src>
IMG_HD inline void jpg_skip(JpgBits<Src>& b, int k) { b.acc <<= k; b.n -= k; }

// k in 1..16
template <class Src>
IMG_HD inline int jpg_receive(JpgBits<Src>& b, int k) {
  if (b.n < k) jpg_fill(b);
  const int v = (int)(b.acc >> (32 - k));
  jpg_skip(b, k);
  return v;
}

IMG_HD inline int jpg_extend(int v, int k) { return v >= (1 << (k - 1)) ? v : v - (1 << k) + 1; }

// the next symbol of table t, or -1 for a code the table does not hold
template <class Src>
IMG_HD inline int jpg_symbol(JpgBits<Src>& b, const int* t) {
  if (b.n < 16) jpg_fill(b);
  const int look = t[b.acc >> (32 - JPG_HUFF_LOOK)];
  if (look) {
    jpg_skip(b, look >> 8);
    return look & 255;
  }
  const int code16 = (int)(b.acc >> 16);
  for (int l = JPG_HUFF_LOOK + 1; l <= 16; ++l) {
    const int code = code16 >> (16 - l);
    if (code <= t[JPG_HUFF_MAXCODE + l]) {
      jpg_skip(b, l);
      return t[JPG_HUFF_VAL + ((t[JPG_HUFF_VALOFF + l] + code) & 255)];
    }
  }
  return -1;
}

// At a restart: the rest of the current byte is dropped, RSTm (m = index & 7) must follow, predictions start over.
template <class Src>
IMG_HD inline int jpg_restart(JpgBits<Src>& b, int index) {
  if (b.n < b.pad) return JPG_ERR_TRUNCATED;
  if (b.n - b.pad >= 8) return JPG_ERR_RESTART;             // whole data bytes in front of the marker
  int q = b.pos;
  if (q >= b.end || b.src.byte(q) != 0xFF) return JPG_ERR_RESTART;
  while (q < b.end && b.src.byte(q) == 0xFF) ++q;
  if (q >= b.end || b.src.byte(q) != 0xD0 + (index & 7)) return JPG_ERR_RESTART;
  b.pos = q + 1;
  b.acc = 0;
  b.n = 0;
  b.pad = 0;
  b.marker = false;
  return JPG_OK;
}

// Entropy decoding of one image.  d: its descriptor; src: its stream (d[JD_BASE] applied); dctab / actab: the lookup
// tables of each component.  Sink: begin() starts a block of zeros, put(k, value) sets the k-th coefficient in ZIGZAG
// order (the sink knows img_zigzag), end(block) stores the block.
template <class Src, class Sink>
IMG_HD inline int jpg_entropy(const int* d, const Src& src, const int* const dctab[3], const int* const actab[3],
                              Sink& sink) {
  JpgLayout L;
  jpg_layout(d, L);
  JpgBits<Src> b;
  b.src = src;
  b.pos = d[JD_BEGIN];
  b.end = d[JD_END];
  b.acc = 0;
  b.n = 0;
  b.pad = 0;
  b.marker = false;
  const int ri = d[JD_RI], mcux = d[JD_MCUX], mcuy = d[JD_MCUY];
  int pred[3] = {0, 0, 0};
  int left = ri, rst = 0;
  for (int my = 0; my < mcuy; ++my) {
    for (int mx = 0; mx < mcux; ++mx) {
      if (ri) {
        if (left == 0) {
          const int e = jpg_restart(b, rst++);
          if (e) return e;
          pred[0] = pred[1] = pred[2] = 0;
          left = ri;
        }
        --left;
      }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int c = 0; c < 3; ++c) {
        if (c >= L.ncomp) break;
        const int* dct = dctab[c];
        const int* act = actab[c];
        for (int v = 0; v < L.cv[c]; ++v) {
          for (int h = 0; h < L.ch[c]; ++h) {
            sink.begin();
            int sy = jpg_symbol(b, dct);
            if (sy < 0) return JPG_ERR_CODE;
            if (sy > 11) return JPG_ERR_CATEGORY;
            if (sy) pred[c] = (int)(int16_t)(pred[c] + jpg_extend(jpg_receive(b, sy), sy));
            sink.put(0, pred[c]);
            for (int k = 1; k < 64;) {
              sy = jpg_symbol(b, act);
              if (sy < 0) return JPG_ERR_CODE;
              const int r = sy >> 4, sz = sy & 15;
              if (sz == 0) {
                if (r != 15) break;                          // end of block
                k += 16;
                if (k > 64) return JPG_ERR_INDEX;
                continue;
              }
              if (sz > 10) return JPG_ERR_CATEGORY;
              k += r;
              if (k > 63) return JPG_ERR_INDEX;
              sink.put(k, jpg_extend(jpg_receive(b, sz), sz));
              ++k;
            }
            sink.end(L.cbase[c] + (long)(my * L.cv[c] + v) * L.bw[c] + (mx * L.ch[c] + h));
          }
        }
      }
      if (b.n < b.pad) return JPG_ERR_TRUNCATED;
    }
  }
  return JPG_OK;
}

// ---- dequantisation + JDCT_ISLOW ------------------------------------------------------------------------------------
// 32-bit arithmetic that wraps (unsigned): equal to libjpeg's for every coefficient a real encoder writes, and defined
// for every other.
IMG_HD inline int jpg_descale(uint32_t x, int n) { return (int)(x + (1u << (n - 1))) >> n; }

IMG_HD inline void jpg_idct_1d(const uint32_t in[8], int out[8], int n) {
  const uint32_t z1e = (in[2] + in[6]) * 4433u;
  const uint32_t t2 = z1e - in[6] * 15137u, t3 = z1e + in[2] * 6270u;
  const uint32_t t0 = (in[0] + in[4]) << 13, t1 = (in[0] - in[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a0 = in[7], a1 = in[5], a2 = in[3], a3 = in[1];
  uint32_t z1 = a0 + a3, z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5;
  z4 = z4 * (uint32_t)-3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  out[0] = jpg_descale(t10 + a3, n); out[7] = jpg_descale(t10 - a3, n);
  out[1] = jpg_descale(t11 + a2, n); out[6] = jpg_descale(t11 - a2, n);
  out[2] = jpg_descale(t12 + a1, n); out[5] = jpg_descale(t12 - a1, n);
  out[3] = jpg_descale(t13 + a0, n); out[4] = jpg_descale(t13 - a0, n);
}

// coef: 64 coefficients in natural order; q: the quantisation table in natural order; out: 8 rows of 8 samples
IMG_HD inline void jpg_idct(const int16_t* coef, const int* q, unsigned char* out, long pitch) {
  int wsp[64];
  for (int x = 0; x < 8; ++x) {
    uint32_t in[8];
    int o[8];
    for (int y = 0; y < 8; ++y) in[y] = (uint32_t)((int)coef[y * 8 + x] * q[y * 8 + x]);
    jpg_idct_1d(in, o, 11);
    for (int y = 0; y < 8; ++y) wsp[y * 8 + x] = o[y];
  }
  for (int y = 0; y < 8; ++y) {
    uint32_t in[8];
    int o[8];
    for (int x = 0; x < 8; ++x) in[x] = (uint32_t)wsp[y * 8 + x];
    jpg_idct_1d(in, o, 18);
    for (int x = 0; x < 8; ++x) {
      const int v = o[x] + 128;
      out[y * pitch + x] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  }
}

// ---- upsampling + colour ---------------------------------------------------------------------------------------------
// One chroma sample at output (x, y).  p: the component plane, dw x dh its cropped size, hs / vs the expansion (1 or 2).
IMG_HD inline int jpg_chroma(const unsigned char* p, long pitch, int dw, int dh, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(long)y * pitch + x];
  const int i = x >> 1;
  if (vs == 1) {
    const unsigned char* row = p + (long)y * pitch;
    if (dw <= 2) return row[i];
    if ((x & 1) == 0) return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
    return i == dw - 1 ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
  }
  const int r = y >> 1;
  const unsigned char* r0 = p + (long)r * pitch;
  if (dw <= 2) return r0[i];
  int rn = (y & 1) == 0 ? r - 1 : r + 1;
  rn = rn < 0 ? 0 : (rn > dh - 1 ? dh - 1 : rn);
  const unsigned char* r1 = p + (long)rn * pitch;
  const int s = 3 * r0[i] + r1[i];
  if ((x & 1) == 0) return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
  return i == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
}

IMG_HD inline int jpg_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// The pixel (x, y) of the image whose workspace is ws: rgb[0..2] = R, G, B (all Y for a gray stream).
IMG_HD inline void jpg_pixel(const int* d, const JpgLayout& L, const unsigned char* ws, int x, int y, int rgb[3]) {
  const int yy = ws[L.pbase[0] + (long)y * (L.bw[0] * 8) + x];
  if (L.ncomp == 1) {
    rgb[0] = rgb[1] = rgb[2] = yy;
    return;
  }
  const int hs = d[JD_HMAX], vs = d[JD_VMAX];
  const int dw = (d[JD_W] + hs - 1) / hs, dh = (d[JD_H] + vs - 1) / vs;
  const int cb = jpg_chroma(ws + L.pbase[1], L.bw[1] * 8, dw, dh, hs, vs, x, y) - 128;
  const int cr = jpg_chroma(ws + L.pbase[2], L.bw[2] * 8, dw, dh, hs, vs, x, y) - 128;
  rgb[0] = jpg_clamp8(yy + ((91881 * cr + 32768) >> 16));
  rgb[1] = jpg_clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = jpg_clamp8(yy + ((116130 * cb + 32768) >> 16));
}

// The descriptor checks msml_jpeg_decode makes on the host before it launches (also the host check's).  0 = fine.
inline int jpg_desc_ok(const int* d, long stream_bytes, int nq, int nh) {
  if (d[JD_STATUS] != 0) return d[JD_STATUS] > 0;           // a refused stream: nothing else is read
  const int H = d[JD_H], W = d[JD_W], nc = d[JD_NCOMP], hm = d[JD_HMAX], vm = d[JD_VMAX];
  if (H < 1 || H > 32767 || W < 1 || W > 32767) return 0;
  if (nc != 1 && nc != 3) return 0;
  if (!((hm == 1 && vm == 1) || (nc == 3 && hm == 2 && (vm == 1 || vm == 2)))) return 0;
  if (d[JD_MCUX] != (W + 8 * hm - 1) / (8 * hm) || d[JD_MCUY] != (H + 8 * vm - 1) / (8 * vm)) return 0;
  for (int c = 0; c < nc; ++c)
    if (d[JD_QT + c] < 0 || d[JD_QT + c] >= nq || d[JD_DC + c] < 0 || d[JD_DC + c] >= nh || d[JD_AC + c] < 0 ||
        d[JD_AC + c] >= nh)
      return 0;
  if (d[JD_RI] < 0 || d[JD_BASE] < 0 || d[JD_BEGIN] < 0 || d[JD_BEGIN] > d[JD_END]) return 0;
  if ((long)d[JD_BASE] * 4 + d[JD_END] > stream_bytes) return 0;
  return 1;
}
#endif
