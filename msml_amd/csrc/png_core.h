// PNG decoding, the per-image code: plain C++ that the device code (png.hip) and the host check
// (tools/png_hostcheck.cpp, built with the host compiler and the sanitizers) both compile.  No intrinsics, no
// allocation, no floating point.  Written from RFC 1950 (zlib wrapper), RFC 1951 (DEFLATE) and the PNG specification
// (filters, sample unpacking); the pixels are those of Pillow's Image.open(f).convert("L" / "RGB" / "RGBA").
// tests/png_cases.py restates the same in numpy.
//
//   png_inflate   one zlib stream -> the filtered rows, through a sink (the host writes a buffer, the device a ring of
//                 the last 32 KiB in LDS).  Accepts exactly the streams for which zlib's inflate reaches the end of the
//                 stream without an error AND that hold exactly `expected` bytes.
//   png_unfilter  filters 0-4, in place
//   png_expand    one pixel of an unfiltered row -> R, G, B, A
//
// The code is written for `nl` cooperating lanes that all run the same statements with the same values (the host: one
// lane; the device: the 64 lanes of a wavefront).  Loops of the form `for (i = lane; i < n; i += nl)` divide work;
// PNG_SYNC() separates a lane's writes to the shared tables from another lane's reads.
//
// Every read of the stream is bounded by [0, end), every table index by the table's size, every output byte by
// `expected`: a hostile byte string ends in a status, never in an access outside those ranges.
#ifndef MSML_PNG_CORE_H
#define MSML_PNG_CORE_H
#include <stdint.h>

#include "packed_image.h"
#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_SYNC() __syncthreads()
#define PNG_COUNT(p) atomicAdd((p), 1u)
#else
#define PNG_SYNC() ((void)0)
#define PNG_COUNT(p) (++*(p))
#endif

// ---- the descriptor: PNG_DESC_WORDS int32 per image (msml_amd/png.py writes it, msml_png_decode checks it) ----------
#define PNG_DESC_WORDS 16
#define PD_BASE 0     // offset of the image's zlib stream (its IDAT payloads back to back) in the packed buffer, in dwords
#define PD_END 1      // length of that stream in bytes
#define PD_H 2
#define PD_W 3
#define PD_DEPTH 4    // 1, 2, 4, 8
#define PD_CTYPE 5    // 0 gray, 2 RGB, 3 palette, 4 gray + alpha, 6 RGBA
#define PD_PAL 6      // palette streams: index of the 256-entry RGBA palette
#define PD_STATUS 7   // the parser's verdict: 0, or a reason (16..) the device copies into status[n]
#define PD_WS 8       // offset of the image's workspace, in units of PNG_WS_ALIGN bytes (msml_png_workspace writes it)
#define PD_KEY 9      // 1: a tRNS colour key (gray: PD_KEY0; RGB: PD_KEY0..2), alpha 0 for pixels equal to it
#define PD_KEY0 10
#define PNG_WS_ALIGN 256

// ---- statuses ------------------------------------------------------------------------------------------------------
#define PNG_OK 0
#define PNG_ERR_HEADER 1     // zlib header: CM != 8, CINFO > 7, check bits, FDICT
#define PNG_ERR_BTYPE 2      // block type 3
#define PNG_ERR_STORED 3     // LEN != ~NLEN
#define PNG_ERR_LENGTHS 4    // over-subscribed or incomplete code lengths, bad repeat, HLIT / HDIST too large, no end code
#define PNG_ERR_SYMBOL 5     // an unused code, literal/length symbol 286 / 287, distance symbol 30 / 31
#define PNG_ERR_DISTANCE 6   // a distance that reaches before the first output byte
#define PNG_ERR_TRUNCATED 7  // the stream ends early, or holds fewer bytes than the image
#define PNG_ERR_TOO_LONG 8   // more bytes than the image holds
#define PNG_ERR_ADLER 9
#define PNG_ERR_FILTER 10    // filter byte above 4
#define PNG_ERR_OUTPUT 11    // meta_out does not describe an H x W rectangle inside dst
#define PNG_ERR_EXPAND 12    // 4 channels asked of a stream the expand step has no rule for (none at present)
// 16.. : the parser's reasons (msml_amd/png.py STATUS)

#define PNG_LIT_BITS 10
#define PNG_DIST_BITS 9

// The decode tables of the current block.  A code set is kept canonically: cnt[l] codes of length l, their symbols in
// `sorted` (by length, then by symbol), plus a primary lookup indexed by the next BITS stream bits: (symbol << 4) |
// length, 0 for a longer (or unused) code, which the bit-by-bit walk of png_slow resolves.
struct PngTables {
  unsigned int cnt[2][16];
  unsigned short off[2][16];
  unsigned short sorted[2][288];
  unsigned short look_lit[1 << PNG_LIT_BITS];
  unsigned short look_dist[1 << PNG_DIST_BITS];
  unsigned char lens[320];
};

IMG_HD inline int png_row_bytes(const int* d) {
  const int ct = d[PD_CTYPE];
  const int spp = ct == 2 ? 3 : (ct == 4 ? 2 : (ct == 6 ? 4 : 1));
  return (int)(((long)d[PD_W] * spp * d[PD_DEPTH] + 7) >> 3);
}
IMG_HD inline int png_bpp(const int* d) {
  const int ct = d[PD_CTYPE];
  const int spp = ct == 2 ? 3 : (ct == 4 ? 2 : (ct == 6 ? 4 : 1));
  const int b = spp * d[PD_DEPTH] >> 3;
  return b < 1 ? 1 : b;
}
IMG_HD inline long png_expected(const int* d) { return (long)d[PD_H] * (1 + png_row_bytes(d)); }
IMG_HD inline long png_ws_bytes(const int* d) {
  return (png_expected(d) + (PNG_WS_ALIGN - 1)) / PNG_WS_ALIGN * PNG_WS_ALIGN;
}

// ---- bit reader (LSB first) ------------------------------------------------------------------------------------------
// acc holds n valid bits at its bottom.  It is refilled four bytes at a time while four are left (pos stays a multiple
// of 4 until then), byte by byte at the tail.  Past the end of the data zero bytes are fed and counted in `pad`: the
// decoder has consumed bits that were never there exactly when n < pad.
// Src: byte(i) for i in [0, end) only; word(i) = bytes i .. i + 3, little-endian, for i % 4 == 0 and i + 4 <= end only.
struct PngPtrSrc {
  const unsigned char* p;
  IMG_HD int byte(int i) { return p[i]; }
  IMG_HD uint32_t word(int i) {
    return (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16) | ((uint32_t)p[i + 3] << 24);
  }
};

template <class Src>
struct PngBits {
  Src src;
  int pos, end;
  uint64_t acc;
  int n, pad;
};

// k in 0..16: called with n < 16, so a refill of 32 bits fits
template <class Src>
IMG_HD inline void png_need(PngBits<Src>& b, int k) {
  while (b.n < k) {
    if (b.pos + 4 <= b.end) {
      b.acc |= (uint64_t)b.src.word(b.pos) << b.n;
      b.pos += 4;
      b.n += 32;
    } else {
      uint64_t c = 0;
      if (b.pos < b.end) c = (uint64_t)b.src.byte(b.pos++);
      else b.pad += 8;
      b.acc |= c << b.n;
      b.n += 8;
    }
  }
}
template <class Src>
IMG_HD inline void png_drop(PngBits<Src>& b, int k) { b.acc >>= k; b.n -= k; }
// k in 0..16
template <class Src>
IMG_HD inline int png_bits(PngBits<Src>& b, int k) {
  png_need(b, k);
  const int v = (int)((uint32_t)b.acc & ((1u << k) - 1u));
  png_drop(b, k);
  return v;
}
template <class Src>
IMG_HD inline bool png_over(const PngBits<Src>& b) { return b.n < b.pad; }

// ---- code tables ------------------------------------------------------------------------------------------------------
// Build the tables of the n code lengths lens[0..n).  Returns -1 for an over-subscribed set, otherwise what is left of
// the code space (0: complete); maxlen: the longest code.
template <int BITS>
IMG_HD inline int png_build(unsigned int* cnt, unsigned short* off, unsigned short* sorted, unsigned short* look,
                            const unsigned char* lens, int n, int lane, int nl, int& maxlen) {
  PNG_SYNC();
  for (int i = lane; i < 16; i += nl) cnt[i] = 0;
  PNG_SYNC();
  for (int i = lane; i < n; i += nl) PNG_COUNT(&cnt[lens[i] & 15]);
  PNG_SYNC();
  int left = 1, o = 0;
  maxlen = 0;
  for (int l = 1; l <= 15; ++l) {
    const int c = (int)cnt[l];
    left = (left << 1) - c;
    if (left < 0) return -1;
    if (c) maxlen = l;
    if (lane == 0) off[l] = (unsigned short)o;
    o += c;
  }
  PNG_SYNC();
  for (int i = lane; i < n; i += nl) {
    const int l = lens[i] & 15;
    if (l) {
      int r = 0;
      for (int j = 0; j < i; ++j) r += lens[j] == l;
      sorted[off[l] + r] = (unsigned short)i;
    }
  }
  PNG_SYNC();
  for (int e = lane; e < (1 << BITS); e += nl) {
    int code = 0, first = 0, index = 0, v = 0;
    for (int l = 1; l <= BITS; ++l) {
      code |= (e >> (l - 1)) & 1;
      const int c = (int)cnt[l];
      if (code - c < first) {
        v = (sorted[index + (code - first)] << 4) | l;
        break;
      }
      index += c;
      first = (first + c) << 1;
      code <<= 1;
    }
    look[e] = (unsigned short)v;
  }
  PNG_SYNC();
  return left;
}

// the code at the bottom of acc, bit by bit: (symbol << 4) | length, or 0 for a code the set does not hold
IMG_HD inline int png_slow(const unsigned int* cnt, const unsigned short* sorted, uint32_t acc) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)(acc & 1u);
    acc >>= 1;
    const int c = (int)cnt[l];
    if (code - c < first) return ((int)sorted[index + (code - first)] << 4) | l;
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return 0;
}

// the next symbol, or -1 for a code the set does not hold
template <class Src>
IMG_HD inline int png_symbol(PngBits<Src>& b, const unsigned int* cnt, const unsigned short* sorted,
                             const unsigned short* look, int bits) {
  png_need(b, 15);
  int e = look[(uint32_t)b.acc & ((1u << bits) - 1u)];
  if (!e) e = png_slow(cnt, sorted, (uint32_t)b.acc);
  if (!e) return -1;
  png_drop(b, e & 15);
  return e >> 4;
}

// ---- inflate ------------------------------------------------------------------------------------------------------------
// Sink: `long count` bytes written so far; put(byte); copy(distance, length) with distance <= count (the j-th byte is
// the byte `distance` back, repeating for distance < length); finish() flushes and returns the Adler-32 of all bytes.
// The sink is never asked to hold more than `expected` bytes.
template <class Src, class Sink>
IMG_HD inline int png_inflate(const Src& src, int end, long expected, Sink& sink, PngTables* T, int lane, int nl) {
  constexpr unsigned short lbase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                        31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  constexpr unsigned char lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  constexpr unsigned char clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  PngBits<Src> b;
  b.src = src;
  b.pos = 0;
  b.end = end;
  b.acc = 0;
  b.n = 0;
  b.pad = 0;
  const int cmf = png_bits(b, 8), flg = png_bits(b, 8);
  if (png_over(b)) return PNG_ERR_TRUNCATED;
  if (((cmf << 8) | flg) % 31 != 0 || (cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 32)) return PNG_ERR_HEADER;
  for (;;) {
    const int final = png_bits(b, 1), type = png_bits(b, 2);
    if (png_over(b)) return PNG_ERR_TRUNCATED;
    if (type == 3) return PNG_ERR_BTYPE;
    if (type == 0) {
      png_drop(b, b.n & 7);
      const int len = png_bits(b, 16), nlen = png_bits(b, 16);
      if (png_over(b)) return PNG_ERR_TRUNCATED;
      if ((len ^ 0xffff) != nlen) return PNG_ERR_STORED;
      for (int i = 0; i < len; ++i) {
        const int v = png_bits(b, 8);
        if (png_over(b)) return PNG_ERR_TRUNCATED;
        if (sink.count >= expected) return PNG_ERR_TOO_LONG;
        sink.put(v);
      }
    } else {
      int hlit = 288, hdist = 32;
      if (type == 1) {
        PNG_SYNC();
        for (int i = lane; i < 320; i += nl) T->lens[i] = (unsigned char)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : (i < 288 ? 8 : 5))));
      } else {
        hlit = png_bits(b, 5) + 257;
        hdist = png_bits(b, 5) + 1;
        const int hclen = png_bits(b, 4) + 4;
        if (png_over(b)) return PNG_ERR_TRUNCATED;
        if (hlit > 286 || hdist > 30) return PNG_ERR_LENGTHS;
        PNG_SYNC();
        for (int i = lane; i < 19; i += nl) T->lens[i] = 0;
        PNG_SYNC();
        for (int i = 0; i < hclen; ++i) {
          const int v = png_bits(b, 3);
          if (lane == 0) T->lens[clorder[i]] = (unsigned char)v;
        }
        if (png_over(b)) return PNG_ERR_TRUNCATED;
        int mx;
        // the code-length code borrows the distance tables; it must be complete
        if (png_build<7>(T->cnt[1], T->off[1], T->sorted[1], T->look_dist, T->lens, 19, lane, nl, mx) != 0)
          return PNG_ERR_LENGTHS;
        const int total = hlit + hdist;
        int prev = -1;
        for (int i = 0; i < total;) {
          const int sy = png_symbol(b, T->cnt[1], T->sorted[1], T->look_dist, 7);
          if (sy < 0) return b.pad ? PNG_ERR_TRUNCATED : PNG_ERR_LENGTHS;
          int rep = 1, v = sy;
          if (sy == 16) {
            if (prev < 0) return png_over(b) ? PNG_ERR_TRUNCATED : PNG_ERR_LENGTHS;
            rep = 3 + png_bits(b, 2);
            v = prev;
          } else if (sy == 17) {
            rep = 3 + png_bits(b, 3);
            v = 0;
          } else if (sy == 18) {
            rep = 11 + png_bits(b, 7);
            v = 0;
          }
          if (png_over(b)) return PNG_ERR_TRUNCATED;
          if (i + rep > total) return PNG_ERR_LENGTHS;
          if (lane == 0)
            for (int k = 0; k < rep; ++k) T->lens[i + k] = (unsigned char)v;
          i += rep;
          prev = v;
        }
        PNG_SYNC();
        if ((int)T->lens[256] == 0) return PNG_ERR_LENGTHS;
      }
      int mx;
      int left = png_build<PNG_LIT_BITS>(T->cnt[0], T->off[0], T->sorted[0], T->look_lit, T->lens, hlit, lane, nl, mx);
      if (left < 0 || (left > 0 && mx > 1)) return PNG_ERR_LENGTHS;
      left = png_build<PNG_DIST_BITS>(T->cnt[1], T->off[1], T->sorted[1], T->look_dist, T->lens + hlit, hdist, lane, nl, mx);
      if (left < 0 || (left > 0 && mx > 1)) return PNG_ERR_LENGTHS;
      for (;;) {
        // the common case on a short path: a literal whose code the primary lookup holds, read from real bits, with
        // room for it; anything else leaves for the general statements below with nothing consumed
        for (;;) {
          png_need(b, 15);
          const int e = T->look_lit[(uint32_t)b.acc & ((1u << PNG_LIT_BITS) - 1u)];
          if (e == 0 || e >= (256 << 4) || b.pad != 0 || sink.count >= expected) break;
          png_drop(b, e & 15);
          sink.put(e >> 4);
        }
        int sy = png_symbol(b, T->cnt[0], T->sorted[0], T->look_lit, PNG_LIT_BITS);
        if (sy < 0) return b.pad ? PNG_ERR_TRUNCATED : PNG_ERR_SYMBOL;
        if (png_over(b)) return PNG_ERR_TRUNCATED;
        if (sy < 256) {
          if (sink.count >= expected) return PNG_ERR_TOO_LONG;
          sink.put(sy);
          continue;
        }
        if (sy == 256) break;
        if (sy > 285) return PNG_ERR_SYMBOL;
        const int len = lbase[sy - 257] + png_bits(b, lext[sy - 257]);
        sy = png_symbol(b, T->cnt[1], T->sorted[1], T->look_dist, PNG_DIST_BITS);
        if (sy < 0) return b.pad ? PNG_ERR_TRUNCATED : PNG_ERR_SYMBOL;
        if (sy > 29) return png_over(b) ? PNG_ERR_TRUNCATED : PNG_ERR_SYMBOL;
        const int dx = sy < 2 ? 0 : (sy >> 1) - 1;
        const int dist = (sy < 4 ? sy + 1 : ((2 + (sy & 1)) << dx) + 1) + png_bits(b, dx);
        if (png_over(b)) return PNG_ERR_TRUNCATED;
        if (dist > sink.count) return PNG_ERR_DISTANCE;
        if (sink.count + len > expected) return PNG_ERR_TOO_LONG;
        sink.copy(dist, len);
      }
    }
    if (final) break;
  }
  png_drop(b, b.n & 7);
  uint32_t sum = 0;
  for (int i = 0; i < 4; ++i) sum = (sum << 8) | (uint32_t)png_bits(b, 8);
  if (png_over(b)) return PNG_ERR_TRUNCATED;
  if (sum != sink.finish()) return PNG_ERR_ADLER;
  if (sink.count != expected) return PNG_ERR_TRUNCATED;
  return PNG_OK;
}

// ---- filters ----------------------------------------------------------------------------------------------------------
IMG_HD inline int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

// Sub (1), Average (3) or Paeth (4) along one row for the bytes k, k + bpp, k + 2 bpp ...: each depends on the one
// before it.  The filtered bytes and the row above are read 8 at a time ahead of the chain, which runs in registers.
IMG_HD inline void png_unfilter_chain(unsigned char* row, const unsigned char* prior, int rowbytes, int bpp, int ft, int k) {
  int a = 0, c = 0;
  for (int x0 = k; x0 < rowbytes; x0 += 8 * bpp) {
    int r[8], p[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 8; ++e) {
      const int i = x0 + e * bpp;
      r[e] = i < rowbytes ? row[i] : 0;
      p[e] = prior && i < rowbytes ? prior[i] : 0;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 8; ++e) {
      const int b = p[e];
      const int add = ft == 1 ? a : (ft == 3 ? (a + b) >> 1 : png_paeth(a, b, c));
      a = (r[e] + add) & 255;
      c = b;
      r[e] = a;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 8; ++e) {
      const int i = x0 + e * bpp;
      if (i < rowbytes) row[i] = (unsigned char)r[e];
    }
  }
}

// raw: H rows of 1 filter byte + rowbytes, unfiltered in place.  The first row's prior row is zeros.
IMG_HD inline int png_unfilter(unsigned char* raw, int H, int rowbytes, int bpp, int lane, int nl) {
  const long stride = (long)rowbytes + 1;
  for (int y = 0; y < H; ++y) {
    unsigned char* row = raw + (long)y * stride + 1;
    const unsigned char* prior = y ? row - stride : nullptr;
    const int ft = row[-1];
    if (ft > 4) return PNG_ERR_FILTER;
    if (ft == 2) {
      if (prior)
        for (int i = lane; i < rowbytes; i += nl) row[i] = (unsigned char)(row[i] + prior[i]);
    } else if (ft != 0) {
      for (int k = lane; k < bpp; k += nl) png_unfilter_chain(row, prior, rowbytes, bpp, ft, k);
    }
    PNG_SYNC();
  }
  return PNG_OK;
}

// ---- pixels -------------------------------------------------------------------------------------------------------------
// Pixel x of an unfiltered row -> out[0..3] = R, G, B, A as Pillow's convert("RGBA") gives them (convert("RGB") drops
// A, convert("L") of a gray stream is R).  pal: the stream's 256 RGBA entries (palette streams only).
IMG_HD inline void png_expand(const int* d, const unsigned char* row, const unsigned char* pal, int x, int out[4]) {
  const int depth = d[PD_DEPTH], ct = d[PD_CTYPE];
  if (ct == 0 || ct == 3) {
    int s;
    if (depth == 8) {
      s = row[x];
    } else {
      const int bit = x * depth;
      s = (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
    }
    if (ct == 3) {
      for (int k = 0; k < 4; ++k) out[k] = pal[s * 4 + k];
    } else {
      const int v = s * (255 / ((1 << depth) - 1));
      out[0] = out[1] = out[2] = v;
      out[3] = d[PD_KEY] && s == d[PD_KEY0] ? 0 : 255;
    }
  } else if (ct == 4) {
    out[0] = out[1] = out[2] = row[2 * x];
    out[3] = row[2 * x + 1];
  } else if (ct == 2) {
    for (int k = 0; k < 3; ++k) out[k] = row[3 * x + k];
    out[3] = d[PD_KEY] && out[0] == d[PD_KEY0] && out[1] == d[PD_KEY0 + 1] && out[2] == d[PD_KEY0 + 2] ? 0 : 255;
  } else {
    for (int k = 0; k < 4; ++k) out[k] = row[4 * x + k];
  }
}

// The descriptor checks msml_png_decode makes on the host before it launches (also the host check's).  1 = fine.
inline int png_desc_ok(const int* d, long stream_bytes, long npal) {
  if (d[PD_STATUS] != 0) return d[PD_STATUS] > 0;           // a refused stream: nothing else is read
  const int H = d[PD_H], W = d[PD_W], dp = d[PD_DEPTH], ct = d[PD_CTYPE];
  if (H < 1 || H > 32767 || W < 1 || W > 32767) return 0;
  if (ct == 0 || ct == 3) {
    if (dp != 1 && dp != 2 && dp != 4 && dp != 8) return 0;
  } else if (ct == 2 || ct == 4 || ct == 6) {
    if (dp != 8) return 0;
  } else {
    return 0;
  }
  if (ct == 3 && (d[PD_PAL] < 0 || d[PD_PAL] >= npal)) return 0;
  if (d[PD_KEY] != 0 && (d[PD_KEY] != 1 || (ct != 0 && ct != 2))) return 0;
  if (d[PD_BASE] < 0 || d[PD_END] < 1 || d[PD_WS] < 0) return 0;
  if ((long)d[PD_BASE] * 4 + d[PD_END] > stream_bytes) return 0;
  return 1;
}
#endif
