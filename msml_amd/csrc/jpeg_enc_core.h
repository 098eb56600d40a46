// Baseline JPEG encoding, the arithmetic: plain C++ that the device code (jpeg_enc.hip) and the host check
// (tools/jpeg_enc_hostcheck.cpp, built with the host compiler and the sanitizers) both compile.  No intrinsics, no
// allocation, no floating point.  libjpeg's defaults restated: the 16-bit fixed-point RGB -> YCbCr conversion
// (jccolor.c), edge expansion and h2v1 / h2v2 downsampling (jcprepct.c, jcsample.c), JDCT_ISLOW forward
// (jfdctint.c), quantisation (jcdctmgr.c), dummy blocks (jccoefct.c) and Huffman coding with the standard tables of
// Annex K and restart intervals (jchuff.c).  tests/jpeg_enc_cases.py restates the same in numpy.
//
// Every function takes the thread's share as (t0, step) or one block / one byte group, so the kernels call them per
// thread and the host check calls them in plain loops: one copy of every rule.
#ifndef MSML_JPEG_ENC_CORE_H
#define MSML_JPEG_ENC_CORE_H
#include <stdint.h>

#include "packed_image.h"

// ---- the descriptor: JPE_DESC_WORDS int32 per image (msml_amd/jpeg.py writes it, msml_jpeg_encode checks it) ---------
#define JPE_DESC_WORDS 12
#define JE_SAMP 0   // 0 gray (one component), 1 4:4:4, 2 4:2:2, 3 4:2:0
#define JE_H 1
#define JE_W 2
#define JE_QT 3     // [2] quantisation table of luma and of chroma (index into qtabs)
#define JE_RI 5     // restart interval in MCUs, 0 = none, at most 65535 (DRI holds 16 bits)
#define JE_HOFF 6   // the image's header (SOI .. SOS) in `headers`: byte offset and length
#define JE_HLEN 7
#define JE_WS 8     // offset of the image's workspace in units of JPE_WS_ALIGN bytes (msml_jpeg_encode_workspace writes it)
#define JPE_WS_ALIGN 256

#define JPE_OK 0
#define JPE_ERR_SOURCE 1   // the meta row is not this image inside src
#define JPE_ERR_SLOT 2     // the slot is not inside dst, or is too small for the stream (or the stream is over 2^31 - 1 bytes)

// The most bits one block can take: 9 + 11 for the DC difference, (16 + 10) for each of 63 coefficients.
#define JPE_BLOCK_BITS (20 + 63 * 26)
#define JPE_BLOCK_BYTES 208   // JPE_BLOCK_BITS rounded up to whole bytes, then to a multiple of 16

struct JpeGeom {
  int samp, ncomp, hs, vs;   // sampling factors of luma (chroma is 1 x 1)
  int ny, bpm;               // luma blocks / all blocks of one MCU
  int H, W, mcux, mcuy, ri;
  int wib, hib;              // luma's width_in_blocks / height_in_blocks: blocks of an MCU past these are dummies
  long nmcu, nblk, nint;     // MCUs, blocks (dummies included), restart intervals
  // workspace of one image: coefficients int16 [nblk][64] (zigzag order, blocks in scan order), bit counts / offsets
  // int64 [nblk], interval byte offsets int64 [nint + 1], the unstuffed bit buffer uint32 [nblk * 52]
  long o_boff, o_ioff, o_ubuf, bytes;
};

IMG_HD inline void jpe_geom(const int* d, JpeGeom& G) {
  G.samp = d[JE_SAMP];
  G.ncomp = G.samp == 0 ? 1 : 3;
  G.hs = G.samp >= 2 ? 2 : 1;
  G.vs = G.samp == 3 ? 2 : 1;
  G.ny = G.hs * G.vs;
  G.bpm = G.samp == 0 ? 1 : G.ny + 2;
  G.H = d[JE_H];
  G.W = d[JE_W];
  G.ri = d[JE_RI];
  G.mcux = (G.W + 8 * G.hs - 1) / (8 * G.hs);
  G.mcuy = (G.H + 8 * G.vs - 1) / (8 * G.vs);
  G.wib = (G.W + 7) / 8;
  G.hib = (G.H + 7) / 8;
  G.nmcu = (long)G.mcux * G.mcuy;
  G.nblk = G.nmcu * G.bpm;
  G.nint = G.ri > 0 ? (G.nmcu + G.ri - 1) / G.ri : 1;
  G.o_boff = G.nblk * 128;
  G.o_ioff = G.o_boff + G.nblk * 8;
  G.o_ubuf = (G.o_ioff + (G.nint + 1) * 8 + 15) / 16 * 16;
  G.bytes = (G.o_ubuf + G.nblk * JPE_BLOCK_BYTES + (JPE_WS_ALIGN - 1)) / JPE_WS_ALIGN * JPE_WS_ALIGN;
}

// The checks msml_jpeg_encode makes on the host descriptors before it launches.  1 = fine.
inline int jpe_desc_ok(const int* d, int nq, long header_bytes) {
  if (d[JE_SAMP] < 0 || d[JE_SAMP] > 3) return 0;
  if (d[JE_H] < 1 || d[JE_H] > 32767 || d[JE_W] < 1 || d[JE_W] > 32767) return 0;
  if (d[JE_QT] < 0 || d[JE_QT] >= nq || d[JE_QT + 1] < 0 || d[JE_QT + 1] >= nq) return 0;
  if (d[JE_RI] < 0 || d[JE_RI] > 65535) return 0;
  if (d[JE_HOFF] < 0 || d[JE_HLEN] < 0 || (long)d[JE_HOFF] + d[JE_HLEN] > header_bytes || d[JE_WS] < 0) return 0;
  return 1;
}

// A slot capacity no stream of this geometry can exceed: every block at its most bits, every byte stuffed, one RSTn
// per interval, the header and EOI.  0 for arguments outside the supported range.
inline long jpe_bound(int H, int W, int samp, int ri, int header_bytes) {
  if (H < 1 || H > 32767 || W < 1 || W > 32767 || samp < 0 || samp > 3 || ri < 0 || ri > 65535 || header_bytes < 0) return 0;
  int d[JPE_DESC_WORDS] = {samp, H, W, 0, 0, ri, 0, 0, 0, 0, 0, 0};
  JpeGeom G;
  jpe_geom(d, G);
  return header_bytes + 2 * G.nblk * JPE_BLOCK_BYTES + 2 * G.nint + 2;
}

// The meta row [offset, H, W, pitch] of a source against the descriptor and the buffer: read, so its last row ends with
// its last pixel.
IMG_HD inline bool jpe_source_ok(const JpeGeom& G, const long* mt, int channels, long src_bytes) {
  const long rowb = (long)G.W * channels;
  return img_rect_ok(mt, G.H, G.W, rowb, rowb, src_bytes);
}

// ---- colour (jccolor.c) ---------------------------------------------------------------------------------------------
IMG_HD inline int jpe_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
IMG_HD inline int jpe_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
IMG_HD inline int jpe_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// The source row a chroma sample of full-resolution row y comes from (jcprepct.c, jcsample.c): the source is replicated
// only up to a multiple of vs, and the last DOWNSAMPLED row is what fills the rest of the block rows.
IMG_HD inline int jpe_chroma_row(const JpeGeom& G, int y) {
  const int cy = y / G.vs, j = y - cy * G.vs, chh = (G.H + G.vs - 1) / G.vs;
  const int r = (cy < chh ? cy : chh - 1) * G.vs + j;
  return r < G.H ? r : G.H - 1;
}

// ---- the tile: a run of MCUs of one MCU row, its samples staged as full-resolution Y, Cb, Cr planes ------------------------
// JPE_TILE_PIXELS samples per plane in every sampling: vs * 8 rows of jpe_tile_mcus() * hs * 8 columns.
#define JPE_TILE_PIXELS 2048
IMG_HD inline int jpe_tile_mcus(const JpeGeom& G) { return G.samp == 0 ? 32 : (G.samp == 3 ? 8 : 16); }

// Thread t0 of `step` stages its share of the tile at MCU row my, MCU column mx0.  img: the image's first byte.
// Columns past W repeat the last one (the right edge of every component is the replicated source); rows as above.
IMG_HD inline void jpe_stage(const JpeGeom& G, const unsigned char* img, long pitch, int channels, int swap_rb, int my,
                             int mx0, unsigned char* Y, unsigned char* Cb, unsigned char* Cr, int t0, int step) {
  const int tw = jpe_tile_mcus(G) * G.hs * 8, tr = G.vs * 8;
  const int xend = (G.mcux - mx0) * G.hs * 8;                // columns of the tile that belong to an MCU of the image
  const int ir = swap_rb ? 2 : 0, ib = swap_rb ? 0 : 2;
  const int sh = tw == 256 ? 8 : 7;                          // tw is 128 or 256
  for (int p = t0; p < tw * tr; p += step) {
    const int ty = p >> sh, tx = p - (ty << sh);
    if (tx >= xend) continue;
    int x = mx0 * G.hs * 8 + tx;
    x = x < G.W ? x : G.W - 1;
    const int y = my * tr + ty, ry = y < G.H ? y : G.H - 1;
    const unsigned char* s = img + (long)ry * pitch + (long)x * channels;
    if (channels == 1) {
      Y[p] = s[0];
      continue;
    }
    int r = s[ir], g = s[1], b = s[ib];
    Y[p] = (unsigned char)jpe_y(r, g, b);
    if (G.ncomp == 1) continue;
    const int rc = jpe_chroma_row(G, y);
    if (rc != ry) {
      s = img + (long)rc * pitch + (long)x * channels;
      r = s[ir], g = s[1], b = s[ib];
    }
    Cb[p] = (unsigned char)jpe_cb(r, g, b);
    Cr[p] = (unsigned char)jpe_cr(r, g, b);
  }
}

// Block j of the tile's MCU mloc: which component, where in the MCU, and whether it is a dummy (jccoefct.c).
IMG_HD inline void jpe_block_place(const JpeGeom& G, int my, int mx, int j, int& comp, int& jx, int& jy, bool& dummy) {
  comp = j < G.ny ? 0 : j - G.ny + 1;
  jx = comp == 0 ? j % G.hs : 0;
  jy = comp == 0 ? j / G.hs : 0;
  dummy = comp == 0 && (mx * G.hs + jx >= G.wib || my * G.vs + jy >= G.hib);
}

// The 64 samples of that block minus 128, chroma downsampled (jcsample.c: h2v1 bias 0, 1, 0, 1, .. and h2v2 bias
// 1, 2, 1, 2, .. by output column).
IMG_HD inline void jpe_block_samples(const JpeGeom& G, const unsigned char* Y, const unsigned char* Cb,
                                     const unsigned char* Cr, int mloc, int comp, int jx, int jy, int blk[64]) {
  const int tw = jpe_tile_mcus(G) * G.hs * 8;
  if (comp == 0 || G.hs == 1) {
    const unsigned char* p = (comp == 0 ? Y : (comp == 1 ? Cb : Cr)) + (jy * 8) * tw + (mloc * G.hs + jx) * 8;
    for (int r = 0; r < 8; ++r)
      for (int c = 0; c < 8; ++c) blk[r * 8 + c] = p[r * tw + c] - 128;
    return;
  }
  const unsigned char* p = (comp == 1 ? Cb : Cr) + mloc * 16;
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c) {
      if (G.vs == 1) {
        const unsigned char* q = p + r * tw + 2 * c;
        blk[r * 8 + c] = ((q[0] + q[1] + (c & 1)) >> 1) - 128;
      } else {
        const unsigned char* q = p + (2 * r) * tw + 2 * c;
        blk[r * 8 + c] = ((q[0] + q[1] + q[tw] + q[tw + 1] + 1 + (c & 1)) >> 2) - 128;
      }
    }
}

// ---- JDCT_ISLOW forward (jfdctint.c), CONST_BITS 13, PASS1_BITS 2 ----------------------------------------------------------
IMG_HD inline int jpe_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass over 8 values: pass 0 (rows) scales up by 4, pass 1 (columns) takes that out and divides by 8 less than a true DCT
IMG_HD inline void jpe_fdct_1d(const int d[8], int o[8], int pass) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int n = pass == 0 ? 11 : 15;
  o[0] = pass == 0 ? (t10 + t11) * 4 : jpe_descale(t10 + t11, 2);
  o[4] = pass == 0 ? (t10 - t11) * 4 : jpe_descale(t10 - t11, 2);
  const int z1e = (t12 + t13) * 4433;
  o[2] = jpe_descale(z1e + t13 * 6270, n);
  o[6] = jpe_descale(z1e - t12 * 15137, n);
  int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o[7] = jpe_descale(a4 + z1 + z3, n);
  o[5] = jpe_descale(a5 + z2 + z4, n);
  o[3] = jpe_descale(a6 + z2 + z3, n);
  o[1] = jpe_descale(a7 + z1 + z4, n);
}

IMG_HD inline void jpe_fdct(int blk[64]) {
  for (int r = 0; r < 8; ++r) {
    int d[8], o[8];
    for (int c = 0; c < 8; ++c) d[c] = blk[r * 8 + c];
    jpe_fdct_1d(d, o, 0);
    for (int c = 0; c < 8; ++c) blk[r * 8 + c] = o[c];
  }
  for (int c = 0; c < 8; ++c) {
    int d[8], o[8];
    for (int r = 0; r < 8; ++r) d[r] = blk[r * 8 + c];
    jpe_fdct_1d(d, o, 1);
    for (int r = 0; r < 8; ++r) blk[r * 8 + c] = o[r];
  }
}

// ---- quantisation (jcdctmgr.c): sign(c) * ((|c| + divisor / 2) / divisor), divisor = 8 q --------------------------------------
// The division is a multiplication by ceil(2^32 / divisor): exact while (|c| + divisor / 2) * divisor < 2^32, and
// |c| < 2^15, divisor <= 2040.  One division per table entry instead of one per coefficient.
IMG_HD inline uint32_t jpe_recip(uint32_t divisor) { return (uint32_t)(((1ull << 32) + divisor - 1) / divisor); }

// -> the coefficient, clamped to what the entropy coder can write (DC +-1024 so that differences stay within category
// 11, AC +-1023 = category 10; 8-bit samples never reach the clamps)
IMG_HD inline int jpe_quant(int c, uint32_t divisor, uint32_t recip, int limit) {
  const uint32_t a = (uint32_t)(c < 0 ? -c : c) + (divisor >> 1);
  int v = (int)(uint32_t)(((uint64_t)a * recip) >> 32);
  v = v > limit ? limit : v;
  return c < 0 ? -v : v;
}

// ---- the standard Huffman tables (Annex K.3 - K.6) --------------------------------------------------------------------------
// Code tables: JPE_HUFF_WORDS uint32 = DC luma [16], DC chroma [16], AC luma [256], AC chroma [256], indexed by the
// symbol, each (code << 5) | length.
#define JPE_HUFF_WORDS 544
#define JPE_HUFF_AC 32

struct JpeStdTable {
  unsigned char bits[16];
  unsigned char nval;
  unsigned char val[162];
};

IMG_HD inline const JpeStdTable& jpe_std_table(int which) {   // 0 DC luma, 1 DC chroma, 2 AC luma, 3 AC chroma
  static constexpr JpeStdTable T[4] = {
      {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
      {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
      {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
       162,
       {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
        0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
        0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
        0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
        0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
        0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
        0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
        0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
        0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
      {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
       162,
       {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
        0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
        0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
        0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
        0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
        0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
        0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
        0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
        0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}}};
  return T[which & 3];
}

// Thread t0 of `step` writes its share of the code tables: zeros first, then (after a barrier where step > 1) the p-th
// symbol of each table gets the canonical code of its length.
IMG_HD inline void jpe_huff_zero(uint32_t* tab, int t0, int step) {
  for (int i = t0; i < JPE_HUFF_WORDS; i += step) tab[i] = 0;
}
IMG_HD inline void jpe_huff_fill(uint32_t* tab, int t0, int step) {
  for (int w = 0; w < 4; ++w) {
    const JpeStdTable& T = jpe_std_table(w);
    uint32_t* out = tab + (w < 2 ? 16 * w : JPE_HUFF_AC + 256 * (w - 2));
    for (int p = t0; p < T.nval; p += step) {
      uint32_t code = 0;
      int k = 0;
      for (int l = 1; l <= 16; ++l) {
        const int cnt = T.bits[l - 1];
        if (p < k + cnt) {
          out[T.val[p]] = ((code + (uint32_t)(p - k)) << 5) | (uint32_t)l;
          break;
        }
        code = (code + cnt) << 1;
        k += cnt;
      }
    }
  }
}

// ---- entropy coding of one block (jchuff.c) ------------------------------------------------------------------------------------
IMG_HD inline int jpe_nbits(int a) { return a == 0 ? 0 : 32 - __builtin_clz((unsigned int)a); }

// The block whose DC this block's difference is taken from: the previous block of the same component in scan order,
// -1 at the start of a restart interval (prediction 0).
IMG_HD inline long jpe_pred_block(const JpeGeom& G, long b) {
  const long m = b / G.bpm;
  const int j = (int)(b - m * G.bpm);
  const bool first = G.ri > 0 ? m % G.ri == 0 : m == 0;
  if (j < G.ny) return j > 0 ? b - 1 : (first ? -1 : b - G.bpm + G.ny - 1);
  return first ? -1 : b - G.bpm;
}

// Sink: put(code, length) with length 1..16.  zz: the block in zigzag order.  One walk for the size pass and the emit pass.
template <class Sink>
IMG_HD inline void jpe_block_code(const int16_t* zz, int pred, const uint32_t* dct, const uint32_t* act, Sink& s) {
  int diff = (int)zz[0] - pred;
  diff = diff > 2047 ? 2047 : (diff < -2047 ? -2047 : diff);
  int cat = jpe_nbits(diff < 0 ? -diff : diff);
  s.put(dct[cat] >> 5, (int)(dct[cat] & 31));
  if (cat) s.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1), cat);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    int v = zz[k];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      s.put(act[0xF0] >> 5, (int)(act[0xF0] & 31));
      run -= 16;
    }
    v = v > 1023 ? 1023 : (v < -1023 ? -1023 : v);
    cat = jpe_nbits(v < 0 ? -v : v);
    const uint32_t e = act[(run << 4) | cat];
    s.put(e >> 5, (int)(e & 31));
    s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1), cat);
    run = 0;
  }
  if (run) s.put(act[0] >> 5, (int)(act[0] & 31));
}

struct JpeCountSink {
  int bits;
  IMG_HD void put(uint32_t, int len) { bits += len; }
};

// Bits into a zeroed buffer of 32-bit words at any bit position: the stream is big-endian, so a finished word is
// byte-swapped and OR-ed in (Word::merge: an integer OR-atomic on the device, a plain OR on the host).  The first and
// the last word of a block are shared with its neighbours; an OR never disturbs their bits.  nwords bounds every write.
template <class Word>
struct JpeBitSink {
  Word out;
  long w, nwords;
  uint64_t acc;
  int n;
  IMG_HD void begin(long bitpos) {
    w = bitpos >> 5;
    n = (int)(bitpos & 31);
    acc = 0;
  }
  IMG_HD void put(uint32_t code, int len) {
    acc |= (uint64_t)code << (64 - n - len);
    n += len;
    if (n >= 32) {
      flush((uint32_t)(acc >> 32));
      acc <<= 32;
      n -= 32;
    }
  }
  IMG_HD void flush(uint32_t v) {
    if (v != 0 && w >= 0 && w < nwords) out.merge(w, __builtin_bswap32(v));
    ++w;
  }
  // the end of a restart interval (or of the scan): 1 bits up to the byte boundary
  IMG_HD void pad() {
    const int k = (8 - (n & 7)) & 7;
    if (k) put((1u << k) - 1, k);
  }
  IMG_HD void end() {
    if (n > 0) flush((uint32_t)(acc >> 32));
  }
};

// ---- byte stuffing and markers: the unstuffed bytes of all intervals lie back to back ------------------------------------------
// the interval that holds unstuffed byte j: the last i with ioff[i] <= j (every interval has at least one byte)
IMG_HD inline long jpe_interval_of(const long* ioff, long nint, long j) {
  long lo = 0, hi = nint;
  while (hi - lo > 1) {
    const long mid = (lo + hi) >> 1;
    if (ioff[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Out: put(position in the slot, byte), which refuses positions outside the slot.  Unstuffed bytes [j0, j1) of the
// image, `ff` = the FF bytes in front of j0: every byte lands after the header, the stuffing bytes and the restart
// markers in front of it; an FF is followed by 00; the first byte of interval i > 0 is preceded by RST((i - 1) & 7).
template <class Out>
IMG_HD inline void jpe_pack_bytes(const unsigned char* ub, long j0, long j1, const long* ioff, long nint, long ff,
                                  int hlen, Out& out) {
  if (j0 >= j1) return;
  long i = jpe_interval_of(ioff, nint, j0);
  for (long j = j0; j < j1; ++j) {
    if (i + 1 < nint && j >= ioff[i + 1]) ++i;
    const long pos = hlen + j + ff + 2 * i;
    if (i > 0 && j == ioff[i]) {
      out.put(pos - 2, 0xFF);
      out.put(pos - 1, 0xD0 + (int)((i - 1) & 7));
    }
    const int v = ub[j];
    out.put(pos, v);
    if (v == 0xFF) {
      out.put(pos + 1, 0);
      ++ff;
    }
  }
}
#endif
