// PNG encoding, the per-image arithmetic shared by csrc/png_enc.hip and the host check (tools/png_enc_hostcheck.cpp):
// geometry and workspace layout, the row filters and their adaptive choice, the deflate symbol maps, the Huffman code
// builder, the dynamic block header, the bit writer, Adler-32 / CRC-32 algebra and the container.  Plain C++ (IMG_HD).
// tests/png_enc_cases.py restates the filter pass, the container and the bound.
#ifndef MSML_PNG_ENC_CORE_H
#define MSML_PNG_ENC_CORE_H
#include <stdint.h>

#include "packed_image.h"

#define PNGE_DESC_WORDS 4
enum { PE_H = 0, PE_W = 1, PE_WS = 2 };                      // descriptor words: height, width, workspace offset (units)
enum { PNGE_OK = 0, PNGE_ERR_SOURCE = 1, PNGE_ERR_SLOT = 2, PNGE_ERR_GEOMETRY = 3 };
enum { PNGE_NONE = 0, PNGE_SUB = 1, PNGE_UP = 2, PNGE_AVERAGE = 3, PNGE_PAETH = 4, PNGE_ADAPTIVE = 5 };
enum { PNGE_MODE_SKIPPED = 0, PNGE_MODE_FIXED = 1, PNGE_MODE_DYNAMIC = 2, PNGE_MODE_LITERALS = 3 };

#define PNGE_WS_ALIGN 256
#define PNGE_CHUNK 65535                                     // filtered bytes per deflate block = the largest stored block
#define PNGE_WINDOW 32768
#define PNGE_MIN_MATCH 4
#define PNGE_MAX_MATCH 258
#define PNGE_HASH_BITS 13
#define PNGE_MAX_BYTES 0x3fffffffL                           // filtered bytes of one image: positions stay in an int
#define PNGE_NLL 286
#define PNGE_ND 30
#define PNGE_NCL 19
#define PNGE_MAX_ITEMS 352                                   // 1 + 19 + 316 header items, rounded up
#define PNGE_REC_WORDS 8                                     // per-chunk record: mode, bits, adler sums

struct PngeGeom {
  int H, W, channels;
  long rb, stride, n;                                        // row bytes, filtered row bytes, filtered bytes
  long nchunks, bits_stride;
  long o_filt, o_tok, o_bits, o_rec, bytes;
};

IMG_HD inline bool pnge_size_ok(int H, int W, int channels) {
  return H >= 1 && H <= 32767 && W >= 1 && W <= 32767 && channels >= 1 && channels <= 4 &&
         (long)H * ((long)W * channels + 1) <= PNGE_MAX_BYTES;
}

IMG_HD inline long pnge_align(long v, long a) { return (v + a - 1) / a * a; }

IMG_HD inline void pnge_geom(int H, int W, int channels, PngeGeom& G) {
  G.H = H, G.W = W, G.channels = channels;
  G.rb = (long)W * channels;
  G.stride = G.rb + 1;
  G.n = (long)H * G.stride;
  G.nchunks = (G.n + PNGE_CHUNK - 1) / PNGE_CHUNK;
  G.bits_stride = pnge_align((G.n < PNGE_CHUNK ? G.n : PNGE_CHUNK) + 129, 64);
  G.o_filt = 0;
  G.o_tok = pnge_align(G.n + 8, 64);                         // tokens: one uint32 per filtered byte at most
  G.o_bits = G.o_tok + pnge_align(G.n * 4, 64);
  G.o_rec = G.o_bits + G.nchunks * G.bits_stride;
  G.bytes = pnge_align(G.o_rec + G.nchunks * PNGE_REC_WORDS * 4, PNGE_WS_ALIGN);
}

// 8 signature + 25 IHDR + 12 IDAT overhead + 2 zlib header + n + 5 per stored block + 4 Adler-32 + 12 IEND
IMG_HD inline long pnge_bound(int H, int W, int channels) {
  if (!pnge_size_ok(H, W, channels)) return 0;
  const long n = (long)H * ((long)W * channels + 1);
  return 8 + 25 + 12 + 2 + n + 5 * ((n + 65534) / 65535) + 4 + 12;
}

IMG_HD inline int pnge_colour_type(int channels) { return channels == 1 ? 0 : channels == 2 ? 4 : channels == 3 ? 2 : 6; }

// ------------------------------------------------------------------------------------------------------ filters
IMG_HD inline int pnge_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// x: the byte, a: left, b: above, c: above left (0 outside the image)
IMG_HD inline int pnge_filter(int f, int x, int a, int b, int c) {
  const int pred = f == PNGE_NONE ? 0 : f == PNGE_SUB ? a : f == PNGE_UP ? b : f == PNGE_AVERAGE ? (a + b) >> 1 : pnge_paeth(a, b, c);
  return (x - pred) & 255;
}

IMG_HD inline int pnge_abs8(int v) { return v < 128 ? v : 256 - v; }   // abs((int8) v)

// byte j of a source row with R and B exchanged (3 or 4 channels)
IMG_HD inline long pnge_src_index(long j, int channels, int swap_rb) {
  if (!swap_rb || channels < 3) return j;
  const int k = (int)(j % channels);
  return k == 0 ? j + 2 : k == 2 ? j - 2 : j;
}

// ---------------------------------------------------------------------------------------------- deflate symbols
IMG_HD inline int pnge_log2(unsigned int v) { return 31 - __builtin_clz(v); }

IMG_HD inline void pnge_len_symbol(int len, int& sym, int& ebits, int& extra) {   // len 3..258
  const int l = len - 3;
  if (l < 8) {
    sym = 257 + l, ebits = 0, extra = 0;
  } else if (len == 258) {
    sym = 285, ebits = 0, extra = 0;
  } else {
    const int k = pnge_log2((unsigned)l);
    ebits = k - 2;
    sym = 257 + 4 * (k - 1) + ((l - (1 << k)) >> ebits);
    extra = l & ((1 << ebits) - 1);
  }
}

IMG_HD inline void pnge_dist_symbol(int dist, int& sym, int& ebits, int& extra) { // dist 1..32768
  const int d = dist - 1;
  if (d < 4) {
    sym = d, ebits = 0, extra = 0;
  } else {
    const int k = pnge_log2((unsigned)d);
    ebits = k - 1;
    sym = 2 * k + ((d >> ebits) & 1);
    extra = d & ((1 << ebits) - 1);
  }
}

// a token: a literal byte, or bit 31 | (len - 3) << 16 | (dist - 1)
IMG_HD inline uint32_t pnge_match_token(int len, int dist) { return 0x80000000u | ((uint32_t)(len - 3) << 16) | (uint32_t)(dist - 1); }

IMG_HD inline uint32_t pnge_hash(uint32_t v) { return (v * 2654435761u) >> (32 - PNGE_HASH_BITS); }

IMG_HD inline int pnge_fixed_ll_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// -------------------------------------------------------------------------------------------------- Huffman codes
struct PngeScratch {                                         // working arrays of the builder (LDS on the device)
  uint32_t w[PNGE_NLL + 2], iw[PNGE_NLL + 2];
  uint16_t lp[PNGE_NLL + 2], ip[PNGE_NLL + 2], idepth[PNGE_NLL + 2], num[PNGE_NLL + 2];
  uint16_t seq[PNGE_NLL + PNGE_ND + 4];                      // code-length symbols: sym | extra << 8
  uint32_t cl_cnt[PNGE_NCL];
  uint16_t cl_sorted[PNGE_NCL], cl_code[PNGE_NCL];
  uint8_t cl_len[PNGE_NCL];
};

struct PngeBlockCode {                                       // one candidate coding of a block
  uint8_t ll_len[PNGE_NLL + 2], d_len[PNGE_ND + 2];
  uint16_t ll_code[PNGE_NLL + 2], d_code[PNGE_ND + 2];
  uint32_t items[PNGE_MAX_ITEMS];                            // header: value | nbits << 16, without the 3 block bits
  int nitems;
  long header_bits, body_bits;                               // body: the symbols and end of block, without extra bits
};

// sorted[0..m): the symbols with a count, ascending by (count, symbol).  -> len[0..n): an optimal prefix code where no
// length passes `limit` in the unlimited tree; a deeper tree is flattened the way miniz does (Kraft sum restored by
// lengthening the cheapest codes), which is valid but may cost a few bits more than package-merge.  Fewer than two
// symbols: two codes of one bit, which every inflater takes for all three alphabets.
IMG_HD inline void pnge_huff_lengths(const uint32_t* cnt, int n, const uint16_t* sorted, int m, int limit, uint8_t* len,
                                     PngeScratch& S) {
  for (int i = 0; i < n; ++i) len[i] = 0;
  if (m < 2) {
    const int s = m == 1 ? sorted[0] : 0;
    len[s] = 1;
    len[s == 0 ? 1 : 0] = 1;
    return;
  }
  for (int i = 0; i < m; ++i) S.w[i] = cnt[sorted[i]];
  int li = 0, ij = 0;
  for (int k = 0; k < m - 1; ++k) {                          // two queues: leaves and internal nodes, both ascending
    uint32_t sum = 0;
    for (int r = 0; r < 2; ++r) {
      if (li < m && (ij >= k || S.w[li] <= S.iw[ij])) {
        sum += S.w[li];
        S.lp[li++] = (uint16_t)k;
      } else {
        sum += S.iw[ij];
        S.ip[ij++] = (uint16_t)k;
      }
    }
    S.iw[k] = sum;
  }
  S.idepth[m - 2] = 0;
  for (int k = m - 3; k >= 0; --k) S.idepth[k] = (uint16_t)(S.idepth[S.ip[k]] + 1);
  for (int i = 0; i <= limit; ++i) S.num[i] = 0;
  for (int i = 0; i < m; ++i) {
    int d = S.idepth[S.lp[i]] + 1;
    S.num[d > limit ? limit : d]++;
  }
  long total = 0;
  for (int i = limit; i >= 1; --i) total += (long)S.num[i] << (limit - i);
  while (total > (1L << limit)) {
    S.num[limit]--;
    for (int i = limit - 1; i >= 1; --i)
      if (S.num[i]) {
        S.num[i]--;
        S.num[i + 1] += 2;
        break;
      }
    total--;
  }
  int idx = 0;
  for (int l = limit; l >= 1; --l)
    for (int c = S.num[l]; c > 0; --c) len[sorted[idx++]] = (uint8_t)l;   // the rarest symbols get the longest codes
}

// canonical codes, bit-reversed (deflate sends Huffman codes from their most significant bit)
IMG_HD inline void pnge_canonical(const uint8_t* len, int n, uint16_t* code) {
  int count[16], next[16];
  for (int i = 0; i < 16; ++i) count[i] = 0;
  for (int i = 0; i < n; ++i) count[len[i]]++;
  count[0] = 0;
  int c = 0;
  next[0] = 0;
  for (int b = 1; b < 16; ++b) {
    c = (c + count[b - 1]) << 1;
    next[b] = c;
  }
  for (int i = 0; i < n; ++i) {
    const int l = len[i];
    int v = l ? next[l]++ : 0, r = 0;
    for (int b = 0; b < l; ++b) r |= ((v >> b) & 1) << (l - 1 - b);
    code[i] = (uint16_t)r;
  }
}

IMG_HD inline void pnge_sort_small(const uint32_t* cnt, int n, uint16_t* sorted, int& m) {   // insertion sort
  m = 0;
  for (int s = 0; s < n; ++s) {
    if (!cnt[s]) continue;
    int i = m++;
    while (i > 0 && cnt[sorted[i - 1]] > cnt[s]) {
      sorted[i] = sorted[i - 1];
      --i;
    }
    sorted[i] = (uint16_t)s;
  }
}

IMG_HD inline int pnge_cl_order(int i) {
  constexpr unsigned char o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return o[i];
}

// From the counts and the code lengths already in B.ll_len / B.d_len: the canonical codes, the header of a dynamic block
// (HLIT, HDIST, HCLEN, the code-length code, the run-length coded lengths) as items, and the bit costs.
IMG_HD inline void pnge_dynamic_header(const uint32_t* ll_cnt, const uint32_t* d_cnt, PngeBlockCode& B, PngeScratch& S) {
  pnge_canonical(B.ll_len, PNGE_NLL, B.ll_code);
  pnge_canonical(B.d_len, PNGE_ND, B.d_code);
  int hlit = PNGE_NLL, hdist = PNGE_ND;
  while (hlit > 257 && B.ll_len[hlit - 1] == 0) --hlit;
  while (hdist > 1 && B.d_len[hdist - 1] == 0) --hdist;
  const int total = hlit + hdist;
  int ns = 0;
  for (int i = 0; i < PNGE_NCL; ++i) S.cl_cnt[i] = 0;
  for (int i = 0; i < total;) {
    const int v = i < hlit ? B.ll_len[i] : B.d_len[i - hlit];
    int run = 1;
    while (i + run < total && (i + run < hlit ? B.ll_len[i + run] : B.d_len[i + run - hlit]) == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int r = run > 138 ? 138 : run;
        S.seq[ns++] = (uint16_t)(18 | ((r - 11) << 8));
        S.cl_cnt[18]++;
        run -= r;
      }
      if (run >= 3) {
        S.seq[ns++] = (uint16_t)(17 | ((run - 3) << 8));
        S.cl_cnt[17]++;
        run = 0;
      }
    } else {
      S.seq[ns++] = (uint16_t)v;
      S.cl_cnt[v]++;
      --run;
      while (run >= 3) {
        const int r = run > 6 ? 6 : run;
        S.seq[ns++] = (uint16_t)(16 | ((r - 3) << 8));
        S.cl_cnt[16]++;
        run -= r;
      }
    }
    for (; run > 0; --run) {
      S.seq[ns++] = (uint16_t)v;
      S.cl_cnt[v]++;
    }
  }
  int m;
  pnge_sort_small(S.cl_cnt, PNGE_NCL, S.cl_sorted, m);
  pnge_huff_lengths(S.cl_cnt, PNGE_NCL, S.cl_sorted, m, 7, S.cl_len, S);
  pnge_canonical(S.cl_len, PNGE_NCL, S.cl_code);
  int hclen = PNGE_NCL;
  while (hclen > 4 && S.cl_len[pnge_cl_order(hclen - 1)] == 0) --hclen;
  int k = 0;
  long bits = 14 + 3 * hclen;
  B.items[k++] = (uint32_t)((hlit - 257) | ((hdist - 1) << 5) | ((hclen - 4) << 10)) | (14u << 16);
  for (int i = 0; i < hclen; ++i) B.items[k++] = (uint32_t)S.cl_len[pnge_cl_order(i)] | (3u << 16);
  for (int i = 0; i < ns; ++i) {
    const int s = S.seq[i] & 255, x = S.seq[i] >> 8;
    const int eb = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
    const int nb = S.cl_len[s] + eb;
    B.items[k++] = (uint32_t)(S.cl_code[s] | (x << S.cl_len[s])) | ((uint32_t)nb << 16);
    bits += nb;
  }
  B.nitems = k;
  B.header_bits = bits;
  long body = 0;
  for (int s = 0; s < PNGE_NLL; ++s) body += (long)ll_cnt[s] * B.ll_len[s];
  for (int s = 0; s < PNGE_ND; ++s) body += (long)d_cnt[s] * B.d_len[s];
  B.body_bits = body;
}

// the fixed code of a block and its cost for the same counts
IMG_HD inline void pnge_fixed_code(const uint32_t* ll_cnt, const uint32_t* d_cnt, PngeBlockCode& B) {
  for (int s = 0; s < PNGE_NLL + 2; ++s) B.ll_len[s] = (uint8_t)pnge_fixed_ll_len(s);
  for (int s = 0; s < PNGE_ND + 2; ++s) B.d_len[s] = 5;
  pnge_canonical(B.ll_len, PNGE_NLL + 2, B.ll_code);
  pnge_canonical(B.d_len, PNGE_ND + 2, B.d_code);
  B.nitems = 0;
  B.header_bits = 0;
  long body = 0;
  for (int s = 0; s < PNGE_NLL; ++s) body += (long)ll_cnt[s] * B.ll_len[s];
  for (int s = 0; s < PNGE_ND; ++s) body += 5L * d_cnt[s];
  B.body_bits = body;
}

// the bits of one token under a code, least significant bit first: -> nbits (at most 48)
IMG_HD inline int pnge_token_bits(uint32_t tok, const uint8_t* ll_len, const uint16_t* ll_code, const uint8_t* d_len,
                                  const uint16_t* d_code, uint64_t& v) {
  if (!(tok & 0x80000000u)) {
    v = ll_code[tok & 255];
    return ll_len[tok & 255];
  }
  int ls, le, lx, ds, de, dx;
  pnge_len_symbol((int)((tok >> 16) & 255) + 3, ls, le, lx);
  pnge_dist_symbol((int)(tok & 0xffff) + 1, ds, de, dx);
  int nb = 0;
  v = ll_code[ls];
  nb += ll_len[ls];
  v |= (uint64_t)lx << nb;
  nb += le;
  v |= (uint64_t)d_code[ds] << nb;
  nb += d_len[ds];
  v |= (uint64_t)dx << nb;
  nb += de;
  return nb;
}

// the largest size a compressed block may have and still be written to the scratch: a stored block costs at most that
IMG_HD inline long pnge_stored_max_bits(long len) { return 8 * len + 42; }
// where a stored block of len bytes that starts at bit `bo` ends
IMG_HD inline long pnge_stored_end(long bo, long len) { return ((bo + 3 + 7) & ~7L) + 32 + 8 * len; }

// ------------------------------------------------------------------------------------------- Adler-32 and CRC-32
#define PNGE_ADLER 65521u
// (a, b) after `len` more bytes whose plain sums are sa = sum d_i and sb = sum (len - i) d_i, both already mod 65521
IMG_HD inline void pnge_adler_append(uint32_t& a, uint32_t& b, uint32_t sa, uint32_t sb, long len) {
  b = (uint32_t)((b + (uint64_t)(len % PNGE_ADLER) * a + sb) % PNGE_ADLER);
  a = (a + sa) % PNGE_ADLER;
}

IMG_HD inline uint32_t pnge_crc_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
  return c;
}

// a * b mod the CRC polynomial, bit-reflected operands (x^0 is bit 31)
IMG_HD inline uint32_t pnge_gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}

// x^(8 n): the operator that n zero bytes apply to a CRC register
IMG_HD inline uint32_t pnge_gf_x8n(long n) {
  uint32_t r = 0x80000000u, p = 0x00800000u;                 // 1 and x^8
  for (; n; n >>= 1) {
    if (n & 1) r = pnge_gf_mul(r, p);
    p = pnge_gf_mul(p, p);
  }
  return r;
}

// raw register (start 0, no final xor) over bytes; the CRC-32 of a message of n bytes is
// raw ^ pnge_gf_mul(pnge_gf_x8n(n), 0xffffffff) ^ 0xffffffff
IMG_HD inline uint32_t pnge_crc_finish(uint32_t raw, long n) { return raw ^ pnge_gf_mul(pnge_gf_x8n(n), 0xffffffffu) ^ 0xffffffffu; }

// ------------------------------------------------------------------------------------------------------ container
#define PNGE_HEAD_BYTES 41                                   // signature, IHDR chunk, IDAT length and type
// the 41 bytes in front of the zlib stream; idat_len: the stream's bytes.  table: the 256 CRC entries.
template <class Out>
IMG_HD inline void pnge_head(Out& out, int H, int W, int channels, long idat_len, const uint32_t* table) {
  const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  unsigned char h[17] = {'I', 'H', 'D', 'R', (unsigned char)(W >> 24), (unsigned char)(W >> 16), (unsigned char)(W >> 8),
                         (unsigned char)W, (unsigned char)(H >> 24), (unsigned char)(H >> 16), (unsigned char)(H >> 8),
                         (unsigned char)H, 8, (unsigned char)pnge_colour_type(channels), 0, 0, 0};
  for (int i = 0; i < 8; ++i) out.put(i, sig[i]);
  out.put(8, 0), out.put(9, 0), out.put(10, 0), out.put(11, 13);
  uint32_t c = 0xffffffffu;
  for (int i = 0; i < 17; ++i) {
    out.put(12 + i, h[i]);
    c = table[(c ^ h[i]) & 255] ^ (c >> 8);
  }
  c ^= 0xffffffffu;
  for (int i = 0; i < 4; ++i) out.put(29 + i, (int)((c >> (24 - 8 * i)) & 255));
  for (int i = 0; i < 4; ++i) out.put(33 + i, (int)((idat_len >> (24 - 8 * i)) & 255));
  out.put(37, 'I'), out.put(38, 'D'), out.put(39, 'A'), out.put(40, 'T');
}

// what follows the stream at `pos`: the IDAT chunk's CRC and the IEND chunk (16 bytes)
template <class Out>
IMG_HD inline void pnge_tail(Out& out, long pos, uint32_t idat_crc) {
  const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
  for (int i = 0; i < 4; ++i) out.put(pos + i, (int)((idat_crc >> (24 - 8 * i)) & 255));
  for (int i = 0; i < 12; ++i) out.put(pos + 4 + i, iend[i]);
}

#endif
