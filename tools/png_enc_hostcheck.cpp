// Host check of the PNG encoder's core (msml_amd/csrc/png_enc_core.h): the device passes of csrc/png_enc.hip restated
// step for step as sequential code around the same header (64 positions per step, the table read before it is
// updated, the greedy walk, the candidates' costs, the chunk walk of the emit pass, the CRC from 256 pieces), built
// with -fsanitize=address,undefined by tests/hostcheck.py and run as a process of its own.
//   png_enc_hostcheck in.bin out.bin
// in.bin: int32 count, then per case int32 H, W, channels, filter, swap_rb and H * W * channels bytes.
// out.bin: per case int32 length and the file.  The test inflates every file with zlib and compares.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../msml_amd/csrc/png_enc_core.h"

struct VecOut {
  std::vector<unsigned char>& v;
  long base;
  void put(long pos, int x) { v.at((size_t)(base + pos)) = (unsigned char)x; }
};

static void sort_symbols(const uint32_t* cnt, int n, uint16_t* sorted, int& m) {
  m = 0;
  for (int s = 0; s < n; ++s)
    if (cnt[s]) sorted[m++] = (uint16_t)s;
  std::sort(sorted, sorted + m, [&](uint16_t a, uint16_t b) { return cnt[a] != cnt[b] ? cnt[a] < cnt[b] : a < b; });
}

struct BitOut {
  std::vector<unsigned char>& v;
  long bits = 0;
  void put(uint64_t x, int nb) {
    for (int i = 0; i < nb; ++i, ++bits) {
      if ((size_t)(bits >> 3) >= v.size()) v.push_back(0);
      v[(size_t)(bits >> 3)] |= (unsigned char)(((x >> i) & 1) << (bits & 7));
    }
  }
};

struct ChunkOut {
  int mode;
  long bits;
  uint32_t sa, sb;
  std::vector<unsigned char> data;
};

static int match_len(const unsigned char* a, const unsigned char* b, int maxlen) {
  int l = 0;
  while (l < maxlen && a[l] == b[l]) ++l;
  return l;
}

static void deflate_chunk(const std::vector<unsigned char>& filt, const PngeGeom& G, long chunk, ChunkOut& out) {
  const unsigned char* f = filt.data();
  const int ntot = (int)G.n, c0 = (int)(chunk * PNGE_CHUNK);
  const int len = ntot - c0 < PNGE_CHUNK ? ntot - c0 : PNGE_CHUNK, cend = c0 + len;
  const int stride = (int)(G.stride <= PNGE_WINDOW ? G.stride : 0);
  std::vector<uint32_t> hash(1 << PNGE_HASH_BITS, 0), tok;
  uint32_t ll[PNGE_NLL + 2] = {0}, dd[PNGE_ND + 2] = {0}, lit[PNGE_NLL + 2] = {0}, nod[PNGE_ND + 2] = {0};
  auto word = [&](int p) { return (uint32_t)(f[p] | (f[p + 1] << 8) | (f[p + 2] << 16) | ((uint32_t)f[p + 3] << 24)); };
  for (int p = c0 > PNGE_WINDOW ? c0 - PNGE_WINDOW : 0; p < c0; ++p)
    if (p + 4 <= ntot) hash[pnge_hash(word(p))] = std::max(hash[pnge_hash(word(p))], (uint32_t)(p + 1));
  int next = c0;
  long extra = 0;
  unsigned long long sa = 0, sb = 0;
  for (int b0 = c0; b0 < cend; b0 += 64) {
    int best[64] = {0}, bdist[64] = {0};
    uint32_t cand[64] = {0};
    const int lim = std::min(b0 + 64, cend);
    for (int p = b0; p < lim; ++p) {
      lit[f[p]]++;
      sa += f[p];
      sb += (unsigned long long)(cend - p) * f[p];
      if (p + 4 <= ntot) cand[p - b0] = hash[pnge_hash(word(p))];
    }
    for (int p = b0; p < lim; ++p)
      if (p + 4 <= ntot) hash[pnge_hash(word(p))] = std::max(hash[pnge_hash(word(p))], (uint32_t)(p + 1));
    for (int p = std::max(b0, next); p < lim; ++p) {
      const int maxlen = std::min(cend - p, PNGE_MAX_MATCH);
      int b = 0, bd = 0;
      if (maxlen >= PNGE_MIN_MATCH) {
        if (cand[p - b0]) {
          const int dist = p - (int)(cand[p - b0] - 1);
          if (dist >= 1 && dist <= PNGE_WINDOW) b = match_len(f + p - dist, f + p, maxlen), bd = dist;
        }
        if (stride && p >= stride && stride != bd) {
          const int l = match_len(f + p - stride, f + p, maxlen);
          if (l > b || (l == b && stride < bd)) b = l, bd = stride;
        }
      }
      best[p - b0] = b < PNGE_MIN_MATCH ? 0 : b;
      bdist[p - b0] = bd;
    }
    int cur = std::max(next, b0);
    while (cur < lim) {
      const int l = best[cur - b0];
      if (l) {
        int ls, le, lx, ds, de, dx;
        pnge_len_symbol(l, ls, le, lx);
        pnge_dist_symbol(bdist[cur - b0], ds, de, dx);
        tok.push_back(pnge_match_token(l, bdist[cur - b0]));
        ll[ls]++, dd[ds]++;
        extra += le + de;
      } else {
        tok.push_back(f[cur]);
        ll[f[cur]]++;
      }
      cur += l ? l : 1;
    }
    next = cur;
  }
  ll[256] = 1, lit[256] = 1;
  out.sa = (uint32_t)(sa % PNGE_ADLER), out.sb = (uint32_t)(sb % PNGE_ADLER);
  static PngeScratch S;
  static PngeBlockCode B[2];
  uint16_t sorted[PNGE_NLL + 2];
  int m;
  pnge_fixed_code(ll, dd, B[0]);
  const long cost_fixed = 3 + B[0].body_bits + extra;
  sort_symbols(ll, PNGE_NLL, sorted, m);
  pnge_huff_lengths(ll, PNGE_NLL, sorted, m, 15, B[0].ll_len, S);
  sort_symbols(dd, PNGE_ND, sorted, m);
  pnge_huff_lengths(dd, PNGE_ND, sorted, m, 15, B[0].d_len, S);
  pnge_dynamic_header(ll, dd, B[0], S);
  const long cost_dyn = 3 + B[0].header_bits + B[0].body_bits + extra;
  sort_symbols(lit, PNGE_NLL, sorted, m);
  pnge_huff_lengths(lit, PNGE_NLL, sorted, m, 15, B[1].ll_len, S);
  pnge_huff_lengths(nod, PNGE_ND, sorted, 0, 15, B[1].d_len, S);
  pnge_dynamic_header(lit, nod, B[1], S);
  const long cost_lit = 3 + B[1].header_bits + B[1].body_bits;
  int mode = PNGE_MODE_FIXED;
  long bits = cost_fixed;
  if (cost_dyn < bits) mode = PNGE_MODE_DYNAMIC, bits = cost_dyn;
  if (cost_lit < bits) mode = PNGE_MODE_LITERALS, bits = cost_lit;
  if (bits > pnge_stored_max_bits(len)) mode = PNGE_MODE_SKIPPED;
  out.mode = mode;
  out.bits = mode == PNGE_MODE_SKIPPED ? 0 : bits;
  out.data.clear();
  if (mode == PNGE_MODE_SKIPPED) return;
  if (mode == PNGE_MODE_FIXED) pnge_fixed_code(ll, dd, B[0]);
  const PngeBlockCode& C = B[mode == PNGE_MODE_LITERALS ? 1 : 0];
  BitOut bo{out.data};
  bo.put((uint64_t)((chunk + 1 == G.nchunks ? 1 : 0) | ((mode == PNGE_MODE_FIXED ? 1 : 2) << 1)), 3);
  for (int i = 0; i < C.nitems; ++i) bo.put(C.items[i] & 0xffffu, (int)(C.items[i] >> 16));
  const int nbody = mode == PNGE_MODE_LITERALS ? len : (int)tok.size();
  for (int k = 0; k < nbody; ++k) {
    uint64_t v;
    const int nb = pnge_token_bits(mode == PNGE_MODE_LITERALS ? (uint32_t)f[c0 + k] : tok[k], C.ll_len, C.ll_code, C.d_len,
                                   C.d_code, v);
    bo.put(v, nb);
  }
  bo.put(C.ll_code[256], C.ll_len[256]);
  if (bo.bits != bits) {
    fprintf(stderr, "chunk %ld: %ld bits written, %ld counted\n", chunk, bo.bits, bits);
    exit(3);
  }
}

static std::vector<unsigned char> encode(const unsigned char* px, int H, int W, int channels, int filter, int swap_rb) {
  PngeGeom G;
  pnge_geom(H, W, channels, G);
  std::vector<unsigned char> filt((size_t)G.n);
  for (int y = 0; y < H; ++y) {
    const unsigned char* row = px + (size_t)y * G.rb;
    const unsigned char* up = y ? row - G.rb : nullptr;
    int f = filter;
    auto val = [&](int k, long j) {
      const long js = pnge_src_index(j, channels, swap_rb);
      return pnge_filter(k, row[js], j >= channels ? row[js - channels] : 0, y ? up[js] : 0,
                         (y && j >= channels) ? up[js - channels] : 0);
    };
    if (filter == PNGE_ADAPTIVE) {
      unsigned sum[5] = {0, 0, 0, 0, 0};
      for (long j = 0; j < G.rb; ++j)
        for (int k = 0; k < 5; ++k) sum[k] += pnge_abs8(val(k, j));
      f = 0;
      for (int k = 1; k < 5; ++k)
        if (sum[k] < sum[f]) f = k;
    }
    filt[(size_t)y * G.stride] = (unsigned char)f;
    for (long j = 0; j < G.rb; ++j) filt[(size_t)(y * G.stride + 1 + j)] = (unsigned char)val(f, j);
  }
  std::vector<ChunkOut> ch((size_t)G.nchunks);
  for (long c = 0; c < G.nchunks; ++c) deflate_chunk(filt, G, c, ch[(size_t)c]);
  // the emit pass
  uint32_t table[256];
  for (uint32_t i = 0; i < 256; ++i) table[i] = pnge_crc_entry(i);
  long bo = 16;
  uint32_t a = 1, b = 0;
  std::vector<long> at((size_t)G.nchunks);
  std::vector<char> packed((size_t)G.nchunks);
  for (long c = 0; c < G.nchunks; ++c) {
    const long c0 = c * PNGE_CHUNK, len = std::min<long>(G.n - c0, PNGE_CHUNK), se = pnge_stored_end(bo, len);
    packed[c] = ch[c].mode != PNGE_MODE_SKIPPED && ch[c].bits > 0 && bo + ch[c].bits < se;
    at[c] = bo;
    bo = packed[c] ? bo + ch[c].bits : se;
    pnge_adler_append(a, b, ch[c].sa, ch[c].sb, len);
  }
  const long zend = (bo + 7) >> 3, idat = zend + 4, total = PNGE_HEAD_BYTES + idat + 16;
  if (total > pnge_bound(H, W, channels)) {
    fprintf(stderr, "%d x %d x %d: %ld bytes pass the bound %ld\n", H, W, channels, total, pnge_bound(H, W, channels));
    exit(4);
  }
  std::vector<unsigned char> file((size_t)total, 0xEE);
  VecOut fo{file, 0}, z{file, PNGE_HEAD_BYTES};
  z.put(0, 0x78), z.put(1, 0x01);
  int carry = 0;
  for (long c = 0; c < G.nchunks; ++c) {
    const long c0 = c * PNGE_CHUNK, len = std::min<long>(G.n - c0, PNGE_CHUNK);
    const int s = (int)(at[c] & 7);
    const long d0 = at[c] >> 3;
    const bool last = c + 1 == G.nchunks;
    if (packed[c]) {
      const unsigned char* sp = ch[c].data.data();
      const long nb = ch[c].bits, nsrc = (nb + 7) >> 3, e = at[c] + nb, dl = (e - 1) >> 3;
      const bool whole = (e & 7) == 0 || last;
      auto byte = [&](long k) {
        const int lo = k < nsrc ? sp[k] : 0, hi = (k >= 1 && k - 1 < nsrc) ? sp[k - 1] : 0;
        return (((lo << s) | (hi >> (8 - s))) & 255) | (k == 0 ? carry : 0);
      };
      for (long k = 0; k < dl - d0 + (whole ? 1 : 0); ++k) z.put(d0 + k, byte(k));
      carry = whole ? 0 : byte(dl - d0);
    } else {
      const long p = (at[c] + 3 + 7) >> 3;
      z.put(d0, carry | ((last ? 1 : 0) << s));
      for (long j = d0 + 1; j < p; ++j) z.put(j, 0);
      z.put(p, (int)(len & 255)), z.put(p + 1, (int)(len >> 8));
      z.put(p + 2, (int)(~len & 255)), z.put(p + 3, (int)((~len >> 8) & 255));
      for (long k = 0; k < len; ++k) z.put(p + 4 + k, filt[(size_t)(c0 + k)]);
      carry = 0;
    }
  }
  const uint32_t adler = (b << 16) | a;
  for (int i = 0; i < 4; ++i) z.put(zend + i, (int)((adler >> (24 - 8 * i)) & 255));
  pnge_head(fo, H, W, channels, idat, table);
  const long M = 4 + idat, P = (M + 255) / 256, pad = 256 * P - M;
  const unsigned char* m = file.data() + 37;
  const uint32_t op = pnge_gf_x8n(P);
  uint32_t acc = 0;
  for (int t = 0; t < 256; ++t) {
    uint32_t cr = 0;
    for (long v = std::max<long>(t * P - pad, 0); v < t * P - pad + P; ++v) cr = table[(cr ^ m[v]) & 255] ^ (cr >> 8);
    acc = pnge_gf_mul(op, acc) ^ cr;
  }
  pnge_tail(fo, PNGE_HEAD_BYTES + idat, pnge_crc_finish(acc, M));
  return file;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) {
    perror("open");
    return 2;
  }
  int count = 0;
  if (fread(&count, 4, 1, fi) != 1 || count < 0) return 2;
  for (int i = 0; i < count; ++i) {
    int hd[5];
    if (fread(hd, 4, 5, fi) != 5 || !pnge_size_ok(hd[0], hd[1], hd[2]) || hd[3] < 0 || hd[3] > 5) {
      fprintf(stderr, "bad case %d\n", i);
      return 2;
    }
    std::vector<unsigned char> px((size_t)hd[0] * hd[1] * hd[2]);
    if (fread(px.data(), 1, px.size(), fi) != px.size()) return 2;
    const std::vector<unsigned char> file = encode(px.data(), hd[0], hd[1], hd[2], hd[3], hd[4]);
    const int n = (int)file.size();
    fwrite(&n, 4, 1, fo);
    fwrite(file.data(), 1, file.size(), fo);
  }
  fclose(fi);
  fclose(fo);
  printf("ok %d\n", count);
  return 0;
}
