// Host check of the JPEG encoder's arithmetic: msml_amd/csrc/jpeg_enc_core.h compiled with the host compiler (and
// -fsanitize=address,undefined by tests/test_jpeg_enc_cpu.py), run in the order the kernels of csrc/jpeg_enc.hip run it.
//   jpeg_enc_hostcheck <input> <output>
// input  (tests/jpeg_enc_cases.write_hostcheck_input): int32 [8] = magic, cases, nq, header bytes, source bytes, random
//        cases, seed, 0; desc int32 [cases][12]; meta int64 [cases][4]; qtabs int32 [nq][64]; headers; sources (RGB).
// output: per case int32 status, int32 length, the stream.
// Every workspace and every slot is a heap block of exactly its size, so a write outside one is an ASan report.  After
// the fixture's cases come `random` images of random sizes, samplings, restart intervals, channel counts and pitches,
// each encoded into a slot of the bound (checked: status 0, length within the bound, two runs equal) and into a slot one
// byte too small (checked: status 2, length 0).  Last, the rules of img_rect_ok on hand-made meta rows.
// stdout: "R <random cases> <failures>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../msml_amd/csrc/jpeg_enc_core.h"

struct HostWord {
  uint32_t* p;
  void merge(long w, uint32_t v) { p[w] |= v; }
};

struct HostOut {
  unsigned char* slot;
  long cap;
  void put(long pos, int v) {
    if (pos >= 0 && pos < cap) slot[pos] = (unsigned char)v;
  }
};

static int encode_one(const int* d, const unsigned char* src, long src_bytes, const long* mt, int channels, int swap_rb,
                      const int* qtabs, const unsigned char* headers, unsigned char* slot, long cap, int* length) {
  JpeGeom G;
  jpe_geom(d, G);
  *length = 0;
  if (!jpe_source_ok(G, mt, channels, src_bytes)) return JPE_ERR_SOURCE;
  std::vector<unsigned char> wsv((size_t)G.bytes);
  unsigned char* ws = wsv.data();
  int16_t* coef = reinterpret_cast<int16_t*>(ws);
  long* boff = reinterpret_cast<long*>(ws + G.o_boff);
  long* ioff = reinterpret_cast<long*>(ws + G.o_ioff);
  uint32_t* ubuf = reinterpret_cast<uint32_t*>(ws + G.o_ubuf);
  uint32_t huff[JPE_HUFF_WORDS];
  jpe_huff_zero(huff, 0, 1);
  jpe_huff_fill(huff, 0, 1);
  uint32_t div[2][64], rcp[2][64];
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      div[t][k] = 8u * (uint32_t)qtabs[(long)d[JE_QT + t] * 64 + img_zigzag(k)];
      rcp[t][k] = jpe_recip(div[t][k]);
    }
  // k_jpeg_enc_dct
  const int tm = jpe_tile_mcus(G);
  std::vector<unsigned char> Y(JPE_TILE_PIXELS), Cb(JPE_TILE_PIXELS), Cr(JPE_TILE_PIXELS);
  std::vector<int> dc(64);
  for (int my = 0; my < G.mcuy; ++my)
    for (int mx0 = 0; mx0 < G.mcux; mx0 += tm) {
      jpe_stage(G, src + mt[0], mt[3], channels, swap_rb, my, mx0, Y.data(), Cb.data(), Cr.data(), 0, 1);
      for (int pass = 0; pass < 2; ++pass)
        for (int t = 0; t < tm * G.bpm; ++t) {
          const int mloc = t / G.bpm, j = t % G.bpm, mx = mx0 + mloc;
          if (mx >= G.mcux) continue;
          int comp, jx, jy;
          bool dummy;
          jpe_block_place(G, my, mx, j, comp, jx, jy, dummy);
          const long b = ((long)my * G.mcux + mx) * G.bpm + j;
          int16_t* out = coef + b * 64;
          if (pass == 0 && !dummy) {
            int blk[64];
            jpe_block_samples(G, Y.data(), Cb.data(), Cr.data(), mloc, comp, jx, jy, blk);
            jpe_fdct(blk);
            const int tb = comp ? 1 : 0;
            for (int k = 0; k < 64; ++k)
              out[k] = (int16_t)jpe_quant(blk[img_zigzag(k)], div[tb][k], rcp[tb][k], k ? 1023 : 1024);
            dc[t] = out[0];
            memset(ubuf + b * (JPE_BLOCK_BYTES / 4), 0, JPE_BLOCK_BYTES);
          } else if (pass == 1 && dummy) {
            int s = t - 1;
            for (;;) {
              int c2, x2, y2;
              bool d2;
              jpe_block_place(G, my, mx, s - mloc * G.bpm, c2, x2, y2, d2);
              if (!d2) break;
              --s;
            }
            for (int k = 0; k < 64; ++k) out[k] = 0;
            out[0] = (int16_t)dc[s];
            memset(ubuf + b * (JPE_BLOCK_BYTES / 4), 0, JPE_BLOCK_BYTES);
          }
        }
    }
  // k_jpeg_enc_size
  for (long b = 0; b < G.nblk; ++b) {
    const long pb = jpe_pred_block(G, b);
    const int j = (int)(b % G.bpm), tb = j < G.ny ? 0 : 1;
    JpeCountSink cs = {0};
    jpe_block_code(coef + b * 64, pb < 0 ? 0 : coef[pb * 64], huff + 16 * tb, huff + JPE_HUFF_AC + 256 * tb, cs);
    boff[b] = cs.bits;
  }
  // k_jpeg_enc_scan
  const long per = G.ri > 0 ? (long)G.ri * G.bpm : G.nblk;   // blocks of a whole interval
  long run = 0;
  for (long b = 0; b < G.nblk; ++b) {
    if (b % per == 0) run = 0;
    const long v = boff[b];
    boff[b] = run;
    run += v;
    if (b + 1 == G.nblk || (b + 1) % per == 0) ioff[b / per] = (run + 7) >> 3;
  }
  long U = 0;
  for (long i = 0; i < G.nint; ++i) {
    const long v = ioff[i];
    ioff[i] = U;
    U += v;
  }
  ioff[G.nint] = U;
  // k_jpeg_enc_emit
  for (long b = 0; b < G.nblk; ++b) {
    const long pb = jpe_pred_block(G, b);
    const int j = (int)(b % G.bpm), tb = j < G.ny ? 0 : 1;
    JpeBitSink<HostWord> bs;
    bs.out.p = ubuf;
    bs.nwords = G.nblk * (JPE_BLOCK_BYTES / 4);
    bs.begin(ioff[b / per] * 8 + boff[b]);
    jpe_block_code(coef + b * 64, pb < 0 ? 0 : coef[pb * 64], huff + 16 * tb, huff + JPE_HUFF_AC + 256 * tb, bs);
    if (b + 1 == G.nblk || (b + 1) % per == 0) bs.pad();
    bs.end();
  }
  // k_jpeg_enc_pack
  HostOut out = {slot, cap};
  const int hlen = d[JE_HLEN];
  for (int i = 0; i < hlen; ++i) out.put(i, headers[d[JE_HOFF] + i]);
  const unsigned char* ub = reinterpret_cast<const unsigned char*>(ubuf);
  long ff = 0;
  for (long j0 = 0; j0 < U; j0 += 4) {
    const long j1 = j0 + 4 < U ? j0 + 4 : U;
    jpe_pack_bytes(ub, j0, j1, ioff, G.nint, ff, hlen, out);
    for (long j = j0; j < j1; ++j) ff += ub[j] == 0xFF;
  }
  const long L = hlen + U + ff + 2 * (G.nint - 1) + 2;
  if (L > cap || L > 0x7fffffffL) return JPE_ERR_SLOT;
  out.put(L - 2, 0xFF);
  out.put(L - 1, 0xD9);
  *length = (int)L;
  return JPE_OK;
}

static uint32_t rng_state;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int head[8];
  if (fread(head, 4, 8, f) != 8 || head[0] != 0x4A454331) return 2;
  const int n = head[1], nq = head[2], hbytes = head[3], sbytes = head[4], nrandom = head[5];
  rng_state = (uint32_t)head[6];
  std::vector<int> desc((size_t)n * JPE_DESC_WORDS), qtabs((size_t)nq * 64);
  std::vector<long> meta((size_t)n * 4);
  std::vector<unsigned char> headers((size_t)hbytes), src((size_t)sbytes);
  if (fread(desc.data(), 4, desc.size(), f) != desc.size() || fread(meta.data(), 8, meta.size(), f) != meta.size() ||
      fread(qtabs.data(), 4, qtabs.size(), f) != qtabs.size() || fread(headers.data(), 1, hbytes, f) != (size_t)hbytes ||
      fread(src.data(), 1, sbytes, f) != (size_t)sbytes)
    return 2;
  fclose(f);
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 2;
  for (int i = 0; i < n; ++i) {
    const int* d = &desc[(size_t)i * JPE_DESC_WORDS];
    if (!jpe_desc_ok(d, nq, hbytes)) return 3;
    const long cap = jpe_bound(d[JE_H], d[JE_W], d[JE_SAMP], d[JE_RI], d[JE_HLEN]);
    std::vector<unsigned char> slot((size_t)cap);
    int len = 0;
    const int st = encode_one(d, src.data(), sbytes, &meta[(size_t)i * 4], 3, 0, qtabs.data(), headers.data(), slot.data(),
                              cap, &len);
    fwrite(&st, 4, 1, g);
    fwrite(&len, 4, 1, g);
    fwrite(slot.data(), 1, (size_t)len, g);
  }
  fclose(g);
  int failures = 0;
  for (int i = 0; i < nrandom; ++i) {
    int d[JPE_DESC_WORDS] = {0};
    const int big = rnd() % 16 == 0;
    d[JE_SAMP] = (int)(rnd() % 4);
    d[JE_H] = 1 + (int)(rnd() % (big ? 150 : 40));
    d[JE_W] = 1 + (int)(rnd() % (big ? 300 : 40));
    d[JE_QT] = (int)(rnd() % nq);
    d[JE_QT + 1] = (int)(rnd() % nq);
    d[JE_RI] = rnd() % 2 ? 0 : 1 + (int)(rnd() % 7);
    d[JE_HLEN] = (int)(rnd() % (hbytes + 1));
    d[JE_HOFF] = (int)(rnd() % (hbytes - d[JE_HLEN] + 1));
    const int channels = d[JE_SAMP] == 0 && rnd() % 2 ? 1 : 3, swap_rb = (int)(rnd() % 2);
    const long pitch = (long)d[JE_W] * channels + rnd() % 5, off = rnd() % 7;
    const long mt[4] = {off, d[JE_H], d[JE_W], pitch};
    const long need = off + (long)(d[JE_H] - 1) * pitch + (long)d[JE_W] * channels;
    std::vector<unsigned char> img((size_t)need);
    const int flat = rnd() % 4 == 0;
    for (auto& v : img) v = (unsigned char)(flat ? (rnd() & 1 ? 255 : 0) : rnd());
    const long cap = jpe_bound(d[JE_H], d[JE_W], d[JE_SAMP], d[JE_RI], d[JE_HLEN]);
    std::vector<unsigned char> a((size_t)cap), b((size_t)cap);
    int la = 0, lb = 0;
    const int sa = encode_one(d, img.data(), need, mt, channels, swap_rb, qtabs.data(), headers.data(), a.data(), cap, &la);
    const int sb = encode_one(d, img.data(), need, mt, channels, swap_rb, qtabs.data(), headers.data(), b.data(), cap, &lb);
    bool ok = sa == 0 && sb == 0 && la == lb && la > d[JE_HLEN] + 2 && la <= cap && memcmp(a.data(), b.data(), (size_t)la) == 0;
    ok = ok && a[la - 2] == 0xFF && a[la - 1] == 0xD9;
    if (ok) {
      std::vector<unsigned char> c((size_t)(la - 1));
      int lc = -1;
      const int sc = encode_one(d, img.data(), need, mt, channels, swap_rb, qtabs.data(), headers.data(), c.data(), la - 1, &lc);
      ok = sc == JPE_ERR_SLOT && lc == 0;
      int ld = -1;
      const int sd = encode_one(d, img.data(), need - 1, mt, channels, swap_rb, qtabs.data(), headers.data(), a.data(), cap, &ld);
      ok = ok && sd == JPE_ERR_SOURCE && ld == 0;
    }
    if (!ok) {
      ++failures;
      fprintf(stderr, "random case %d failed: samp %d %dx%d ri %d status %d %d length %d %d\n", i, d[JE_SAMP], d[JE_W],
              d[JE_H], d[JE_RI], sa, sb, la, lb);
    }
  }
  // img_rect_ok (csrc/packed_image.h), the rule behind jpe_source_ok and the decoders' destination check: a 5 x 7 image
  // with rows of 21 bytes at offset 8 with pitch 24 ends at byte 8 + 4 * 24 + 21 = 125 for a reader, at 128 for a
  // writer that fills its rows up to the pitch.
  {
    struct Rect { long mt[4]; long last, bytes; bool ok; };
    const long huge = 0x7fffffffL;
    const Rect rects[] = {
        {{8, 5, 7, 24}, 21, 125, true},        {{8, 5, 7, 24}, 21, 124, false},      // the last row one byte past the buffer
        {{8, 5, 7, 24}, 24, 128, true},        {{8, 5, 7, 24}, 24, 127, false},      // the same for a writer
        {{5, 5, 7, 24}, 21, 122, true},        {{5, 5, 7, 24}, 21, 121, false},      // any offset: alignment is the caller's
        {{-4, 5, 7, 24}, 21, 4096, false},     {{4100, 5, 7, 24}, 21, 4096, false},  // an offset outside the buffer
        {{8, 5, 7, 20}, 21, 4096, false},      {{8, 5, 7, 21}, 21, 4096, true},      // pitch < row bytes
        {{0, 5, 7, huge}, 21, 0x7fffffffffffL, true},
        {{0, 5, 7, huge + 1}, 21, 0x7fffffffffffL, false},                           // pitch >= 2^31
        {{8, 0, 7, 24}, 21, 4096, false},      {{8, 5, 0, 24}, 21, 4096, false},     // H or W that is not the image's
        {{8, 32768, 7, 24}, 21, 0x7fffffffffffL, false}, {{8, 5, 32768, 98304}, 21, 0x7fffffffffffL, false},
        {{0, 5, 7, 24}, 21, 0, false},         {{0x7ffffffffffffff0L, 5, 7, 24}, 21, 0x7fffffffffffffffL, false},
    };
    for (const Rect& r : rects)
      if (img_rect_ok(r.mt, 5, 7, 21, r.last, r.bytes) != r.ok) {
        ++failures;
        fprintf(stderr, "img_rect_ok(offset %ld, %ld x %ld, pitch %ld; last row %ld, buffer %ld) is not %d\n", r.mt[0],
                r.mt[1], r.mt[2], r.mt[3], r.last, r.bytes, (int)r.ok);
      }
    // H or W of 0 and of 32768 as the image's own size never reach the device (the descriptor checks refuse them);
    // the sizes the subtraction argument allows do not overflow at their largest
    const long big[4] = {0, 32767, 32767, huge};
    if (!img_rect_ok(big, 32767, 32767, 32767L * 4, huge, 32767L * huge) ||
        img_rect_ok(big, 32767, 32767, 32767L * 4, huge, 32767L * huge - 1)) {
      ++failures;
      fprintf(stderr, "img_rect_ok fails at the largest sizes\n");
    }
  }
  printf("R %d %d\n", nrandom, failures);
  return failures ? 1 : 0;
}
