// Host check of the progressive JPEG decoder: the per-scan code of msml_amd/csrc/jpeg_prog_core.h (and jpeg_core.h
// behind the coefficients), compiled by the host compiler with -fsanitize=address,undefined and run as a program of its
// own (tests/test_jpeg_prog_cpu.py builds and runs it; it is never loaded into Python and needs no GPU).  It decodes
// every stream of the input file (tests/jpeg_prog_cases.py writes it from the fixture: descriptors, scan table, tables,
// streams, expected pixels) and a few thousand mutations of them, each from a heap copy of exactly the stream's length
// and into a workspace of exactly the image's size, so that any access outside them is reported.  The headers were
// parsed on the host before this program runs, as they are before the device runs, so a mutation is one of the stream
// bytes, of the scan records, or of both:
//   subst    a seeded byte of a scan's entropy-coded segment replaced
//   ffxx     FF followed by every second byte at one place of the smallest stream
//   trunc    the stream cut at every scan's first byte, middle and end; records past the cut are clamped to it
//   drop     one scan's record left out (every scan in turn)
//   swap     the parameters of two neighbouring scans exchanged, their byte ranges kept
//   seltab   a scan decoded with the next table of the batch, and with a table index past the last one
//   scanhdr  seeded values in Ss, Se, Ah, Al or the restart interval of a record
// Prints one line per decode (status -1: the checks in front of the launch refuse the records):
//   C <image> <status> <pixels equal the expected ones: 1 / 0>
//   M <kind> <image> <a> <b> <status>                    every mutation
//   D <kind> <image> <a> <b> <status> <hex> <hex>        some of them again with the mutated stream and records
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_prog_hostcheck.cpp -o check
//   ./check input.bin
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../msml_amd/csrc/jpeg_prog_core.h"

struct HostSink {                                            // a baseline image of the batch (jpeg_hostcheck.cpp's)
  int16_t* coef;
  int16_t blk[64];
  void begin() { memset(blk, 0, sizeof(blk)); }
  void put(int k, int v) { blk[img_zigzag(k)] = (int16_t)v; }
  void end(long b) { memcpy(coef + b * 64, blk, sizeof(blk)); }
};

struct HostBlk {                                             // c[k]: coefficient k in zigzag order, no index masked
  int16_t* coef;
  int16_t* c;
  void dc_store(long b, int v) { coef[b * 64] = (int16_t)v; }
  void dc_or(long b, int bit) { coef[b * 64] = (int16_t)(coef[b * 64] | bit); }
  void clear() { memset(c, 0, 128); }
  void put(int k, int v) { c[k] = (int16_t)v; }
  void load(long b) {
    for (int k = 0; k < 64; ++k) c[k] = coef[b * 64 + img_zigzag(k)];
  }
  void store(long b, int ss, int se) {
    for (int k = ss; k <= se; ++k) coef[b * 64 + img_zigzag(k)] = c[k];
  }
  uint64_t nonzero(int ss, int se) {
    uint64_t m = 0;
    for (int k = ss; k <= se; ++k) m |= (uint64_t)(c[k] != 0) << k;
    return m;
  }
  void correct(uint64_t m, int base, int bits, int cnt, int p1) {
    int rank = -base;
    for (int k = 0; k < 64; ++k) {
      if (!((m >> k) & 1)) continue;
      if (rank >= 0 && rank < cnt && ((bits >> (cnt - 1 - rank)) & 1) && (c[k] & p1) == 0)
        c[k] = (int16_t)(c[k] + (c[k] >= 0 ? p1 : -p1));
      ++rank;
    }
  }
};

struct Input {
  int N, nq, nh;
  long stream_bytes, nscan;
  std::vector<int> desc, scans, qtabs, htabs;
  std::vector<unsigned char> streams;
  std::vector<std::vector<unsigned char>> expect;
};

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// Decode one image from `bytes` (the whole stream) under descriptor d0 and the scan records `rec` (its own, from 0).
// Returns the status, -1 for records the host checks refuse; rgb gets H * W * 3 bytes when it is 0.
static int decode(const int* d0, const std::vector<unsigned char>& bytes, const std::vector<int>& rec, const Input& in,
                  std::vector<unsigned char>& rgb) {
  int d[JPG_DESC_WORDS];
  memcpy(d, d0, sizeof(d));
  d[JD_BASE] = 0;
  d[JD_END] = (int)bytes.size();
  d[JD_WS] = 0;
  d[JD_NSCAN] = (int)(rec.size() / JPG_SCAN_WORDS);
  d[JD_SCAN0] = 0;
  if (d[JD_BEGIN] > d[JD_END]) d[JD_BEGIN] = d[JD_END];
  if (jpg_desc_ok(d, (long)bytes.size(), in.nq, in.nh) != 1) return -1;
  if (!jpg_scans_ok(d, rec.data(), (long)rec.size() / JPG_SCAN_WORDS, in.nh)) return -1;
  unsigned char* s = (unsigned char*)malloc(bytes.size() ? bytes.size() : 1);   // exactly the stream: no slack
  memcpy(s, bytes.data(), bytes.size());
  JpgLayout L;
  jpg_layout(d, L);
  unsigned char* ws = (unsigned char*)malloc(L.bytes);
  memset(ws, 0x5a, L.bytes);
  JpgPtrSrc src;
  src.p = s;
  int st = JPG_OK;
  if (d[JD_NSCAN] == 0) {
    HostSink sink;
    sink.coef = (int16_t*)ws;
    const int* dctab[3];
    const int* actab[3];
    for (int c = 0; c < 3; ++c) {
      dctab[c] = in.htabs.data() + (size_t)(c < L.ncomp ? d[JD_DC + c] : 0) * JPG_HUFF_WORDS;
      actab[c] = in.htabs.data() + (size_t)(c < L.ncomp ? d[JD_AC + c] : 0) * JPG_HUFF_WORDS;
    }
    st = jpg_entropy(d, src, dctab, actab, sink);
  } else {
    memset(ws, 0, (size_t)L.nblk * 128);                     // as k_jpeg_prog does before the first scan
    HostBlk blk;
    blk.coef = (int16_t*)ws;
    blk.c = (int16_t*)malloc(128);                           // on the heap: an index past 63 is reported
    memset(blk.c, 0, 128);
    for (int i = 0; i < d[JD_NSCAN] && st == JPG_OK; ++i) {
      const int* sc = rec.data() + (size_t)i * JPG_SCAN_WORDS;
      const int* tab[3];
      for (int c = 0; c < 3; ++c) tab[c] = in.htabs.data() + (size_t)(c < sc[JS_NCOMP] ? sc[JS_TAB + c] : 0) * JPG_HUFF_WORDS;
      st = jpg_prog_scan(d, L, sc, src, tab, blk);
    }
    free(blk.c);
  }
  if (st == 0) {
    for (int c = 0; c < L.ncomp; ++c)
      for (int by = 0; by < L.bh[c]; ++by)
        for (int bx = 0; bx < L.bw[c]; ++bx) {
          const long i = L.cbase[c] + (long)by * L.bw[c] + bx;
          const long pitch = (long)L.bw[c] * 8;
          jpg_idct((const int16_t*)ws + i * 64, in.qtabs.data() + (long)d[JD_QT + c] * 64,
                   ws + L.pbase[c] + (long)by * 8 * pitch + bx * 8, pitch);
        }
    rgb.resize((size_t)d[JD_H] * d[JD_W] * 3);
    for (int y = 0; y < d[JD_H]; ++y)
      for (int x = 0; x < d[JD_W]; ++x) {
        int px[3];
        jpg_pixel(d, L, ws, x, y, px);
        for (int k = 0; k < 3; ++k) rgb[((size_t)y * d[JD_W] + x) * 3 + k] = (unsigned char)px[k];
      }
  }
  free(ws);
  free(s);
  return st;
}

static unsigned long g_count = 0;

static void report(const char* kind, int n, long a, long b, int st, const std::vector<unsigned char>& bytes,
                   const std::vector<int>& rec) {
  printf("M %s %d %ld %ld %d\n", kind, n, a, b, st);
  if (bytes.size() <= 1024 && g_count++ % 9 == 0) {
    printf("D %s %d %ld %ld %d ", kind, n, a, b, st);
    for (unsigned char c : bytes) printf("%02x", c);
    printf(" ");
    for (int v : rec) printf("%08x", (unsigned)v);
    printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s input.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  Input in;
  int head[8];
  if (!read_all(f, head, sizeof(head)) || head[0] != 0x4A504831) {
    fprintf(stderr, "bad input file\n");
    return 2;
  }
  in.N = head[1]; in.nq = head[2]; in.nh = head[3]; in.stream_bytes = head[4]; in.nscan = head[5];
  uint32_t seed = (uint32_t)head[6];
  if (in.N < 1 || in.N > 100000 || in.nq < 1 || in.nq > 4096 || in.nh < 1 || in.nh > 65536 || in.stream_bytes < 0 ||
      in.nscan < 1 || in.nscan > 1000000)
    return 2;
  in.desc.resize((size_t)in.N * JPG_DESC_WORDS);
  in.scans.resize((size_t)in.nscan * JPG_SCAN_WORDS);
  in.qtabs.resize((size_t)in.nq * 64);
  in.htabs.resize((size_t)in.nh * JPG_HUFF_WORDS);
  in.streams.resize((size_t)in.stream_bytes);
  bool ok = read_all(f, in.desc.data(), in.desc.size() * 4) && read_all(f, in.scans.data(), in.scans.size() * 4) &&
            read_all(f, in.qtabs.data(), in.qtabs.size() * 4) && read_all(f, in.htabs.data(), in.htabs.size() * 4) &&
            read_all(f, in.streams.data(), in.streams.size());
  in.expect.resize(in.N);
  for (int n = 0; ok && n < in.N; ++n) {
    const int* d = &in.desc[(size_t)n * JPG_DESC_WORDS];
    if (jpg_desc_ok(d, in.stream_bytes, in.nq, in.nh) != 1 || !jpg_scans_ok(d, in.scans.data(), in.nscan, in.nh)) ok = false;
    else if (d[JD_STATUS] == 0) {
      in.expect[n].resize((size_t)d[JD_H] * d[JD_W] * 3);
      ok = read_all(f, in.expect[n].data(), in.expect[n].size());
    }
  }
  fclose(f);
  if (!ok) {
    fprintf(stderr, "inconsistent input file\n");
    return 2;
  }
  auto desc_of = [&](int n) { return &in.desc[(size_t)n * JPG_DESC_WORDS]; };
  auto stream_of = [&](int n) {
    const int* d = desc_of(n);
    const unsigned char* p = in.streams.data() + (size_t)d[JD_BASE] * 4;
    return std::vector<unsigned char>(p, p + d[JD_END]);
  };
  auto records_of = [&](int n) {
    const int* d = desc_of(n);
    const int* p = in.scans.data() + (size_t)d[JD_SCAN0] * JPG_SCAN_WORDS;
    return std::vector<int>(p, p + (size_t)d[JD_NSCAN] * JPG_SCAN_WORDS);
  };
  auto rnd = [&]() {
    seed = seed * 1664525u + 1013904223u;
    return seed >> 8;
  };
  std::vector<unsigned char> rgb;
  // the streams as they are
  int smallest = -1;
  for (int n = 0; n < in.N; ++n) {
    const int* d = desc_of(n);
    if (d[JD_STATUS] != 0) {
      printf("C %d %d 0\n", n, d[JD_STATUS]);
      continue;
    }
    const int st = decode(d, stream_of(n), records_of(n), in, rgb);
    printf("C %d %d %d\n", n, st, st == 0 && rgb == in.expect[n] ? 1 : 0);
    if (d[JD_NSCAN] > 0 && d[JD_NCOMP] == 3 && d[JD_W] >= 9 && (smallest < 0 || d[JD_END] < desc_of(smallest)[JD_END]))
      smallest = n;
  }
  for (int n = 0; n < in.N; ++n) {
    const int* d = desc_of(n);
    if (d[JD_STATUS] != 0 || d[JD_NSCAN] == 0) continue;
    const bool big = d[JD_END] > 8192;                      // the large streams: fewer mutations each
    const std::vector<unsigned char> full = stream_of(n);
    const std::vector<int> rec = records_of(n);
    const int ns = d[JD_NSCAN];
    auto R = [&](std::vector<int>& r, int i, int w) -> int& { return r[(size_t)i * JPG_SCAN_WORDS + w]; };
    // seeded single-byte substitutions inside the scans
    for (int k = 0; k < (big ? 4 : 24); ++k) {
      std::vector<int> r = rec;
      const int i = (int)(rnd() % (uint32_t)ns);
      const int b0 = R(r, i, JS_BEGIN), e0 = R(r, i, JS_END);
      if (e0 <= b0) continue;
      std::vector<unsigned char> m = full;
      const long pos = b0 + rnd() % (uint32_t)(e0 - b0);
      const int v = rnd() & 255;
      m[pos] = (unsigned char)v;
      report("subst", n, pos, v, decode(d, m, r, in, rgb), m, r);
    }
    if (big) continue;
    // cuts at every scan's first byte, middle and end
    for (int i = 0; i < ns; ++i) {
      std::vector<int> r0 = rec;
      const int b0 = R(r0, i, JS_BEGIN), e0 = R(r0, i, JS_END);
      for (int len : {b0, (b0 + e0) / 2, e0}) {
        if (len >= (int)full.size()) continue;
        std::vector<unsigned char> cut(full.begin(), full.begin() + len);
        std::vector<int> r = rec;
        for (int j = 0; j < ns; ++j) {
          if (R(r, j, JS_BEGIN) > len) R(r, j, JS_BEGIN) = len;
          if (R(r, j, JS_END) > len) R(r, j, JS_END) = len;
        }
        report("trunc", n, len, i, decode(d, cut, r, in, rgb), cut, r);
      }
    }
    // one scan left out
    for (int i = 0; i < ns && ns >= 2; ++i) {
      std::vector<int> r = rec;
      r.erase(r.begin() + (size_t)i * JPG_SCAN_WORDS, r.begin() + (size_t)(i + 1) * JPG_SCAN_WORDS);
      report("drop", n, i, 0, decode(d, full, r, in, rgb), full, r);
    }
    // two neighbours decoded as each other
    for (int i = 0; i + 1 < ns; ++i) {
      std::vector<int> r = rec;
      for (int w = JS_NCOMP; w < JPG_SCAN_WORDS; ++w) {
        const int t = R(r, i, w);
        R(r, i, w) = R(r, i + 1, w);
        R(r, i + 1, w) = t;
      }
      report("swap", n, i, i + 1, decode(d, full, r, in, rgb), full, r);
    }
    // another table, and a table index past the last
    for (int i = 0; i < ns; ++i) {
      std::vector<int> r = rec;
      R(r, i, JS_TAB) = (R(r, i, JS_TAB) + 1) % in.nh;
      report("seltab", n, i, R(r, i, JS_TAB), decode(d, full, r, in, rgb), full, r);
    }
    {
      std::vector<int> r = rec;
      const int i = (int)(rnd() % (uint32_t)ns);
      R(r, i, JS_TAB) = in.nh;
      report("seltab", n, i, in.nh, decode(d, full, r, in, rgb), full, r);
    }
    // seeded scan parameters
    for (int k = 0; k < 16; ++k) {
      std::vector<int> r = rec;
      const int i = (int)(rnd() % (uint32_t)ns);
      const int words[5] = {JS_SS, JS_SE, JS_AH, JS_AL, JS_RI};
      const int w = words[rnd() % 5];
      const int v = (int)(rnd() % (w == JS_SS || w == JS_SE ? 66u : 16u)) - (rnd() % 16 == 0 ? 1 : 0);
      R(r, i, w) = v;
      report("scanhdr", n, i * 100 + w, v, decode(d, full, r, in, rgb), full, r);
    }
  }
  // FF followed by every second byte, in the middle of the longest scan of the smallest colour stream
  if (smallest >= 0) {
    const int* d = desc_of(smallest);
    const std::vector<int> rec = records_of(smallest);
    int best = 0;
    for (int i = 1; i < d[JD_NSCAN]; ++i)
      if (rec[(size_t)i * JPG_SCAN_WORDS + JS_END] - rec[(size_t)i * JPG_SCAN_WORDS + JS_BEGIN] >
          rec[(size_t)best * JPG_SCAN_WORDS + JS_END] - rec[(size_t)best * JPG_SCAN_WORDS + JS_BEGIN])
        best = i;
    const int b0 = rec[(size_t)best * JPG_SCAN_WORDS + JS_BEGIN], e0 = rec[(size_t)best * JPG_SCAN_WORDS + JS_END];
    if (e0 - b0 >= 4) {
      const long pos = b0 + (e0 - b0) / 3;
      for (int v = 0; v < 256; ++v) {
        std::vector<unsigned char> m = stream_of(smallest);
        m[pos] = 0xFF;
        m[pos + 1] = (unsigned char)v;
        report("ffxx", smallest, pos, v, decode(d, m, rec, in, rgb), m, rec);
      }
    }
  }
  return 0;
}
