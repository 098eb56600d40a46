// Host check of the JPEG decoder: the per-image code of msml_amd/csrc/jpeg_core.h, compiled by the host compiler with
// -fsanitize=address,undefined and run as a program of its own (tests/test_jpeg_cpu.py builds and runs it; it is never
// loaded into Python and needs no GPU).  It decodes every stream of the input file (tests/jpeg_cases.py writes it from
// the fixture: descriptors, tables, streams, expected pixels) and a few thousand mutations of their entropy-coded
// bytes -- truncations at every length, seeded single-byte substitutions, FF followed by every second byte, the
// training-sized streams cut in half, restart markers removed or swapped -- each from a heap copy of exactly the stream's length and into a workspace of exactly
// the image's size, so that any access outside them is reported.  Prints one line per decode:
//   C <image> <status> <pixels equal the expected ones: 1 / 0>
//   M <kind> <image> <a> <b> <status>            every mutation
//   D <kind> <image> <a> <b> <status> <hex>      some of them again with the whole mutated stream, for the GPU tests
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_hostcheck.cpp -o hostcheck
//   ./hostcheck input.bin
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../msml_amd/csrc/jpeg_core.h"

struct HostSink {
  int16_t* coef;
  int16_t blk[64];
  void begin() { memset(blk, 0, sizeof(blk)); }
  void put(int k, int v) { blk[img_zigzag(k)] = (int16_t)v; }
  void end(long b) { memcpy(coef + b * 64, blk, sizeof(blk)); }
};

struct Input {
  int N, nq, nh, trunc_a, trunc_b;
  long stream_bytes;
  std::vector<int> desc, qtabs, htabs;
  std::vector<unsigned char> streams;
  std::vector<std::vector<unsigned char>> expect;
};

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// Decode one image from `bytes` (the whole stream, header included) under descriptor d.  Returns the status; rgb gets
// H * W * 3 bytes when it is 0.
static int decode(const int* d0, const std::vector<unsigned char>& bytes, const Input& in,
                  std::vector<unsigned char>& rgb) {
  int d[JPG_DESC_WORDS];
  memcpy(d, d0, sizeof(d));
  d[JD_BASE] = 0;
  d[JD_END] = (int)bytes.size();
  d[JD_WS] = 0;
  if (d[JD_BEGIN] > d[JD_END]) d[JD_BEGIN] = d[JD_END];
  if (jpg_desc_ok(d, (long)bytes.size(), in.nq, in.nh) != 1) return -1;
  unsigned char* s = (unsigned char*)malloc(bytes.size() ? bytes.size() : 1);   // exactly the stream: no slack
  memcpy(s, bytes.data(), bytes.size());
  JpgLayout L;
  jpg_layout(d, L);
  unsigned char* ws = (unsigned char*)malloc(L.bytes);
  memset(ws, 0x5a, L.bytes);
  HostSink sink;
  sink.coef = (int16_t*)ws;
  const int* dctab[3];
  const int* actab[3];
  for (int c = 0; c < 3; ++c) {
    dctab[c] = in.htabs.data() + (size_t)(c < L.ncomp ? d[JD_DC + c] : 0) * JPG_HUFF_WORDS;
    actab[c] = in.htabs.data() + (size_t)(c < L.ncomp ? d[JD_AC + c] : 0) * JPG_HUFF_WORDS;
  }
  JpgPtrSrc src;
  src.p = s;
  const int st = jpg_entropy(d, src, dctab, actab, sink);
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
                   bool dump = false) {
  printf("M %s %d %ld %ld %d\n", kind, n, a, b, st);
  if (dump || (bytes.size() <= 1024 && g_count++ % 7 == 0)) {
    printf("D %s %d %ld %ld %d ", kind, n, a, b, st);
    for (unsigned char c : bytes) printf("%02x", c);
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
  if (!read_all(f, head, sizeof(head)) || head[0] != 0x4A484331) {
    fprintf(stderr, "bad input file\n");
    return 2;
  }
  in.N = head[1]; in.nq = head[2]; in.nh = head[3]; in.stream_bytes = head[4]; in.trunc_a = head[5]; in.trunc_b = head[6];
  uint32_t seed = (uint32_t)head[7];
  if (in.N < 1 || in.N > 100000 || in.nq < 1 || in.nq > 4096 || in.nh < 1 || in.nh > 4096 || in.stream_bytes < 0) return 2;
  in.desc.resize((size_t)in.N * JPG_DESC_WORDS);
  in.qtabs.resize((size_t)in.nq * 64);
  in.htabs.resize((size_t)in.nh * JPG_HUFF_WORDS);
  in.streams.resize((size_t)in.stream_bytes);
  bool ok = read_all(f, in.desc.data(), in.desc.size() * 4) && read_all(f, in.qtabs.data(), in.qtabs.size() * 4) &&
            read_all(f, in.htabs.data(), in.htabs.size() * 4) && read_all(f, in.streams.data(), in.streams.size());
  in.expect.resize(in.N);
  for (int n = 0; ok && n < in.N; ++n) {
    const int* d = &in.desc[(size_t)n * JPG_DESC_WORDS];
    if (jpg_desc_ok(d, in.stream_bytes, in.nq, in.nh) != 1) ok = false;
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
  auto stream_of = [&](int n) {
    const int* d = &in.desc[(size_t)n * JPG_DESC_WORDS];
    const unsigned char* p = in.streams.data() + (size_t)d[JD_BASE] * 4;
    return std::vector<unsigned char>(p, p + d[JD_END]);
  };
  auto rnd = [&]() {
    seed = seed * 1664525u + 1013904223u;
    return seed >> 8;
  };
  std::vector<unsigned char> rgb;
  // the streams as they are
  for (int n = 0; n < in.N; ++n) {
    const int* d = &in.desc[(size_t)n * JPG_DESC_WORDS];
    if (d[JD_STATUS] != 0) {
      printf("C %d %d 0\n", n, d[JD_STATUS]);
      continue;
    }
    const int st = decode(d, stream_of(n), in, rgb);
    printf("C %d %d %d\n", n, st, st == 0 && rgb == in.expect[n] ? 1 : 0);
  }
  // truncations at every length of two small streams
  for (int t : {in.trunc_a, in.trunc_b}) {
    if (t < 0 || t >= in.N) continue;
    const int* d = &in.desc[(size_t)t * JPG_DESC_WORDS];
    if (d[JD_STATUS] != 0) continue;
    const std::vector<unsigned char> full = stream_of(t);
    for (int len = d[JD_BEGIN]; len < d[JD_END]; ++len) {
      std::vector<unsigned char> cut(full.begin(), full.begin() + len);
      report("trunc", t, len, 0, decode(d, cut, in, rgb), cut);
    }
  }
  // FF followed by every second byte, at one place of the same two streams
  for (int t : {in.trunc_a, in.trunc_b}) {
    if (t < 0 || t >= in.N) continue;
    const int* d = &in.desc[(size_t)t * JPG_DESC_WORDS];
    if (d[JD_STATUS] != 0 || d[JD_END] - d[JD_BEGIN] < 8) continue;
    const long pos = d[JD_BEGIN] + (d[JD_END] - d[JD_BEGIN]) / 3;
    for (int v = 0; v < 256; ++v) {
      std::vector<unsigned char> m = stream_of(t);
      m[pos] = 0xFF;
      m[pos + 1] = (unsigned char)v;
      report("ffxx", t, pos, v, decode(d, m, in, rgb), m);
    }
  }
  // single-byte substitutions at seeded positions of every stream
  for (int n = 0; n < in.N; ++n) {
    const int* d = &in.desc[(size_t)n * JPG_DESC_WORDS];
    if (d[JD_STATUS] != 0 || d[JD_END] <= d[JD_BEGIN]) continue;
    for (int k = 0; k < 12; ++k) {
      std::vector<unsigned char> m = stream_of(n);
      const long pos = d[JD_BEGIN] + rnd() % (uint32_t)(d[JD_END] - d[JD_BEGIN]);
      const int v = rnd() & 255;
      m[pos] = (unsigned char)v;
      report("subst", n, pos, v, decode(d, m, in, rgb), m);
    }
  }
  // the 112-wide streams cut in the middle of their coded bytes: recorded whole, as corrupt records of training size
  for (int n = 0; n < in.N; ++n) {
    const int* d = &in.desc[(size_t)n * JPG_DESC_WORDS];
    if (d[JD_STATUS] != 0 || d[JD_W] != 112) continue;
    const std::vector<unsigned char> full = stream_of(n);
    const int len = d[JD_BEGIN] + (d[JD_END] - d[JD_BEGIN]) / 2;
    std::vector<unsigned char> cut(full.begin(), full.begin() + len);
    report("cut", n, len, 0, decode(d, cut, in, rgb), cut, true);
  }
  // restart markers removed or swapped
  for (int n = 0; n < in.N; ++n) {
    const int* d = &in.desc[(size_t)n * JPG_DESC_WORDS];
    if (d[JD_STATUS] != 0 || d[JD_RI] == 0) continue;
    const std::vector<unsigned char> full = stream_of(n);
    std::vector<long> marks;
    for (long p = d[JD_BEGIN]; p + 1 < d[JD_END]; ++p)
      if (full[p] == 0xFF && full[p + 1] >= 0xD0 && full[p + 1] <= 0xD7) marks.push_back(p);
    if (marks.empty()) continue;
    std::vector<unsigned char> m = full;
    m.erase(m.begin() + marks[0], m.begin() + marks[0] + 2);
    report("rstdel", n, marks[0], 0, decode(d, m, in, rgb), m);
    if (marks.size() >= 2) {
      m = full;
      const unsigned char a = m[marks[0] + 1];
      m[marks[0] + 1] = m[marks[1] + 1];
      m[marks[1] + 1] = a;
      report("rstswap", n, marks[0], marks[1], decode(d, m, in, rgb), m);
    }
  }
  return 0;
}
