// Host check of the PNG decoder: the per-image code of msml_amd/csrc/png_core.h, compiled by the host compiler with
// -fsanitize=address,undefined and run as a program of its own (tests/test_png_cpu.py builds and runs it; it is never
// loaded into Python and needs no GPU).  It decodes every stream of the input file (tests/png_cases.py writes it from
// the fixture: descriptors, palettes, zlib streams, expected RGBA pixels) and every mutated zlib stream the file lists
// (truncations, byte substitutions, bit flips in the headers, cut-and-splice, trailer damage), each from a heap copy
// of exactly the stream's length, into an output buffer of exactly the image's size and with tables of exactly their
// size, so that any access outside them is reported.  Prints one line per decode:
//   C <image> <status> <pixels equal the expected ones: 1 / 0>
//   M <index> <image> <status>                   every mutation, in the file's order
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_hostcheck.cpp -o hostcheck
//   ./hostcheck input.bin
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../msml_amd/csrc/png_core.h"

struct HostSink {
  unsigned char* out;
  long count;
  void put(int v) { out[count++] = (unsigned char)v; }
  void copy(int dist, int len) {
    for (int j = 0; j < len; ++j) out[count + j] = out[count - dist + (j % dist)];
    count += len;
  }
  uint32_t finish() {
    uint32_t a = 1, b = 0;
    for (long i = 0; i < count; ++i) {
      a = (a + out[i]) % 65521u;
      b = (b + a) % 65521u;
    }
    return (b << 16) | a;
  }
};

struct Input {
  int N, npal;
  long stream_bytes;
  std::vector<int> desc;
  std::vector<unsigned char> palettes, streams;
  std::vector<std::vector<unsigned char>> expect;
};

static bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// Decode one image from the zlib stream `bytes` under descriptor d0.  Returns the status; rgba gets H * W * 4 bytes
// when it is 0.
static int decode(const int* d0, const std::vector<unsigned char>& bytes, const Input& in,
                  std::vector<unsigned char>& rgba) {
  int d[PNG_DESC_WORDS];
  memcpy(d, d0, sizeof(d));
  d[PD_BASE] = 0;
  d[PD_END] = (int)bytes.size();
  d[PD_WS] = 0;
  if (bytes.empty()) return PNG_ERR_TRUNCATED;               // the parser refuses a zero-length stream before the device
  if (png_desc_ok(d, (long)bytes.size(), in.npal) != 1) return -1;
  unsigned char* s = (unsigned char*)malloc(bytes.size());   // exactly the stream: no slack
  memcpy(s, bytes.data(), bytes.size());
  const long expected = png_expected(d);
  unsigned char* raw = (unsigned char*)malloc(expected);
  memset(raw, 0x5a, expected);
  PngTables* T = (PngTables*)malloc(sizeof(PngTables));
  memset(T, 0x5a, sizeof(PngTables));
  HostSink sink;
  sink.out = raw;
  sink.count = 0;
  PngPtrSrc src;
  src.p = s;
  int st = png_inflate(src, d[PD_END], expected, sink, T, 0, 1);
  if (st == 0) st = png_unfilter(raw, d[PD_H], png_row_bytes(d), png_bpp(d), 0, 1);
  if (st == 0) {
    const unsigned char* pal = in.palettes.data() + (d[PD_CTYPE] == 3 ? (size_t)d[PD_PAL] * 1024 : 0);
    rgba.resize((size_t)d[PD_H] * d[PD_W] * 4);
    for (int y = 0; y < d[PD_H]; ++y)
      for (int x = 0; x < d[PD_W]; ++x) {
        int px[4];
        png_expand(d, raw + (long)y * (png_row_bytes(d) + 1) + 1, pal, x, px);
        for (int k = 0; k < 4; ++k) rgba[((size_t)y * d[PD_W] + x) * 4 + k] = (unsigned char)px[k];
      }
  }
  free(T);
  free(raw);
  free(s);
  return st;
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
  if (!read_all(f, head, sizeof(head)) || head[0] != 0x504E4731) {
    fprintf(stderr, "bad input file\n");
    return 2;
  }
  in.N = head[1]; in.npal = head[2]; in.stream_bytes = head[3];
  const int nmut = head[5];
  if (in.N < 1 || in.N > 100000 || in.npal < 1 || in.npal > 100000 || in.stream_bytes < 0 || nmut < 0) return 2;
  in.desc.resize((size_t)in.N * PNG_DESC_WORDS);
  in.palettes.resize((size_t)in.npal * 1024);
  in.streams.resize((size_t)in.stream_bytes);
  bool ok = read_all(f, in.desc.data(), in.desc.size() * 4) && read_all(f, in.palettes.data(), in.palettes.size()) &&
            read_all(f, in.streams.data(), in.streams.size());
  in.expect.resize(in.N);
  for (int n = 0; ok && n < in.N; ++n) {
    const int* d = &in.desc[(size_t)n * PNG_DESC_WORDS];
    if (d[PD_STATUS] != 0 || png_desc_ok(d, in.stream_bytes, in.npal) != 1) ok = false;
    else {
      in.expect[n].resize((size_t)d[PD_H] * d[PD_W] * 4);
      ok = read_all(f, in.expect[n].data(), in.expect[n].size());
    }
  }
  if (!ok) {
    fprintf(stderr, "inconsistent input file\n");
    return 2;
  }
  std::vector<unsigned char> rgba;
  for (int n = 0; n < in.N; ++n) {
    const int* d = &in.desc[(size_t)n * PNG_DESC_WORDS];
    const unsigned char* p = in.streams.data() + (size_t)d[PD_BASE] * 4;
    const int st = decode(d, std::vector<unsigned char>(p, p + d[PD_END]), in, rgba);
    printf("C %d %d %d\n", n, st, st == 0 && rgba == in.expect[n] ? 1 : 0);
  }
  for (int m = 0; m < nmut; ++m) {
    int hd[2];
    if (!read_all(f, hd, sizeof(hd)) || hd[0] < 0 || hd[0] >= in.N || hd[1] < 0 || hd[1] > (1 << 28)) {
      fprintf(stderr, "inconsistent mutation %d\n", m);
      return 2;
    }
    std::vector<unsigned char> z((size_t)hd[1]);
    if (!read_all(f, z.data(), z.size())) return 2;
    printf("M %d %d %d\n", m, hd[0], decode(&in.desc[(size_t)hd[0] * PNG_DESC_WORDS], z, in, rgba));
  }
  fclose(f);
  return 0;
}
