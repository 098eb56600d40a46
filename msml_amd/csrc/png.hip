// PNG decoding on the device, Pillow's pixels: the PIL.Image.open(f).convert(mode) in front of the folder evaluation,
// the alignment tool and the occluder folders of the reference (eval/qeval_folder.py, eval/align_dataset.py,
// datasets/augment/rand_occ.py).  The per-image code is csrc/png_core.h, shared with the host check;
// tests/png_cases.py restates it.
//   k_png_inflate   one wavefront per image: the bit walk is the same for all 64 lanes (every table address is
//                   wave-uniform) out of LDS: a window of the stream, the block's decode tables (built here, by all
//                   lanes) and the last 32 KiB of output as a ring.  A match is copied by the lanes 64 bytes at a time;
//                   a finished half of the ring leaves for the workspace as 16-byte stores, its Adler-32 summed on
//                   the way.  Writes status[n].
//   k_png_unfilter  one wavefront per image, rows in order, in place in the workspace
//   k_png_store     one thread per 4 output pixels: unpack, palette / gray scaling, alpha, into the packed destination
// No floating point, no global atomics, one writer per byte: two runs give the same bits.  An image whose status is
// not 0 is skipped by the later passes: its output rectangle is left as it was.
#include "common.h"
#include "png_core.h"

#define PNG_RING 32768
#define PNG_HALF 16384

// The last 32 KiB of output in LDS.  All source bytes of a match precede its first output byte, so the lanes copy it
// without a dependency between them; a slot that a later byte of the same match overwrites (distances near 32768) is
// read by the same or an earlier 64-byte step than the one that writes it, and a step reads before it writes.
struct PngRingSink {
  unsigned char* ring;
  unsigned char* ws;
  long count;
  unsigned int a, b;
  int lane;
  __device__ void put(int v) {
    if (lane == 0) ring[count & (PNG_RING - 1)] = (unsigned char)v;
    ++count;
    if ((count & (PNG_HALF - 1)) == 0) flush(count - PNG_HALF, PNG_HALF);
  }
  __device__ void copy(int dist, int len) {
    __syncthreads();
    const int p = (int)(count & (PNG_RING - 1));
    for (int j0 = 0; j0 < len; j0 += 64) {
      const int j = j0 + lane;
      int v = 0;
      if (j < len) v = ring[(p - dist + (dist < len ? j % dist : j)) & (PNG_RING - 1)];
      __syncthreads();
      if (j < len) ring[(p + j) & (PNG_RING - 1)] = (unsigned char)v;
    }
    const long old = count;
    count += len;
    if ((old >> 14) != (count >> 14)) flush((count >> 14 << 14) - PNG_HALF, PNG_HALF);
  }
  // nbytes of the ring from output position `start` (a multiple of PNG_HALF) to the workspace, and into the Adler sums
  __device__ void flush(long start, int nbytes) {
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(ring + (start & (PNG_RING - 1)));
    uint4* dst = reinterpret_cast<uint4*>(ws + start);
    unsigned int s1 = 0, s2 = 0;
    for (int q = lane; q * 16 < nbytes; q += 64) {
      uint4 v = src[q];
      unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = q * 16 + e;
        if (i >= nbytes) w[e >> 2] &= ~(0xffu << ((e & 3) * 8));
        const unsigned int c = (w[e >> 2] >> ((e & 3) * 8)) & 0xffu;
        s1 += c;
        s2 += c * (unsigned int)(nbytes - i);
      }
      dst[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    s2 %= 65521u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      s1 += __shfl_xor(s1, m, 64);
      s2 += __shfl_xor(s2, m, 64);
    }
    b = (b + (unsigned int)nbytes * a + s2) % 65521u;
    a = (a + s1) % 65521u;
    __syncthreads();
  }
  __device__ unsigned int finish() {
    const long start = count & ~(long)(PNG_HALF - 1);
    if (count > start) flush(start, (int)(count - start));
    return (b << 16) | a;
  }
};

__global__ void __launch_bounds__(64) k_png_inflate(const unsigned char* __restrict__ streams,
                                                    const int* __restrict__ desc, unsigned char* __restrict__ ws,
                                                    int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) unsigned char s_ring[PNG_RING];
  __shared__ unsigned int s_win[IMG_CHUNK / 4];
  __shared__ PngTables s_tab;
  const int n = blockIdx.x;
  const int* d = desc + (long)n * PNG_DESC_WORDS;
  int st = d[PD_STATUS];
  if (st == 0) {
    PngRingSink sink;
    sink.ring = s_ring;
    sink.ws = ws + (long)d[PD_WS] * PNG_WS_ALIGN;
    sink.count = 0;
    sink.a = 1;
    sink.b = 0;
    sink.lane = threadIdx.x;
    LdsStreamSrc src = {streams + (long)d[PD_BASE] * 4, s_win, -IMG_CHUNK, d[PD_END], (int)threadIdx.x};
    st = png_inflate(src, d[PD_END], png_expected(d), sink, &s_tab, (int)threadIdx.x, 64);
  }
  if (threadIdx.x == 0) status[n] = st;
}

__global__ void __launch_bounds__(64) k_png_unfilter(const int* __restrict__ desc, unsigned char* __restrict__ ws,
                                                     int* __restrict__ status) {
  const int n = blockIdx.x;
  if (status[n] != 0) return;
  const int* d = desc + (long)n * PNG_DESC_WORDS;
  const int st = png_unfilter(ws + (long)d[PD_WS] * PNG_WS_ALIGN, d[PD_H], png_row_bytes(d), png_bpp(d),
                              (int)threadIdx.x, 64);
  __syncthreads();
  if (st != 0 && threadIdx.x == 0) status[n] = st;
}

// channels 4: R, G, B, A; 3: R, G, B; 1: the gray sample (gray and gray + alpha streams).  swap_rb exchanges R and B.
// A thread owns 4 pixels of a row; where the image's offset and pitch are multiples of 4 they leave as dwords, and the
// bytes between the row and its pitch as 0.
__global__ void __launch_bounds__(256) k_png_store(const int* __restrict__ desc, const unsigned char* __restrict__ ws,
                                                   const unsigned char* __restrict__ palettes,
                                                   unsigned char* __restrict__ dst, long dst_bytes,
                                                   const long* __restrict__ meta, int channels, int swap_rb,
                                                   int* __restrict__ status) {
  const int n = blockIdx.y;
  if (status[n] != 0) return;
  const int* d = desc + (long)n * PNG_DESC_WORDS;
  const int H = d[PD_H], W = d[PD_W];
  const long* mt = meta + (long)n * 4;
  const long off = mt[0], pitch = mt[3];
  const long rowb = (long)W * channels;
  // the destination rectangle is checked here, on the device, where meta_out lives.  Every thread of the image sees
  // the same values and leaves; nobody reads status[n] after this point in this launch but through the same test.
  if (!img_rect_ok(mt, H, W, rowb, img_aligned(off, pitch) ? pitch : rowb, dst_bytes)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) status[n] = PNG_ERR_OUTPUT;
    return;
  }
  const int gw = (W + 3) / 4;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)gw * H) return;
  const int y = (int)(g / gw), x0 = (int)(g - (long)y * gw) * 4;
  const unsigned char* src = ws + (long)d[PD_WS] * PNG_WS_ALIGN + (long)y * (png_row_bytes(d) + 1) + 1;
  const unsigned char* pal = palettes + (d[PD_CTYPE] == 3 ? (long)d[PD_PAL] * 1024 : 0);
  unsigned char px[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) px[e] = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (x0 + e < W) {
      int c[4];
      png_expand(d, src, pal, x0 + e, c);
      if (channels == 1) {
        px[e] = (unsigned char)c[0];
      } else if (channels == 3) {
        px[e * 3 + 0] = (unsigned char)c[swap_rb ? 2 : 0];
        px[e * 3 + 1] = (unsigned char)c[1];
        px[e * 3 + 2] = (unsigned char)c[swap_rb ? 0 : 2];
      } else {
        px[e * 4 + 0] = (unsigned char)c[swap_rb ? 2 : 0];
        px[e * 4 + 1] = (unsigned char)c[1];
        px[e * 4 + 2] = (unsigned char)c[swap_rb ? 0 : 2];
        px[e * 4 + 3] = (unsigned char)c[3];
      }
    }
  }
  img_store4<4>(dst + off + (long)y * pitch, off, pitch, rowb, x0, W, channels, px);
}

extern "C" long msml_png_workspace(int* desc, int N) {
  if (!desc || N < 1) return 0;
  long units = 0;
  for (int n = 0; n < N; ++n) {
    int* d = desc + (long)n * PNG_DESC_WORDS;
    d[PD_WS] = 0;
    if (d[PD_STATUS] != 0) continue;
    if (png_desc_ok(d, 0x7fffffffffffL, 0x7fffffff) != 1) return 0;
    if (units > 0x7fffffffL) return 0;
    d[PD_WS] = (int)units;
    units += png_ws_bytes(d) / PNG_WS_ALIGN;
  }
  return units * PNG_WS_ALIGN;
}

extern "C" int msml_png_decode(const unsigned char* streams, long stream_bytes, const int* desc, const int* desc_host,
                               const unsigned char* palettes, long palette_bytes, unsigned char* dst, long dst_bytes,
                               const long* meta_out, int channels, int swap_rb, int* status, unsigned char* ws,
                               long ws_bytes, int N, void* stream) {
  MSML_CHECK(N >= 1 && N <= 65535, MSML_ERR_UNSUPPORTED, "png_decode: N=%d outside 1..65535", N);
  MSML_CHECK(channels == 1 || channels == 3 || channels == 4, MSML_ERR_UNSUPPORTED,
             "png_decode: channels=%d (1, 3 or 4)", channels);
  MSML_CHECK(streams && desc && desc_host && palettes && dst && meta_out && status && ws, MSML_ERR_SHAPE,
             "png_decode: null pointer");
  MSML_CHECK(((uintptr_t)streams & 3) == 0 && ((uintptr_t)desc & 3) == 0 && ((uintptr_t)palettes & 3) == 0 &&
                 ((uintptr_t)dst & 3) == 0 && ((uintptr_t)status & 3) == 0 && ((uintptr_t)meta_out & 7) == 0 &&
                 ((uintptr_t)ws & 15) == 0,
             MSML_ERR_SHAPE, "png_decode: streams, desc, palettes, dst, status must be 4-byte, meta_out 8-byte, ws "
                             "16-byte aligned");
  MSML_CHECK(stream_bytes % 4 == 0, MSML_ERR_SHAPE, "png_decode: stream_bytes=%ld is not whole dwords", stream_bytes);
  MSML_CHECK(stream_bytes >= 0 && dst_bytes >= 0 && ws_bytes >= 0 && palette_bytes >= 1024 && palette_bytes % 1024 == 0,
             MSML_ERR_SHAPE, "png_decode: stream_bytes=%ld dst_bytes=%ld ws_bytes=%ld palette_bytes=%ld (whole palettes "
             "of 1024 bytes)", stream_bytes, dst_bytes, ws_bytes, palette_bytes);
  long units = 0, max_grp = 0;
  for (int n = 0; n < N; ++n) {
    const int* d = desc_host + (long)n * PNG_DESC_WORDS;
    MSML_CHECK(png_desc_ok(d, stream_bytes, palette_bytes / 1024) == 1, MSML_ERR_SHAPE,
               "png_decode: descriptor %d is inconsistent", n);
    if (d[PD_STATUS] != 0) continue;
    MSML_CHECK(channels != 1 || d[PD_CTYPE] == 0 || d[PD_CTYPE] == 4, MSML_ERR_UNSUPPORTED,
               "png_decode: image %d has colour type %d, channels=1 takes gray streams", n, d[PD_CTYPE]);
    MSML_CHECK(d[PD_WS] == units, MSML_ERR_SHAPE, "png_decode: descriptor %d: workspace offset %d, not the %ld "
               "msml_png_workspace writes", n, d[PD_WS], units);
    units += png_ws_bytes(d) / PNG_WS_ALIGN;
    MSML_CHECK(units * PNG_WS_ALIGN <= ws_bytes, MSML_ERR_WORKSPACE, "png_decode: workspace of %ld bytes is too small "
               "(image %d ends at %ld)", ws_bytes, n, units * PNG_WS_ALIGN);
    const long grp = (long)((d[PD_W] + 3) / 4) * d[PD_H];
    max_grp = grp > max_grp ? grp : max_grp;
  }
  k_png_inflate<<<N, 64, 0, (hipStream_t)stream>>>(streams, desc, ws, status);
  MSML_LAUNCH_OK("png_inflate");
  if (max_grp == 0) return MSML_OK;                          // only refused streams: their statuses are written
  k_png_unfilter<<<N, 64, 0, (hipStream_t)stream>>>(desc, ws, status);
  MSML_LAUNCH_OK("png_unfilter");
  k_png_store<<<dim3(cdiv(max_grp, 256), N), 256, 0, (hipStream_t)stream>>>(desc, ws, palettes, dst, dst_bytes,
                                                                            meta_out, channels, swap_rb, status);
  MSML_LAUNCH_OK("png_store");
  return MSML_OK;
}
