// The packed image buffer on the device side (msml_amd/packed.py is the host side): a flat uint8 buffer and meta int64
// [N][4] = byte offset, H, W, row pitch.  What the codecs share around it: the check of a meta row against its image
// and the buffer, the store of 4 pixels of a row, the window over a compressed stream in LDS, and the zigzag order.
// Plain C++ but for the part behind __HIPCC__, so the host checks (tools/*_hostcheck.cpp) compile it too.
#ifndef MSML_PACKED_IMAGE_H
#define MSML_PACKED_IMAGE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define IMG_HD __host__ __device__
#else
#define IMG_HD
#endif

// The meta row mt = [offset, H, W, pitch] describes the H x W image with rows of row_bytes inside a buffer of
// buffer_bytes.  last_row_bytes: how far the last row reaches: row_bytes for a reader, the pitch for a writer that
// fills its rows up to the pitch.  Compared by subtraction: H <= 32767 and pitch < 2^31 keep the span below 2^46, and
// off <= buffer_bytes, so nothing overflows.
IMG_HD inline bool img_rect_ok(const long* mt, int H, int W, long row_bytes, long last_row_bytes, long buffer_bytes) {
  const long off = mt[0], pitch = mt[3];
  return !(off < 0 || off > buffer_bytes || mt[1] != H || mt[2] != W || pitch < row_bytes || pitch > 0x7fffffffL ||
           (long)(H - 1) * pitch + last_row_bytes > buffer_bytes - off);
}

// Rows leave as dwords, padded with zeros up to the pitch, where the image's offset and pitch are multiples of 4.
IMG_HD inline bool img_aligned(long off, long pitch) { return ((off | pitch) & 3) == 0; }

// natural (row-major) index of the k-th coefficient of an 8 x 8 block in zigzag order
IMG_HD inline int img_zigzag(int k) {
  constexpr unsigned char zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return zz[k & 63];
}

#if defined(__HIPCC__)
// The 4 pixels of `channels` bytes each that start at pixel x0 of a row of W pixels: px holds them back to back, zeros
// behind the row's last pixel.  One writer per byte: the thread of a group writes that group's bytes and nothing else,
// and the row's last group also the zeros between row_bytes and the pitch.  An aligned image (img_aligned) leaves as
// dwords; any other byte by byte, and then the bytes between row_bytes and the pitch are not touched.
template <int MAXC>
__device__ inline void img_store4(unsigned char* row, long off, long pitch, long row_bytes, int x0, int W, int channels,
                                  const unsigned char (&px)[MAXC * 4]) {
  const long b0 = (long)x0 * channels;
  if (img_aligned(off, pitch)) {
#pragma unroll
    for (int w = 0; w < MAXC; ++w) {
      if (w < channels && b0 + w * 4 < pitch) {
        *reinterpret_cast<unsigned int*>(row + b0 + w * 4) =
            px[w * 4] | (px[w * 4 + 1] << 8) | (px[w * 4 + 2] << 16) | ((unsigned int)px[w * 4 + 3] << 24);
      }
    }
    if (x0 + 4 >= W)                                         // the last group of the row: zeros up to the pitch
      for (long p = b0 + channels * 4; p < pitch; p += 4) *reinterpret_cast<unsigned int*>(row + p) = 0u;
  } else {
#pragma unroll
    for (int e = 0; e < MAXC * 4; ++e)
      if (e < channels * 4 && b0 + e < row_bytes) row[b0 + e] = px[e];
  }
}

// The stream of one image behind a window of IMG_CHUNK bytes in LDS, read by one wavefront: the decoder reads forward,
// and a read outside the window makes all 64 lanes fetch the chunk that holds it (aligned dwords, none past the dword
// of the stream's last byte; the decode entry points check that the stream buffer is whole dwords).
#define IMG_CHUNK 2048
struct LdsStreamSrc {
  const unsigned char* g;
  unsigned int* win;                                         // IMG_CHUNK / 4 dwords of LDS
  int w0, end, lane;                                         // w0: the window's first byte, -IMG_CHUNK before any read
  __device__ int byte(int i) {
    if ((unsigned int)(i - w0) >= (unsigned int)IMG_CHUNK) {
      w0 = i & ~(IMG_CHUNK - 1);
      __syncthreads();
      for (int k = lane; k < IMG_CHUNK / 4; k += 64) {
        const int o = w0 + k * 4;
        win[k] = o < end ? *reinterpret_cast<const unsigned int*>(g + o) : 0u;
      }
      __syncthreads();
    }
    return reinterpret_cast<const unsigned char*>(win)[i - w0];
  }
  __device__ unsigned int word(int i) {                      // i % 4 == 0, i + 4 <= end
    if ((unsigned int)(i - w0) >= (unsigned int)IMG_CHUNK) (void)byte(i);
    return win[(i - w0) >> 2];
  }
};
#endif

#endif
