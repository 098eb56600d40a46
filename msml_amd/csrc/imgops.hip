// Whole-photo uint8 operations in front of the detector, for the oriented and resized copies MTCNN.align_fully and
// MTCNN.get_landmarks make (eval/preprocess/mtcnn.py:41-158), on packed images of any sizes in one launch each:
//   k_img_orient     PIL Image.transpose(method) for FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, ROTATE_90, ROTATE_180, ROTATE_270
//   k_img_resize_h   the horizontal pass of PIL Image.resize on 3-channel uint8 (Resample.c ImagingResampleHorizontal_8bpc)
//   k_img_resize_v   the vertical pass (ImagingResampleVertical_8bpc) on the rounded uint8 intermediate
// Source and destination are packed as msml_align_warp takes its sources: meta[n] = {byte offset, H, W, row pitch}.  The
// destinations have rows of a multiple of 4 bytes; the bytes between 3 W and the pitch are written as 0.
// Integer arithmetic only (the coefficient tables come from the host in 22-bit fixed point).  No atomics, every output
// dword has one writer, all global stores are whole dwords: two runs give the same bits.
#include "common.h"

#define IMG_THREADS 256
#define ORI_TW 64                 // output pixels per tile row (192 bytes: tile rows start on a 4-byte boundary)
#define ORI_TH 32                 // output rows per tile
#define ORI_STRIDE 204            // LDS bytes per staged source row: 3 lead + 192 + 3 rounded up, an odd number of dwords
#define IMG_PREC 22               // Resample.c PRECISION_BITS

// A dword of `src` at the 4-byte aligned byte address a; the last dword of a buffer whose length is not a multiple of 4
// is assembled from the bytes that exist.
__device__ __forceinline__ unsigned int img_load_dword(const unsigned char* __restrict__ src, long a, long src_bytes) {
  if (a + 4 <= src_bytes) return *reinterpret_cast<const unsigned int*>(src + a);
  unsigned int v = 0;
  for (int k = 0; k < 4; ++k)
    if (a + k < src_bytes) v |= (unsigned int)src[a + k] << (8 * k);
  return v;
}

// One workgroup = one 32 x 64 tile of one output image.  The source rectangle of the tile (32 x 64 pixels, or 64 x 32 for
// the quarter turns) is staged in LDS by aligned dword loads, one wave per source row; then a lane assembles one output
// dword from four LDS bytes and a wave stores 196 contiguous bytes of an output row.
__global__ void __launch_bounds__(IMG_THREADS) k_img_orient(const unsigned char* __restrict__ src,
                                                            const long* __restrict__ meta,
                                                            const int* __restrict__ method,
                                                            unsigned char* __restrict__ dst,
                                                            const long* __restrict__ meta_out, long src_bytes) {
  __shared__ unsigned int s_src[ORI_TW * ORI_STRIDE / 4];
  const int n = blockIdx.y;
  const long* mi = meta + (long)n * 4;
  const long* mo = meta_out + (long)n * 4;
  const long off = mi[0], pitch = mi[3], ooff = mo[0], opitch = mo[3];
  const int H = (int)mi[1], W = (int)mi[2], OH = (int)mo[1], OW = (int)mo[2];
  const int m = method[n];
  const int tiles_x = (OW + ORI_TW - 1) / ORI_TW, tiles_y = (OH + ORI_TH - 1) / ORI_TH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;                       // the grid is sized for the largest image
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int oy0 = ty * ORI_TH, ox0 = tx * ORI_TW;
  const int th = OH - oy0 < ORI_TH ? OH - oy0 : ORI_TH, tw = OW - ox0 < ORI_TW ? OW - ox0 : ORI_TW;
  const bool turn = m == 2 || m == 4;
  // the source rectangle: rows [sy0, sy0 + R), pixels [sx0, sx0 + C)
  const int R = turn ? tw : th, C = turn ? th : tw;
  int sx0, sy0;
  switch (m) {
    case 0: sx0 = W - ox0 - tw; sy0 = oy0; break;                         // out(y, x) = in(y, W - 1 - x)
    case 1: sx0 = ox0; sy0 = H - oy0 - th; break;                         // out(y, x) = in(H - 1 - y, x)
    case 2: sx0 = W - oy0 - th; sy0 = ox0; break;                         // out(y, x) = in(x, W - 1 - y)
    case 3: sx0 = W - ox0 - tw; sy0 = H - oy0 - th; break;                // out(y, x) = in(H - 1 - y, W - 1 - x)
    default: sx0 = oy0; sy0 = H - ox0 - tw; break;                        // out(y, x) = in(H - 1 - x, y)
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long first = off + (long)sx0 * 3;                                 // byte of the rectangle's first pixel in row 0
  for (int r = wave; r < R; r += IMG_THREADS / 64) {
    const long g = first + (long)(sy0 + r) * pitch;
    const long a = g & ~3L;
    const int ndw = ((int)(g - a) + 3 * C + 3) >> 2;                      // at most (3 + 192 + 3) / 4 = 49
    if (lane < ndw) s_src[r * (ORI_STRIDE / 4) + lane] = img_load_dword(src, a + 4L * lane, src_bytes);
  }
  __syncthreads();
  const unsigned char* s_bytes = reinterpret_cast<const unsigned char*>(s_src);
  // the last tile of a row also writes the zero bytes up to the pitch
  const int row_bytes = tx == tiles_x - 1 ? (int)(opitch - (long)ox0 * 3) : ORI_TW * 3;
  const int row_dw = row_bytes >> 2;                                      // at most 192 / 4 + 0: pitch - 3 OW < 4
  for (int y = wave; y < th; y += IMG_THREADS / 64) {
    if (lane >= row_dw) continue;
    unsigned int v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int b = lane * 4 + k, px = b / 3, c = b - px * 3;
      if (px >= tw) continue;
      int lr, lc;
      switch (m) {
        case 0: lr = y; lc = tw - 1 - px; break;
        case 1: lr = th - 1 - y; lc = px; break;
        case 2: lr = px; lc = th - 1 - y; break;
        case 3: lr = th - 1 - y; lc = tw - 1 - px; break;
        default: lr = tw - 1 - px; lc = y; break;
      }
      const int lead = (int)((first + (long)(sy0 + lr) * pitch) & 3);
      v |= (unsigned int)s_bytes[lr * ORI_STRIDE + lead + lc * 3 + c] << (8 * k);
    }
    *reinterpret_cast<unsigned int*>(dst + ooff + (long)(oy0 + y) * opitch + (long)ox0 * 3 + lane * 4) = v;
  }
}

// jobs[n] = {offset of the horizontal table in `tables` (ints), its taps per output, offset of the vertical table, its
// taps, byte offset of the intermediate in ws}.  A table row of an axis = {first tap, taps, coefficients[ksize]}.
#define IMG_JOB 5

// One workgroup = 256 output pixels of one row of the intermediate [H][pitch of the output].  A lane sums its pixel's
// taps from global memory (neighbouring lanes share cache lines), the three bytes meet in LDS and leave as dwords.
__global__ void __launch_bounds__(IMG_THREADS) k_img_resize_h(const unsigned char* __restrict__ src,
                                                              const long* __restrict__ meta,
                                                              const long* __restrict__ meta_out,
                                                              const int* __restrict__ tables,
                                                              const long* __restrict__ jobs,
                                                              unsigned char* __restrict__ ws) {
  __shared__ unsigned int s_out[IMG_THREADS * 3 / 4];
  const int n = blockIdx.y;
  const long* mi = meta + (long)n * 4;
  const long* mo = meta_out + (long)n * 4;
  const long* job = jobs + (long)n * IMG_JOB;
  const int H = (int)mi[1], OW = (int)mo[2];
  const long ipitch = mo[3];
  const int chunks = (OW + IMG_THREADS - 1) / IMG_THREADS;
  if ((long)blockIdx.x >= (long)H * chunks) return;
  const int y = blockIdx.x / chunks, chunk = blockIdx.x - y * chunks;
  const int x0 = chunk * IMG_THREADS, t = threadIdx.x, x = x0 + t;
  unsigned char* s_bytes = reinterpret_cast<unsigned char*>(s_out);
  int r0 = 0, r1 = 0, r2 = 0;
  if (x < OW) {
    const int ksize = (int)job[1];
    const int* row = tables + job[0] + (long)x * (ksize + 2);
    const int xmin = row[0], cnt = row[1];
    const unsigned char* p = src + mi[0] + (long)y * mi[3] + (long)xmin * 3;
    int a0 = 1 << (IMG_PREC - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < cnt; ++j, p += 3) {
      const int k = row[2 + j];
      a0 += (int)p[0] * k;
      a1 += (int)p[1] * k;
      a2 += (int)p[2] * k;
    }
    a0 >>= IMG_PREC; a1 >>= IMG_PREC; a2 >>= IMG_PREC;
    r0 = a0 < 0 ? 0 : (a0 > 255 ? 255 : a0);
    r1 = a1 < 0 ? 0 : (a1 > 255 ? 255 : a1);
    r2 = a2 < 0 ? 0 : (a2 > 255 ? 255 : a2);
  }
  s_bytes[t * 3] = (unsigned char)r0;                                     // pixels beyond OW: the zero bytes of the pitch
  s_bytes[t * 3 + 1] = (unsigned char)r1;
  s_bytes[t * 3 + 2] = (unsigned char)r2;
  __syncthreads();
  const long row_bytes = ipitch - (long)x0 * 3;
  const int row_dw = row_bytes < IMG_THREADS * 3 ? (int)(row_bytes >> 2) : IMG_THREADS * 3 / 4;
  if (t < row_dw) *reinterpret_cast<unsigned int*>(ws + job[4] + (long)y * ipitch + (long)x0 * 3 + t * 4) = s_out[t];
}

// One workgroup = 256 dwords of one output row; a lane owns 4 consecutive bytes of the row and reads the same 4 bytes of
// every tap row of the intermediate (rows of both are a multiple of 4 bytes: aligned dwords, contiguous across the wave).
__global__ void __launch_bounds__(IMG_THREADS) k_img_resize_v(const unsigned char* __restrict__ ws,
                                                              const long* __restrict__ meta_out,
                                                              const int* __restrict__ tables,
                                                              const long* __restrict__ jobs,
                                                              unsigned char* __restrict__ dst) {
  const int n = blockIdx.y;
  const long* mo = meta_out + (long)n * 4;
  const long* job = jobs + (long)n * IMG_JOB;
  const int OH = (int)mo[1];
  const long opitch = mo[3];
  const int row_dw = (int)(opitch >> 2);
  const int chunks = (row_dw + IMG_THREADS - 1) / IMG_THREADS;
  if ((long)blockIdx.x >= (long)OH * chunks) return;
  const int y = blockIdx.x / chunks, chunk = blockIdx.x - y * chunks;
  const int d = chunk * IMG_THREADS + threadIdx.x;
  if (d >= row_dw) return;
  const int ksize = (int)job[3];
  const int* row = tables + job[2] + (long)y * (ksize + 2);
  const int ymin = row[0], cnt = row[1];
  const unsigned char* p = ws + job[4] + (long)ymin * opitch + (long)d * 4;
  int a0 = 1 << (IMG_PREC - 1), a1 = a0, a2 = a0, a3 = a0;
  for (int j = 0; j < cnt; ++j, p += opitch) {
    const unsigned int v = *reinterpret_cast<const unsigned int*>(p);
    const int k = row[2 + j];
    a0 += (int)(v & 255u) * k;
    a1 += (int)((v >> 8) & 255u) * k;
    a2 += (int)((v >> 16) & 255u) * k;
    a3 += (int)(v >> 24) * k;
  }
  a0 >>= IMG_PREC; a1 >>= IMG_PREC; a2 >>= IMG_PREC; a3 >>= IMG_PREC;
  a0 = a0 < 0 ? 0 : (a0 > 255 ? 255 : a0);
  a1 = a1 < 0 ? 0 : (a1 > 255 ? 255 : a1);
  a2 = a2 < 0 ? 0 : (a2 > 255 ? 255 : a2);
  a3 = a3 < 0 ? 0 : (a3 > 255 ? 255 : a3);
  *reinterpret_cast<unsigned int*>(dst + mo[0] + (long)y * opitch + (long)d * 4) =
      (unsigned int)a0 | ((unsigned int)a1 << 8) | ((unsigned int)a2 << 16) | ((unsigned int)a3 << 24);
}

static inline bool img_size_ok(long v) { return v >= 1 && v <= 32767; }

// plan [N][3] (HOST) = method, out_h, out_w of every image: what the library can check before the launch
extern "C" int msml_img_orient(const unsigned char* src, long src_bytes, const long* meta, const int* method,
                               unsigned char* dst, const long* meta_out, const long* plan, int N, void* stream) {
  MSML_CHECK(N >= 1, MSML_ERR_UNSUPPORTED, "img_orient: N=%d", N);
  MSML_CHECK(N <= 65535, MSML_ERR_UNSUPPORTED, "img_orient: N=%d is more than 65535 images in one launch", N);
  MSML_CHECK(src && meta && method && dst && meta_out && plan && src_bytes > 0, MSML_ERR_SHAPE,
             "img_orient: null pointer");
  MSML_CHECK(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)method & 3) == 0 &&
                 ((uintptr_t)meta & 7) == 0 && ((uintptr_t)meta_out & 7) == 0,
             MSML_ERR_SHAPE, "img_orient: src, dst and method must be 4-byte, meta and meta_out 8-byte aligned");
  long tiles = 0;
  for (int i = 0; i < N; ++i) {
    const long* p = plan + (long)i * 3;
    MSML_CHECK(p[0] >= 0 && p[0] <= 4, MSML_ERR_UNSUPPORTED, "img_orient: method %ld of image %d is outside 0..4", p[0], i);
    MSML_CHECK(img_size_ok(p[1]) && img_size_ok(p[2]), MSML_ERR_UNSUPPORTED,
               "img_orient: image %d is %ld x %ld, outside 1..32767", i, p[1], p[2]);
    const long t = (long)cdiv(p[1], ORI_TH) * cdiv(p[2], ORI_TW);
    tiles = t > tiles ? t : tiles;
  }
  k_img_orient<<<dim3((unsigned)tiles, N), IMG_THREADS, 0, (hipStream_t)stream>>>(src, meta, method, dst, meta_out,
                                                                                  src_bytes);
  MSML_LAUNCH_OK("img_orient");
  return MSML_OK;
}

// sizes [N][4] (HOST) = in_h, in_w, out_h, out_w: the intermediates [in_h][pitch of out_w] of all images back to back;
// 0 for a size outside 1..32767
extern "C" long msml_img_resize_workspace(const long* sizes, int N) {
  if (!sizes || N < 1) return 0;
  long total = 0;
  for (int i = 0; i < N; ++i) {
    const long* s = sizes + (long)i * 4;
    if (!img_size_ok(s[0]) || !img_size_ok(s[1]) || !img_size_ok(s[2]) || !img_size_ok(s[3])) return 0;
    total += s[0] * ((s[3] * 3 + 3) & ~3L);
  }
  return total;
}

extern "C" int msml_img_resize(const unsigned char* src, const long* meta, unsigned char* dst, const long* meta_out,
                               const int* tables, const long* jobs, const long* sizes, int N, int filter,
                               unsigned char* ws, long ws_bytes, void* stream) {
  MSML_CHECK(N >= 1, MSML_ERR_UNSUPPORTED, "img_resize: N=%d", N);
  MSML_CHECK(N <= 65535, MSML_ERR_UNSUPPORTED, "img_resize: N=%d is more than 65535 images in one launch", N);
  MSML_CHECK(filter == 2 || filter == 3, MSML_ERR_UNSUPPORTED,
             "img_resize: filter %d is neither 2 (bilinear) nor 3 (bicubic)", filter);
  MSML_CHECK(src && meta && dst && meta_out && tables && jobs && sizes && ws, MSML_ERR_SHAPE,
             "img_resize: null pointer");
  MSML_CHECK(((uintptr_t)dst & 3) == 0 && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)tables & 3) == 0 &&
                 ((uintptr_t)meta & 7) == 0 && ((uintptr_t)meta_out & 7) == 0 && ((uintptr_t)jobs & 7) == 0,
             MSML_ERR_SHAPE, "img_resize: dst, ws and tables must be 4-byte, meta, meta_out and jobs 8-byte aligned");
  long gh = 0, gv = 0;
  for (int i = 0; i < N; ++i) {
    const long* s = sizes + (long)i * 4;
    MSML_CHECK(img_size_ok(s[0]) && img_size_ok(s[1]) && img_size_ok(s[2]) && img_size_ok(s[3]), MSML_ERR_UNSUPPORTED,
               "img_resize: image %d goes from %ld x %ld to %ld x %ld, outside 1..32767", i, s[0], s[1], s[2], s[3]);
    const long h = s[0] * cdiv(s[3], IMG_THREADS), v = s[2] * cdiv((s[3] * 3 + 3) >> 2, IMG_THREADS);
    gh = h > gh ? h : gh;
    gv = v > gv ? v : gv;
  }
  const long need = msml_img_resize_workspace(sizes, N);
  MSML_CHECK(ws_bytes >= need, MSML_ERR_WORKSPACE,
             "img_resize: workspace of %ld bytes, msml_img_resize_workspace asks for %ld", ws_bytes, need);
  k_img_resize_h<<<dim3((unsigned)gh, N), IMG_THREADS, 0, (hipStream_t)stream>>>(src, meta, meta_out, tables, jobs, ws);
  MSML_LAUNCH_OK("img_resize (horizontal)");
  k_img_resize_v<<<dim3((unsigned)gv, N), IMG_THREADS, 0, (hipStream_t)stream>>>(ws, meta_out, tables, jobs, dst);
  MSML_LAUNCH_OK("img_resize (vertical)");
  return MSML_OK;
}
