// Baseline JPEG decoding on the device, bit-exact with libjpeg's defaults (JDCT_ISLOW, fancy upsampling): the
// mx.image.imdecode / cv2.imread in front of every input path of the reference (datasets/load_dataset.py,
// eval/verification.py).  The arithmetic is csrc/jpeg_core.h, shared with the host check; tests/jpeg_cases.py restates it.
//   k_jpeg_entropy  one wavefront per image: the Huffman walk is the same for all 64 lanes (every address it reads is
//                   wave-uniform) out of LDS: the image's Huffman tables and a window of its stream.  Lane k keeps the
//                   k-th coefficient of the current block, so a finished block leaves as one 128-byte vector store.
//                   Writes status[n].
//                   (csrc/jpeg_entropy_kernel.h; for a batch with progressive images msml_jpeg_decode_scans hands this
//                   pass to csrc/jpeg_prog.hip, which also walks those images: k_jpeg_prog)
//   k_jpeg_idct     one thread per 8 x 8 block: dequantise, IDCT, into the component planes of the workspace
//   k_jpeg_store    one thread per 4 output pixels: upsample, convert, store into the packed destination
// No atomics, one writer per byte: two runs give the same bits.  An image whose status is not 0 is skipped by the two
// later passes: its output rectangle is left as it was.
#include "common.h"
#include "jpeg_entropy_kernel.h"

// jpeg_prog.hip: the entropy pass of a batch that holds progressive images
int jpeg_prog_entropy(const unsigned char* streams, const int* desc, const int* scans, const int* htabs,
                      unsigned char* ws, int* status, int N, int progressive, hipStream_t stream);

__global__ void __launch_bounds__(256) k_jpeg_idct(const int* __restrict__ desc, const int* __restrict__ qtabs,
                                                   unsigned char* __restrict__ ws, const int* __restrict__ status) {
  const int n = blockIdx.y;
  if (status[n] != 0) return;
  const int* d = desc + (long)n * JPG_DESC_WORDS;
  JpgLayout L;
  jpg_layout(d, L);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= L.nblk) return;
  // the component of block i, and its fields picked by comparison: indexing L's arrays with a run-time c would put
  // the whole struct into scratch
  const int c = i >= L.cbase[2] && L.ncomp == 3 ? 2 : (i >= L.cbase[1] && L.ncomp == 3 ? 1 : 0);
  const long cbase = c == 2 ? L.cbase[2] : (c == 1 ? L.cbase[1] : L.cbase[0]);
  const long pbase = c == 2 ? L.pbase[2] : (c == 1 ? L.pbase[1] : L.pbase[0]);
  const int bw = c == 2 ? L.bw[2] : (c == 1 ? L.bw[1] : L.bw[0]);
  const long j = i - cbase;
  const int by = (int)(j / bw), bx = (int)(j - (long)by * bw);
  unsigned char* base = ws + (long)d[JD_WS] * JPG_WS_ALIGN;
  const long pitch = (long)bw * 8;
  jpg_idct(reinterpret_cast<const int16_t*>(base) + i * 64, qtabs + (long)d[JD_QT + c] * 64,
           base + pbase + (long)by * 8 * pitch + bx * 8, pitch);
}

// channels 3: R, G, B (B, G, R with swap_rb); channels 1: the Y plane.  A thread owns 4 pixels of a row; where the
// image's offset and pitch are multiples of 4 they leave as dwords, and the bytes between the row and its pitch as 0.
__global__ void __launch_bounds__(256) k_jpeg_store(const int* __restrict__ desc, const unsigned char* __restrict__ ws,
                                                    unsigned char* __restrict__ dst, long dst_bytes,
                                                    const long* __restrict__ meta, int channels, int swap_rb,
                                                    int* __restrict__ status) {
  const int n = blockIdx.y;
  if (status[n] != 0) return;
  const int* d = desc + (long)n * JPG_DESC_WORDS;
  const int H = d[JD_H], W = d[JD_W];
  const long* mt = meta + (long)n * 4;
  const long off = mt[0], pitch = mt[3];
  const long rowb = (long)W * channels;
  // the destination rectangle is checked here, on the device, where meta_out lives: an image that does not fit is
  // not written (every workgroup of the image sees the same values and leaves)
  if (!img_rect_ok(mt, H, W, rowb, img_aligned(off, pitch) ? pitch : rowb, dst_bytes)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) status[n] = JPG_ERR_OUTPUT;
    return;
  }
  const int gw = (W + 3) / 4;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)gw * H) return;
  const int y = (int)(g / gw), x0 = (int)(g - (long)y * gw) * 4;
  JpgLayout L;
  jpg_layout(d, L);
  const unsigned char* base = ws + (long)d[JD_WS] * JPG_WS_ALIGN;
  unsigned char px[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) px[e] = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (x0 + e < W) {
      if (channels == 1) {
        px[e] = base[L.pbase[0] + (long)y * (L.bw[0] * 8) + x0 + e];
      } else {
        int rgb[3];
        jpg_pixel(d, L, base, x0 + e, y, rgb);
        px[e * 3 + 0] = (unsigned char)rgb[swap_rb ? 2 : 0];
        px[e * 3 + 1] = (unsigned char)rgb[1];
        px[e * 3 + 2] = (unsigned char)rgb[swap_rb ? 0 : 2];
      }
    }
  }
  img_store4<3>(dst + off + (long)y * pitch, off, pitch, rowb, x0, W, channels, px);
}

extern "C" long msml_jpeg_workspace(int* desc, int N) {
  if (!desc || N < 1) return 0;
  long units = 0;
  for (int n = 0; n < N; ++n) {
    int* d = desc + (long)n * JPG_DESC_WORDS;
    d[JD_WS] = 0;
    if (d[JD_STATUS] != 0) continue;
    if (jpg_desc_ok(d, 0x7fffffffffffL, 0x7fffffff, 0x7fffffff) != 1) return 0;
    if (units > 0x7fffffffL) return 0;
    JpgLayout L;
    jpg_layout(d, L);
    d[JD_WS] = (int)units;
    units += L.bytes / JPG_WS_ALIGN;
  }
  return units * JPG_WS_ALIGN;
}

// msml_jpeg_decode (scans == nullptr: every image is baseline) and msml_jpeg_decode_scans
static int jpeg_decode_any(const unsigned char* streams, long stream_bytes, const int* desc, const int* desc_host,
                           const int* scans, const int* scans_host, long nscan, const int* qtabs, int nq,
                           const int* htabs, int nh, unsigned char* dst, long dst_bytes, const long* meta_out,
                           int channels, int swap_rb, int* status, unsigned char* ws, long ws_bytes, int N,
                           void* stream) {
  MSML_CHECK(N >= 1 && N <= 65535, MSML_ERR_UNSUPPORTED, "jpeg_decode: N=%d outside 1..65535", N);
  MSML_CHECK(channels == 1 || channels == 3, MSML_ERR_UNSUPPORTED, "jpeg_decode: channels=%d (1 or 3)", channels);
  MSML_CHECK(streams && desc && desc_host && qtabs && htabs && dst && meta_out && status && ws, MSML_ERR_SHAPE,
             "jpeg_decode: null pointer");
  MSML_CHECK(((uintptr_t)streams & 3) == 0 && ((uintptr_t)desc & 3) == 0 && ((uintptr_t)qtabs & 3) == 0 &&
                 ((uintptr_t)htabs & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)status & 3) == 0 &&
                 ((uintptr_t)meta_out & 7) == 0 && ((uintptr_t)ws & 15) == 0,
             MSML_ERR_SHAPE, "jpeg_decode: streams, desc, tables, dst, status must be 4-byte, meta_out 8-byte, ws 16-byte "
                             "aligned");
  MSML_CHECK(stream_bytes % 4 == 0, MSML_ERR_SHAPE, "jpeg_decode: stream_bytes=%ld is not whole dwords", stream_bytes);
  MSML_CHECK(stream_bytes >= 0 && dst_bytes >= 0 && ws_bytes >= 0 && nq >= 1 && nh >= 1, MSML_ERR_SHAPE,
             "jpeg_decode: stream_bytes=%ld dst_bytes=%ld ws_bytes=%ld nq=%d nh=%d", stream_bytes, dst_bytes, ws_bytes,
             nq, nh);
  long units = 0, max_blk = 0, max_grp = 0;
  int progressive = 0;
  for (int n = 0; n < N; ++n) {
    const int* d = desc_host + (long)n * JPG_DESC_WORDS;
    MSML_CHECK(jpg_desc_ok(d, stream_bytes, nq, nh) == 1, MSML_ERR_SHAPE, "jpeg_decode: descriptor %d is inconsistent", n);
    if (d[JD_STATUS] != 0) continue;
    if (scans) {
      MSML_CHECK(jpg_scans_ok(d, scans_host, nscan, nh), MSML_ERR_SHAPE,
                 "jpeg_decode_scans: the scan records of image %d are inconsistent", n);
      progressive += d[JD_NSCAN] > 0;
    }
    MSML_CHECK(channels == 3 || d[JD_NCOMP] == 1, MSML_ERR_UNSUPPORTED,
               "jpeg_decode: image %d has 3 components, channels=1 takes gray streams", n);
    JpgLayout L;
    jpg_layout(d, L);
    MSML_CHECK(d[JD_WS] == units, MSML_ERR_SHAPE, "jpeg_decode: descriptor %d: workspace offset %d, not the %ld "
               "msml_jpeg_workspace writes", n, d[JD_WS], units);
    units += L.bytes / JPG_WS_ALIGN;
    MSML_CHECK(units * JPG_WS_ALIGN <= ws_bytes, MSML_ERR_WORKSPACE, "jpeg_decode: workspace of %ld bytes is too small "
               "(image %d ends at %ld)", ws_bytes, n, units * JPG_WS_ALIGN);
    const long grp = (long)((d[JD_W] + 3) / 4) * d[JD_H];
    max_blk = L.nblk > max_blk ? L.nblk : max_blk;
    max_grp = grp > max_grp ? grp : max_grp;
  }
  if (scans) {
    const int rc = jpeg_prog_entropy(streams, desc, scans, htabs, ws, status, N, max_blk ? progressive : 0, (hipStream_t)stream);
    if (rc != MSML_OK) return rc;
  } else {
    k_jpeg_entropy<false><<<N, 64, 0, (hipStream_t)stream>>>(streams, desc, htabs, ws, status);
    MSML_LAUNCH_OK("jpeg_entropy");
  }
  if (max_blk == 0) return MSML_OK;                          // only refused streams: their statuses are written
  k_jpeg_idct<<<dim3(cdiv(max_blk, 256), N), 256, 0, (hipStream_t)stream>>>(desc, qtabs, ws, status);
  MSML_LAUNCH_OK("jpeg_idct");
  k_jpeg_store<<<dim3(cdiv(max_grp, 256), N), 256, 0, (hipStream_t)stream>>>(desc, ws, dst, dst_bytes, meta_out,
                                                                             channels, swap_rb, status);
  MSML_LAUNCH_OK("jpeg_store");
  return MSML_OK;
}

extern "C" int msml_jpeg_decode(const unsigned char* streams, long stream_bytes, const int* desc, const int* desc_host,
                                const int* qtabs, int nq, const int* htabs, int nh, unsigned char* dst, long dst_bytes,
                                const long* meta_out, int channels, int swap_rb, int* status, unsigned char* ws,
                                long ws_bytes, int N, void* stream) {
  return jpeg_decode_any(streams, stream_bytes, desc, desc_host, nullptr, nullptr, 0, qtabs, nq, htabs, nh, dst,
                         dst_bytes, meta_out, channels, swap_rb, status, ws, ws_bytes, N, stream);
}

extern "C" int msml_jpeg_decode_scans(const unsigned char* streams, long stream_bytes, const int* desc,
                                      const int* desc_host, const int* scans, const int* scans_host, long nscan,
                                      const int* qtabs, int nq, const int* htabs, int nh, unsigned char* dst,
                                      long dst_bytes, const long* meta_out, int channels, int swap_rb, int* status,
                                      unsigned char* ws, long ws_bytes, int N, void* stream) {
  MSML_CHECK(scans && scans_host && nscan >= 1 && ((uintptr_t)scans & 3) == 0, MSML_ERR_SHAPE,
             "jpeg_decode_scans: needs a scan table of at least one record, 4-byte aligned (nscan=%ld)", nscan);
  return jpeg_decode_any(streams, stream_bytes, desc, desc_host, scans, scans_host, nscan, qtabs, nq, htabs, nh, dst,
                         dst_bytes, meta_out, channels, swap_rb, status, ws, ws_bytes, N, stream);
}
