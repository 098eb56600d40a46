// Face alignment of the template (IJB-B / IJB-C) evaluation on the device: the per-image work of Embedding.get and
// the staging copy of get_image_feature (eval/qeval_ijbc.py:145-187, 257-293) after the transform estimate:
//   k_align_warp    cv2.warpAffine(rimg, M, (W, H), borderValue=0.0) (:161-163) + cv2.cvtColor(BGR2RGB) (:164) of N
//                   decoded sources of any size in one launch, with OpenCV's fixed-point arithmetic restated
//                   operation by operation (classic warpAffine + remap, INTER_LINEAR, BORDER_CONSTANT)
//   k_align_pairs   RandomBlock (black) from a descriptor (:166-173), np.fliplr + the two transposes + the copy into
//                   the [2N][3][H][W] batch (:181-187, :266-267) and forward_db's div_(255).sub_(0.5).div_(0.5) (:192)
// Integer and f64 arithmetic only in the warp, three f32 steps in the pairs: tests/align_cases.py restates both bit for
// bit.  No atomics, every output byte has one writer: two runs give the same bits.
#include "common.h"

// every floating-point expression below is restated operation by operation on the CPU: no FMA contraction
#pragma clang fp contract(off)

#define ALIGN_BAND 16          // output rows per workgroup
#define ALIGN_MAX 256          // largest out_h / out_w

// cv::saturate_cast<int>(double) as the issue of this kernel defines it: round half to even, clamp in f64, convert.
// (NaN goes to INT_MIN; the host never passes one.)
__device__ __forceinline__ int align_sat_int(double v) {
  v = rint(v);
  if (!(v >= -2147483648.0)) return (int)0x80000000;
  if (v > 2147483647.0) return 0x7fffffff;
  return (int)v;
}
// 32-bit two's-complement addition (what the compiled C++ of the original does when a saturated term overflows)
__device__ __forceinline__ int align_wrap_add(int a, int b) { return (int)((unsigned int)a + (unsigned int)b); }
__device__ __forceinline__ int align_clamp16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// One workgroup = one image x one band of ALIGN_BAND output rows; lane x owns output column x for the whole band.
// meta[n] = {byte offset of the source in src, H, W, row pitch in bytes}; minv[n][6] = the inverse map (dst -> src).
// The band is assembled in LDS (3 * out_w bytes per row, rows contiguous as in dst) and leaves as whole dwords.
__global__ void __launch_bounds__(ALIGN_MAX) k_align_warp(const unsigned char* __restrict__ src,
                                                          const long* __restrict__ meta,
                                                          const double* __restrict__ minv,
                                                          unsigned char* __restrict__ dst, int out_h, int out_w,
                                                          int bands, int swap_rb) {
  __shared__ unsigned int s_band[ALIGN_BAND * ALIGN_MAX * 3 / 4];
  __shared__ int s_x0[ALIGN_BAND], s_y0[ALIGN_BAND];
  const int n = blockIdx.x / bands, band = blockIdx.x - n * bands;
  const int t = threadIdx.x;
  const int y_first = band * ALIGN_BAND;
  const int rows = out_h - y_first < ALIGN_BAND ? out_h - y_first : ALIGN_BAND;
  const long* mt = meta + (long)n * 4;
  const long off = mt[0], pitch = mt[3];
  const int H = (int)mt[1], W = (int)mt[2];
  const double* m = minv + (long)n * 6;
  if (t < rows) {                               // the per-row terms, once per band
    const double y = (double)(y_first + t);
    s_x0[t] = align_wrap_add(align_sat_int((m[1] * y + m[2]) * 1024.0), 16);
    s_y0[t] = align_wrap_add(align_sat_int((m[4] * y + m[5]) * 1024.0), 16);
  }
  __syncthreads();
  if (t < out_w) {
    const int adelta = align_sat_int(m[0] * (double)t * 1024.0);
    const int bdelta = align_sat_int(m[3] * (double)t * 1024.0);
    const unsigned char* base = src + off;
    unsigned char* row = reinterpret_cast<unsigned char*>(s_band) + t * 3;
    for (int r = 0; r < rows; ++r, row += out_w * 3) {
      const int X = align_wrap_add(s_x0[r], adelta) >> 5, Y = align_wrap_add(s_y0[r], bdelta) >> 5;
      const int sx = align_clamp16(X >> 5), sy = align_clamp16(Y >> 5);
      const int fx = X & 31, fy = Y & 31;
      const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32;
      const int w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
      const bool x0in = (unsigned)sx < (unsigned)W, x1in = (unsigned)(sx + 1) < (unsigned)W;
      const bool y0in = (unsigned)sy < (unsigned)H, y1in = (unsigned)(sy + 1) < (unsigned)H;
      const unsigned char* p0 = base + (long)sy * pitch + (long)sx * 3;      // dereferenced only under the flags
      const unsigned char* p1 = p0 + pitch;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int v00 = (y0in && x0in) ? (int)p0[c] : 0, v01 = (y0in && x1in) ? (int)p0[3 + c] : 0;
        const int v10 = (y1in && x0in) ? (int)p1[c] : 0, v11 = (y1in && x1in) ? (int)p1[3 + c] : 0;
        const int sum = v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11;
        row[swap_rb ? 2 - c : c] = (unsigned char)((sum + 16384) >> 15);
      }
    }
  }
  __syncthreads();
  const int words = rows * out_w * 3 / 4;
  unsigned int* o = reinterpret_cast<unsigned int*>(dst + ((long)n * out_h + y_first) * out_w * 3);
  for (int i = t; i < words; i += blockDim.x) o[i] = s_band[i];
}

// A thread owns 4 consecutive pixels of one row: three dwords in, three f32x4 into row 2i and the three mirrored ones
// into row 2i + 1.  A descriptor kind other than none / block poisons the image's two rows with NaN.
__global__ void __launch_bounds__(256) k_align_pairs(const unsigned char* __restrict__ faces,
                                                     const int* __restrict__ desc, float* __restrict__ out, long total,
                                                     int H, int W) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int wq = W / 4;
  const int xq = (int)(i % wq);
  const long ny = i / wq;
  const int y = (int)(ny % H);
  const long n = ny / H;
  const int x = xq * 4;
  int kind = 0, bx = 0, by = 0, bw = 0, bh = 0;
  if (desc) {
    const int* d = desc + n * 64;
    kind = d[0]; bx = d[1]; by = d[2]; bw = d[3]; bh = d[4];
  }
  const unsigned int* p = reinterpret_cast<const unsigned int*>(faces + ((n * H + y) * W + x) * 3);
  const unsigned int w0 = p[0], w1 = p[1], w2 = p[2];
  const bool rowin = kind == 3 && y >= by && y < by + bh;
  const long HW = (long)H * W;
  float* o0 = out + (2 * n) * 3 * HW + (long)y * W;
  float* o1 = o0 + 3 * HW;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = e * 3 + c;                       // byte k of the 12
      const unsigned int wd = k < 4 ? w0 : (k < 8 ? w1 : w2);
      unsigned int v = (wd >> (8 * (k & 3))) & 255u;
      if (rowin && x + e >= bx && x + e < bx + bw) v = 0;
      float f = (float)v / 255.0f;                   // div_(255)
      f = f - 0.5f;                                  // sub_(0.5)
      f = f / 0.5f;                                  // div_(0.5)
      if (kind != 0 && kind != 3) f = __int_as_float(0x7fc00000);
      a[e] = f;
      b[3 - e] = f;
    }
    *reinterpret_cast<f32x4*>(o0 + c * HW + x) = a;
    *reinterpret_cast<f32x4*>(o1 + c * HW + (W - 4 - x)) = b;
  }
}

extern "C" int msml_align_warp(const unsigned char* src, const long* meta, const double* minv, unsigned char* dst,
                               int N, int out_h, int out_w, int swap_rb, void* stream) {
  MSML_CHECK(out_w % 4 == 0, MSML_ERR_UNSUPPORTED, "align_warp: output width %d is not a multiple of 4 (dword stores)",
             out_w);
  MSML_CHECK(out_h >= 4 && out_h <= ALIGN_MAX && out_w >= 4 && out_w <= ALIGN_MAX, MSML_ERR_UNSUPPORTED,
             "align_warp: output %dx%d outside 4..%d", out_h, out_w, ALIGN_MAX);
  MSML_CHECK(N >= 1, MSML_ERR_UNSUPPORTED, "align_warp: N=%d", N);
  MSML_CHECK(src && meta && minv && dst, MSML_ERR_SHAPE, "align_warp: null pointer");
  MSML_CHECK(((uintptr_t)dst & 3) == 0 && ((uintptr_t)meta & 7) == 0 && ((uintptr_t)minv & 7) == 0, MSML_ERR_SHAPE,
             "align_warp: dst must be 4-byte, meta and minv 8-byte aligned");
  const int bands = cdiv(out_h, ALIGN_BAND);
  MSML_CHECK((long)N * bands < 2147483647L, MSML_ERR_SHAPE, "align_warp: N=%d is too many workgroups", N);
  k_align_warp<<<N * bands, cdiv(out_w, 64) * 64, 0, (hipStream_t)stream>>>(src, meta, minv, dst, out_h, out_w, bands,
                                                                            swap_rb);
  MSML_LAUNCH_OK("align_warp");
  return MSML_OK;
}

extern "C" int msml_align_pairs(const unsigned char* faces, const int* desc, float* out, int N, int H, int W,
                                void* stream) {
  MSML_CHECK(faces && out && N > 0 && H > 0 && W > 0, MSML_ERR_SHAPE, "align_pairs: bad arguments N=%d H=%d W=%d", N, H,
             W);
  MSML_CHECK(W % 4 == 0, MSML_ERR_UNSUPPORTED, "align_pairs: width %d is not a multiple of 4 (16-byte stores)", W);
  MSML_CHECK(((uintptr_t)faces & 3) == 0 && ((uintptr_t)out & 15) == 0, MSML_ERR_SHAPE,
             "align_pairs: faces must be 4-byte and out 16-byte aligned");
  const long total = (long)N * H * (W / 4);
  MSML_CHECK(total < 256L * 2147483647L, MSML_ERR_SHAPE, "align_pairs: N=%d is too many workgroups", N);
  k_align_pairs<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(faces, desc, out, total, H, W);
  MSML_LAUNCH_OK("align_pairs");
  return MSML_OK;
}
