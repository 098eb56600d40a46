// Model inputs of the occlusion sweep of test.py on the device: the per-image PIL loop of _load_one_input
// (eval/qeval_mxnet.py:173-189, called 2 x num times per extraction by start_extract :302-312) and the normalisation
// of :319-324, for N decoded faces in one launch:
//   k_eval_pairs   transpose(FLIP_LEFT_RIGHT) (:175-176, mirrored rows only) -> CenterCrop((out_h, out_w)) with its
//                  zero padding (:178-180) -> Grayscale() (:97-101) -> RandomBlock.paste with the black / white / gauss
//                  fill (:544-547, datasets/augment/rand_occ.py:43-72), every row (BB) or even images only (NB,
//                  qeval_mxnet.py:184-187) -> ToTensor -> sub_(0.5).div_(0.5)
// Integer arithmetic up to the byte, then one to three f32 steps; the gauss fill draws its normals with Box-Muller in
// f64 from the counter-based generator of occ.hip.  tests/sweep_cases.py restates all of it with PIL itself.  No
// atomics, every output element has one writer: two runs give the same bits.
#include "common.h"

// every floating-point expression below is restated operation by operation on the CPU: no FMA contraction
#pragma clang fp contract(off)

#define EVAL_ROWS 4            // output rows per workgroup
#define EVAL_MAX 256           // largest H, W, out_h, out_w
#define EVAL_GAUSS_SALT 0x6761757373ULL      // "gauss": keeps the fill's stream apart from the descriptor draws

// splitmix64, the generator of occ.hip (occ_mix)
__host__ __device__ inline unsigned long long eval_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// One standard normal per (row key, block row, block column, channel): Box-Muller in f64 on the two halves of one
// 64-bit draw, u1 in (0, 1], u2 in [0, 1).
__device__ __forceinline__ double eval_normal(unsigned long long rowkey, long ry, long rx, int c) {
  const unsigned long long r = eval_mix(rowkey + (((unsigned long long)ry * 256ULL + (unsigned long long)rx) * 4ULL +
                                                  (unsigned long long)c));
  const double u1 = ((double)(unsigned int)(r >> 32) + 1.0) * (1.0 / 4294967296.0);
  const double u2 = (double)(unsigned int)r * (1.0 / 4294967296.0);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// One workgroup = one image x one band of EVAL_ROWS output rows, for the plain AND the mirrored output row: the
// source rows of the band are read once, as whole dwords, into LDS; a work item is 4 consecutive output pixels of one
// (mirrored?, y), which leave as one 16-byte store per channel.  (offy, offx) = crop origin - padding: output pixel
// (y, x) is pixel (y + offy, x + offx) of the (mirrored) source, or the padding's 0 outside it.
template <bool GRAY>
__global__ void __launch_bounds__(256) k_eval_pairs(const unsigned char* __restrict__ src, long total_bytes,
                                                    const int* __restrict__ desc, float* __restrict__ out, int H, int W,
                                                    int out_h, int out_w, int offy, int offx, int bands, int norm,
                                                    int fill, int protocol, unsigned long long seedkey, long index0) {
  __shared__ unsigned int s_rows[EVAL_ROWS * EVAL_MAX * 3 / 4 + 4];
  __shared__ int s_desc[2][5];
  const int n = blockIdx.x / bands, band = blockIdx.x - n * bands;
  const int t = threadIdx.x;
  const int y_first = band * EVAL_ROWS;
  const int rows = out_h - y_first < EVAL_ROWS ? out_h - y_first : EVAL_ROWS;
  const long g = index0 + n;                                   // the image's global index
  const bool skip = protocol == 1 && (g & 1);                  // NB: odd images stay clean
  if (t < 10) {
    const int f = t / 5, k = t - f * 5;
    s_desc[f][k] = (desc && !skip) ? desc[((long)2 * n + f) * 64 + k] : 0;
  }
  // the band's source rows, contiguous in src: [b0, b1) widened to whole dwords
  const int sy_lo = y_first + offy > 0 ? y_first + offy : 0;
  const int sy_hi = y_first + rows - 1 + offy < H - 1 ? y_first + rows - 1 + offy : H - 1;
  long head = 0;
  if (sy_lo <= sy_hi) {
    const long b0 = ((long)n * H + sy_lo) * W * 3, b1 = ((long)n * H + sy_hi + 1) * W * 3;
    const long a0 = b0 & ~3L;
    head = b0 - a0;
    const int words = (int)((b1 - a0 + 3) >> 2);               // <= EVAL_ROWS * 768 / 4 + 1
    for (int i = t; i < words; i += 256) {
      const long a = a0 + 4L * i;
      unsigned int w;
      if (a + 4 <= total_bytes) w = *reinterpret_cast<const unsigned int*>(src + a);
      else {                                                   // the last, partial dword of the whole buffer
        w = 0;
        for (int k = 0; k < 4; ++k)
          if (a + k < total_bytes) w |= (unsigned int)src[a + k] << (8 * k);
      }
      s_rows[i] = w;
    }
  }
  __syncthreads();
  const unsigned char* lds = reinterpret_cast<const unsigned char*>(s_rows) + head;
  constexpr int C = GRAY ? 1 : 3;
  const int wq = out_w / 4;
  const long plane = (long)out_h * out_w;
  const int items = 2 * rows * wq;
  for (int item = t; item < items; item += 256) {
    const int f = item / (rows * wq), rem = item - f * rows * wq;
    const int r = rem / wq, x = (rem - r * wq) * 4;
    const int y = y_first + r, sy = y + offy;
    const bool yin = sy >= 0 && sy < H;
    const int kind = s_desc[f][0];
    const long bx = s_desc[f][1], by = s_desc[f][2], bw = s_desc[f][3], bh = s_desc[f][4];
    const bool brow = kind == 3 && y >= by && y < by + bh;
    const bool poison = kind != 0 && kind != 3;
    const unsigned long long rowkey = eval_mix(seedkey + (unsigned long long)(2 * g + f));
    const unsigned char* row = lds + (long)(sy - sy_lo) * W * 3;           // dereferenced only under yin
    f32x4 o[C];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ox = x + e, sxm = ox + offx;
      unsigned int v[3] = {0u, 0u, 0u};
      if (yin && sxm >= 0 && sxm < W) {
        const unsigned char* p = row + (f ? W - 1 - sxm : sxm) * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
      }
      if (GRAY) v[0] = (19595u * v[0] + 38470u * v[1] + 7471u * v[2] + 0x8000u) >> 16;
      if (brow && ox >= bx && ox < bx + bw) {
        if (fill == 0) v[0] = v[1] = v[2] = 0u;
        else if (fill == 1) v[0] = v[1] = v[2] = 255u;
        else if (GRAY) {                         // Image.paste of a mode-F block into L: f32, clip to 0..255, truncate
          const float fv = (float)(eval_normal(rowkey, y - by, ox - bx, 0) * 255.0);
          v[0] = fv <= 0.0f ? 0u : (fv >= 255.0f ? 255u : (unsigned int)fv);
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c)            // .astype(uint8): truncate toward zero, wrap modulo 256
            v[c] = (unsigned int)((long)(eval_normal(rowkey, y - by, ox - bx, c) * 255.0) & 255L);
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float q = (float)v[c] / 255.0f;          // ToTensor
        if (norm) {
          q = q - 0.5f;                          // sub_(0.5)
          q = q / 0.5f;                          // div_(0.5)
        }
        if (poison) q = __int_as_float(0x7fc00000);
        o[c][e] = q;
      }
    }
    float* dst = out + ((long)2 * n + f) * C * plane + (long)y * out_w + x;
#pragma unroll
    for (int c = 0; c < C; ++c) *reinterpret_cast<f32x4*>(dst + c * plane) = o[c];
  }
}

// round((d) / 2.0) of Python for d >= 0: half to even
static inline int eval_crop_origin(int d) {
  const int q = d / 2;
  return (d & 1) ? q + (q & 1) : q;
}

extern "C" int msml_eval_pairs(const unsigned char* src, int N, int H, int W, const int* desc, float* out, int out_h,
                               int out_w, int gray, int norm, int fill, int protocol, long seed, long index0,
                               void* stream) {
  MSML_CHECK(src && out, MSML_ERR_SHAPE, "eval_pairs: null pointer");
  MSML_CHECK(N >= 1, MSML_ERR_UNSUPPORTED, "eval_pairs: N=%d", N);
  MSML_CHECK(out_w % 4 == 0, MSML_ERR_UNSUPPORTED, "eval_pairs: output width %d is not a multiple of 4 (16-byte stores)",
             out_w);
  MSML_CHECK(H >= 4 && H <= EVAL_MAX && W >= 4 && W <= EVAL_MAX && out_h >= 4 && out_h <= EVAL_MAX && out_w >= 4 &&
                 out_w <= EVAL_MAX,
             MSML_ERR_UNSUPPORTED, "eval_pairs: source %dx%d or output %dx%d outside 4..%d", H, W, out_h, out_w, EVAL_MAX);
  MSML_CHECK(fill >= 0 && fill <= 2, MSML_ERR_UNSUPPORTED, "eval_pairs: fill %d (0 black, 1 white, 2 gauss)", fill);
  MSML_CHECK(protocol >= 0 && protocol <= 1, MSML_ERR_UNSUPPORTED, "eval_pairs: protocol %d (0 BB, 1 NB)", protocol);
  MSML_CHECK(!(protocol == 1 && gray), MSML_ERR_UNSUPPORTED,
             "eval_pairs: the NB protocol has no gray form (the reference's own raises there)");
  MSML_CHECK(index0 >= 0 && index0 < (1L << 60), MSML_ERR_SHAPE, "eval_pairs: index0=%ld", index0);
  MSML_CHECK(((uintptr_t)src & 3) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 3) == 0, MSML_ERR_SHAPE,
             "eval_pairs: src and desc must be 4-byte and out 16-byte aligned");
  const int bands = cdiv(out_h, EVAL_ROWS);
  MSML_CHECK((long)N * bands < 2147483647L, MSML_ERR_SHAPE, "eval_pairs: N=%d is too many workgroups", N);
  const int offy = H < out_h ? -((out_h - H) / 2) : eval_crop_origin(H - out_h);
  const int offx = W < out_w ? -((out_w - W) / 2) : eval_crop_origin(W - out_w);
  const unsigned long long key = eval_mix((unsigned long long)seed + EVAL_GAUSS_SALT);
  const long total = (long)N * H * W * 3;
  if (gray)
    k_eval_pairs<true><<<N * bands, 256, 0, (hipStream_t)stream>>>(src, total, desc, out, H, W, out_h, out_w, offy, offx,
                                                                   bands, norm != 0, fill, protocol, key, index0);
  else
    k_eval_pairs<false><<<N * bands, 256, 0, (hipStream_t)stream>>>(src, total, desc, out, H, W, out_h, out_w, offy, offx,
                                                                    bands, norm != 0, fill, protocol, key, index0);
  MSML_LAUNCH_OK("eval_pairs");
  return MSML_OK;
}
