// Split-bf16 ("bf16x3") storage for the inference path: f32-class accuracy on the bf16 MFMA.
//
// gfx950 has no TF32/xf32 matrix path; exact-f32 MFMA runs at 1/16 of the bf16 rate.  An f32 value x
// is carried as hi = bf16(x), lo = bf16(x - hi) (16 significant bits), and a product of two such
// values as  x.w ~= xh.wh + xl.wh + xh.wl  (three bf16 MFMAs with f32 accumulation, the dropped xl.wl
// term is 2^-16 relative): the embedding error against the f32 reference drops from 5e-3 (bf16) to
// 1e-5 and the occlusion-mask indices are bit-exact on the reference goldens.
//
// Storage layout (MSML_BF16X3): a pixel holds 3*C bf16 channels [hi(C) | lo(C) | hi(C)].  With the packed
// weight laid out [wh | wh | wl] along K, the three products are ONE implicit GEMM over 3*C input
// channels: the conv main loops (LDS-DMA fills, fragment reads, MFMA issue) are the bf16 kernels,
// unchanged; only the epilogue (conv_fast.hip, X3) and the element-wise kernels below know the format.
#include "common.h"

// 8 consecutive channels [c, c+8) of pixel `pix` as f32 (hi + lo)
__device__ __forceinline__ Vec8 x3_load(const unsigned short* __restrict__ base, long pix, int C, int c) {
  const unsigned short* p = base + pix * (3L * C) + c;
  Vec8 h = load8<unsigned short>(p), l = load8<unsigned short>(p + C);
#pragma unroll
  for (int j = 0; j < 8; j++) h.v[j] += l.v[j];
  return h;
}
// hi = bf16(v), lo = bf16(v - hi), hi again.  v = +-inf, and a finite |v| >= 2^128 - 2^119 (0x7F7F8000 up, FLT_MAX among
// them: it rounds to the bf16 infinity), give an infinite hi: lo is 0 there (x3_lo, common.h), so the pair reads back as
// the infinity the f32 path keeps.  A NaN stays a NaN in all three planes.  hi + lo carries 16 significant bits of a
// normal v; an f32 subnormal v (and a lo below 2^-126) goes through the device's bf16 conversion like any other store.
__device__ __forceinline__ void x3_store(unsigned short* __restrict__ base, long pix, int C, int c, const Vec8& v) {
  unsigned short* p = base + pix * (3L * C) + c;
  Vec8 h = round8<unsigned short>(v), l;
#pragma unroll
  for (int j = 0; j < 8; j++) l.v[j] = x3_lo(v.v[j], h.v[j]);
  store8<unsigned short>(p, h);
  store8<unsigned short>(p + C, l);
  store8<unsigned short>(p + 2 * C, h);
}

static inline int x3_grid(long n8) {
  long b = (n8 + 255) / 256;
  return (int)(b < 2048 ? b : 2048);
}

struct C8 {
  float v[8];
};
__device__ __forceinline__ C8 x3_coef(const float* p, int c, float dflt) {
  C8 r;
#pragma unroll
  for (int j = 0; j < 8; j++) r.v[j] = p ? p[c + j] : dflt;
  return r;
}

// y = prelu(x * scale + shift [+ residual]) [+ residual]   (msml_bn_act_fwd on split tensors)
__global__ void __launch_bounds__(256) k_x3_bn_act_fwd(const unsigned short* __restrict__ x,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const float* __restrict__ alpha,
                                                       const unsigned short* __restrict__ residual, int res_first,
                                                       unsigned short* __restrict__ y, long M, int C) {
  const int C8n = C / 8;
  const long n8 = M * C8n;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const long pix = i / C8n;
    const int c = (int)(i - pix * C8n) * 8;
    const C8 sc = x3_coef(scale, c, 1.f), sh = x3_coef(shift, c, 0.f), al = x3_coef(alpha, c, 1.f);
    Vec8 v = x3_load(x, pix, C, c), r;
    if (residual) r = x3_load(residual, pix, C, c);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float z = v.v[j] * sc.v[j] + sh.v[j];
      if (residual && res_first) z += r.v[j];
      if (alpha) z = z > 0.f ? z : z * al.v[j];
      if (residual && !res_first) z += r.v[j];
      v.v[j] = z;
    }
    x3_store(y, pix, C, c, v);
  }
}

__device__ __forceinline__ float x3_act(float x, int act) {
  if (act == MSML_ACT_SIGMOID) return 1.f / (1.f + __expf(-x));
  return tanhf(x);
}

// z = arith(yf, act(x)) + yf   (msml_fm_fuse_fwd on split tensors)
__global__ void __launch_bounds__(256) k_x3_fm_fwd(const unsigned short* __restrict__ x,
                                                   const unsigned short* __restrict__ yf,
                                                   unsigned short* __restrict__ z, long M, int C, int act, int arith) {
  const int C8n = C / 8;
  const long n8 = M * C8n;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const long pix = i / C8n;
    const int c = (int)(i - pix * C8n) * 8;
    Vec8 a = x3_load(x, pix, C, c), f = x3_load(yf, pix, C, c), o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float m = x3_act(a.v[j], act), yv = f.v[j];
      float r;
      if (arith == MSML_ARITH_ADD) r = yv + m;
      else if (arith == MSML_ARITH_SUB) r = yv - m;
      else if (arith == MSML_ARITH_MUL) r = yv * m;
      else r = yv / m;
      o.v[j] = r + yv;
    }
    x3_store(z, pix, C, c, o);
  }
}

__global__ void __launch_bounds__(256) k_x3_add(const unsigned short* __restrict__ a, const unsigned short* __restrict__ b,
                                                unsigned short* __restrict__ out, long M, int C) {
  const int C8n = C / 8;
  const long n8 = M * C8n;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const long pix = i / C8n;
    const int c = (int)(i - pix * C8n) * 8;
    Vec8 u = x3_load(a, pix, C, c), v = x3_load(b, pix, C, c);
#pragma unroll
    for (int j = 0; j < 8; j++) u.v[j] += v.v[j];
    x3_store(out, pix, C, c, u);
  }
}

__global__ void __launch_bounds__(256) k_x3_from_f32(const float* __restrict__ src, unsigned short* __restrict__ dst,
                                                     long M, int C) {
  const int C8n = C / 8;
  const long n8 = M * C8n;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const long pix = i / C8n;
    const int c = (int)(i - pix * C8n) * 8;
    x3_store(dst, pix, C, c, load8<float>(src + pix * C + c));
  }
}

__global__ void __launch_bounds__(256) k_x3_to_f32(const unsigned short* __restrict__ src, float* __restrict__ dst,
                                                   long M, int C) {
  const int C8n = C / 8;
  const long n8 = M * C8n;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const long pix = i / C8n;
    const int c = (int)(i - pix * C8n) * 8;
    store8<float>(dst + pix * C + c, x3_load(src, pix, C, c));
  }
}

#define X3_SHAPE(name)                                                                         \
  MSML_CHECK(M > 0 && C > 0 && C % 8 == 0, MSML_ERR_SHAPE, name ": bad shape M=%ld C=%d", M, C)

extern "C" int msml_x3_bn_act_fwd(const void* x, const float* scale, const float* shift, const float* alpha,
                                  const void* residual, int res_first, void* y, long M, int C, void* stream) {
  X3_SHAPE("x3_bn_act_fwd");
  MSML_CHECK(x && y, MSML_ERR_SHAPE, "x3_bn_act_fwd: null pointer");
  k_x3_bn_act_fwd<<<x3_grid(M * (C / 8)), 256, 0, (hipStream_t)stream>>>(
      (const unsigned short*)x, scale, shift, alpha, (const unsigned short*)residual, res_first, (unsigned short*)y, M, C);
  MSML_LAUNCH_OK("x3_bn_act_fwd");
  return MSML_OK;
}

extern "C" int msml_x3_fm_fuse_fwd(const void* x, const void* yf, void* z, long M, int C, int act, int arith,
                                   void* stream) {
  X3_SHAPE("x3_fm_fuse_fwd");
  MSML_CHECK(x && yf && z, MSML_ERR_SHAPE, "x3_fm_fuse_fwd: null pointer");
  MSML_CHECK(act >= 0 && act <= 1 && arith >= 0 && arith <= 3, MSML_ERR_UNSUPPORTED, "x3_fm_fuse_fwd: act=%d arith=%d",
             act, arith);
  k_x3_fm_fwd<<<x3_grid(M * (C / 8)), 256, 0, (hipStream_t)stream>>>(
      (const unsigned short*)x, (const unsigned short*)yf, (unsigned short*)z, M, C, act, arith);
  MSML_LAUNCH_OK("x3_fm_fuse_fwd");
  return MSML_OK;
}

extern "C" int msml_x3_add(const void* a, const void* b, void* out, long M, int C, void* stream) {
  X3_SHAPE("x3_add");
  MSML_CHECK(a && b && out, MSML_ERR_SHAPE, "x3_add: null pointer");
  k_x3_add<<<x3_grid(M * (C / 8)), 256, 0, (hipStream_t)stream>>>((const unsigned short*)a, (const unsigned short*)b,
                                                                  (unsigned short*)out, M, C);
  MSML_LAUNCH_OK("x3_add");
  return MSML_OK;
}

extern "C" int msml_x3_from_f32(const float* src, void* dst, long M, int C, void* stream) {
  X3_SHAPE("x3_from_f32");
  MSML_CHECK(src && dst, MSML_ERR_SHAPE, "x3_from_f32: null pointer");
  k_x3_from_f32<<<x3_grid(M * (C / 8)), 256, 0, (hipStream_t)stream>>>(src, (unsigned short*)dst, M, C);
  MSML_LAUNCH_OK("x3_from_f32");
  return MSML_OK;
}

extern "C" int msml_x3_to_f32(const void* src, float* dst, long M, int C, void* stream) {
  X3_SHAPE("x3_to_f32");
  MSML_CHECK(src && dst, MSML_ERR_SHAPE, "x3_to_f32: null pointer");
  k_x3_to_f32<<<x3_grid(M * (C / 8)), 256, 0, (hipStream_t)stream>>>((const unsigned short*)src, dst, M, C);
  MSML_LAUNCH_OK("x3_to_f32");
  return MSML_OK;
}
