// LightCNN-29v2 FRB element-wise kernels (reference: backbones/frb/lightcnn.py).
//
//   msml_mfm_bwd    backward of the max-feature-map (lightcnn.py:36-39, torch.max(a, b)): routes dY of the C output
//                   channels to the 2C filter channels through the selector msml_conv2d_mfm wrote (conv_igemm.hip)
//   msml_pool2_*    F.max_pool2d(x, 2) + F.avg_pool2d(x, 2) (lightcnn.py:211,216,221,228) and its backward
//
// All NHWC, f32 or bf16 storage, f32 arithmetic; one thread per (pixel, 8-channel chunk): 16-B (bf16) / 32-B (f32)
// accesses along the channel dimension.
#include "common.h"

// dz[m][k], k < czp: the gradient of filter channel k = dy[m][k mod C] if its half won (sel 1 for k < C, 2 for k >= C),
// half of it on a tie (sel 0), all of it when the pair is unordered (sel 3: torch.max passes a NaN's gradient to both
// inputs); pad channels k >= 2C are zero.
template <typename T>
__global__ void __launch_bounds__(256) k_mfm_bwd(const T* __restrict__ dy, const unsigned char* __restrict__ sel,
                                                 T* __restrict__ dz, long M, int cp, int C, int czp) {
  const int K8 = czp / 8;
  const long total = M * K8;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / K8;
    const int k0 = (int)(i - m * K8) * 8;
    const T* dyr = dy + m * cp;
    const unsigned char* sr = sel + m * cp;
    Vec8 v;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int k = k0 + j;
      float g = 0.f;
      if (k < 2 * C) {
        const int second = k >= C;
        const int c = second ? k - C : k;
        const unsigned s = sr[c];
        const float d = load1<T>(dyr + c);
        g = (s == 3u || s == (second ? 2u : 1u)) ? d : (s == 0u ? 0.5f * d : 0.f);
      }
      v.v[j] = g;
    }
    store8<T>(dz + m * czp + k0, v);
  }
}

extern "C" int msml_mfm_bwd(const void* dy, const unsigned char* sel, void* dz, long M, int cp, int C, int czp,
                            int dtype, void* stream) {
  MSML_CHECK(dy && sel && dz, MSML_ERR_SHAPE, "mfm_bwd: null pointer");
  MSML_CHECK(M > 0 && C > 0 && cp >= C && czp >= 2 * C && czp % 8 == 0, MSML_ERR_SHAPE,
             "mfm_bwd: bad sizes M=%ld cp=%d C=%d czp=%d", M, cp, C, czp);
  const long total = M * (czp / 8);
  const int grid = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  MSML_DISPATCH_DTYPE(dtype, "mfm_bwd",
                      k_mfm_bwd<DT><<<grid, 256, 0, (hipStream_t)stream>>>((const DT*)dy, sel, (DT*)dz, M, cp, C, czp);)
  MSML_LAUNCH_OK("mfm_bwd");
  return MSML_OK;
}

// torch's max_pool2d update rule, in window order (0,0) (0,1) (1,0) (1,1): take v if v > max or v is NaN -- ties keep the
// first maximum, a NaN wins.
__device__ __forceinline__ bool pool_takes(float v, float m) { return v > m || v != v; }

template <typename T>
__global__ void __launch_bounds__(256) k_pool2_fwd(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W,
                                                   int cp) {
  const int P = H / 2, Q = W / 2, K8 = cp / 8;
  const long total = (long)N * P * Q * K8;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int k0 = (int)(i % K8) * 8;
    const long pix = i / K8;
    const int ox = (int)(pix % Q);
    const long t = pix / Q;
    const int oy = (int)(t % P), n = (int)(t / P);
    const T* x00 = x + (((long)n * H + 2 * oy) * W + 2 * ox) * cp + k0;
    const Vec8 a = load8<T>(x00), b = load8<T>(x00 + cp), c = load8<T>(x00 + (long)W * cp),
               d = load8<T>(x00 + (long)W * cp + cp);
    Vec8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float m = a.v[j];
      if (pool_takes(b.v[j], m)) m = b.v[j];
      if (pool_takes(c.v[j], m)) m = c.v[j];
      if (pool_takes(d.v[j], m)) m = d.v[j];
      o.v[j] = m + ((a.v[j] + b.v[j]) + c.v[j] + d.v[j]) * 0.25f;
    }
    store8<T>(y + pix * cp + k0, o);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) k_pool2_bwd(const T* __restrict__ dy, const T* __restrict__ x, T* __restrict__ dx,
                                                   int N, int H, int W, int cp) {
  const int P = H / 2, Q = W / 2, K8 = cp / 8;
  const long total = (long)N * P * Q * K8;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int k0 = (int)(i % K8) * 8;
    const long pix = i / K8;
    const int ox = (int)(pix % Q);
    const long t = pix / Q;
    const int oy = (int)(t % P), n = (int)(t / P);
    const long o00 = (((long)n * H + 2 * oy) * W + 2 * ox) * cp + k0;
    const long off[4] = {o00, o00 + cp, o00 + (long)W * cp, o00 + (long)W * cp + cp};
    Vec8 v[4];
#pragma unroll
    for (int w = 0; w < 4; w++) v[w] = load8<T>(x + off[w]);
    const Vec8 g = load8<T>(dy + pix * cp + k0);
    int arg[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float m = v[0].v[j];
      int a = 0;
#pragma unroll
      for (int w = 1; w < 4; w++)
        if (pool_takes(v[w].v[j], m)) { m = v[w].v[j]; a = w; }
      arg[j] = a;
    }
#pragma unroll
    for (int w = 0; w < 4; w++) {
      Vec8 o;
#pragma unroll
      for (int j = 0; j < 8; j++) o.v[j] = (arg[j] == w ? g.v[j] : 0.f) + 0.25f * g.v[j];
      store8<T>(dx + off[w], o);
    }
  }
}

static int pool_check(const void* a, const void* b, const void* c, int N, int H, int W, int cp, const char* name) {
  MSML_CHECK(a && b && c, MSML_ERR_SHAPE, "%s: null pointer", name);
  MSML_CHECK(N > 0 && H >= 2 && W >= 2 && (H & 1) == 0 && (W & 1) == 0 && cp > 0 && cp % 8 == 0, MSML_ERR_SHAPE,
             "%s: bad dims N=%d H=%d W=%d cp=%d (H, W even, cp a multiple of 8)", name, N, H, W, cp);
  return MSML_OK;
}

extern "C" int msml_pool2_fwd(const void* x, void* y, int N, int H, int W, int cp, int dtype, void* stream) {
  const int rc = pool_check(x, y, y, N, H, W, cp, "pool2_fwd");
  if (rc != MSML_OK) return rc;
  const long total = (long)N * (H / 2) * (W / 2) * (cp / 8);
  const int grid = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  MSML_DISPATCH_DTYPE(dtype, "pool2_fwd",
                      k_pool2_fwd<DT><<<grid, 256, 0, (hipStream_t)stream>>>((const DT*)x, (DT*)y, N, H, W, cp);)
  MSML_LAUNCH_OK("pool2_fwd");
  return MSML_OK;
}

extern "C" int msml_pool2_bwd(const void* dy, const void* x, void* dx, int N, int H, int W, int cp, int dtype,
                              void* stream) {
  const int rc = pool_check(dy, x, dx, N, H, W, cp, "pool2_bwd");
  if (rc != MSML_OK) return rc;
  const long total = (long)N * (H / 2) * (W / 2) * (cp / 8);
  const int grid = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  MSML_DISPATCH_DTYPE(dtype, "pool2_bwd",
                      k_pool2_bwd<DT><<<grid, 256, 0, (hipStream_t)stream>>>((const DT*)dy, (const DT*)x, (DT*)dx, N, H,
                                                                             W, cp);)
  MSML_LAUNCH_OK("pool2_bwd");
  return MSML_OK;
}
