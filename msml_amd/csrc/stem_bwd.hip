// Backward-data of the stem convs, straight to the image: the adjoint of msml_stem_im2col + the 1x1 conv over the patches
// (layout.hip; iresnet.py:209 `conv1`, unet.py:193, lightcnn.py:150) in ONE launch.
//
//   dx[n][c][iy][ix] = sum over k, r, s of dy[n][oy][ox][k] * w[k][c][r][s],   iy = oy*stride - pad + r, ix = ox*stride - pad + s
//
// dy is the NHWC gradient of the stem's output ([N][P][Q][ldy], the first Cout channels real: no other channel is read),
// w the parameter's own f32 OIHW memory, dx the dense NCHW f32 image gradient; every element of dx is stored, so there is
// nothing to zero beforehand and no accumulate mode.
//
// bf16 dy (k_stem_bwd_data): a workgroup owns a band of B input rows of one image and the ND output rows whose taps reach
// the band.  Those rows are one contiguous run of pixels in NHWC; the eight waves take 32-pixel tiles of it:
//   MFMA 32x32x16, M = 32 pixels of dy (each lane loads its pixel's 16 B of channels straight from memory: the A operand
//   of lane (pixel, half) IS 8 consecutive channels), K = the Cout channels, N = the R*S*C (tap, c) columns padded to 32
//   (the filter, rounded to bf16 and transposed to [column][channel] in LDS, staged once per workgroup).
// The f32 accumulators -- the patch gradient of the im2col formulation, which never reaches memory -- go to an LDS tile
// [pixel][PITCH] (PITCH = R*S*C made odd: the fold below walks pixels at one column, stride PITCH dwords, conflict-free),
// and after one barrier every thread folds (col2im) the taps of the dx elements it owns IN A FIXED ORDER and stores them
// coalesced along ix: no atomics, one writer per element, two runs give the same bits.  The price of the band is that a
// dy row whose taps reach two bands is read by both: (B + R - 1) / B of the bytes at stride 1; B is the largest band whose
// tile leaves room for two workgroups per CU, or for one where that band would be shorter than the filter.
//
// f32 dy (k_stem_bwd_data_f32, the LightCNN f32 mode: not a hot path): one thread per dx element gathers its taps with f32
// FMAs, the filter unrounded in LDS.
#include <mutex>

#include "common.h"

namespace {

constexpr int SB_THREADS = 512, SB_MAX_BAND = 16;
constexpr size_t SB_LDS_TWO = 78 * 1024, SB_LDS_ONE = 156 * 1024;       // two workgroups / one workgroup per CU

template <int C, int R, int STRIDE>
__global__ void __launch_bounds__(SB_THREADS) k_stem_bwd_data(const unsigned short* __restrict__ dy, const float* __restrict__ w,
                                                              float* __restrict__ dx, int H, int W, int P, int Q, int Cout,
                                                              int ldy, int B, int ND) {
  constexpr int S = R, PAD = R / 2, RSC = R * S * C, PITCH = RSC | 1;
  extern __shared__ __align__(16) unsigned char sb_lds[];
  const int WP = Cout + 8;                                   // filter row pitch (bf16 elements): rows stay 16-B aligned
  unsigned short* wB = reinterpret_cast<unsigned short*>(sb_lds);
  float* pt = reinterpret_cast<float*>(sb_lds + (size_t)32 * WP * 2);
  MSML_LDS_REGION(wB, (size_t)32 * WP * 2);
  MSML_LDS_REGION(pt, (size_t)ND * Q * PITCH * 4);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nbands = (H + B - 1) / B;
  const int n = blockIdx.x / nbands, iy0 = (blockIdx.x % nbands) * B;
  const int nb = min(B, H - iy0);
  // output rows with a tap inside the band: oy*STRIDE - PAD + r in [iy0, iy0 + nb) for some r in [0, R)
  const int lo_num = iy0 + PAD - (R - 1);
  const int oy_lo = lo_num <= 0 ? 0 : (lo_num + STRIDE - 1) / STRIDE;
  const int oy_hi = min(P - 1, (iy0 + nb - 1 + PAD) / STRIDE);
  const int nd = min(max(oy_hi - oy_lo + 1, 0), ND);

  // the filter as the B operand: wB[column = (r*S + s)*C + c][channel k], zero columns above R*S*C
  for (int i = t; i < 32 * Cout; i += SB_THREADS) {
    const int col = i / Cout, k = i - col * Cout;
    const int tap = col / C, c = col - tap * C, r = tap / S, s = tap - r * S;
    wB[col * WP + k] = col < RSC ? f2bf(w[((k * C + c) * R + r) * S + s]) : (unsigned short)0;
  }
  __syncthreads();

  const int npix = nd * Q, nks = Cout >> 4;
  const int r32 = lane & 31, h = lane >> 5;
  const unsigned short* dyb = dy + ((long)n * P + oy_lo) * Q * ldy;
  for (int tile = wave; tile * 32 < npix; tile += SB_THREADS / 64) {
    const int pix = tile * 32 + r32;
    const unsigned short* src = dyb + (long)pix * ldy + 8 * h;
    u32x4 a[8];
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
      a[ks] = u32x4{0u, 0u, 0u, 0u};
      if (ks < nks && pix < npix) a[ks] = *reinterpret_cast<const u32x4*>(src + ks * 16);
    }
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ks++)
      if (ks < nks) {
        const u32x4 b = *reinterpret_cast<const u32x4*>(wB + r32 * WP + ks * 16 + 8 * h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[ks]), __builtin_bit_cast(bf16x8, b), acc,
                                                      0, 0, 0);
      }
    // D: column (tap, c) = lane & 31, pixel row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int p = tile * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (r32 < RSC && p < npix) pt[p * PITCH + r32] = acc[reg];
    }
  }
  __syncthreads();

  // col2im: each dx element of the band sums its taps from the tile, r then s ascending
  const int elems = C * nb * W;
  for (int i = t; i < elems; i += SB_THREADS) {
    const int c = i / (nb * W), rem = i - c * (nb * W), row = rem / W, ix = rem - row * W;
    const int iy = iy0 + row;
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int ty = iy + PAD - r;
      if (ty < 0 || ty % STRIDE != 0) continue;
      const int orow = ty / STRIDE - oy_lo;
      if (orow < 0 || orow >= nd) continue;
#pragma unroll
      for (int s = 0; s < S; s++) {
        const int tx = ix + PAD - s;
        if (tx < 0 || tx % STRIDE != 0 || tx / STRIDE >= Q) continue;
        sum += pt[(orow * Q + tx / STRIDE) * PITCH + (r * S + s) * C + c];
      }
    }
    dx[(((long)n * C + c) * H + iy) * W + ix] = sum;
  }
}

__global__ void __launch_bounds__(256) k_stem_bwd_data_f32(const float* __restrict__ dy, const float* __restrict__ w,
                                                           float* __restrict__ dx, int N, int C, int H, int W, int P, int Q,
                                                           int Cout, int ldy, int R, int stride, int pad) {
  __shared__ __align__(16) float wl[32 * 128];               // [column (r*S + s)*C + c][channel k]
  const int RSC = R * R * C;
  for (int i = threadIdx.x; i < RSC * Cout; i += 256) {
    const int col = i / Cout, k = i - col * Cout;
    const int tap = col / C, c = col - tap * C, r = tap / R, s = tap - r * R;
    wl[i] = w[((k * C + c) * R + r) * R + s];
  }
  __syncthreads();
  const long total = (long)N * C * H * W;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int ix = (int)(i % W);
    long u = i / W;
    const int iy = (int)(u % H);
    u /= H;
    const int c = (int)(u % C), n = (int)(u / C);
    float sum = 0.f;
    for (int r = 0; r < R; r++) {
      const int ty = iy + pad - r;
      if (ty < 0 || ty % stride != 0 || ty / stride >= P) continue;
      for (int s = 0; s < R; s++) {
        const int tx = ix + pad - s;
        if (tx < 0 || tx % stride != 0 || tx / stride >= Q) continue;
        const float* d = dy + (((long)n * P + ty / stride) * Q + tx / stride) * ldy;
        const float* wv = wl + ((r * R + s) * C + c) * Cout;
        f32x4 part = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < Cout; k += 4)
          part += *reinterpret_cast<const f32x4*>(d + k) * *reinterpret_cast<const f32x4*>(wv + k);
        sum += (part[0] + part[1]) + (part[2] + part[3]);
      }
    }
    dx[i] = sum;
  }
}

// the shapes the stems have (the conditions of the stems' im2col path)
bool sb_served(int C, int H, int W, int P, int Q, int Cout, int ldy, int R, int S, int stride, int pad) {
  if (!((C == 1 || C == 3) && R == S && (R == 3 || R == 5) && R * S * C <= 32)) return false;
  if (!((stride == 1 || stride == 2) && pad == R / 2)) return false;
  if (!(Cout >= 32 && Cout <= 128 && Cout % 32 == 0 && ldy >= Cout && ldy % 8 == 0)) return false;
  if (!(H >= 1 && W >= 1 && W <= 128 && H <= 32767)) return false;
  return P == (H + 2 * pad - R) / stride + 1 && Q == (W + 2 * pad - S) / stride + 1 && P >= 1 && Q >= 1;
}

// band height and dy rows of the bf16 kernel for a served shape
void sb_band(int C, int H, int Q, int Cout, int R, int stride, int* band, int* nd, size_t* lds) {
  const size_t wbytes = (size_t)32 * (Cout + 8) * 2, row = (size_t)Q * ((R * R * C) | 1) * 4;
  int b = 0;
  for (size_t budget : {SB_LDS_TWO, SB_LDS_ONE}) {
    const long ndmax = (long)((budget - wbytes) / row);
    b = (int)(ndmax * stride - R + 1 < SB_MAX_BAND ? ndmax * stride - R + 1 : SB_MAX_BAND);
    if (b >= R || b >= H) break;
  }
  if (b > H) b = H;
  *band = b;
  *nd = (b + R - 2) / stride + 1;
  *lds = wbytes + (size_t)*nd * row;
}

template <int C, int R, int STRIDE>
void sb_launch(const unsigned short* dy, const float* w, float* dx, int N, int H, int W, int P, int Q, int Cout, int ldy,
               hipStream_t st) {
  int band, nd;
  size_t lds;
  sb_band(C, H, Q, Cout, R, STRIDE, &band, &nd, &lds);
  static std::once_flag attr_once;
  std::call_once(attr_once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_stem_bwd_data<C, R, STRIDE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)SB_LDS_ONE);
  });
  const int grid = N * ((H + band - 1) / band);
  k_stem_bwd_data<C, R, STRIDE><<<grid, SB_THREADS, lds, st>>>(dy, w, dx, H, W, P, Q, Cout, ldy, band, nd);
}

}  // namespace

extern "C" int msml_stem_bwd_data_band(int C, int H, int W, int Cout, int R, int stride) {
  const int pad = R / 2;
  const int P = (H + 2 * pad - R) / stride + 1, Q = (W + 2 * pad - R) / stride + 1;
  if (stride < 1 || !sb_served(C, H, W, P, Q, Cout, Cout, R, R, stride, pad)) return 0;
  int band, nd;
  size_t lds;
  sb_band(C, H, Q, Cout, R, stride, &band, &nd, &lds);
  return band;
}

extern "C" int msml_stem_bwd_data(const void* dy, const float* w, float* dx, int N, int C, int H, int W, int P, int Q,
                                  int Cout, int ldy, int R, int S, int stride, int pad, int dtype, void* stream) {
  MSML_CHECK(dy && w && dx, MSML_ERR_SHAPE, "stem_bwd_data: null pointer");
  MSML_CHECK(((uintptr_t)dy & 15) == 0 && ((uintptr_t)w & 3) == 0 && ((uintptr_t)dx & 3) == 0, MSML_ERR_SHAPE,
             "stem_bwd_data: misaligned pointer (dy 16 bytes, w and dx 4)");
  MSML_CHECK(N >= 1 && (long)N * H <= 0x7fffffffL / 16 && stride >= 1 &&
                 sb_served(C, H, W, P, Q, Cout, ldy, R, S, stride, pad),
             MSML_ERR_SHAPE,
             "stem_bwd_data: serves C in {1, 3}, R = S in {3, 5} with R*S*C <= 32, stride 1 or 2, pad = R/2, Cout a multiple "
             "of 32 up to 128 (ldy >= Cout, ldy %% 8 == 0), W <= 128 and P, Q of that conv; got N %d C %d H %d W %d P %d Q %d "
             "Cout %d ldy %d R %d S %d stride %d pad %d",
             N, C, H, W, P, Q, Cout, ldy, R, S, stride, pad);
  MSML_CHECK(dtype == MSML_F32 || dtype == MSML_BF16, MSML_ERR_DTYPE, "stem_bwd_data: unsupported dtype %d", dtype);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MSML_F32) {
    const long total = (long)N * C * H * W;
    const int grid = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    k_stem_bwd_data_f32<<<grid, 256, 0, st>>>((const float*)dy, w, dx, N, C, H, W, P, Q, Cout, ldy, R, stride, pad);
  } else {
    const unsigned short* d = (const unsigned short*)dy;
    if (C == 3 && stride == 1) sb_launch<3, 3, 1>(d, w, dx, N, H, W, P, Q, Cout, ldy, st);
    else if (C == 3) sb_launch<3, 3, 2>(d, w, dx, N, H, W, P, Q, Cout, ldy, st);
    else if (R == 3 && stride == 1) sb_launch<1, 3, 1>(d, w, dx, N, H, W, P, Q, Cout, ldy, st);
    else if (R == 3) sb_launch<1, 3, 2>(d, w, dx, N, H, W, P, Q, Cout, ldy, st);
    else if (stride == 1) sb_launch<1, 5, 1>(d, w, dx, N, H, W, P, Q, Cout, ldy, st);
    else sb_launch<1, 5, 2>(d, w, dx, N, H, W, P, Q, Cout, ldy, st);
  }
  MSML_LAUNCH_OK("stem_bwd_data");
  return MSML_OK;
}
