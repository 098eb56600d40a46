// Progressive JPEG decoding on the device: the entropy pass of msml_jpeg_decode_scans (jpeg.hip holds the entry point
// and the two passes behind the coefficients, which a progressive image shares with a baseline one).  The arithmetic is
// csrc/jpeg_prog_core.h, shared with the host check; tests/jpeg_prog_cases.py restates it.
//   k_jpeg_entropy<true>  the baseline images of the batch, as msml_jpeg_decode walks them
//   k_jpeg_prog           one wavefront per progressive image: its scans in file order, lane k owning coefficient k
// Both are launched over all N images and each leaves the other's at once.  No atomics, one writer per byte.
#include "jpeg_entropy_kernel.h"

// The current block of a progressive scan: lane k keeps coefficient k (zigzag order), loaded from and stored to the
// block's 128-byte row at its natural index.  The nonzero-history mask of a refinement scan is one ballot; a lane
// finds the correction bit that is its own by its rank in the mask.
struct JpgProgBlk {
  int16_t* coef;
  int lane, nat;
  int c;
  __device__ void dc_store(long blk, int v) {
    if (lane == 0) coef[blk * 64] = (int16_t)v;
  }
  __device__ void dc_or(long blk, int bit) {
    if (lane == 0) coef[blk * 64] = (int16_t)(coef[blk * 64] | bit);
  }
  __device__ void clear() { c = 0; }
  __device__ void put(int k, int v) {
    if (lane == k) c = v;
  }
  __device__ void load(long blk) { c = coef[blk * 64 + nat]; }
  __device__ void store(long blk, int ss, int se) {
    if (lane >= ss && lane <= se) coef[blk * 64 + nat] = (int16_t)c;
  }
  __device__ uint64_t nonzero(int ss, int se) { return __ballot(c != 0 && lane >= ss && lane <= se); }
  __device__ void correct(uint64_t m, int base, int bits, int cnt, int p1) {
    const int rank = __popcll(m & ((1ull << lane) - 1)) - base;
    if (((m >> lane) & 1) && rank >= 0 && rank < cnt && ((bits >> (cnt - 1 - rank)) & 1) && (c & p1) == 0)
      c = (int)(int16_t)(c + (c >= 0 ? p1 : -p1));
  }
};

// One wavefront per progressive image, its scans in file order.  Leaves baseline and refused images at once
// (k_jpeg_entropy writes their statuses).  The coefficient area is zeroed first: a band no block of a scan reaches,
// and the AC of the blocks that only pad the plane to whole MCUs, are read by k_jpeg_idct as they are left here.
__global__ void __launch_bounds__(64) k_jpeg_prog(const unsigned char* __restrict__ streams, const int* __restrict__ desc,
                                                  const int* __restrict__ scans, const int* __restrict__ huff,
                                                  unsigned char* __restrict__ ws, int* __restrict__ status) {
  __shared__ int s_tab[3 * JPG_HUFF_WORDS];                  // this scan's tables: three DC or one AC
  __shared__ unsigned int s_win[IMG_CHUNK / 4];
  const int n = blockIdx.x;
  const int* d = desc + (long)n * JPG_DESC_WORDS;
  if (d[JD_STATUS] != 0 || d[JD_NSCAN] <= 0) return;
  JpgLayout L;
  jpg_layout(d, L);
  unsigned char* base = ws + (long)d[JD_WS] * JPG_WS_ALIGN;
  uint4* z = reinterpret_cast<uint4*>(base);
  for (long i = threadIdx.x; i < L.nblk * 8; i += 64) z[i] = make_uint4(0u, 0u, 0u, 0u);
  JpgProgBlk blk;
  blk.coef = reinterpret_cast<int16_t*>(base);
  blk.lane = threadIdx.x;
  blk.nat = img_zigzag(threadIdx.x);
  blk.c = 0;
  LdsStreamSrc src = {streams + (long)d[JD_BASE] * 4, s_win, -IMG_CHUNK, d[JD_END], (int)threadIdx.x};
  const int* tab[3];
  for (int c = 0; c < 3; ++c) tab[c] = s_tab + c * JPG_HUFF_WORDS;
  const int nscan = d[JD_NSCAN];
  int st = JPG_OK;
  for (int i = 0; i < nscan && st == JPG_OK; ++i) {
    const int* s = scans + (long)(d[JD_SCAN0] + i) * JPG_SCAN_WORDS;
    __syncthreads();                                         // the scan before: its stores are out, its tables read
    const int nt = s[JS_NCOMP];
    for (int c = 0; c < 3; ++c) {
      if (c < nt) {
        const int* g = huff + (long)s[JS_TAB + c] * JPG_HUFF_WORDS;
        for (int k = threadIdx.x; k < JPG_HUFF_WORDS; k += 64) s_tab[c * JPG_HUFF_WORDS + k] = g[k];
      }
    }
    __syncthreads();
    st = jpg_prog_scan(d, L, s, src, tab, blk);
  }
  if (threadIdx.x == 0) status[n] = st;
}

// The entropy pass of a batch with a scan table, called by msml_jpeg_decode_scans after its host checks.  progressive:
// how many images have scans (0: k_jpeg_prog is not launched).
int jpeg_prog_entropy(const unsigned char* streams, const int* desc, const int* scans, const int* htabs,
                      unsigned char* ws, int* status, int N, int progressive, hipStream_t stream) {
  k_jpeg_entropy<true><<<N, 64, 0, stream>>>(streams, desc, htabs, ws, status);
  MSML_LAUNCH_OK("jpeg_entropy");
  if (progressive) {
    k_jpeg_prog<<<N, 64, 0, stream>>>(streams, desc, scans, htabs, ws, status);
    MSML_LAUNCH_OK("jpeg_prog");
  }
  return MSML_OK;
}
