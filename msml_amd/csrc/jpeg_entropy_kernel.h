// k_jpeg_entropy, the baseline entropy pass, for the two translation units that launch it: jpeg.hip (SCANS = false,
// every call of msml_jpeg_decode) and jpeg_prog.hip (SCANS = true, a batch that may hold progressive images).  Each
// unit instantiates one form only, so the baseline form is compiled as it always was: with the progressive code in
// the same unit the shared bit-reader functions gain callers, are inlined differently, and the baseline walk measured
// 2.7 % slower.
#ifndef MSML_JPEG_ENTROPY_KERNEL_H
#define MSML_JPEG_ENTROPY_KERNEL_H
#include "common.h"
#include "jpeg_prog_core.h"

// lane k keeps the k-th coefficient (zigzag order) of the current block and stores it at its natural index
struct JpgWaveSink {
  int16_t* coef;
  int lane, nat;
  int c;
  __device__ void begin() { c = 0; }
  __device__ void put(int k, int v) {
    if (lane == k) c = v;
  }
  __device__ void end(long blk) { coef[blk * 64 + nat] = (int16_t)c; }
};

// SCANS: progressive images are k_jpeg_prog's and are left at once.  Without it descriptor word 22 is not read.
template <bool SCANS>
__global__ void __launch_bounds__(64) k_jpeg_entropy(const unsigned char* __restrict__ streams,
                                                     const int* __restrict__ desc, const int* __restrict__ huff,
                                                     unsigned char* __restrict__ ws, int* __restrict__ status) {
  __shared__ int s_tab[6 * JPG_HUFF_WORDS];                  // the DC and AC table of each component
  __shared__ unsigned int s_win[IMG_CHUNK / 4];
  const int n = blockIdx.x;
  const int* d = desc + (long)n * JPG_DESC_WORDS;
  if (SCANS && d[JD_STATUS] == 0 && d[JD_NSCAN] > 0) return;  // a progressive image
  int st = d[JD_STATUS];
  if (st == 0) {
    const int nc = d[JD_NCOMP];
    const int* dctab[3];
    const int* actab[3];
    for (int c = 0; c < 3; ++c) {
      dctab[c] = s_tab + (2 * c) * JPG_HUFF_WORDS;
      actab[c] = s_tab + (2 * c + 1) * JPG_HUFF_WORDS;
      if (c < nc) {
        const int* gd = huff + (long)d[JD_DC + c] * JPG_HUFF_WORDS;
        const int* ga = huff + (long)d[JD_AC + c] * JPG_HUFF_WORDS;
        for (int k = threadIdx.x; k < JPG_HUFF_WORDS; k += 64) {
          s_tab[(2 * c) * JPG_HUFF_WORDS + k] = gd[k];
          s_tab[(2 * c + 1) * JPG_HUFF_WORDS + k] = ga[k];
        }
      }
    }
    __syncthreads();
    JpgWaveSink sink;
    sink.coef = reinterpret_cast<int16_t*>(ws + (long)d[JD_WS] * JPG_WS_ALIGN);
    sink.lane = threadIdx.x;
    sink.nat = img_zigzag(threadIdx.x);
    sink.c = 0;
    LdsStreamSrc src = {streams + (long)d[JD_BASE] * 4, s_win, -IMG_CHUNK, d[JD_END], (int)threadIdx.x};
    st = jpg_entropy(d, src, dctab, actab, sink);
  }
  if (threadIdx.x == 0) status[n] = st;
}
#endif
