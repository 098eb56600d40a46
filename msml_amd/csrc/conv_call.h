// One conv call as it travels from a C entry point (conv_igemm.hip) to the launch site of a kernel family, and the only
// declarations of the functions that choose between the families.  Host code only: the kernels keep their own argument
// structs (ConvArgs, ConvFastArgs, ConvHaloArgs, ...), filled from a ConvCall at the launch site.
#pragma once
#include "common.h"

// What the shape predicates need.  The name query (msml_conv2d_kernel) and the *_applies entry points build one without
// pointers: kop is then the row count a packed weight of coutp channels has at least.
struct ConvShape {
  int c0p = 0, c1p = 0;        // padded channels of the two input segments (c1p = 0: one segment)
  int kop = 0, coutp = 0;      // packed weight rows, padded output channels
  int N = 0, H = 0, W = 0, P = 0, Q = 0, R = 0, S = 0, stride = 1, pad_h = 0, pad_w = 0, transposed = 0;
  int in_dtype = MSML_BF16, out_dtype = MSML_BF16;
  int want_stats = 0;          // the launch produces the per-channel (sum, sumsq) of its output (ConvCall: stats != nullptr)
  int stats_acc = 0;           // ... in ACCUMULATOR mode (common.h): `stats` / bnb->partial are f64 accumulators
};

// A ConvShape plus the operands and the epilogue of one call.
struct ConvCall : ConvShape {
  const void* in0 = nullptr;
  const void* in1 = nullptr;
  const void* wp = nullptr;
  const float* bias = nullptr;             // (the shift of the fused entry points)
  void* out = nullptr;
  float* stats = nullptr;
  const float* scale = nullptr;
  const float* alpha = nullptr;
  const void* residual = nullptr;
  int res_first = 0;
  const BnBwdFuse* bnb = nullptr;          // fused BatchNorm backward sums (msml_conv2d_bnbwd)
  int* bnb_rows = nullptr;                 // out: partial rows the chosen kernel writes
  const BnIn* xin = nullptr;               // BatchNorm(+PReLU) applied to the input in LDS (msml_conv2d_bnin[_acc])
  int x3 = 0;                              // split-bf16 inference (out_dtype == MSML_BF16X3; c0p / c1p are 3 x logical)
  int bias9 = 0;                           // border-class bias (common.h): `bias` is float[9][coutp]
  hipStream_t st = nullptr;
};

// ---- the bf16 fast path: msml_conv_fast_dispatch (conv_fast.hip) tries the families in a fixed order and ends on its own
// im2col kernel; false = not taken, nothing launched ------------------------------------------------------------------
bool msml_conv_fast_dispatch(const ConvCall& c);
bool msml_conv_r32_dispatch(const ConvCall& c);           // conv_r32.hip
bool msml_conv_pw_dispatch(const ConvCall& c);            // conv_pw.hip
bool msml_conv_s2r_dispatch(const ConvCall& c);           // conv_s2r.hip
bool msml_conv_s2r_x3_dispatch(const ConvCall& c);
bool msml_conv_ws_dispatch(const ConvCall& c);            // conv_ws.hip
bool msml_conv_halo_dispatch(const ConvCall& c);          // conv_halo.hip
bool msml_conv_halo2_dispatch(const ConvCall& c);         // conv_halo2.hip
// tried by msml_conv2d / msml_conv2d_fused in front of the fast path, each behind its own *_applies
bool msml_conv_line_dispatch(const ConvCall& c);          // conv_line.hip
bool msml_deconv4_dispatch(const ConvCall& c);            // conv_d4.hip

// ---- shape predicates, shared by the dispatch functions, msml_conv2d_kernel and the *_applies entry points ------------
bool msml_conv_line_applies(const ConvShape& s);
bool msml_deconv4_applies(const ConvShape& s);
bool msml_conv_ws_applies(const ConvShape& s);
bool msml_conv_halo_applies(const ConvShape& s);
int msml_conv_halo_persist_shape(const ConvShape& s);
int msml_conv_s2r_applies(const ConvShape& s);
int msml_conv_halo2_tiling(const ConvShape& s);           // 0 none, 1 plain 14 x 14 tiles, 2 / 3 mosaics

// Split-K GEMM on the im2col kernel (conv_fast.hip; PartialFC dX, conv_wgrad.hip): not a conv call, plain arguments.
bool msml_conv_fast_splitk(const void* in0, int c0p, const void* wp, int kop, float* ws, int coutp, int N, int ksplits,
                           hipStream_t st);
