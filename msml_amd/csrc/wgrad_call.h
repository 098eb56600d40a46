// One weight-gradient call as it travels from a C entry point (conv_wgrad.hip) to the launch site of a kernel family, the
// decision taken for it, and the only declarations of the host functions that cross a file boundary on this path: the
// counterpart of conv_call.h.  Host code only: the kernels keep their own argument structs (WgradArgs, WgradFastArgs,
// WgradHaloArgs, WgradN32Args, WgradLineArgs, FcWgradArgs), filled from a WgradCall and a WgradPlan at the launch site.
#pragma once
#include "common.h"

// Layers of one shape that may share a launch: the pointer arrays of WgradFastArgs, WgradHaloArgs and DwPtrs.
#define WGRAD_MAXGROUP 8
// No family ever takes more split-K slabs per layer than this.
#define WGRAD_MAXSPLITS 512

// Everything the choice of a kernel depends on.  The shape queries build one without pointers.
struct WgradShape {
  int up = 0, vp = 0;          // stored channels of U (pixel grid P x Q) and V (pixel grid H x W)
  int A = 0, Breal = 0, Btot = 0, boff = 0;      // dw[a < A][boff + b, b < Breal][R][S], Btot columns
  int N = 0, H = 0, W = 0, P = 0, Q = 0, R = 0, S = 0, stride = 1, pad_h = 0, pad_w = 0;
  int dtype = MSML_BF16;
  int group = 1;               // layers of this shape in the launch
  int bnin = 0;                // V is the input of a BatchNorm(+PReLU) applied in LDS (WgradCall: xin != nullptr)
  int dw_aligned = 1;          // every dw pointer is 16-byte aligned (the fc kernel's row stores); a pure query assumes so
};

// A WgradShape plus the operands of one call.  u / v / dw: host arrays of `group` device pointers.
struct WgradCall : WgradShape {
  const void* const* u = nullptr;
  const void* const* v = nullptr;
  float* const* dw = nullptr;
  int accumulate = 0;
  float* ws = nullptr;                     // split-K slabs [group][splits][up][taps][vp]
  long ws_bytes = 0;
  hipStream_t st = nullptr;
  const BnIn* xin = nullptr;
};

enum WgradFamily { WGRAD_NONE = 0, WGRAD_FC, WGRAD_N32, WGRAD_LINE, WGRAD_HALO, WGRAD_FAST, WGRAD_GENERIC };
enum { WGRAD_HALO_64 = 64, WGRAD_HALO_128 = 128, WGRAD_HALO_PAIR7 = 7 };     // WgradPlan::variant of the halo family

// The whole decision for one call (wgrad_plan, conv_wgrad.hip).
struct WgradPlan {
  int family = WGRAD_NONE;
  int variant = 0;             // halo: rows of the dW tile, or the image-pair strips of the 7 x 7 maps
  int ba = 0, bb = 0, ntw = 0; // fast / generic: tile rows, tile columns, taps per workgroup
  int splits = 0;              // per layer
  int chunk = 0;               // fast / generic: pixels per split (the strip kernels derive theirs from their strip count)
  int direct = 0;              // tiles go straight into dw: no slabs, no reduce
  long slab_bytes = 0;         // what the launch writes into the workspace: group * splits * up * taps * vp * 4, 0 when direct
  const char* refused = nullptr;           // why no kernel takes the shape (family == WGRAD_NONE), nullptr otherwise
};

// ---- one predicate per family: the splits per layer it would use, 0 = not taken.  *_max_splits: the largest answer over
// every completion of the fields msml_conv_wgrad_workspace does not have (H, W, stride, padding, dtype, switches aside)
bool msml_wgrad_fc_applies(const WgradShape& s);             // fc_wgrad.hip (no split-K)
int msml_wgrad_n32_applies(const WgradShape& s);             // wgrad_n32.hip
int msml_wgrad_n32_max_splits(const WgradShape& s);
int msml_wgrad_line_applies(const WgradShape& s);
int msml_wgrad_line_max_splits(const WgradShape& s);
int msml_wgrad_halo_applies(const WgradShape& s);            // wgrad_halo.hip (honours group and bnin)
int msml_wgrad_halo_variant(const WgradShape& s);
int msml_wgrad_halo_max_splits(const WgradShape& s);
bool msml_wgrad_fast_applies(const WgradShape& s);           // wgrad_fast.hip: false = tensors beyond 32-bit buffer offsets

// ---- one launcher per family; the plan is one that wgrad_plan made for this call
void msml_wgrad_fc_launch(const WgradCall& c, const WgradPlan& p);
void msml_wgrad_n32_launch(const WgradCall& c, const WgradPlan& p);
void msml_wgrad_line_launch(const WgradCall& c, const WgradPlan& p);
void msml_wgrad_halo_launch(const WgradCall& c, const WgradPlan& p);
void msml_wgrad_fast_launch(const WgradCall& c, const WgradPlan& p);
