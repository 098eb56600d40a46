/* libmsml_hip.so -- C ABI of the MI355X (gfx950) MSML hot path.
 *
 * This is the drop-in boundary: every entry point replaces a
 * torch.nn / torch.nn.functional / torch.distributed call site of the reference
 * (ygtxr1997/MSML), cited per function as <file>:<line> relative to the reference root.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  All pointers are DEVICE pointers owned
 *     by the caller (PyTorch caching allocator); the library never allocates, frees,
 *     synchronises or changes the current device.
 *   - every function enqueues on `stream` (a hipStream_t passed as void*) and returns
 *     immediately: 0 on success, a negative MSML_ERR_* otherwise; the message is available
 *     from msml_last_error() (thread-local).  No C++ exception crosses the ABI.
 *   - activations are NHWC ("pixel-major"): [N][H][W][Cp], Cp = channel count rounded up to a
 *     multiple of 8 (the Python host uses 8 or a multiple of 32, which selects the LDS-DMA
 *     fast conv path); pad channels hold exact zeros.  `dtype` selects the STORAGE type of
 *     activations / packed weights: MSML_F32 (exact-f32 MFMA path, parity mode) or MSML_BF16
 *     (bf16 operands, f32 accumulate).  Parameters, statistics and gradients of parameters
 *     are always f32 in the reference's own layouts (OIHW etc.).
 *   - reentrant: no global mutable state besides the thread-local error string and the option table below.
 */
#ifndef MSML_HIP_H
#define MSML_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSML_ABI_VERSION 1

enum { MSML_F32 = 0, MSML_BF16 = 1, MSML_BF16X3 = 2,     /* BF16X3: split-bf16 planes, see msml_conv2d_x3 */
       MSML_F64 = 3 };                                   /* msml_search_topk, msml_allpairs_pass */

enum {
  MSML_OK = 0,
  MSML_ERR_SHAPE = -1,       /* bad / inconsistent dimensions */
  MSML_ERR_DTYPE = -2,       /* unsupported dtype enum */
  MSML_ERR_LAUNCH = -3,      /* hipGetLastError() after launch */
  MSML_ERR_UNSUPPORTED = -4, /* valid request this build has no kernel for */
  MSML_ERR_WORKSPACE = -5,   /* workspace too small */
  MSML_ERR_CAPACITY = -6     /* more candidates than a fixed capacity holds (msml_det_nms) */
};

/* FM operator enums: backbones/fm/fmoperator.py:110-126 */
enum { MSML_ACT_TANH = 0, MSML_ACT_SIGMOID = 1 };
enum { MSML_ARITH_ADD = 0, MSML_ARITH_SUB = 1, MSML_ARITH_MUL = 2, MSML_ARITH_DIV = 3 };

int msml_version(void);
const char* msml_last_error(void);
/* Id of the graph capture `stream` is currently part of (hipStreamGetCaptureInfo; every stream forked into
 * one capture reports the same id), 0 when the stream is not capturing, negative on a HIP error.  The host
 * side keys per-capture scratch state on it (zeroed accumulator chunks: a second capture must not inherit the
 * first one's slices, whose zero fill only the first graph replays). */
long msml_stream_capture_id(void* stream);
/* `waiter` waits for everything queued on `src` so far: torch.cuda.Stream.wait_stream (the fork of the weight-gradient
 * side stream, backbones/msml.py has no counterpart: the reference runs one stream) through one re-recorded hipEvent per
 * calling thread.  Valid inside a graph capture (the waiter joins the capture). */
int msml_stream_wait_stream(void* waiter, void* src);

/* Switches (the MSML_* variables of the README's table; the list lives in msml_amd/csrc/options.h).  The environment is
 * read ONCE, at the library's first use of any switch; a later setenv changes nothing -- later changes go through
 * msml_set_option.  `name` is the environment name, `value` the PARSED value: 0 / 1 for the switches that only test
 * whether the variable exists (MSML_NO_*, ...), the number otherwise.  A set is visible to every thread's next launch
 * (relaxed atomics: setting while another thread launches is allowed, the launch sees the old or the new value).
 * MSML_ERR_UNSUPPORTED for an unknown name (named in msml_last_error()), MSML_ERR_SHAPE for a null pointer.
 * msml_option_name(index) enumerates the table: NULL past the end. */
int msml_set_option(const char* name, long value);
int msml_get_option(const char* name, long* value);
const char* msml_option_name(int index);

/* ---------------------------------------------------------------- layout (boundary) ------
 * The reference keeps NCHW f32 tensors end to end (backbones/msml.py:150); the HIP path
 * converts once at the MSML.forward boundary. */
int msml_nchw_to_nhwc(const float* src, void* dst, int N, int C, int H, int W, int Cp,
                      int dtype, void* stream);
int msml_nhwc_to_nchw(const void* src, float* dst, int N, int C, int H, int W, int Cp,
                      int dtype, void* stream);

/* Pack a 4-D f32 parameter w[A][B][R][S] (Conv2d: A=Cout,B=Cin; ConvTranspose2d: A=Cin,
 * B=Cout) into the GEMM operand the conv kernel streams: dst[KOp][Ktot] with
 *   transpose == 0: ko = a, ci = b      (conv forward, deconv backward-data)
 *   transpose == 1: ko = b, ci = a      (conv backward-data, deconv forward)
 * ci is split into up to two input segments (channel concat, e.g. cat(yf, yo)
 * fmoperator.py:285): segment 0 = ci in [0, C1), segment 1 = ci in [C1, C1+C2); each segment
 * is laid out [r][s][c] with c padded to C1p / C2p and the segment's K padded to a multiple
 * of 32 with zeros.  ko is padded to KOp rows of zeros.  Ktot = Kseg0 + Kseg1. */
int msml_pack_weight(const float* w, void* dst, int A, int B, int R, int S, int transpose,
                     int C1, int C1p, int C2, int C2p, int KOp, int dtype, void* stream);

/* ---------------------------------------------------------------- FM fusion ---------------
 * backbones/fm/fmoperator.py:288,304-310: M = act(x); z = arith(yf, M) + yf.
 * x, yf, z: [n] elements, storage dtype.  Algorithmic bytes: 3 * n * sizeof(dtype). */
int msml_fm_fuse_fwd(const void* x, const void* yf, void* z, long n, int act, int arith,
                     int dtype, void* stream);
/* backward: reads dz, x, yf; writes dx (grad of the pre-activation) and dyf.  5 streams. */
int msml_fm_fuse_bwd(const void* dz, const void* x, const void* yf, void* dx, void* dyf,
                     long n, int act, int arith, int dtype, void* stream);

/* Peer-guided branch of the FM operators (backbones/fm/fmoperator.py:293-308) and dropout
 * (backbones/frb/iresnet.py:231).  n elements (a multiple of 8), storage dtype.
 *   msml_fm_act_fwd / _bwd : M = act(x) as a tensor (the input of conv_m, :294-296) / dx = dM * act'(x)
 *   msml_mul_fwd / _bwd    : m_bar * identity, m_bar * yt (:297,300); da / db may be NULL
 *   msml_axpb              : y = a*x + b ('invert' mask transform 1 - M, :163-164)
 *   msml_mse_fwd / _bwd    : torch.nn.MSELoss()(f_occ, f_out) (:302): loss[0] = sum (a-b)^2 / count (f64
 *                            partial sums, fixed order; workspace >= 2048 doubles); da = 2 g (a-b) / count,
 *                            db = -da with g a device scalar
 *   msml_dropout           : y = x * keep / (1 - p), keep from a counter-based hash of (seed, index); the
 *                            backward is the same call on dy */
int msml_fm_act_fwd(const void* x, void* m, long n, int act, int dtype, void* stream);
int msml_fm_act_bwd(const void* dm, const void* x, void* dx, long n, int act, int dtype, void* stream);
int msml_mul_fwd(const void* a, const void* b, void* out, long n, int dtype, void* stream);
int msml_mul_bwd(const void* g, const void* a, const void* b, void* da, void* db, long n, int dtype,
                 void* stream);
int msml_axpb(const void* x, void* y, long n, float a, float b, int dtype, void* stream);
int msml_mse_fwd(const void* a, const void* b, long n, double count, float* loss, double* workspace,
                 long ws_doubles, int dtype, void* stream);
int msml_mse_bwd(const void* a, const void* b, const float* g, double count, void* da, void* db, long n,
                 int dtype, void* stream);
int msml_dropout(const void* x, void* y, long n, float p, long seed, int dtype, void* stream);
/* the same with the seed read from device memory (seed[0]): a dropout captured into a hipGraph draws a new mask on
 * every replay once the host side advances the seed tensor inside the graph */
int msml_dropout_dev(const void* x, void* y, long n, float p, const long* seed, int dtype, void* stream);

/* ---------------------------------------------------------------- convolution -------------
 * Implicit-GEMM convolution on MFMA.  Replaces nn.Conv2d / nn.ConvTranspose2d / nn.Linear
 * forward and backward-data at: backbones/frb/iresnet.py:56-67,209,232 (IBasicBlock, stem,
 * fc), backbones/fm/fmoperator.py:40-48,285-286 (bottleneck, same_conv on cat(yf, yo)),
 * backbones/osb/unet.py:32-38,193-221 (encoder, GCM 7x1/1x7, deconvs on cat(seg, gcm)),
 * headers/partial_fc.py:98 (logits GEMM) and the autograd of all of them.
 *
 *   out[n,oy,ox,ko] = bias[ko] + sum_seg sum_{r,s,c} in_seg[n,iy,ix,c] * wp[ko][seg,r,s,c]
 *   transposed == 0:  iy = oy*stride - pad_h + r                    (conv fwd, deconv bwd-data)
 *   transposed == 1:  iy = (oy + pad_h - r)/stride when divisible   (conv bwd-data, deconv fwd)
 *
 * in0/in1: NHWC [N][H][W][c0p]/[c1p] (in1 may be NULL with c1p = 0); wp from
 * msml_pack_weight with kop rows (>= coutp rounded up to msml_conv_tile_n(coutp));
 * out: NHWC [N][P][Q][coutp]; bias: [coutp] f32 or NULL.
 * stats (or NULL): [ceil(N*P*Q / msml_conv_tile_m(coutp))][2][coutp] f32 partial per-channel
 * (sum, sum of squares) of the f32 results, one row pair per pixel tile, for training-mode
 * BatchNorm (finalised by msml_bn_finalize).  in_dtype/out_dtype: (F32,F32), (BF16,BF16),
 * (BF16,F32). */
int msml_conv_tile_m(int coutp);
int msml_conv_tile_n(int coutp);
int msml_conv2d(const void* in0, int c0p, const void* in1, int c1p, const void* wp, int kop,
                const float* bias, void* out, int coutp, float* stats, int N, int H, int W,
                int P, int Q, int R, int S, int stride, int pad_h, int pad_w, int transposed,
                int in_dtype, int out_dtype, void* stream);

/* msml_conv2d whose BatchNorm statistics go to an ACCUMULATOR instead of partial rows: `acc` is a zero-initialised
 * double[8][2][coutp]; every workgroup adds its per-channel (sum, sumsq) with f64 atomics into row (workgroup index % 8).
 * The sums are those of row mode: of the f32 results (acc + bias) BEFORE they are rounded to the storage type, in every
 * kernel family (tests/conv_cases.py, STATDEF) -- not of the stored bf16 output, which differs from them by up to half a
 * bf16 ulp per element.  f64 sums of f32 partials are exact unless two partials differ by more than 2^29, so the
 * totals do not depend on the order of the adds.  Consumed by msml_bn_fin_act_fwd (no finalize launch in between:
 * the nn.BatchNorm2d that follows a conv in IBasicBlock, backbones/frb/iresnet.py:56-67). */
int msml_conv2d_acc(const void* in0, int c0p, const void* in1, int c1p, const void* wp, int kop,
                    const float* bias, void* out, int coutp, double* acc, int N, int H, int W,
                    int P, int Q, int R, int S, int stride, int pad_h, int pad_w, int transposed,
                    int in_dtype, int out_dtype, void* stream);

/* Weight gradient of the same family of layers (autograd of the call sites above, and
 * headers/partial_fc.py:169 sub_weight.grad):
 *   dw[a][boff+b][r][s] (+)= sum_{n,py,px} u[n,py,px,a] * v[n, py*stride-pad_h+r, px*stride-pad_w+s, b]
 * u: NHWC [N][P][Q][up] on the natural grid; v: NHWC [N][H][W][vp] shifted operand.
 * Conv2d: u = dY, v = X -> dw = [Cout][Cin][R][S]; ConvTranspose2d: u = X, v = dY ->
 * dw = [Cin][Cout][R][S].  dw is f32 in the parameter's own layout with Btot columns; only
 * a < A and b < Breal are written (channel-concat inputs call once per segment with boff).
 * Deterministic split-K: partial slabs in `workspace` (msml_conv_wgrad_workspace bytes),
 * summed in a fixed order.  N*P*Q must be < 2^24. */
long msml_conv_wgrad_workspace(int up, int vp, int N, int P, int Q, int R, int S);
int msml_conv_wgrad(const void* u, int up, const void* v, int vp, float* dw, int A, int Breal,
                    int Btot, int boff, int N, int H, int W, int P, int Q, int R, int S,
                    int stride, int pad_h, int pad_w, int accumulate, void* workspace,
                    long ws_bytes, int dtype, void* stream);

/* Weight gradients of `group` same-shape 3x3 / stride-1 / pad-1 conv layers in ONE launch pair (backbones/frb/
 * iresnet.py:40-67: consecutive IBasicBlocks of a stage share every dimension).  u / v / dw are HOST arrays of `group`
 * device pointers (dY, X, dW of each layer); everything else as msml_conv_wgrad.  The split-K slab traffic per layer
 * falls by the factor `group`.  MSML_ERR_UNSUPPORTED when the strip / halo kernel does not cover the shape.
 * msml_conv_wgrad_group_max: the largest useful group for a shape (1 = call msml_conv_wgrad instead). */
int msml_conv_wgrad_group_max(int up, int vp, int A, int Breal, int N, int H, int W, int P, int Q, int R, int S,
                              int stride, int pad_h, int pad_w);
int msml_conv_wgrad_group(const void* const* u, const void* const* v, float* const* dw, int group, int up, int vp,
                          int A, int Breal, int Btot, int boff, int N, int H, int W, int P, int Q, int R, int S,
                          int stride, int pad_h, int pad_w, int accumulate, void* workspace, long ws_bytes, int dtype,
                          void* stream);

/* 1 when msml_conv_wgrad (bf16) runs this shape on the narrow-operand kernel (wgrad_n32.hip: both operands
 * 32 stored channels, 4x4 / stride-2 transposed convs of the OSB decoder or 3x3 / stride-1). */
int msml_conv_wgrad_kernel_is_n32(int up, int vp, int N, int H, int W, int P, int Q, int R, int S, int stride,
                                  int pad_h, int pad_w);

/* How a weight-gradient call of this shape would run (tests, profiling labels): the decision of msml_conv_wgrad
 * (group 1), msml_conv_wgrad_group (group > 1: the consecutive IBasicBlocks of backbones/frb/iresnet.py:40-67) or
 * msml_conv_wgrad_bnin (bnin != 0), and the status that entry point returns before it launches, given valid pointers, a
 * 16-byte aligned dw and enough workspace.  plan[8] = family (0 none, 1 fc, 2 narrow-operand, 3 line, 4 strip / halo,
 * 5 im2col, 6 generic), variant (strip / halo: 64- or 128-row tiles, 7 = image-pair strips), tile rows, tile columns,
 * taps per workgroup (im2col / generic), split-K slabs per layer, pixels per split (im2col / generic), 1 when the tiles go
 * straight into dw.  *slab_bytes: what the launch writes into the workspace (0: nothing).  A pure shape query: no GPU. */
int msml_conv_wgrad_plan(int up, int vp, int A, int Breal, int Btot, int boff, int N, int H, int W, int P, int Q, int R,
                         int S, int stride, int pad_h, int pad_w, int dtype, int group, int bnin, int* plan,
                         long* slab_bytes);

/* ---------------------------------------------------------------- BatchNorm / PReLU --------
 * nn.BatchNorm2d(eps=1e-5, momentum=0.1) + nn.PReLU + residual of IBasicBlock
 * (backbones/frb/iresnet.py:56-67, backbones/osb/unet.py:80-91), resblock_bottle
 * (backbones/fm/fmoperator.py:53-68), the stems (iresnet.py:209-211, unet.py:193-195), bn2 and
 * BatchNorm1d `features` (iresnet.py:225,233).  Tensors are [M pixels][C], C % 8 == 0.
 *
 * msml_bn_stats: per-channel partial (sum, sumsq) rows -> partial[msml_bn_stats_rows(M,C)][2][C]
 * (the conv kernel's `stats` output has the same row format).
 * msml_bn_finalize: rows > 0 (training): mean / biased var from the partial rows (f64, fixed
 *   order), running stats updated in place like torch (unbiased var, momentum), mean/invstd saved;
 *   rows == 0 (eval): coefficients from the running stats.  Outputs scale = gamma*invstd,
 *   shift = beta - mean*scale.  gamma/beta NULL mean 1/0.
 * msml_bn_act_fwd: res_first == 0: y = prelu(x*scale[c] + shift[c], alpha[c]) + residual
 *   (IBasicBlock); res_first == 1: y = prelu(x*scale[c] + shift[c] + residual, alpha[c])
 *   (resblock_bottle, fmoperator.py:65-67).  alpha / residual optional.
 * msml_bn_act_bwd (training statistics): dx, dgamma, dbeta, dalpha from dy and the saved x;
 *   residual_first (the saved residual, only for res_first == 1) and dres (gradient flowing
 *   to that residual) optional; accumulate != 0 adds the parameter gradients into dgamma / dbeta /
 *   dalpha (the flat gradient arena) instead of overwriting; workspace >= rows*3*C + 2*C floats.
 * The apply loops keep a thread's per-channel coefficients in registers: msml_bn_act_fwd_stats and msml_bn_act_bwd
 *   (C <= 2048) need C / 8 to divide 256, msml_bn_act_fwd needs C / 8 to divide 256 or be a multiple of it;
 *   MSML_ERR_UNSUPPORTED otherwise.  msml_bn_stats takes any C % 8 == 0 up to 2048, msml_bias_grad any Cp % 8 == 0 up to 2048,
 *   msml_bn_finalize any C > 0. */
int msml_bn_stats_rows(long M, int C);
int msml_bn_stats(const void* x, long M, int C, float* partial, int dtype, void* stream);
int msml_bn_finalize(const float* partial, int rows, int C, double count, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, float momentum,
                     float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                     void* stream);
int msml_bn_act_fwd(const void* x, const float* scale, const float* shift, const float* alpha,
                    const void* residual, int res_first, void* y, long M, int C, int dtype,
                    void* stream);
/* msml_bn_act_fwd that also emits (sum, sumsq) partial rows of its OUTPUT (as stored), in the row
 * format of msml_bn_stats: the statistics of the next IBasicBlock's leading BatchNorm
 * (iresnet.py:57 bn1 on the previous block's output) without re-reading the tensor. */
int msml_bn_act_fwd_stats_rows(long M, int C);
int msml_bn_act_fwd_stats(const void* x, const float* scale, const float* shift, const float* alpha,
                          const void* residual, int res_first, void* y, long M, int C,
                          float* stats, int dtype, void* stream);
/* msml_bn_finalize (training mode) + msml_bn_act_fwd[_stats] in ONE launch from an accumulator (msml_conv2d_acc):
 * every workgroup folds acc[8][2][C] and derives the coefficients itself, workgroup 0 writes scale / shift /
 * save_mean / save_invstd and updates the running statistics; acc_out (optional, zero-initialised
 * double[8][2][C]) receives the (sum, sumsq) of the stored output.  C / 8 must divide 256. */
int msml_bn_fin_act_fwd(const double* acc, double count, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps, float* scale,
                        float* shift, float* save_mean, float* save_invstd, const void* x,
                        const float* alpha, const void* residual, int res_first, void* y, long M, int C,
                        double* acc_out, int dtype, void* stream);
int msml_bn_stats_acc(const void* x, long M, int C, double* acc, int dtype, void* stream);
/* Backward in accumulator mode (the three sums sum g, sum g*xhat, sum dy*min(z,0) as double[8][3][C], f64 atomics of
 * the producer): msml_conv2d_bnbwd_acc is msml_conv2d_bnbwd with that output; msml_bn_fin_bwd_apply is
 * k_bn_bwd_finalize + msml_bn_act_bwd_apply[_next][_s2] in one launch (add_h > 0: compact stride-2 `add`; next_acc:
 * zero-initialised accumulator of the activation-free BatchNorm whose output gradient dx is); msml_bn_act_bwd_acc is
 * msml_bn_act_bwd with its reduce pass adding into `acc`.  C / 8 must divide 256: MSML_ERR_UNSUPPORTED otherwise
 * (msml_bn_act_bwd_acc refuses before its reduce launch, `acc` stays untouched). */
int msml_conv2d_bnbwd_acc(const void* in0, int c0p, const void* wp, int kop, void* out, int coutp, int N,
                          int H, int W, int P, int Q, int R, int S, int stride, int pad_h, int pad_w,
                          int transposed, const void* bn_x, const float* bn_scale, const float* bn_shift,
                          const float* bn_alpha, const float* bn_mean, const float* bn_invstd, double* acc,
                          void* stream);
int msml_bn_fin_bwd_apply(const void* dy, const void* x, const float* scale, const float* shift,
                          const float* alpha, const float* save_mean, const float* save_invstd,
                          const double* acc, const void* residual_first, const void* add, int add_h,
                          int add_w, void* dx, void* dres, float* dgamma, float* dbeta, float* dalpha,
                          int accumulate, long M, int C, const void* next_x, const float* next_mean,
                          const float* next_invstd, double* next_acc, int dtype, void* stream);
int msml_bn_act_bwd_acc(const void* dy, const void* x, const float* scale, const float* shift,
                        const float* alpha, const float* save_mean, const float* save_invstd,
                        const void* residual_first, const void* add, void* dx, void* dres, float* dgamma,
                        float* dbeta, float* dalpha, int accumulate, long M, int C, double* acc, int dtype,
                        void* stream);
int msml_bn_act_bwd(const void* dy, const void* x, const float* scale, const float* shift,
                    const float* alpha, const float* save_mean, const float* save_invstd,
                    const void* residual_first, void* dx, void* dres, float* dgamma, float* dbeta,
                    float* dalpha, int accumulate, long M, int C, float* workspace, long ws_floats,
                    int dtype, void* stream);
/* Backward through an EVAL-mode (frozen) BatchNorm: (scale, shift) come from the running statistics and are constants
 * of the graph.  With z = x * scale + shift [+ residual_first] and g = dy * (z <= 0 ? alpha : 1) (g = dy without alpha):
 *   dx = scale * g, dres = g, dbeta = sum g, dgamma = sum g * (x - mean) * invstd, dalpha = sum dy * min(z, 0)
 * (mean / invstd: the running mean and 1 / sqrt(running_var + eps), needed for dgamma only).  One streaming pass; dgamma,
 * dbeta and dalpha are each optional, and with none of them there is no reduction, no second launch and `workspace` may
 * be null.  With any of them: workspace >= msml_bn_eval_act_bwd_rows(M, C) * 3 * C floats (MSML_ERR_WORKSPACE
 * otherwise); accumulate as in msml_bn_act_bwd.  C % 8 == 0, C <= 2048 (MSML_ERR_SHAPE), C / 8 divides 256
 * (MSML_ERR_UNSUPPORTED); every refusal comes before any launch. */
int msml_bn_eval_act_bwd_rows(long M, int C);
int msml_bn_eval_act_bwd(const void* dy, const void* x, const float* scale, const float* shift,
                         const float* alpha, const float* mean, const float* invstd,
                         const void* residual_first, void* dx, void* dres, float* dgamma, float* dbeta,
                         float* dalpha, int accumulate, long M, int C, float* workspace, long ws_floats,
                         int dtype, void* stream);
/* db[c] = sum over pixels of dy (biased GCM convs, backbones/osb/unet.py:23-30);
 * workspace >= msml_bn_stats_rows(M,Cp)*2*Cp floats. */
int msml_bias_grad(const void* dy, long M, int Cp, int Creal, float* db, int accumulate,
                   float* workspace, long ws_floats, int dtype, void* stream);
/* out = a + b (GCM branch sum unet.py:37; gradient joins) */
int msml_add(const void* a, const void* b, void* out, long n, int dtype, void* stream);

/* ---------------------------------------------------------------- OSB tail + seg loss -------
 * msml_dap_fwd: DAP = PixelShuffle(3)->AvgPool2d(3) (backbones/osb/unet.py:158-161,223) == mean
 *   over 9-channel groups; x NHWC [N][H][W][Cp>=18] -> seg NCHW f32 [N][2][H][W] and (optional)
 *   mask[N][H][W] u8 = argmax over the 2 classes, ties -> 0 (train.py:357). */
int msml_dap_fwd(const void* x, float* seg, unsigned char* mask, int N, int H, int W, int Cp,
                 int dtype, void* stream);
int msml_dap_bwd(const float* dseg, void* dx, int N, int H, int W, int Cp, int dtype, void* stream);
/* StructureConsensuLossFunction(alpha, beta, 'idx', 'idx')(logit, msk, msk)
 * (tricks/consensus_loss.py:65-167, train.py:258).  logit NCHW f32 [N][2][H][W], msk int64
 * [N][H][W] in {0,1}; loss[1]; dlogit (optional) = d loss / d logit.  workspace >= 20*N floats. */
int msml_seg_consensus_loss(const float* logit, const long* msk, int N, int H, int W, float alpha,
                            float beta, float* loss, float* dlogit, float* workspace,
                            long ws_floats, void* stream);
/* the same with the reference's other reductions (tricks/consensus_loss.py:42-57,127-133,159-162): reduce_pixel_all != 0
 * divides the blob mean by H * W ('all') instead of the blob's pixel count ('idx'); reduce_pixel_kl_all != 0 averages the
 * consensus term over N * H * W instead of its non-zero entries. */
int msml_seg_consensus_loss_r(const float* logit, const long* msk, int N, int H, int W, float alpha, float beta,
                              int reduce_pixel_all, int reduce_pixel_kl_all, float* loss, float* dlogit,
                              float* workspace, long ws_floats, void* stream);

/* ---------------------------------------------------------------- classification head -------
 * kind: 0 = AMArcFace (headers/margin_losses.py:356-418), 1 = AMCosFace (:241-305).
 * msml_rownorm_fwd: F.normalize rows of w[R][E] (margin_losses.py:371, partial_fc.py:115) into
 *   dst[Rp][ld] (storage dtype, zero padded) + inv_norm[R].
 * msml_rownorm_bwd: dw (+)= (dy - y<y,dy>) * inv_norm  with dy f32 [R][ldy].
 * msml_gather_target / msml_margin_fwd / msml_margin_bwd: margin on the target logits, in place
 *   on the f32 cosine matrix [N][ld]; backward emits dcos in storage dtype [N][ldo].
 * msml_pfc_rowstats / msml_pfc_grad: the two local passes of PartialFC's distributed
 *   softmax-CE (partial_fc.py:132-167) around the max / sum / loss all-reduces; the margin is
 *   applied on the fly so the logits are never materialised. */
int msml_rownorm_fwd(const float* w, int R, int Rp, int E, void* dst, int ld, float* inv_norm,
                     int dtype, void* stream);
int msml_rownorm_bwd(const float* w, const float* inv_norm, const float* dy, int ldy, int R, int E,
                     float* dw, int accumulate, void* stream);
int msml_gather_target(const float* cosm, int ld, const long* label, int N, float* out,
                       void* stream);
int msml_margin_fwd(float* cosm, const long* label, int N, int C, int ld, int kind, float s,
                    float m, float a, float k, void* stream);
int msml_margin_bwd(const float* dlogit, int ldg, const long* label, const float* cos_t, int N,
                    int C, void* dcos, int ldo, int kind, float s, float m, float a, float k,
                    int dtype, void* stream);
int msml_pfc_rowstats(const float* cosm, int ld, int N, int C, const long* label, int kind, float s,
                      float m, float a, float k, float* rowmax, float* rowsum, void* stream);
int msml_pfc_grad(const float* cosm, int ld, int N, int C, const long* label, int kind, float s,
                  float m, float a, float k, const float* gmax, const float* gsum, float eps_ls,
                  float inv_n, void* dcos, int ldo, float* ptarget, int dtype, void* stream);
/* torch.optim.SGD(momentum, weight_decay) step on one flat, 16-B aligned f32 buffer
 * (train.py:179-191); clip_coef (device scalar or NULL) multiplies the gradient first.
 * msml_grad_norm_clip: out2[0] = global L2 norm of grad[n], out2[1] = min(1, max_norm /
 * (norm + 1e-6)) = torch.nn.utils.clip_grad_norm_'s factor (train.py:270,275), on device, no
 * host sync; workspace >= 1024 floats. */
int msml_sgd_momentum(float* w, const float* grad, float* mom, long n, float lr, float mu, float wd,
                      int first_step, const float* clip_coef, void* stream);
int msml_grad_norm_clip(const float* grad, long n, float max_norm, float* out2, float* workspace,
                        long ws_floats, void* stream);
/* msml_sgd_momentum_dev: msml_sgd_momentum with the learning rate read from DEVICE memory (lr[0]) and the momentum
 *   buffer always combined (mu * buf + g; a zero buffer gives torch's first step): a step captured into a hipGraph
 *   follows torch.optim.lr_scheduler.LambdaLR (train.py:193-196) without a re-capture.
 * msml_grad_norm_clip_scaled: the gradient buffer holds the SUM over W data-parallel ranks (scale = 1 / W): out2[0] =
 *   norm of the averaged gradient, out2[1] = scale * clip factor -- DistributedDataParallel's division by W
 *   (train.py:136-138) folded into the one coefficient the SGD kernel applies, no separate pass over the gradients. */
int msml_sgd_momentum_dev(float* w, const float* grad, float* mom, long n, const float* lr, float mu, float wd,
                          const float* coef, void* stream);
int msml_grad_norm_clip_scaled(const float* grad, long n, float max_norm, float scale, float* out2, float* workspace,
                               long ws_floats, void* stream);

/* Skinny GEMM with a huge K, split over K with deterministic slab reduction: out[M][coutp] (f32)
 * = a[M][K] (bf16, K % 32 == 0) . wp[kop][K]^T.  PartialFC dX = dcos . Wn (K = local classes,
 * headers/partial_fc.py:169 total_features.grad). */
long msml_gemm_splitk_workspace(int M, int coutp, int K);
int msml_gemm_splitk(const void* a, int M, int K, const void* wp, int kop, float* out, int coutp,
                     void* workspace, long ws_bytes, int dtype, void* stream);

/* Pack many weights (or sub-blocks of weights) in ONE launch.  table: device array of count x 16
 * int64 {w, dst, Afull, Bfull, a_off, A, b_off, B, R, S, transpose, C1, C1p, C2, C2p, KOp}; every
 * entry is packed as msml_pack_weight would pack the sub-block (a_off, A) x (b_off, B) of
 * w[Afull][Bfull][R][S].  Used once per training step for the forward and backward-data operands
 * of every conv / deconv / linear of the model. */
int msml_pack_weights_batched(const long* table, int count, int dtype, void* stream);
/* Same packing through LDS tiles (coalesced on both sides; the per-step refresh).  Only the real
 * elements are written: dst must carry its zero padding already (R*S <= 49).  tile_prefix: device
 * array [count + 1] = the exclusive prefix sum of msml_pack_tiles(A, B, R, S) over the entries
 * followed by the total; optionally [count] = -1 followed by total_tiles entry indices (tile -> entry),
 * which saves the per-block binary search. */
int msml_pack_tiles(int A, int B, int R, int S);
int msml_pack_weights_tiled(const long* table, const int* tile_prefix, int count, int total_tiles,
                            int dtype, void* stream);

/* dst[c][r] = src[r][c] (storage dtype), dst rows ld_d long, zero-filled for r >= R.  Wn^T for the
 * PartialFC dX GEMM (headers/partial_fc.py:169). */
int msml_transpose(const void* src, int R, int C, int ld_s, void* dst, int ld_d, int dtype,
                   void* stream);

/* Inference conv with the eval-mode BatchNorm folded into the epilogue (bf16 tensors only):
 *   res_first == 0: out = prelu(acc*scale[c] + shift[c], alpha[c]) + residual   (IBasicBlock)
 *   res_first == 1: out = prelu(acc*scale[c] + shift[c] + residual, alpha[c])   (resblock_bottle)
 * scale/shift from msml_bn_finalize(rows = 0); alpha, residual optional.  The residual joins the value AS STORED: every
 * kernel rounds prelu(acc*scale + shift) (res_first: acc*scale + shift) to bf16 in its copy-out layout, adds the bf16
 * residual to that in f32 and rounds once more -- the rounding points of the chain the call replaces.  Replaces the
 * conv -> BatchNorm(eval) -> PReLU -> (+identity) chains of backbones/frb/iresnet.py:59-66,
 * backbones/fm/fmoperator.py:55-67 in eval mode (eval/verification.py:271). */
int msml_conv2d_fused(const void* in0, int c0p, const void* in1, int c1p, const void* wp, int kop,
                      const float* scale, const float* shift, const float* alpha,
                      const void* residual, int res_first, void* out, int coutp, int N, int H,
                      int W, int P, int Q, int R, int S, int stride, int pad_h, int pad_w,
                      int transposed, void* stream);

/* ---------------------------------------------------------------- split-bf16 inference ("bf16x3") ---
 * f32-class accuracy on the bf16 MFMA (gfx950 has no TF32; exact-f32 MFMA is 1/16 of the bf16 rate):
 * a value is stored as hi = bf16(x), lo = bf16(x - hi); a pixel of an MSML_BF16X3 tensor holds 3*C bf16
 * channels [hi(C) | lo(C) | hi(C)], a packed weight is laid out [wh | wh | wl] along each tap's channels,
 * so x.w ~= xh.wh + xl.wh + xh.wl is ONE implicit GEMM over 3*C input channels on the unchanged bf16 main
 * loop.  Meets the reference's eval tolerances with fp16=True (embedding <= 1e-3, mask indices bit-exact).
 *
 * msml_conv2d_x3: msml_conv2d_fused on split tensors.  c0p / c1p / coutp are the LOGICAL padded channel
 *   counts (multiples of 32); in0 / in1 / residual / out hold 3x that many bf16 channels per pixel; wp from
 *   msml_pack_weight over the expanded weight ([wh|wh|wl] per segment, C1p = 3*c0p, C2p = 3*c1p).
 *   out = [prelu](acc*scale + shift [+ residual]) [+ residual]; scale NULL = 1, shift NULL = 0 (plain conv
 *   with bias: shift = bias).  Replaces the same call sites as msml_conv2d / msml_conv2d_fused in eval mode.
 * msml_x3_bn_act_fwd / msml_x3_fm_fuse_fwd / msml_x3_add: msml_bn_act_fwd / msml_fm_fuse_fwd / msml_add on
 *   split tensors of M pixels x C channels.  msml_x3_from_f32 / msml_x3_to_f32: [M][C] f32 <-> split. */
int msml_conv2d_x3(const void* in0, int c0p, const void* in1, int c1p, const void* wp, int kop,
                   const float* scale, const float* shift, const float* alpha, const void* residual,
                   int res_first, void* out, int coutp, int N, int H, int W, int P, int Q, int R, int S,
                   int stride, int pad_h, int pad_w, int transposed, void* stream);
/* msml_conv2d_x3_border: the 3x3 / stride-1 / pad-1 forward case of msml_conv2d_x3 with a shift per BORDER CLASS of the
 *   output pixel: shift9 = float[9][coutp], row cy * 3 + cx, cy (cx) = 0 on the first row (column) of the map, 2 on the
 *   last, 1 inside; H, W >= 2.  Lets the caller fold an eval-mode BatchNorm IN FRONT of the conv into it -- bn1 -> conv1
 *   of IBasicBlock (reference backbones/frb/iresnet.py:58-60): conv(W, s x + t) = conv(W s, x) + the sum of W t over
 *   the taps that fall INSIDE the map (the zero padding follows the BatchNorm), which is a constant per class. */
int msml_conv2d_x3_border(const void* in0, int c0p, const void* wp, int kop, const float* scale,
                          const float* shift9, const float* alpha, const void* residual, int res_first,
                          void* out, int coutp, int N, int H, int W, void* stream);
int msml_x3_bn_act_fwd(const void* x, const float* scale, const float* shift, const float* alpha,
                       const void* residual, int res_first, void* y, long M, int C, void* stream);
int msml_x3_fm_fuse_fwd(const void* x, const void* yf, void* z, long M, int C, int act, int arith,
                        void* stream);
int msml_x3_add(const void* a, const void* b, void* out, long M, int C, void* stream);
int msml_x3_from_f32(const float* src, void* dst, long M, int C, void* stream);
int msml_x3_to_f32(const void* src, float* dst, long M, int C, void* stream);

/* ---------------------------------------------------------------- verification metrics -----------
 * Device side of eval/verification.py:54-199 (calculate_roc / calculate_val: 10-fold accuracy over a
 * threshold grid, TAR @ FAR).  msml_pair_sqdist: emb [2*n_pairs][E] f32, rows (2i, 2i+1) = pair i ->
 * dist[i] = || a/|a| - b/|b| ||^2 in f64 (:298-301,78-79).  msml_pair_hist: hist[nfolds][2][nthr + 1]
 * int32, hist[f][s][k] = number of pairs of KFold test fold f (shuffle=False) with issame == s whose
 * first threshold index with dist < thr[k] is k (k == nthr: none); every tp / fp / tn / fn of every
 * threshold and fold is a prefix sum of it.  thr: ascending f64 grid (np.arange(0, 4, 0.01 | 0.001)). */
int msml_pair_sqdist(const float* emb, int n_pairs, int E, double* dist, void* stream);
/* the same on the f64 sum of the orig + flip embedding passes (verification.py:283,299-300 accumulates both passes
 * in float64 arrays before normalising) */
int msml_pair_sqdist_f64(const double* emb, int n_pairs, int E, double* dist, void* stream);
int msml_pair_hist(const double* dist, const unsigned char* same, int n_pairs, const double* thr, int nthr,
                   int nfolds, int* hist, void* stream);

/* ---------------------------------------------------------------- device input pipeline ----------
 * Replaces the per-sample CPU augmentation of FaceByRandOccMask.__getitem__ (datasets/load_dataset.py:
 * 101-139) for the occluders that need no dataset assets: RandomRect (datasets/augment/rand_occ.py:103-139),
 * RandomEllipse (:148-203, analytic ellipse), RandomConnectedPolygon (:217-322, even-odd point-in-polygon test),
 * NoneOcc (:80-90), RandomBlock (:43-72, evaluation), the random
 * horizontal flip (load_dataset.py:119-123), the Gaussian light of _add_gauss_to_face (:183-201, _get_gauss
 * :282-339) and ToTensor + Normalize(0.5, 0.5).
 * msml_occ_draw: per-image descriptors desc[N][64] int32 {kind (0 none, 1 rect, 2 ellipse, 3 block, 4 polygon),
 *   x0|cx, y0|cy, w|aw, h|ah, r, g, b, flip, light cx / cy / scale (f32 bits), polygon vertex count, 0, 0, 0,
 *   up to 24 polygon vertices (x, y)} from a counter-based generator keyed by (seed, offset + image index):
 *   mode 0 = training mix {rect, ellipse, polygon, none}, 1 = rect (lo..hi percent), 2 = black block (lo..hi
 *   percent), 3 = none, 4 = polygon.
 * msml_occ_apply: src [N][H][W][3] uint8 (decoded RGB) -> img [N][3][H][W] f32 in [-1, 1] (occluded,
 *   flipped, lit when light != 0, normalised), msk [N][H][W] int64 (0 occluded / 1 clean,
 *   load_dataset.py:37), ori [N][3][H][W] (clean, flipped, normalised; optional). */
int msml_occ_draw(long seed, long offset, int N, int H, int W, int mode, int lo, int hi, int flip, int* desc,
                  void* stream);
int msml_occ_apply(const unsigned char* src, const int* desc, float* img, long* msk, float* ori, int N, int H,
                   int W, int light, void* stream);

/* Texture occluders of the reference's training mix: RandomGlasses / RandomGlassesList (datasets/augment/rand_occ.py:
 * 337-428), RandomScarf (:431-517), RandomRealObject (:520-600), selected as datasets/load_dataset.py:72-85,155-163.
 * The RGBA images come from the CALLER (atlas: every set's entries [num][h0][w0][4] uint8, preloaded from the user's
 * checkout exactly as the reference's constructors do; nothing ships with this library).
 *   meta[nsets][16] int32: byte offset of the set in `atlas`, entries, h0, w0, kind (5 glasses, 6 scarf, 7 object),
 *     wmin, wmax, hmin, hmax (resampled sizes the tables cover), wdir, hdir, 0...;
 *   dir / rtab: PIL's bicubic resampling coefficients (ImagingResample precompute_coeffs + normalize_coeffs_8bpc,
 *     22-bit fixed point), built on the host: rtab[dir[wdir + w' - wmin] + x * 10 + {0: first tap, 1: taps, 2..9: k}].
 * msml_occ_draw_tex: msml_occ_draw plus modes 5 (ms1m mix: uniform over rect, ellipse, polygon, glasses, scarf, object,
 *   none), 6 (casia mix: none with probability 1/2, else one of the six), 7 / 8 / 9 (glasses / scarf / object only);
 *   texture descriptors: kind, x, y of the paste, resampled w', h', set (word 13), entry (word 14).
 * msml_occ_resize: per image of a texture kind, Image.resize((w', h')) of its RGBA entry, bit for bit (RGBA -> RGBa,
 *   horizontal + vertical fixed-point pass, RGBa -> RGBA) into patch[n][patch_stride] (rows of w' RGBA pixels);
 *   lds_bytes >= (h0 * w0 + h0 * wmax) * 4 of the largest set.
 * msml_occ_apply_tex: msml_occ_apply with the paste: glasses replace the face where alpha > 10, scarf / object where
 *   alpha != 0, the mask is 0 where alpha != 0 (all three), cropped at the image border. */
int msml_occ_draw_tex(long seed, long offset, int N, int H, int W, int mode, int lo, int hi, int flip,
                      const int* meta, int nsets, int* desc, void* stream);
int msml_occ_resize(const unsigned char* atlas, const int* meta, const int* dir, const int* rtab, const int* desc,
                    unsigned char* patch, long patch_stride, int N, int lds_bytes, void* stream);
int msml_occ_apply_tex(const unsigned char* src, const int* desc, const unsigned char* patch, long patch_stride,
                       float* img, long* msk, float* ori, int N, int H, int W, int light, void* stream);

/* Gray / resized / unnormalised output: FaceByRandOccMask.__getitem__ with is_gray, out_size, use_norm
 * (datasets/load_dataset.py:86-139,179,183-201; the LightCNN recipe of config.py:99-102 is gray, 128 x 128, no Normalize).
 * msml_occ_draw_out: msml_occ_draw_tex (all modes; meta may be NULL for modes 0-4) with the light centre drawn over
 *   out_w x out_h, the image the light is added to.  Same draw indices: with out_h = H, out_w = W the descriptors equal
 *   msml_occ_draw[_tex]'s word for word; otherwise only words 9 and 10 differ.
 * msml_occ_apply_out: occlusion at the source size (patch: msml_occ_resize's output for texture descriptors, or NULL),
 *   convert('L') when gray (L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16), Image.resize((out_w, out_h), BILINEAR) of
 *   face, 0 / 255 mask and clean face bit for bit (horizontal pass, uint8 intermediate, vertical pass; an axis whose
 *   size does not change is skipped), flip, ToTensor, light at the output size, mask != 255 -> 0 else 1, Normalize(0.5,
 *   0.5) only when norm != 0.  img / ori [N][C][out_h][out_w] f32 with C = 1 (gray) or 3, msk [N][out_h][out_w] int64;
 *   ori may be NULL.  tabw / tabh: Pillow's triangle-filter coefficients of W -> out_w / H -> out_h in the layout of
 *   msml_occ_resize's tables ([out][10] int32: first tap, taps, 22-bit fixed-point coefficients), built on the host;
 *   NULL for an axis that keeps its size.  One workgroup per image with every intermediate in LDS: returns
 *   MSML_ERR_UNSUPPORTED before any launch when the planes need more than 160 KB (RGB 112 -> 224) or out_w % 4 != 0. */
int msml_occ_draw_out(long seed, long offset, int N, int H, int W, int out_h, int out_w, int mode, int lo, int hi,
                      int flip, const int* meta, int nsets, int* desc, void* stream);
int msml_occ_apply_out(const unsigned char* src, const int* desc, const unsigned char* patch, long patch_stride,
                       const int* tabw, const int* tabh, float* img, long* msk, float* ori, int N, int H, int W,
                       int out_h, int out_w, int gray, int norm, int light, void* stream);

/* The facial-mask branch of the training mix: FaceByRandOccMask.__getitem__ with mask_flag (datasets/load_dataset.py:113,
 * 167-177: the face comes from mask_out.rec, the segmentation target from mask.rec) and _add_gauss_to_mask (:203-280).
 * The renders are the caller's; what is done with them runs here.
 * msml_occ_draw_mask: msml_occ_draw_out with one more draw per image: occ_unif(draw 46) < p_mask makes the image a MASK
 *   sample (kind 8; p_mask = 0.2 is the reference's 2 / 10, :113).  An image that is not flagged gets msml_occ_draw_out's
 *   descriptor word for word; a flagged one gets a descriptor that does not depend on p_mask: words 1-7 and 12-15 zero,
 *   8-11 flip and light as always, 16 type (0 Gaussian light, 1 Gaussian noise, 2 block: trans_type = randint(0, 11)
 *   >= 7, 5-6, <= 4, :219), 17-20 the rectangle lx, ly, rx, ry in OUTPUT pixels (:222-223, :251-252), 21 sign (+1 / -1,
 *   :238, :255), 22-24 the colour-jitter bits (:261), 25-27 the f32 bits of the light's centre x, y (absolute, as
 *   _get_gauss :307-308 draws them) and radius (:316), 28-29 the low / high half of the sample's noise key
 *   mix(mix(seed + 0x6D61736B) + offset + n).  p_mask > 0 needs out_h >= 111 and out_w >= 110 (the reference's
 *   rectangle is not scaled with the size and does not fit below).
 * msml_occ_apply_mask: an overlay launched AFTER msml_occ_apply[_tex | _out] on the same desc / img / msk: one workgroup
 *   per image, which returns at once unless the image is a mask sample whose row r = rows[n] (rows == NULL: r = n) lies
 *   in 0 .. M - 1.  Otherwise it rewrites img[n] and msk[n] from masked[r] ([M][H][W][3] uint8 RGB) and mask[r]
 *   ([M][H][W] uint8, the 'L' plane): convert('L') of the face when gray, Image.resize(BILINEAR) of face and mask as
 *   msml_occ_apply_out, flip, ToTensor, light at the output size and / max (:183-201), then :209-280: mask <= 128 -> 0
 *   (occluded) else 1; on occluded pixels inside the rectangle a float16 offset -- (exp(-0.5 d^2 / r^2) - 0.5) * 2 * 0.4
 *   * sign with the int16-truncated offsets of _get_gauss (relative coordinate minus absolute centre, as written), a
 *   standard normal, or +-1 for the block -- times the jitter bit of the channel (light and noise), folded to gray as
 *   (0.2989 l0 + 0.5870 l1 + 0.1140 l2) / 3 in float16 when gray; img = face - offset in f32, not clamped; Normalize
 *   only when norm != 0.  The normal variate of output pixel (x, y): r = mix(key + y * 65536 + x) with the key of words
 *   28-29 (mix = the splitmix64 step of msml_occ_draw), u1 = ((r >> 40) + 1) / 2^24, u2 = ((r >> 8) & 0xFFFFFF) /
 *   2^24, z = sqrt(-2 ln u1) cos(2 pi u2) in f32, rounded to float16: independent of launch geometry, batch split and
 *   p_mask.  ori is not touched (the clean face msml_occ_apply* wrote).  Same refusals as msml_occ_apply_out:
 *   MSML_ERR_UNSUPPORTED before any launch for out_w % 4 != 0 or more than 160 KB of LDS. */
int msml_occ_draw_mask(long seed, long offset, int N, int H, int W, int out_h, int out_w, int mode, int lo, int hi,
                       int flip, const int* meta, int nsets, float p_mask, int* desc, void* stream);
int msml_occ_apply_mask(const unsigned char* masked, const unsigned char* mask, const int* rows, int M, const int* desc,
                        const int* tabw, const int* tabh, float* img, long* msk, int N, int H, int W, int out_h,
                        int out_w, int gray, int norm, int light, void* stream);

/* Backward-data of the OSB decoder's ConvTranspose2d(36 -> 18, k 4, s 2, p 1) on cat(seg, gcm) (backbones/osb/unet.py:
 * 140-156, autograd of deconv2..5) for BOTH input segments from one pass over dY (bf16):
 *   dxS[n, i, j, ci] = sum_{r, s, co} dy[n, 2i - 1 + r, 2j - 1 + s, co] * w[S * 18 + ci][co][r][s]
 * dy [N][2H][2H][32], dx0 / dx1 [N][H][H][32]; wp0 / wp1 = msml_pack_weight of the segment's rows of the
 * ConvTranspose2d weight (transpose 0, C1 = 18: [32 ci rows][16 taps x 32 co]).  H in {14, 28, 56};
 * MSML_ERR_UNSUPPORTED otherwise (callers then run msml_conv2d per segment). */
int msml_deconv4_bwd_data(const void* dy, const void* wp0, const void* wp1, void* dx0, void* dx1, int N, int H,
                          void* stream);

/* Backward-data conv fused with the backward REDUCE of the BatchNorm(+PReLU) that produced the
 * conv's input in the forward (IBasicBlock: bn1 -> conv1, bn2 -> prelu -> conv2,
 * backbones/frb/iresnet.py:59-64): the conv output dX is that BatchNorm's dy, so the epilogue
 * accumulates sum g, sum g*xhat, sum dy*min(z,0) per channel from the stored (bf16) dX and the
 * saved BatchNorm input bn_x (same [N][P][Q][coutp] layout), one partial row [3][coutp] per
 * workgroup.  bf16 only; MSML_ERR_UNSUPPORTED when the shape is not on the fast path (callers
 * fall back to msml_conv2d + msml_bn_act_bwd).  partial needs msml_conv2d_bnbwd_rows() rows;
 * *rows_used = rows written (all of them fully).  msml_bn_act_bwd_apply finishes the job:
 * finalize over `rows` + dx = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)) [+ add];
 * coef_ws: 98*C floats of scratch (2*C coefficients + 32 folded partial rows).  msml_bn_act_bwd_apply and its
 * _next / _s2 / _next_s2 forms need C / 8 to divide 256 (MSML_ERR_UNSUPPORTED otherwise, before any launch). */
int msml_conv2d_bnbwd_rows(int coutp, int N, int P, int Q);
int msml_conv2d_bnbwd(const void* in0, int c0p, const void* wp, int kop, void* out, int coutp,
                      int N, int H, int W, int P, int Q, int R, int S, int stride, int pad_h,
                      int pad_w, int transposed, const void* bn_x, const float* bn_scale,
                      const float* bn_shift, const float* bn_alpha, const float* bn_mean,
                      const float* bn_invstd, float* partial, int rows_cap, int* rows_used,
                      void* stream);
int msml_bn_act_bwd_apply(const void* dy, const void* x, const float* scale, const float* shift,
                          const float* alpha, const float* save_mean, const float* save_invstd,
                          const float* partial, int rows, const void* add, void* dx,
                          float* dgamma, float* dbeta, float* dalpha, int accumulate, long M,
                          int C, float* coef_ws, int dtype, void* stream);

/* msml_bn_act_bwd_apply / _next with `add` given as the COMPACT input gradient of a 1x1 / stride-2
 * / pad-0 conv over an H x W map (downsample path of a stage's first block,
 * backbones/frb/iresnet.py:52-54,66): add[N][ceil(H/2)][ceil(W/2)][C] is summed into the pixels
 * with even (y, x); the dense gradient (3/4 zeros) is neither written nor re-read.  M = N*H*W < 2^24. */
int msml_bn_act_bwd_apply_s2(const void* dy, const void* x, const float* scale, const float* shift,
                             const float* alpha, const float* save_mean, const float* save_invstd,
                             const float* partial, int rows, const void* add, int H, int W, void* dx,
                             float* dgamma, float* dbeta, float* dalpha, int accumulate, long M,
                             int C, float* coef_ws, int dtype, void* stream);
int msml_bn_act_bwd_apply_next_s2(const void* dy, const void* x, const float* scale,
                                  const float* shift, const float* alpha, const float* save_mean,
                                  const float* save_invstd, const float* partial, int rows,
                                  const void* add, int H, int W, void* dx, float* dgamma, float* dbeta,
                                  float* dalpha, int accumulate, long M, int C, float* coef_ws,
                                  const void* next_x, const float* next_mean,
                                  const float* next_invstd, float* next_partial, int dtype,
                                  void* stream);

/* Training-mode BatchNorm(+PReLU) in FRONT of a 3x3 / stride-1 / pad-1 conv (IBasicBlock:
 * bn1 -> conv1, bn2 -> prelu -> conv2, backbones/frb/iresnet.py:58-63, backbones/osb/unet.py:82-87)
 * applied while the conv's input image sits in LDS: the conv reads the BatchNorm's INPUT in0 and
 * computes on X = bf16(PReLU(in0 * in_scale + in_shift)) (in_alpha NULL: no PReLU; scale / shift
 * from msml_bn_finalize), zero padding applied to X as in the unfused graph, so the result equals
 * msml_bn_act_fwd followed by msml_conv2d bit for bit while X is never written to HBM.
 * msml_conv_wgrad_bnin is the matching weight gradient (u = dY, v = the BatchNorm input).
 * bf16 only, and only the shapes of the halo-tile kernels (the *_applies queries return 1);
 * MSML_ERR_UNSUPPORTED otherwise -- callers then materialise X with msml_bn_act_fwd. */
int msml_conv2d_bnin_applies(int c0p, int coutp, int N, int H, int W, int P, int Q, int R, int S,
                             int stride, int pad_h, int pad_w, int want_stats);
int msml_conv2d_bnin(const void* in0, int c0p, const float* in_scale, const float* in_shift,
                     const float* in_alpha, const void* wp, int kop, void* out, int coutp,
                     float* stats, int N, int H, int W, int P, int Q, int R, int S, int stride,
                     int pad_h, int pad_w, void* stream);
int msml_conv_wgrad_bnin_applies(int up, int vp, int A, int Breal, int N, int H, int W, int P, int Q,
                                 int R, int S, int stride, int pad_h, int pad_w);
int msml_conv_wgrad_bnin(const void* u, int up, const void* v, int vp, const float* x_scale,
                         const float* x_shift, const float* x_alpha, float* dw, int A, int Breal,
                         int Btot, int boff, int N, int H, int W, int P, int Q, int R, int S,
                         int stride, int pad_h, int pad_w, int accumulate, void* workspace,
                         long ws_bytes, void* stream);

/* Name of the kernel the conv entry points launch for a shape (profiling labels only).  want_stats with the
 * MSML_KERNEL_MFM bit set names the kernel of msml_conv2d_mfm (coutp = its GEMM columns, 2 x the output channels). */
#define MSML_KERNEL_MFM 2
const char* msml_conv2d_kernel(int c0p, int c1p, int coutp, int N, int H, int W, int P, int Q,
                               int R, int S, int stride, int pad_h, int pad_w, int transposed,
                               int in_dtype, int out_dtype, int want_stats);

/* Stem im2col (iresnet.py:209 conv1 / unet.py:193 on the 3-channel image): x NCHW f32 ->
 * out[N][P][Q][KP], k = (r*S + s)*C + c, zeros for k >= R*S*C and outside the image; the stem then
 * runs as a 1x1 conv over KP channels with the weight reordered to [Cout][R][S][C]. */
int msml_stem_im2col(const float* x, void* out, int N, int C, int H, int W, int P, int Q, int R,
                     int S, int stride, int pad, int KP, int dtype, void* stream);

/* Backward-data of a stem conv, to the image (the gradient autograd gives iresnet.py:209 `conv1`, unet.py:193 and
 * lightcnn.py:150 for their input): the adjoint of msml_stem_im2col + the 1x1 conv over the patches in ONE launch,
 *   dx[n][c][iy][ix] = sum over k, r, s of dy[n][oy][ox][k] * w[k][c][r][s],  iy = oy*stride - pad + r, ix = ox*stride - pad + s.
 *   dy [N][P][Q][ldy] bf16 or f32 (dtype), the first Cout channels real (the others are never read); w the parameter's
 *   own f32 OIHW [Cout][C][R][S] (bf16 dy: rounded to bf16 in LDS; f32 dy: used as it is); dx NCHW f32 [N][C][H][W],
 *   every element stored (no accumulate mode).  f32 accumulation; one writer per element and a fixed summation order:
 *   two runs give the same bits.
 *   Serves C in {1, 3}, R = S in {3, 5} with R*S*C <= 32, stride in {1, 2}, pad = R/2, Cout % 32 == 0 and <= 128,
 *   ldy >= Cout, ldy % 8 == 0, W <= 128, P / Q the conv's output size; anything else, a null pointer or a misaligned
 *   one (dy 16 bytes) returns MSML_ERR_SHAPE before any launch (another dtype: MSML_ERR_DTYPE).
 * msml_stem_bwd_data_band: input rows per workgroup of the bf16 kernel for such a shape (0: not served). */
int msml_stem_bwd_data(const void* dy, const float* w, float* dx, int N, int C, int H, int W, int P, int Q,
                       int Cout, int ldy, int R, int S, int stride, int pad, int dtype, void* stream);
int msml_stem_bwd_data_band(int C, int H, int W, int Cout, int R, int stride);

/* msml_bn_act_bwd_apply that also reduces the backward sums of the activation-free BatchNorm whose
 * output gradient the written dx is (chained IBasicBlocks: block i+1's bn1 input gradient is block
 * i's output gradient, i.e. the dy of block i's bn3, iresnet.py:65): next_x = that BatchNorm's
 * saved input, next_partial[msml_bn_act_bwd_apply_rows(M, C)][3][C]. */
int msml_bn_act_bwd_apply_rows(long M, int C);
int msml_bn_act_bwd_apply_next(const void* dy, const void* x, const float* scale, const float* shift,
                               const float* alpha, const float* save_mean, const float* save_invstd,
                               const float* partial, int rows, const void* add, void* dx,
                               float* dgamma, float* dbeta, float* dalpha, int accumulate, long M,
                               int C, float* coef_ws, const void* next_x, const float* next_mean,
                               const float* next_invstd, float* next_partial, int dtype, void* stream);

/* Training-mode BatchNorm (+ PReLU) -> 3x3 / stride-1 / pad-1 conv in ONE launch with accumulator-mode statistics on
 * both sides (bn1 -> conv1 and bn2 -> prelu -> conv2 of IBasicBlock, backbones/frb/iresnet.py:58-62): coefficients from
 * acc_in (double[8][2][c0p], the producer's sums) in the kernel prologue, the normalised input applied in LDS and written
 * to act_out (NHWC like in0; the weight gradient reads it), coef_out = float[4][c0p] (scale, shift, mean, invstd), running
 * statistics updated, the output's sums added to acc_out (zero-initialised double[8][2][coutp]).  Bit-identical to
 * msml_bn_fin_act_fwd + msml_conv2d_acc.  Shapes: msml_conv2d_bnin_acc_applies -- 1: served by the halo-tile conv, 3: by
 * the persistent 128-channel halo tile (round 6: 64 k input channels, 128 output channels, at least two rounds of tiles),
 * 0: not covered. */
int msml_conv2d_bnin_acc_applies(int c0p, int coutp, int N, int H, int W, int P, int Q, int R, int S, int stride,
                                 int pad_h, int pad_w);
int msml_conv2d_bnin_acc(const void* in0, int c0p, const double* acc_in, double count, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                         float* coef_out, const float* in_alpha, void* act_out, const void* wp, int kop, void* out,
                         int coutp, double* acc_out, int N, int H, int W, int P, int Q, int R, int S, int stride,
                         int pad_h, int pad_w, void* stream);

/* Block-level entry point: every launch of one IBasicBlock forward (backbones/frb/iresnet.py:56-67; the OSB encoder's
 * copy backbones/osb/unet.py:80-91) in the bf16 training path with accumulator-mode statistics, enqueued by ONE call:
 * bn1 -> conv1 -> bn2 + PReLU -> conv2 (stride) [-> downsample conv 1x1 -> its BatchNorm] -> bn3 + identity, i.e. the
 * sequence msml_bn_fin_act_fwd / msml_conv2d_acc the host otherwise issues launch by launch (same kernels, same order,
 * bit-identical results).  ptrs / ints / flts: tables indexed by the enums at the top of csrc/block.hip
 * (msml_iblock_fwd_tables returns their lengths); every pointer is a device pointer borrowed for the enqueue,
 * coefficient blocks are float[4][C] (scale, shift, mean, invstd), accumulators zero-initialised double[8][2][C]. */
int msml_iblock_fwd_tables(int* nptr, int* nint, int* nflt);
int msml_iblock_fwd(const void* const* ptrs, const int* ints, const float* flts, void* stream);

/* Box calibration probe (bench.py `calibration`, not part of the hot path): `wgs` workgroups of four waves run `iters`
 * rounds of 16 register-resident v_mfma_f32_16x16x32_bf16 on the random bf16 operands in seed[4096]; out[wgs * 256]
 * receives the accumulator sums.  2 * 16 * 16 * 32 * 16 * iters FLOP per wave.  The reference has no counterpart: its
 * benchmark prints images/sec only (train.py:303-318, utils/utils_callbacks.py). */
int msml_probe_mfma(const void* seed, float* out, int wgs, int iters, void* stream);
/* The same with every operand re-read from LDS in the mix of the halo-tile conv's main loop: `wgs` workgroups of eight
 * waves (two per SIMD), per round 9 ds_read_b128 fragments feed 14 MFMAs; iters even; out[wgs * 512].
 * 2 * 16 * 16 * 32 * 14 * iters FLOP per wave. */
int msml_probe_mfma_lds(const void* seed, float* out, int wgs, int iters, void* stream);

/* ---- LightCNN-29v2 FRB (backbones/frb/lightcnn.py) ------------------------------------------------ */

/* mfm (lightcnn.py:25-39): filter conv with 2C outputs + torch.max(z[:, :C], z[:, C:]) in one pass; resblock
 * (lightcnn.py:61-65) adds its input through `residual`.  wp: packed filter weight with interleaved output rows
 * (2k = channel k, 2k + 1 = channel k + C), kop >= the tile-rounded 2 * coutp; bias f32 [2 * coutp] in the same order;
 * out / residual NHWC [N][P][Q][coutp] (coutp = padded C; pad channels come out zero); sel u8 [N][P][Q][coutp]:
 * 0 tie, 1 first half larger, 2 second half larger, 3 unordered.  dtype: MSML_F32 or MSML_BF16 (in = out). */
int msml_conv2d_mfm(const void* in0, int c0p, const void* wp, int kop, const float* bias, void* out, int coutp,
                    const void* residual, unsigned char* sel, int N, int H, int W, int P, int Q, int R, int S,
                    int stride, int pad_h, int pad_w, int dtype, void* stream);

/* Backward of the max-feature-map (torch.max(a, b), lightcnn.py:39): dz [M][czp] in the filter's natural channel
 * order from dy [M][cp] and the selector of msml_conv2d_mfm: the larger input takes the gradient, a tie splits it
 * 0.5 / 0.5, an unordered pair (NaN) passes it to both; channels >= 2C of dz are written zero. */
int msml_mfm_bwd(const void* dy, const unsigned char* sel, void* dz, long M, int cp, int C, int czp, int dtype,
                 void* stream);

/* F.max_pool2d(x, 2) + F.avg_pool2d(x, 2) (lightcnn.py:211,216,221,228) on NHWC [N][H][W][cp], H and W even:
 * y [N][H/2][W/2][cp].  A NaN wins the max, as in torch. */
int msml_pool2_fwd(const void* x, void* y, int N, int H, int W, int cp, int dtype, void* stream);

/* Its backward: dx = 0.25 dy everywhere plus dy at the window's maximum (the first in row-major order; a NaN's
 * position if the window holds one), recomputed from x. */
int msml_pool2_bwd(const void* dy, const void* x, void* dx, int N, int H, int W, int cp, int dtype, void* stream);

/* ---------------------------------------------------------------- template (IJB-B / IJB-C) verification ------
 * Device side of eval/qeval_ijbc.py and of Verification.start_verification (eval/qeval_mxnet.py:422-483).
 * All sums in f64 in a fixed order, no floating-point atomics: two runs give the same bits.
 *
 * msml_template_pool: image2template_feature (eval/qeval_ijbc.py:303-337) with the flip sum and detector-score
 *   weighting of get_template_features (eval/qeval_ijbc.py:484-502) folded in.  feats [n_rows][ld] f32, the first E
 *   columns the embedding, columns E..2E the embedding of the flipped image when flip != 0; faceness [n_rows] f32
 *   or NULL.  order [n_rows]: image rows sorted by (template id, media id, row); media_start [n_media + 1]:
 *   positions in `order`; tmpl_media_start [n_templates + 1]: media indices; launch [n_templates]: the template
 *   each workgroup pools (any permutation; the host lists the largest templates first).  out [n_templates][E] f64,
 *   template rows in ascending id order: sum over the template's medias of the mean of (orig + flip) * faceness
 *   over the media's rows, L2-normalised by sklearn's rule (a zero row stays zero).  E a multiple of 4. */
int msml_template_pool(const float* feats, long n_rows, long ld, int E, int flip, const float* faceness,
                       const int* order, const int* media_start, const int* tmpl_media_start, const int* launch,
                       int n_templates, double* out, void* stream);
/* verification (eval/qeval_ijbc.py:343-369): score[i] = <tn[r1[i]], tn[r2[i]]> in f64; r1 / r2 are ROW indices (the
 * host maps template ids to rows, template2id of :350-352, and rejects unknown ids); a row index outside
 * 0..n_templates-1 gives NaN, never a read outside tn.  E even. */
int msml_template_pair_score(const double* tn, int n_templates, int E, const int* r1, const int* r2, long n_pairs,
                             double* score, void* stream);
/* roc_curve + TPR @ FPR table + auc (eval/qeval_ijbc.py:565-585; also roc_curve of eval/qeval_mxnet.py:433) on
 * integer counts.  sorted: the scores in DESCENDING order, label: their 0/1 labels, n < 2^31.
 *   msml_roc_block_counts: blk[msml_roc_blocks(n)][2] = {positives, ends of runs of equal scores} per block;
 *   msml_roc_points: off = the exclusive scan of blk (done by the caller on that small table) -> tps[k], fps[k] of
 *     the k-th distinct score (sklearn's _binary_clf_curve), k < n_points = the total of run ends;
 *   msml_roc_reduce: keep[k] = 1 where drop_intermediate=True keeps the point; part[msml_roc_reduce_blocks(n_points)]
 *     [2 + 2 * n_targets] 64-bit words per block: points kept, twice the trapezoid area under the block's segments
 *     in count units (exact), and per target FPR the bits of the smallest |fps / fps[last] - target| over the kept
 *     points with its k (ties: the larger k, min(zip(diff, index)) after flipud, :582-583).  n_targets <= 16. */
int msml_roc_blocks(int n);
int msml_roc_block_counts(const double* sorted, const unsigned char* label, int n, int* blk, void* stream);
int msml_roc_points(const double* sorted, const unsigned char* label, int n, const int* off, int* tps, int* fps,
                    void* stream);
int msml_roc_reduce_blocks(int n_points);
int msml_roc_reduce(const int* tps, const int* fps, int n_points, const double* target, int n_targets,
                    unsigned char* keep, unsigned long long* part, void* stream);
/* cdist(a, b, 'cosine') of the sklearn-normalised rows 2i, 2i + 1 (eval/qeval_mxnet.py:419,426-430): dist[i] =
 * 1 - a.b / (|a||b|) in f64, |cos| clipped to 1 as scipy does.  emb [2 * n_pairs][E], NOT normalised. */
int msml_pair_cosdist(const float* emb, int n_pairs, int E, double* dist, void* stream);
int msml_pair_cosdist_f64(const double* emb, int n_pairs, int E, double* dist, void* stream);
/* The counting loops of eval/qeval_mxnet.py:461-478 as rank queries: out[j] = number of sorted[i] < q[j]
 * (strict != 0) or <= q[j]; sorted ascending [n], q [m]. */
int msml_rank_count(const double* sorted, int n, const double* q, int m, int strict, int* out, void* stream);

/* ---------------------------------------------------------------- face alignment of the template evaluation ---
 * The per-image work of Embedding.get (eval/qeval_ijbc.py:145-187) after the transform estimate, for N decoded
 * sources of any size in one launch.
 *
 * msml_align_warp: cv2.warpAffine(rimg, M, (out_w, out_h), borderValue=0.0) (eval/qeval_ijbc.py:161-163) followed by
 *   cv2.cvtColor(BGR2RGB) (:164) when swap_rb != 0.  src: every source back to back, H x W x 3 uint8 with a row
 *   pitch; meta [N][4] int64 = {byte offset in src, H, W, pitch in bytes}, H and W in 1..32767 (the CALLER checks
 *   that every image lies inside src: the library cannot).  minv [N][6] f64: the INVERSE map (dst -> src), inverted
 *   on the host in OpenCV's order of operations.  dst [N][out_h][out_w][3] uint8, 4-byte aligned.  The arithmetic is
 *   that of OpenCV's classic warpAffine + remap (INTER_LINEAR, BORDER_CONSTANT 0), written out: adelta[x] =
 *   sat(rint(minv0 x 1024)), bdelta[x] with minv3; per row X0 = sat(rint((minv1 y + minv2) 1024)) + 16, Y0 with
 *   minv4, minv5; X = (X0 + adelta[x]) >> 5, Y likewise; source pixel (X >> 5, Y >> 5) clamped to int16, fractions
 *   X & 31, Y & 31; weights (32-fx)(32-fy)32, fx(32-fy)32, (32-fx)fy 32, fx fy 32 (sum 32768); a tap outside the
 *   image counts 0; result (sum + 16384) >> 15.  rint rounds half to even, sat clamps to int32 in f64 before the
 *   conversion, the integer additions wrap in 32 bits.  MSML_ERR_UNSUPPORTED before any launch for out_w % 4 != 0,
 *   out_h or out_w outside 4..256, N < 1.
 * msml_align_pairs: faces [N][H][W][3] uint8 RGB -> out [2N][3][H][W] f32: row 2i = (v / 255 - 0.5) / 0.5 in the three
 *   f32 steps of forward_db (eval/qeval_ijbc.py:192) of face i with the block of its descriptor painted black
 *   (RandomBlock, :166-173), row 2i + 1 its horizontal mirror (np.fliplr, :181-187).  desc: msml_occ_draw's 64-word
 *   descriptors or NULL; kind 0 (none) and kind 3 (block, words 1-4 = x0, y0, w, h) are accepted, any other kind
 *   fills the image's two rows with NaN.  W a multiple of 4. */
int msml_align_warp(const unsigned char* src, const long* meta, const double* minv, unsigned char* dst, int N,
                    int out_h, int out_w, int swap_rb, void* stream);
int msml_align_pairs(const unsigned char* faces, const int* desc, float* out, int N, int H, int W, void* stream);

/* ---------------------------------------------------------------- test.py evaluation inputs ------------------
 * msml_eval_pairs: the per-image loop of _load_one_input (eval/qeval_mxnet.py:173-189, run 2 x num times per
 *   extraction by start_extract, :302-312) and the normalisation of :319-324 for N decoded faces in one launch.
 *   src [N][H][W][3] uint8 RGB (one size per call), out [2N][C][out_h][out_w] f32 with C = 1 when gray, else 3: row 2i
 *   is image i, row 2i + 1 its mirrored copy.  Per row, in the reference's order:
 *   1. rows 2i + 1 only: transpose(FLIP_LEFT_RIGHT) of the SOURCE, before any crop (:175-176);
 *   2. CenterCrop((out_h, out_w)) (:178-180) with the arithmetic of torchvision's center_crop: an axis shorter than
 *      the output is first padded with zeros, (out - in) / 2 on the left / top and (out - in + 1) / 2 on the right /
 *      bottom; the crop origin of the other axes is int(round((in - out) / 2.0)) with Python's round (half to even:
 *      a difference of 1 gives 0, 3 gives 2, 5 gives 2), so mirror-then-crop is not crop-then-mirror;
 *   3. gray != 0: Grayscale() (:97-101), L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16;
 *   4. RandomBlock (:544-547, datasets/augment/rand_occ.py:43-72) from the row's descriptor desc[2i + f] (msml_occ_draw's
 *      64 words: kind 0 = none, kind 3 = block with words 1-4 = x0, y0, w, h in OUTPUT coordinates, cropped at the
 *      border as Image.paste crops; any other kind fills that row with NaN).  protocol 0 (BB): every row; protocol 1
 *      (NB, :184-187): rows of images with an odd global index index0 + i skip this step, descriptor unread.
 *      desc = NULL: no occlusion.  fill 0 black, 1 white (255), 2 gauss: every block pixel (every channel for RGB)
 *      draws a standard normal z = sqrt(-2 ln u1) cos(2 pi u2) in f64, u1 = (hi32(r) + 1) / 2^32, u2 = lo32(r) / 2^32,
 *      r = mix(mix(mix(seed + 0x6761757373) + 2 (index0 + i) + f) + ((y - y0) 256 + (x - x0)) 4 + channel) with
 *      mix = the splitmix64 step of msml_occ_draw.  The byte follows rand_occ.py:56-64.  RGB: (z * 255).astype(uint8),
 *      DEFINED here as truncation toward zero, then wrap modulo 256 (what numpy does on x86-64; the cast of a
 *      negative or out-of-range float to uint8 is otherwise undefined).  Gray: Image.paste of the mode-F block into
 *      the L image, which Pillow converts as: round z * 255 to f32; <= 0 gives 0, >= 255 gives 255, else truncate;
 *   5. ToTensor: v / 255 as one f32 division;
 *   6. norm != 0: sub_(0.5) then div_(0.5), two f32 steps (:319-324).
 *   No atomics, one writer per element: two runs give the same bits.  MSML_ERR_SHAPE for null src / out, misaligned
 *   pointers (src, desc 4 bytes, out 16) or index0 < 0; MSML_ERR_UNSUPPORTED before any launch for N < 1,
 *   out_w % 4 != 0, H, W, out_h or out_w outside 4..256, fill outside 0..2, protocol outside 0..1, and NB with gray
 *   (the reference's own NB path puts a 3-channel tensor into the 1-channel batch and raises). */
int msml_eval_pairs(const unsigned char* src, int N, int H, int W, const int* desc, float* out, int out_h, int out_w,
                    int gray, int norm, int fill, int protocol, long seed, long index0, void* stream);

/* ---------------------------------------------------------------- 1:N identification: fused top-k search -----
 * The search behind the identification lists the reference prepares and never evaluates: the MegaFace list
 * (datasets/benchmarks/get_list.py:138-208: 1 000 000 distractors under label 9999 plus FaceScrub probe / mate pairs),
 * the AR list (datasets/benchmarks/get_list.py:100-135) and the 1:N part of IJB-C on the pooled template features of
 * msml_template_pool.
 *
 * msml_search_topk: probe [P][E] and gallery [G][E], both row-major in `dtype` (MSML_F32 or MSML_F64), 16-byte aligned.
 *   For every probe row the k largest inner products with the gallery rows: scores [P][k] in `dtype`, index [P][k] the
 *   gallery rows, in descending score with ties by ascending gallery row (-0.0 and 0.0 are equal and tie): the order of
 *   np.lexsort((arange(G), -s)).  One workgroup owns 64 probe rows and one of `splits` ranges of gallery columns, runs
 *   the reduction over E on the 16x16x4 MFMA of the dtype and keeps per-row sorted lists of k entries in LDS; the
 *   P x G score matrix is never written.  splits > 1: every split writes its partial lists ((-inf, -1) fillers where it
 *   has fewer than k columns) to `workspace` ([splits][P][k] scores, then indices) and a second kernel merges them;
 *   splits == 1 writes the result directly, workspace may be NULL.  Every dot product is summed over the channels in
 *   ascending order by the same instructions whatever the split; no floating-point atomics, no workgroup waits for
 *   another: the result has the same bits for every `splits` and in every run.
 *   Limits: E % 4 == 0, 1 <= k <= 32, k <= G, 1 <= splits <= 65535, P and G below 2^31.  Every violation, a null
 *   pointer, a misaligned pointer, another dtype and a workspace smaller than msml_search_topk_workspace return
 *   MSML_ERR_SHAPE before any launch.  NaN scores are never listed: the caller checks its inputs.
 * msml_search_topk_splits: the default split count: enough workgroups to fill the part, never more than 64-column
 *   tiles, no empty split.  0 for P or G outside their limits.
 * msml_search_topk_workspace: bytes of `workspace` (8-byte aligned) for any dtype: splits * P * k * 12, 0 for one
 *   split. */
int msml_search_topk_splits(long P, long G, int k);
size_t msml_search_topk_workspace(long P, int k, int splits);
int msml_search_topk(const void* probe, long P, const void* gallery, long G, int E, int k, int splits, int dtype,
                     void* scores, int* index, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- all-pairs verification: TAR @ FAR ------------
 * The second protocol of the MegaFace list (datasets/benchmarks/get_list.py:138-208): TAR at a FAR target over EVERY
 * probe x gallery comparison, which the reference prepares and never evaluates.  The threshold of a target is an order
 * statistic of the impostor scores; msml_amd/allpairs.py finds it by a radix select on order-preserving keys, one
 * msml_allpairs_pass per level, and the P x G score matrix is never written.
 *
 * msml_allpairs_pass: probe [P][E] and gallery [G][E], row-major in `dtype` (MSML_F32 or MSML_F64), 16-byte aligned;
 *   probe_code [P] / gallery_code [G]: one non-negative int32 subject code per row.  The score of pair (p, g) is the
 *   inner product of the two rows with the bits msml_search_topk gives it (the same MFMA chain from a zero accumulator,
 *   channels ascending), -0.0 counted as 0.0; the pair is genuine when the codes are equal, an impostor otherwise.
 *   symmetric = 1: gallery and gallery_code are probe and probe_code themselves (G == P) and only the pairs p < g
 *   exist.  The key of a score has W = 32 (f32) or 64 (f64) bits: all bits of a negative flipped, the sign bit of a
 *   non-negative set, so keys order as scores do.  A range (prefix, bits) holds the keys with key >> (W - bits) ==
 *   prefix (bits = 0: all keys).  By `mode`:
 *   MSML_ALLPAIRS_HIST     for each of the n_ranges <= 16 ranges (range_prefix, range_bits: HOST arrays) the impostor
 *                          keys inside it are counted by their next bins_log2 bits into hist [n_ranges][1 << bins_log2]
 *                          (u64); range_bits[r] + bins_log2 <= W and n_ranges << bins_log2 <= 8192 (the workgroup's
 *                          LDS histogram, u32, flushed before a bin could overflow).
 *   MSML_ALLPAIRS_COLLECT  the impostor SCORES (in `dtype`) inside range r of the n_ranges <= 16 are appended to row r
 *                          of cand [n_ranges][cand_cap] in the order they arrive; cand_count [n_ranges] (u64) counts
 *                          every one of them, also those beyond cand_cap, which are not stored.
 *   MSML_ALLPAIRS_COUNT    counts [2][n_thr] (u64): the genuine, then the impostor pairs whose score widened to f64
 *                          is > thresholds[t] (HOST array of n_thr <= 16 doubles, no NaN).
 *   hist, cand_count and counts are ADDED to: the caller zeroes them.  Arguments of another mode are ignored and may
 *   be NULL / 0.  One workgroup owns 64 probe rows and one of `splits` ranges of gallery columns; rows beyond P,
 *   columns beyond G and channels beyond E are not counted.  All results are integer counts (or a set of scores), so
 *   the order of the atomics cannot change them: the same result for every `splits` and in every run.
 *   Limits: E % 4 == 0, 1 <= splits <= 65535, P and G below 2^31.  Every violation, a null or misaligned pointer
 *   (rows 16 bytes, codes 4, hist / cand / cand_count / counts 8) and another dtype or mode return MSML_ERR_SHAPE before
 *   any launch.  NaN scores are not defined: the caller checks its inputs.
 * msml_allpairs_splits: the default split count, as msml_search_topk_splits.  0 for P or G outside their limits. */
enum { MSML_ALLPAIRS_HIST = 0, MSML_ALLPAIRS_COLLECT = 1, MSML_ALLPAIRS_COUNT = 2 };
int msml_allpairs_splits(long P, long G);
int msml_allpairs_pass(const void* probe, long P, const int* probe_code, const void* gallery, long G,
                       const int* gallery_code, int E, int dtype, int symmetric, int mode, int n_ranges,
                       const unsigned long long* range_prefix, const int* range_bits, int bins_log2,
                       unsigned long long* hist, void* cand, unsigned long long* cand_count, long cand_cap,
                       const double* thresholds, int n_thr, unsigned long long* counts, int splits, void* stream);

/* ---------------------------------------------------------------- face detection: MTCNN --------------------------
 * The steps of MTCNN.detect_faces (eval/preprocess/mtcnn.py:160-274 with mtcnn_pytorch/src/first_stage.py, box_utils.py
 * and get_nets.py) between the packed uint8 sources of msml_align_warp (src, meta [N][4] = byte offset, H, W, pitch) and
 * the final boxes and landmarks; msml_amd/detect.py chains them.  A candidate is a ROW of 16 doubles:
 *   x1 y1 x2 y2 score | image | box offsets [4] (stages 1, 2) or landmarks x0..x4 y0..y4 [10] (stage 3).
 * All box arithmetic is f64 without contraction, in the reference's order of operations; the three nets are f32 FMA.
 *
 * msml_det_resample: jobs [njobs][8] (long, on the device) = image, x0, y0, w, h, out_w, out_h, output offset in floats.
 *   PIL Image.resize((out_w, out_h), BILINEAR) of the w x h window at (x0, y0) of the image, pixels outside the image
 *   black, bit for bit (Resample.c: triangle filter, support max(scale, 1), coefficients normalised in f64 and rounded
 *   to 22 bits, computed in the kernel; horizontal pass, clip, vertical pass, clip), then (x - 127.5) * 0.0078125 in
 *   f32, planar [3][out_h][out_w] at out + offset.  A job with w < 1 or h < 1 gives a black crop.  max_out_px: the
 *   largest out_w * out_h of the jobs (the launch grid).
 * msml_det_pnet: levels [L][6] (long) = input offset in floats, H, W, output offset in floats, oh, ow with
 *   oh = (H - 1) / 2 - 4; tiles [ntiles][3] (int) = level, tile row, tile column of msml_det_pnet_tile() square output
 *   tiles.  in: planar levels as msml_det_resample writes them; params: msml_det_pnet_params() floats, conv1 w b a,
 *   conv2 w b a, conv3 w b a, heads w [6][32] b [6] (conv4_1 then conv4_2).  out: planar [6][oh][ow] per level, the two
 *   class LOGITS then the four box offsets.  One fused launch, intermediates in LDS.
 * msml_det_candidates: rowtab [nrows][2] (int) = level, map row; scales [L] f64; images [L] (long).  The reference's
 *   softmax over the WIDTH of the class map (F.softmax(dim=-1) on [1][2][h][w]), channel 1 > threshold in f32.
 *   write = 0: counts [nrows] (long); write = 1: the candidates' rows at offsets [nrows] (the exclusive sum of counts),
 *   x ascending: np.where's order.  Boxes round((2 i + 1) / s), round((2 i + 13) / s), half to even.
 * msml_det_nms: box_utils.nms on every segment [seg_off[s], seg_off[s + 1]) of rows: descending score, among equal
 *   scores the HIGHER index first (np.argsort read from the end), overlap inter / (a + b - inter) or, mode_min = 1,
 *   inter / min(a, b), areas with the reference's + 1.0.  valid (may be NULL): rows with 0 take no part.  keep [n] (int)
 *   receives the picked global row indices of a segment in pick order at seg_off[s], -1 behind them; keep_cnt [nseg].
 *   order [n] (int) is scratch.  max_n: the longest segment, known to the caller from the stage's one count copy;
 *   max_n > capacity returns MSML_ERR_CAPACITY before any launch (capacity <= msml_det_nms_capacity()).
 * msml_det_compact: out[new_off[s] + k] = rows[keep[seg_off[s] + k]], k < keep_cnt[s].
 * msml_det_refine: calibrate_box with the row's offsets, convert_to_square (score := 0), np.round, correct_bboxes.
 *   jobs [n][8] receive the crop windows (the unclipped rounded box) for msml_det_resample at size x size; the row
 *   keeps the box CLIPPED to the image, which is what the reference's in-place views leave behind.  valid[i] = 0 and a
 *   black crop for a box with no pixel inside the image (the reference raises there), with a side of 32768 pixels or
 *   more, or with a coordinate that is not finite.
 * msml_det_net: net 0 = R-Net on [n][3][24][24], net 1 = O-Net on [n][3][48][48] -> out [n][16] = class logits,
 *   offsets [4], landmarks [10] (O-Net).  params: msml_det_net_params(net) floats in layer order, conv w b a, the FC
 *   weight as [In][Out] with Flatten's transpose(3, 2) folded in, heads as [In][16].  ws: msml_det_net_workspace bytes.
 * msml_det_select: valid[i] &= softmax(logits)[1] > threshold (f32); the row's score := that probability.
 *   landmarks = 0: offsets into the row; 1: landmarks xmin + width * l (f64, rounded to f32) then calibrate_box. */
int msml_det_pnet_tile(void);
int msml_det_pnet_params(void);
int msml_det_nms_capacity(void);
long msml_det_net_params(int net);
long msml_det_net_workspace(int net, long n);
int msml_det_resample(const unsigned char* src, const long* meta, const long* jobs, float* out, long njobs,
                      long max_out_px, void* stream);
int msml_det_pnet(const float* in, const long* levels, const int* tiles, const float* params, float* out, long ntiles,
                  void* stream);
int msml_det_candidates(const float* maps, const long* levels, const double* scales, const long* images,
                        const int* rowtab, long nrows, float threshold, int write, long* counts, const long* offsets,
                        double* rows, void* stream);
int msml_det_nms(const double* rows, const long* seg_off, const unsigned char* valid, long nseg, long max_n,
                 long capacity, double threshold, int mode_min, int* order, int* keep, int* keep_cnt, void* stream);
int msml_det_compact(const double* rows, const int* keep, const long* seg_off, const int* keep_cnt,
                     const long* new_off, double* out, long nseg, void* stream);
int msml_det_refine(double* rows, const long* meta, long n, int size, long* jobs, unsigned char* valid, void* stream);
int msml_det_net(int net, const float* in, const float* params, long n, float* ws, long ws_bytes, float* out,
                 void* stream);
int msml_det_select(double* rows, const float* net, long n, float threshold, int landmarks, unsigned char* valid,
                    void* stream);

/* ---------------------------------------------------------------- whole-photo uint8 operations ------------------
 * The oriented and resized copies MTCNN.align_fully and MTCNN.get_landmarks make of a photo before they detect
 * (eval/preprocess/mtcnn.py:41-158), for N packed images of any sizes in one call (msml_amd/mtcnn_align.py).  Source and
 * destination are packed as msml_align_warp takes its sources: meta [N][4] int64 = {byte offset, H, W, row pitch}, 3
 * bytes per pixel; the CALLER checks that every image lies inside its buffer.  In meta_out every offset and pitch is a
 * multiple of 4; the bytes between 3 W and the pitch are written as 0.  Integer arithmetic, no atomics, one writer per
 * output dword, dword stores only: two runs give the same bits.
 *
 * msml_img_orient: PIL Image.transpose(method), method[n] (int, on the device) = 0 FLIP_LEFT_RIGHT, 1 FLIP_TOP_BOTTOM,
 *   2 ROTATE_90, 3 ROTATE_180, 4 ROTATE_270; meta_out holds W x H images for 2 and 4.  src_bytes: the length of src (the
 *   source is read as aligned dwords, never past src_bytes).  plan [N][3] (long, on the HOST) = method, out_h, out_w,
 *   which the library checks: MSML_ERR_UNSUPPORTED before the launch for N < 1 or N > 65535, a method outside 0..4 and
 *   a size outside 1..32767; MSML_ERR_SHAPE for a null pointer and for src, dst, method not 4-byte or meta, meta_out not
 *   8-byte aligned.
 * msml_img_resize: PIL Image.resize((out_w, out_h), filter) on 3-channel uint8, filter 2 = BILINEAR, 3 = BICUBIC
 *   (a = -0.5): ImagingResample's two passes, horizontal then vertical on the rounded uint8 intermediate, each
 *   accumulator started at 2^21, shifted right by 22 and clipped to 0..255.  tables (int, device): per axis and per
 *   output position a row {first tap, taps, coefficients [ksize]} in 22-bit fixed point, built on the host in double
 *   (mtcnn_align.resample_rows, with the filter named here); jobs [N][5] (long, device) = offset of the horizontal table
 *   in ints, its ksize, offset of the vertical table, its ksize, byte offset of the image's intermediate in ws.  An axis
 *   of equal length takes the identity table (one tap of 2^22), which copies.  sizes [N][4] (long, HOST) = in_h, in_w,
 *   out_h, out_w.  ws: msml_img_resize_workspace(sizes, N) bytes, the intermediates [in_h][pitch of out_w] back to back
 *   (0 for a size outside 1..32767).  MSML_ERR_UNSUPPORTED before any launch for N < 1 or N > 65535, another filter,
 *   a size outside 1..32767; MSML_ERR_SHAPE for null or misaligned pointers (dst, ws, tables 4 bytes, meta, meta_out,
 *   jobs 8); MSML_ERR_WORKSPACE for a workspace that is too small. */
int msml_img_orient(const unsigned char* src, long src_bytes, const long* meta, const int* method, unsigned char* dst,
                    const long* meta_out, const long* plan, int N, void* stream);
long msml_img_resize_workspace(const long* sizes, int N);
int msml_img_resize(const unsigned char* src, const long* meta, unsigned char* dst, const long* meta_out,
                    const int* tables, const long* jobs, const long* sizes, int N, int filter, unsigned char* ws,
                    long ws_bytes, void* stream);

/* ---------------------------------------------------------------- baseline JPEG decoding -------------------------
 * mx.image.imdecode / cv2.imread on the device (datasets/load_dataset.py:106-174, eval/verification.py:202-236): N
 * baseline (SOF0, 8-bit, Huffman, one scan) streams of any sizes in one call, the same uint8 pixels libjpeg writes
 * with its defaults (JDCT_ISLOW, fancy upsampling).  The host parses the headers only (msml_amd/jpeg.py); the device
 * walks the entropy-coded bytes.  Integer arithmetic, no atomics, one writer per byte: two runs give the same bits.
 *
 *   streams: the packed byte strings, stream n at dword offset desc[n][0]; stream_bytes: the length of the buffer, a
 *     multiple of 4 (the device reads the streams as aligned dwords, none past the dword of a stream's last byte).
 *   desc / desc_host [N][32] int32: the same descriptors on the device and on the HOST (csrc/jpeg_core.h names the
 *     words: stream range, H, W, components, sampling, table selectors, restart interval, the parser's status, MCU
 *     counts, workspace offset).  The library checks desc_host before it launches: sizes in 1..32767, gray / 4:4:4 /
 *     4:2:2 / 4:2:0, table selectors below nq / nh, the stream inside stream_bytes, the workspace offsets those
 *     msml_jpeg_workspace wrote.  A descriptor whose status word is not 0 (a stream the parser refused) is not decoded.
 *   qtabs [nq][64] int32: quantisation tables in natural order; htabs [nh][832] int32: Huffman tables in lookup form.
 *   dst / meta_out [N][4] int64 (device) = byte offset, H, W, row pitch, as msml_align_warp takes its sources;
 *     channels 3 (R, G, B; B, G, R with swap_rb; a gray stream replicates Y) or 1 (gray streams only, one byte per
 *     pixel).  The device checks each row of meta_out against the stream's H and W and against dst_bytes; where offset
 *     and pitch are multiples of 4 the bytes between the row and its pitch are written as 0.
 *   status [N] int32: 0, or why image n was not decoded: 1 a code in no table, 2 a coefficient index past 63, 3 a DC
 *     category above 11 or an AC category above 10, 4 a restart marker missing or out of sequence, 5 data that ends
 *     before the last MCU, 6 a meta_out row that is not this image inside dst, 16.. the parser's reason.  Such an image
 *     leaves its output rectangle as it was; the other images are unaffected.  For ANY bytes the device reads only
 *     inside the stream's range and the tables and writes only the image's own workspace and rectangle.
 *   msml_jpeg_workspace(desc, N): on the HOST descriptors, writes each image's workspace offset into its descriptor
 *     and returns the bytes msml_jpeg_decode needs (0 for a descriptor it would refuse).
 *   MSML_ERR_UNSUPPORTED before any launch for N outside 1..65535, channels other than 1 or 3, a 3-component stream
 *   with channels 1; MSML_ERR_SHAPE for null or misaligned pointers (4 bytes; meta_out 8, ws 16) and an inconsistent
 *   descriptor; MSML_ERR_WORKSPACE for a workspace that is too small. */
long msml_jpeg_workspace(int* desc, int N);
int msml_jpeg_decode(const unsigned char* streams, long stream_bytes, const int* desc, const int* desc_host,
                     const int* qtabs, int nq, const int* htabs, int nh, unsigned char* dst, long dst_bytes,
                     const long* meta_out, int channels, int swap_rb, int* status, unsigned char* ws, long ws_bytes,
                     int N, void* stream);

/* ---------------------------------------------------------------- progressive JPEG decoding ----------------------
 * msml_jpeg_decode for a batch that may also hold progressive (SOF2, 8-bit, Huffman) streams, baseline and progressive
 * in any mix: the pixels libjpeg writes for a file whose scans bring every coefficient down to bit 0 (its inter-block
 * smoothing stays off for those; the host parser refuses every other progression).  Every argument msml_jpeg_decode
 * has means the same; the workspace is the same (msml_jpeg_workspace), and so are the two passes behind the
 * coefficients.  A progressive image is walked by one wavefront, scan after scan in file order.
 *
 *   desc word 22: the scans of image n (0: a baseline image, decoded as msml_jpeg_decode does), word 23: its first
 *     record in the scan table.
 *   scans / scans_host [nscan][16] int32: the same table on the device and on the HOST (csrc/jpeg_prog_core.h names the
 *     words: byte range of the entropy-coded segment, components, one Huffman table per component -- DC for Ss = 0,
 *     else AC --, Ss, Se, Ah, Al, the restart interval at that scan).  The library checks scans_host before it
 *     launches: records inside the table, at most 4096 per image, byte ranges inside the stream and in ascending
 *     order, component indices ascending and below the frame's, table indices below nh, 0 <= Ss <= Se <= 63, Se = 0
 *     with Ss = 0, one component when Ss > 0, Ah and Al in 0..13.  Whether the scans form a complete progression is
 *     the parser's question (msml_amd/jpeg.py): for ANY records that pass these checks the device reads only inside
 *     the byte ranges and the tables and writes only the image's own workspace and rectangle.
 *   status: as msml_jpeg_decode; 3 is also a refinement symbol whose size is not 1.
 *   MSML_ERR_SHAPE also for a null or misaligned scan table, nscan < 1, and inconsistent records. */
int msml_jpeg_decode_scans(const unsigned char* streams, long stream_bytes, const int* desc, const int* desc_host,
                           const int* scans, const int* scans_host, long nscan, const int* qtabs, int nq,
                           const int* htabs, int nh, unsigned char* dst, long dst_bytes, const long* meta_out,
                           int channels, int swap_rb, int* status, unsigned char* ws, long ws_bytes, int N,
                           void* stream);

/* ---------------------------------------------------------------- baseline JPEG encoding -------------------------
 * PIL.Image.save on the device (eval/align_dataset.py:52-75, iterate_pku.py) and the JPEG inside mx.recordio.pack_img
 * (datasets/3d_tools/cvt_casia_webface.py:57, cvt_casia_webface_masked.py:108-114): N images of any sizes, samplings,
 * qualities and restart intervals in one call, the bytes libjpeg writes for Pillow (JDCT_ISLOW, the standard Huffman
 * tables, no optimisation pass).  The host builds quantisation tables and header bytes (msml_amd/jpeg.py); the device
 * does the rest.  Integer arithmetic; the only atomics are integer ORs into a zeroed buffer: two runs give the same
 * bytes.  The mirror of msml_jpeg_decode.
 *
 *   src / meta [N][4] int64 (device) = byte offset, H, W, row pitch of each source, as msml_align_warp takes them (a
 *     contiguous [N][H][W][channels] tensor is the special case); channels 3 (R, G, B; B, G, R with swap_rb) or 1 (gray
 *     descriptors only).  A 3-channel source with a gray descriptor stores Y.
 *   desc / desc_host [N][12] int32: the same descriptors on the device and on the HOST (csrc/jpeg_enc_core.h names
 *     the words: sampling 0 gray / 1 4:4:4 / 2 4:2:2 / 3 4:2:0, H, W, the luma and chroma table selectors, the restart
 *     interval in MCUs, the header's offset and length in `headers`, the workspace offset).
 *   qtabs [nq][64] int32: quantisation tables in natural order; headers: the packed header bytes (SOI .. SOS).
 *   dst / out_meta [N][2] int64 (device) = byte offset and capacity of each image's slot; length [N] int32: the bytes
 *     written (0 for an image with a status).
 *   status [N] int32: 0, 1 a meta row that is not this image inside src, 2 a slot outside dst or too small.  Such an
 *     image writes nothing outside its own workspace and slot; the other images are unaffected, for ANY input bytes.
 *   msml_jpeg_encode_workspace(desc, N): on the HOST descriptors, writes each image's workspace offset into its
 *     descriptor and returns the bytes msml_jpeg_encode needs (0 for a descriptor it would refuse).
 *   msml_jpeg_encode_bound(H, W, sampling, restart, header_bytes): a slot capacity no stream can exceed (0 for
 *     arguments outside the range): at most 20 bits of DC and 63 x 26 bits of AC per block (rounded up to 208 bytes),
 *     doubled for stuffing, plus two bytes per restart interval, the header and EOI.  Typical output (photographs at
 *     quality 75-97) is 20-40 times smaller than this bound.
 *   MSML_ERR_UNSUPPORTED before any launch for N outside 1..65535, channels other than 1 or 3, a size outside
 *   1..32767, another sampling, channels 1 with a colour sampling; MSML_ERR_SHAPE for null or misaligned pointers (4
 *   bytes; meta, out_meta 8, ws 16) and an inconsistent descriptor; MSML_ERR_WORKSPACE for a workspace that is too
 *   small. */
long msml_jpeg_encode_workspace(int* desc, int N);
long msml_jpeg_encode_bound(int H, int W, int sampling, int restart, int header_bytes);
int msml_jpeg_encode(const unsigned char* src, long src_bytes, const long* meta, int channels, int swap_rb,
                     const int* desc, const int* desc_host, const int* qtabs, int nq, const unsigned char* headers,
                     long header_bytes, unsigned char* dst, long dst_bytes, const long* out_meta, int* length,
                     int* status, unsigned char* ws, long ws_bytes, int N, void* stream);

/* ---------------------------------------------------------------- PNG decoding -----------------------------------
 * PIL.Image.open(f).convert(mode) on the device (eval/qeval_folder.py:43-49, eval/align_dataset.py:44,
 * datasets/augment/rand_occ.py:345-366): N non-interlaced PNG streams of 1 / 2 / 4 / 8-bit samples, of any sizes and
 * colour types, in one call, the uint8 pixels Pillow gives for mode L / RGB / RGBA.  The host walks the chunks only
 * (msml_amd/png.py); the device inflates (zlib wrapper, stored / fixed / dynamic blocks, tables built on the device),
 * undoes the row filters and expands the samples.  Integer arithmetic, no global atomics, one writer per byte: two
 * runs give the same bits.  The mirror of msml_jpeg_decode; every argument it shares means the same.
 *
 *   streams: per image its IDAT payloads back to back (one zlib stream) at dword offset desc[n][0]; stream_bytes a
 *     multiple of 4 (aligned dword reads, none past the dword of a stream's last byte).
 *   desc / desc_host [N][16] int32: the same descriptors on the device and on the HOST (csrc/png_core.h names the
 *     words: stream range, H, W, bit depth, colour type, palette index, the parser's status, workspace offset, tRNS
 *     colour key).  The library checks desc_host before it launches.  A descriptor whose status word is not 0 is not
 *     decoded.
 *   palettes [palette_bytes / 1024][256][4] uint8: R, G, B, A of each distinct palette (PLTE + tRNS).
 *   dst / meta_out [N][4] int64 (device) = byte offset, H, W, row pitch; channels 4 (R, G, B, A), 3 (alpha dropped) or
 *     1 (gray and gray + alpha streams only); swap_rb exchanges R and B.  Where offset and pitch are multiples of 4
 *     the bytes between a row's end and its pitch are written as 0.
 *   status [N] int32: 0, 1 bad zlib header, 2 reserved block type, 3 stored-block length check, 4 bad code-length
 *     set or repeat, 5 bad literal/length or distance symbol, 6 distance before the start, 7 data ends early, 8 more
 *     data than the image holds, 9 Adler-32 mismatch, 10 filter byte above 4, 11 a meta_out row that is not this image
 *     inside dst, 12 reserved, 16.. the parser's reason.  Status 0 exactly when zlib inflates the stream to its end
 *     without an error and it holds H * (1 + row bytes) bytes.  An image with a status leaves its output rectangle as
 *     it was; the other images are unaffected.  For ANY bytes the device reads only inside the stream's range and the
 *     palettes and writes only the image's own workspace and rectangle.
 *   msml_png_workspace(desc, N): on the HOST descriptors, writes each image's workspace offset into its descriptor
 *     and returns the bytes msml_png_decode needs (0 for a descriptor it would refuse).
 *   MSML_ERR_UNSUPPORTED before any launch for N outside 1..65535, channels other than 1, 3, 4, a colour or palette
 *   stream with channels 1; MSML_ERR_SHAPE for null or misaligned pointers (4 bytes; meta_out 8, ws 16) and an
 *   inconsistent descriptor; MSML_ERR_WORKSPACE for a workspace that is too small. */
long msml_png_workspace(int* desc, int N);
int msml_png_decode(const unsigned char* streams, long stream_bytes, const int* desc, const int* desc_host,
                    const unsigned char* palettes, long palette_bytes, unsigned char* dst, long dst_bytes,
                    const long* meta_out, int channels, int swap_rb, int* status, unsigned char* ws, long ws_bytes,
                    int N, void* stream);

/* ---------------------------------------------------------------- PNG encoding -----------------------------------
 * PIL.Image.save of a .png name on the device (eval/align_dataset.py:52-75, the '.png' payloads of
 * datasets/3d_tools/cvt_casia_webface.py:35): N images of any sizes to N complete PNG files (signature, IHDR, one IDAT,
 * IEND) that Pillow, zlib and msml_png_decode read back to exactly the source pixels.  The bytes are not Pillow's: the
 * row filters are libpng's heuristic, the deflate stream is the device's own (one block per 65535 filtered bytes, each
 * the cheapest of stored / fixed / dynamic / dynamic with literals only).  Integer arithmetic, order-independent LDS
 * atomics only, one writer per output byte: two runs, and any batch composition, give the same bytes.  The mirror of
 * msml_jpeg_encode; every argument it shares means the same.
 *
 *   src / meta [N][4] int64 (device) = byte offset, H, W, row pitch; channels 1 (colour type 0), 2 (4: gray + alpha),
 *     3 (2) or 4 (6), 8-bit samples; swap_rb: the sources are B, G, R(, A) (channels 3 or 4 only).
 *   filter: 0 none, 1 sub, 2 up, 3 average, 4 Paeth for every row; 5 adaptive: per row the filter with the smallest sum
 *     of abs((int8) byte), ties to the lowest number.
 *   desc / desc_host [N][4] int32: the same descriptors on the device and on the HOST (H, W, workspace offset, 0).
 *   dst / out_meta [N][2] int64 (device) = byte offset and capacity of each image's slot; length [N] int32: the bytes
 *     written (0 for an image with a status).
 *   status [N] int32: 0, 1 a meta row that is not this image inside src, 2 a slot outside dst or too small, 3 an
 *     unsupported geometry (a size outside 1..32767 or more than 2^30 - 1 filtered bytes).  Such an image writes
 *     nothing outside its own workspace and slot; the other images are unaffected.
 *   msml_png_encode_ws_bytes(desc, channels, N): on the HOST descriptors, writes each image's workspace offset into its
 *     descriptor and returns the bytes msml_png_encode needs (0 for arguments it would refuse).
 *   msml_png_encode_bound(H, W, channels): the all-stored worst case, which no file exceeds (0 for an unsupported
 *     geometry): 8 signature + 25 IHDR + 12 IDAT overhead + 2 zlib header + n = H (W channels + 1) filtered bytes +
 *     5 ceil(n / 65535) stored-block headers + 4 Adler-32 + 12 IEND.
 *   MSML_ERR_UNSUPPORTED before any launch for N outside 1..65535, channels outside 1..4, a filter outside 0..5,
 *   swap_rb with fewer than 3 channels; MSML_ERR_SHAPE for null or misaligned pointers (4 bytes; meta, out_meta 8, ws
 *   16) and an inconsistent descriptor; MSML_ERR_WORKSPACE for a workspace that is too small. */
long msml_png_encode_ws_bytes(int* desc, int channels, int N);
long msml_png_encode_bound(int H, int W, int channels);
int msml_png_encode(const unsigned char* src, long src_bytes, const long* meta, int channels, int swap_rb, int filter,
                    const int* desc, const int* desc_host, unsigned char* dst, long dst_bytes, const long* out_meta,
                    int* length, int* status, unsigned char* ws, long ws_bytes, int N, void* stream);

/* ---------------------------------------------------------------- segmentation-branch evaluation -------------
 * Scores of the occlusion segmentation branch, which the reference only looks at by eye (train.py:357-364 saves
 * _seg.jpg beside _gt_occ.jpg, eval/qeval_mxnet.py:350-363 _learned.jpg beside _truth.jpg).  Integers only: no
 * floating-point sum anywhere, every run gives the same bits.
 *
 * A MASK argument is a pointer with a `kind`, one image size (H, W in 1..256) per call:
 *   MSML_SEG_LOGITS_F32 / MSML_SEG_LOGITS_BF16   logits [N][2][H][W], contiguous NCHW (final_seg).  A pixel is CLEAN
 *       iff channel 1 > channel 0, compared after widening to f32; ties and NaN are OCCLUDED -- train.py:357's
 *       final_seg.max(0)[1] (functional.mask_index);
 *   MSML_SEG_INDEX_U8 / MSML_SEG_INDEX_I64       an index mask [N][H][W]: 0 occluded, anything else clean.
 *   Another kind returns MSML_ERR_DTYPE, a null pointer MSML_ERR_SHAPE, N < 1 or a side outside 1..256
 *   MSML_ERR_UNSUPPORTED; every refusal of the three entry points comes before any launch.
 *
 * msml_seg_counts: the confusion counts the picture pairs of train.py:357 / eval/qeval_mxnet.py:350-363 would be
 *   compared by, in one launch.  pred: any mask kind; gt: an index mask.  counts int64 [N][4] = (tp, fp, fn, tn) per
 *   image, positive = OCCLUDED (tp: predicted occluded and truly occluded); total int64 [4] or NULL: the launch ADDS the
 *   sums over its N images to it (integer atomics: the order does not matter).  One workgroup per image; 16-byte loads
 *   for an image whose planes start on 16 bytes, with a scalar tail for H W % 8 != 0, and a scalar path for the others.
 *   MSML_ERR_SHAPE for counts / total not 8-byte aligned, MSML_ERR_DTYPE for a gt of logits.
 *
 * msml_seg_label: connected components of the OCCLUDED pixels of a mask -- the `blobs` the consensus loss is written
 *   over (tricks/consensus_loss.py:83).  connectivity 4 or 8.  labels int32 [N][H][W] or NULL: 0 on clean pixels, 1..K on
 *   the components, NUMBERED IN RASTER ORDER OF EACH COMPONENT'S FIRST PIXEL (scipy.ndimage.label's numbering);
 *   count int32 [N] = K; status int32 [N]: 0, or 2 for an image on which a loop reached its bound (count 0, labels 0:
 *   no input is known to reach it; the kernel never spins).  One workgroup per image, the parent plane of a union-find in
 *   LDS: rows seed their runs, atomicMin on the parent merges vertically adjacent runs, the roots are ranked by a
 *   prefix sum (docs/KERNELS.md).  MSML_ERR_UNSUPPORTED for H W > 16384 (64 KiB of LDS) and another connectivity.
 *
 * msml_seg_blob_table: per-component statistics of mask A against mask B.  labels / count: msml_seg_label's outputs for
 *   A; b: any mask kind.  table int32 [N][cap][6]: row k - 1 of image n = (area, hit, x0, y0, x1, y1) of A's component
 *   k: its pixel count, how many of those pixels are occluded in B, and its inclusive bounding box.  Rows from
 *   min(count, cap) on are zeros; count > cap is how a caller sees the overflow.  cap in 1..1024
 *   (MSML_ERR_UNSUPPORTED otherwise); labels outside 1..min(count, cap) are not counted. */
enum { MSML_SEG_LOGITS_F32 = 0, MSML_SEG_LOGITS_BF16 = 1, MSML_SEG_INDEX_U8 = 2, MSML_SEG_INDEX_I64 = 3 };
int msml_seg_counts(const void* pred, int pred_kind, const void* gt, int gt_kind, long* counts, long* total, int N, int H,
                    int W, void* stream);
int msml_seg_label(const void* mask, int kind, int* labels, int* count, int* status, int N, int H, int W,
                   int connectivity, void* stream);
int msml_seg_blob_table(const int* labels, const int* count, const void* b, int b_kind, int* table, int N, int H, int W,
                        int cap, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSML_HIP_H */
