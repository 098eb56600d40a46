// Weight gradient of 3x3 / stride-1 / pad-1 convs for bf16 NHWC tensors with Cout % 128 == 0 and
// Cin % 64 == 0 (the 28x28 / 14x14 stages of IResNet and of the OSB encoder,
// backbones/frb/iresnet.py:40-67) -- same math and slab format as wgrad_fast.hip /
// conv_wgrad.hip:   dW[a][tap][b] = sum_pixels dY[p][a] * X[p + tap][b].
//
// wgrad_fast gathers X once per tap (im2col) and is bound by the L2 -> LDS fill rate like the
// im2col conv.  Here a workgroup owns a 128 (Cout) x 64 (Cin) block of dW for ALL 9 taps and walks
// over strips of 7 x 14 output pixels: the dY strip (7 rows x 16-pixel pitch, the 2 padding
// pixels of a row are zero) and the X strip WITH its halo (9 rows x 16) go to LDS once and serve
// the 9 taps -- 48 KB of fill per 16.5 MFLOP (the im2col kernel: 32 KB per 2.1 MFLOP).  A k-step is
// one strip row (16 pixels); tap (r, s) reads the X image r rows down and s pixels right, which
// is a per-lane offset in the blocked image [row][32-channel group][16 px][64 B] (the layout
// whose transposing ds_read_b64_tr_b16 blocks are conflict-free, see wgrad_fast.hip).
// 8 waves.  128-row tile: wave = (one of four 32-row Cout tiles, 32-column Cin half) with all 9 taps: 9 accumulator
// tiles; a k-step reads one dY fragment and the three X fragments (column shifts 0, 1, 2) of halo row j + 2 -- rows j
// and j + 1 are still in registers from the two k-steps before -- for 9 MFMAs: 34 fragment reads per strip and wave.
// 64-row tile: wave = (32-row Cout tile, Cin half, tap group {0-4} / {5-8}): 5 or 4 accumulator tiles, 1 dY + 5 (4) X
// fragments per k-step.  Waves w and w + 4 share a SIMD; every SIMD runs 18 (64-row tile: 9) MFMAs per k-step.
// The strips are double-buffered: strip s + 1 is requested (LDS-DMA) at the top of strip s and must land behind the
// MFMAs of strip s, see wh_dma16.
#include <stdlib.h>

#include <type_traits>

#include <mutex>

#include "common.h"
#include "options.h"
#include "wgrad_call.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) void* lptr_t;

#define WH_OOB 0x78000000u

// One 1-KB LDS-DMA block (16 B per lane).  Issued from an asm statement so that hipcc does not count it: after a
// __builtin_amdgcn_raw_ptr_buffer_load_lds it cannot tell the ring slots apart and puts s_waitcnt vmcnt(0) in front of
// the next ds_read -- the strip requested at the top of the loop then lands BEFORE the first fragment read of the
// current strip instead of behind its MFMAs.  The kernel waits for these requests itself (wh_dma_wait) before the
// barrier that publishes a slot.  M0 (the LDS destination) belongs to the compiler: saved and restored.
typedef __attribute__((ext_vector_type(4))) unsigned int wh_rsrc_t;
__device__ __forceinline__ void wh_dma16(const wh_rsrc_t& rs, unsigned int lds, unsigned int off) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned int keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(off), "s"(rs), "s"(lds)
               : "memory");
#endif
}
__device__ __forceinline__ void wh_dma_wait() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}

struct WgradHaloArgs {
  const unsigned short* u[WGRAD_MAXGROUP]; int up; unsigned int u_bytes;     // dY [N][H][W][up], one per grouped layer
  const unsigned short* v[WGRAD_MAXGROUP]; int vp; unsigned int v_bytes;     // X  [N][H][W][vp]
  int N, H, W, spy, spx;      // dY map; strips per image column / row (7 rows x 14 columns each)
  int XH, XW;                 // unused (the removed stride-2 variant's input map): keeps the offsets of the fields below
  int nstrips, chunk;         // total strips, strips per split
  int zper;                   // splits per layer: grid.z = layers x zper, z = layer * zper + split
  int remap;                  // 1: XCD-aware workgroup order (all dW tiles of one z on one XCD's L2)
  int pair7;                  // 7 x 7 maps: a strip = TWO images side by side (columns 0-6 | gap | 8-14): the P7 instantiation
  float* ws;                  // [z][up][9][vp]
  BnIn xin;                   // xin.scale != nullptr: X is PReLU(v * scale + shift), applied in LDS (common.h)
};

// CO = Cout rows per workgroup: 128 (a wave carries a pair of 32-row tiles) or 64 (one tile)
// XF: the conv input X is a BatchNorm(+PReLU) of the stored tensor v; the strips are normalised in LDS
// P7: 7 x 7 maps, a strip = two images side by side (issue()); compile-time, the 128-row instantiation has no register
// to spare (a run-time switch spilled three dwords: 940 -> 595 TFLOP/s on the 14 x 14 layers)
template <int CO, bool XF = false, bool P7 = false>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) k_wgrad_halo(const WgradHaloArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NXB = 20;                              // X blocks of 1 KB per strip
  constexpr int GU = CO / 32, NI = CO / 64, UBLK = 7 * GU, NBLK = UBLK + NXB, NISS = (NBLK + 7) / 8;
  constexpr int UB = UBLK * 1024, VB = NXB * 1024, STAGE = UB + VB;      // dY strip, X strip + halo (+ 1 row)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  MSML_LDS_REGION(smem, 2 * STAGE + (XF ? 3 * 64 * 4 : 0));
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  // 128-row tile: wave = (one of four 32-row Cout tiles, Cin half), all nine taps; the X fragments of a halo row are
  // read once and serve three k-steps from registers.  64-row tile: wave = (Cout tile, Cin half, tap group).
  constexpr bool R9 = CO == 128;
  const int mp = R9 ? (wave & 3) : (wave & 1), nh = R9 ? (wave >> 2) : ((wave >> 1) & 1), tg = R9 ? 0 : (wave >> 2);
  // Several layers of one shape share a launch (grid.z = layers x zper): the split-K slab traffic per layer falls
  // with the number of workgroups a layer gets.  XCD-aware order: hardware deals consecutive workgroups round-robin
  // to the 8 XCDs; re-numbering them so that the gx * gy dW tiles of one z (same dY / X strips) sit on ONE XCD
  // makes their operand re-reads L2 hits.
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (p.remap) {
    const int T = gridDim.x * gridDim.y, total = T * gridDim.z;
    const int L = bx + gridDim.x * (by + gridDim.y * bz);
    const int Lp = (L & 7) * (total >> 3) + (L >> 3);
    const int tile = Lp % T;
    bz = Lp / T;
    bx = tile % gridDim.x;
    by = tile / gridDim.x;
  }
  const int layer = __builtin_amdgcn_readfirstlane(bz / p.zper);
  const int a0 = bx * CO, b0 = by * 64, split = bz - layer * p.zper;
  const int s_begin = split * p.chunk;
  int s_end = s_begin + p.chunk;
  if (s_end > p.nstrips) s_end = p.nstrips;
  const int spi = p.spy * p.spx;

  auto make_rsrc = [](const void* ptr, unsigned int bytes) -> wh_rsrc_t {
    const unsigned long long a = (unsigned long long)ptr;
    wh_rsrc_t r;
    r[0] = __builtin_amdgcn_readfirstlane((unsigned int)a);
    r[1] = __builtin_amdgcn_readfirstlane((unsigned int)(a >> 32) & 0xffffu);
    r[2] = __builtin_amdgcn_readfirstlane(bytes);
    r[3] = 0x00020000u;
    return r;
  };
  const wh_rsrc_t rs_u = make_rsrc(p.u[layer], p.u_bytes), rs_v = make_rsrc(p.v[layer], p.v_bytes);
  const unsigned int lds0 = __builtin_amdgcn_readfirstlane((unsigned int)(size_t)(lptr_t)smem);
  auto dma = [&](const wh_rsrc_t& rs, const char* dst, unsigned int off) {
    wh_dma16(rs, lds0 + (unsigned int)__builtin_amdgcn_readfirstlane((int)(dst - smem)), off);
  };

  // DMA slot of a lane inside a 1-KB block [16 px][64 B]: pixel lane / 4, 16-B chunk lane % 4
  const int lp = lane >> 2, lc = lane & 3;
  // 7 x 7 maps (pair7): a strip is the PAIR of images 2 strip, 2 strip + 1 laid side by side on the 16-pixel pitch:
  // dY columns 0-6 = image A, 7 = zero, 8-14 = image B, 15 = zero; X halo columns 0 = zero, 1-7 = A, 8 = zero (A's right
  // and B's left padding at once), 9-15 = B, and "column 16" of a row is column 0 of the next one = zero.  Every tap
  // offset of the k loop below then reads exactly the pixels a 7 x 7 conv with zero padding reads: 14 real k-values
  // of 16 per strip row, as on the 14-wide maps, with no change to the MFMA loop.
  auto issue = [&](int strip, int buf) {
    char* ub = smem + buf * STAGE;
    char* vb = ub + UB;
    if constexpr (P7) {
      const int n = 2 * strip + (lp >> 3), x = lp & 7;  // image of the pair, column inside it (7 = the zero gap)
      const bool img = n < p.N;
#pragma unroll
      for (int i = 0; i < NISS; i++) {
        const int blk = wave + 8 * i;
        if (blk >= NBLK) break;
        if (blk < UBLK) {
          const int j = blk / GU, g = blk % GU;
          const unsigned int off = (img & (x < 7)) ? (unsigned int)((n * 7 + j) * 7 + x) * (unsigned int)(p.up * 2) +
                                                         (unsigned int)(a0 + g * 32 + lc * 8) * 2u
                                                   : WH_OOB;
          dma(rs_u, ub + blk * 1024, off);
        } else {
          const int bb = blk - UBLK, hr = bb >> 1, g = bb & 1;
          const int y = hr - 1;                          // halo columns 0 and 8 (x == 0) are the zero padding
          const bool ok = img & ((unsigned)y < 7u) & (x > 0);
          const unsigned int off = ok ? (unsigned int)((n * 7 + y) * 7 + x - 1) * (unsigned int)(p.vp * 2) +
                                            (unsigned int)(b0 + g * 32 + lc * 8) * 2u
                                      : WH_OOB;
          dma(rs_v, vb + bb * 1024, off);
        }
      }
      return;
    }
    const int n = strip / spi, rem = strip - n * spi, sy = rem / p.spx;
    const int y0 = sy * 7, x0 = (rem - sy * p.spx) * 14;
#pragma unroll
    for (int i = 0; i < NISS; i++) {
      const int blk = wave + 8 * i;                    // 7 GU dY blocks, then 20 X blocks
      if (blk >= NBLK) break;
      if (blk < UBLK) {
        const int j = blk / GU, g = blk % GU;
        const int y = y0 + j, x = x0 + lp;
        const bool ok = (lp < 14) & (x < p.W) & (y < p.H);
        const unsigned int off = ok ? (unsigned int)((n * p.H + y) * p.W + x) * (unsigned int)(p.up * 2) +
                                          (unsigned int)(a0 + g * 32 + lc * 8) * 2u
                                    : WH_OOB;
        dma(rs_u, ub + blk * 1024, off);
      } else {
        const int bb = blk - UBLK, hr = bb >> 1, g = bb & 1;
        const int y = y0 + hr - 1, x = x0 + lp - 1;
        const bool ok = (hr < 9) & ((unsigned)y < (unsigned)p.H) & ((unsigned)x < (unsigned)p.W);
        const unsigned int off = ok ? (unsigned int)((n * p.H + y) * p.W + x) * (unsigned int)(p.vp * 2) +
                                          (unsigned int)(b0 + g * 32 + lc * 8) * 2u
                                    : WH_OOB;
        dma(rs_v, vb + bb * 1024, off);
      }
    }
  };

  float* xtab = reinterpret_cast<float*>(smem + 2 * STAGE);    // XF: [3][64] scale, shift, alpha of channels b0 ..
  // XF: every wave normalises the X chunks it DMA'd itself (after its own vmcnt wait); padding stays zero
  auto xform = [&](int strip, int buf) {
    const int n = strip / spi, rem = strip - n * spi, sy = rem / p.spx;
    const int y0 = sy * 7, x0 = (rem - sy * p.spx) * 14;
    char* vb = smem + buf * STAGE + UB;
    const bool has_alpha = p.xin.alpha != nullptr;
#pragma unroll
    for (int i = 0; i < NISS; i++) {
      const int blk = wave + 8 * i;
      if (blk >= NBLK) break;
      if (blk >= UBLK) {
        const int bb = blk - UBLK, hr = bb >> 1, g = bb & 1;
        const int y = y0 + hr - 1, x = x0 + lp - 1;
        if ((hr < 9) & ((unsigned)y < (unsigned)p.H) & ((unsigned)x < (unsigned)p.W))
          bn_in_chunk(vb + bb * 1024 + lane * 16, xtab, 64, g * 32 + lc * 8, has_alpha);
      }
    }
  };

  constexpr int NA = R9 ? 1 : NI, NK = R9 ? 9 : 5;
  f32x16 acc[NA][NK];                                  // [Cout tile of the wave][tap of the group]
#pragma unroll
  for (int i = 0; i < NA; i++)
#pragma unroll
    for (int k = 0; k < NK; k++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][k][e] = 0.f;

  // transposing fragment read (wgrad_fast.hip): the lane addresses pixel px = 8 (g4 >> 1) + q4 (the
  // second read 4 pixels on), 4 channels pp of a 16-channel half g4 & 1
  const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, pp = i16 & 3;
  const int px = 8 * (g4 >> 1) + q4;
  const int chan = (2 * (g4 & 1) + (pp >> 1)) * 16 + (pp & 1) * 8;
  const int aofs = mp * NA * 1024 + px * 64 + chan;    // + row * GU KB, + 1024 for a pair's second tile (+ 256: second read)
  // X: pixel px + s of halo row (row + r); past pixel 15 it continues in the next row's block
  int vlo[3], vhi[3];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const int p0 = px + s, p1 = px + 4 + s;
    vlo[s] = nh * 1024 + (p0 >> 4) * 2048 + (p0 & 15) * 64 + chan;
    vhi[s] = nh * 1024 + (p1 >> 4) * 2048 + (p1 & 15) * 64 + chan;
  }
  // offsets of this wave's taps (wave-uniform choice among the three column shifts, row shift folded in)
  const int ntaps = R9 ? 9 : (tg == 0 ? 5 : 4), tap0 = tg * 5;
  int vlok[5], vhik[5];
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const int tp = tap0 + k, r = tp / 3, sft = tp - r * 3;
    vlok[k] = r * 2048 + (sft == 0 ? vlo[0] : (sft == 1 ? vlo[1] : vlo[2]));
    vhik[k] = r * 2048 + (sft == 0 ? vhi[0] : (sft == 1 ? vhi[1] : vhi[2]));
  }
  typedef __attribute__((address_space(3))) s16x4* tr_ptr;
  auto tr2 = [&](const char* lo, const char* hi) -> s16x8 {
    s16x4 l = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr)(lo));
    s16x4 h = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr)(hi));
    s16x8 o;
    o[0] = l[0]; o[1] = l[1]; o[2] = l[2]; o[3] = l[3];
    o[4] = h[0]; o[5] = h[1]; o[6] = h[2]; o[7] = h[3];
    return o;
  };

  if (s_begin < s_end) issue(s_begin, 0);
  if (XF) bn_in_fill(p.xin, xtab, b0, 64, t, 512);
  wh_dma_wait();
  __syncthreads();
  if (XF) {
    if (s_begin < s_end) xform(s_begin, 0);
    __syncthreads();
  }
  int cur = 0;
  s16x8 fa[2][NA], fb5[2][5], xr[4][3];
  for (int strip = s_begin; strip < s_end; strip++) {
    if (strip + 1 < s_end) issue(strip + 1, cur ^ 1);
    const char* ub = smem + cur * STAGE + aofs;
    const char* vb = smem + cur * STAGE + UB;
    if constexpr (R9) {
      // k-step j multiplies dY row j with X halo rows j, j + 1, j + 2 at the three column shifts; rows j and j + 1
      // are the registers read one and two k-steps ago (xr[row & 3], the loop is unrolled: renaming, no moves).
      // dY row j + 1 and X row j + 3 are requested before the MFMAs of k-step j.
      auto fetch_a = [&](int j) { fa[j & 1][0] = tr2(ub + j * (GU * 1024), ub + j * (GU * 1024) + 256); };
      auto fetch_x = [&](int row) {
#pragma unroll
        for (int sft = 0; sft < 3; sft++) xr[row & 3][sft] = tr2(vb + row * 2048 + vlo[sft], vb + row * 2048 + vhi[sft]);
      };
      fetch_a(0);
      fetch_x(0);
      fetch_x(1);
      fetch_x(2);
#pragma unroll
      for (int j = 0; j < 7; j++) {
        if (j + 1 < 7) {
          fetch_a(j + 1);
          fetch_x(j + 3);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 9; k++)
          acc[0][k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[j & 1][0]),
                                                              __builtin_bit_cast(bf16x8, xr[(j + k / 3) & 3][k % 3]),
                                                              acc[0][k], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (XF && j == 6 && strip + 1 < s_end) {         // (as below: the next strip's own X chunks, normalised in LDS)
          wh_dma_wait();
          xform(strip + 1, cur ^ 1);
        }
      }
      wh_dma_wait();
      __syncthreads();
      cur ^= 1;
      continue;
    }
    // taps tap0 + k, k < ntaps, of this wave's group.  All fragments of k-step j + 1 are requested
    // before the MFMAs of k-step j (register double buffer); the fences keep hipcc from sinking the
    // reads next to their MFMAs.
    auto fetch = [&](int j, int fb) {
#pragma unroll
      for (int i = 0; i < NA; i++)
        fa[fb][i] = tr2(ub + j * (GU * 1024) + i * 1024, ub + j * (GU * 1024) + i * 1024 + 256);
#pragma unroll
      for (int k = 0; k < 5; k++)
        if (k < ntaps) fb5[fb][k] = tr2(vb + j * 2048 + vlok[k], vb + j * 2048 + vhik[k]);
    };
    fetch(0, 0);
#pragma unroll
    for (int j = 0; j < 7; j++) {                      // k-step = strip row j (16 pixels)
      const int fb = j & 1;
      if (j + 1 < 7) fetch(j + 1, fb ^ 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < 5; k++)
        if (k < ntaps) {
#pragma unroll
          for (int i = 0; i < NA; i++)
            acc[i][k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[fb][i]),
                                                                __builtin_bit_cast(bf16x8, fb5[fb][k]), acc[i][k], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
      // next strip's X chunks (requested at the top of this strip).  The 128-row variant has no
      // registers to spare while fragments are live, so it waits for the last k-step (the VALU
      // work then runs in the shadow of the MFMAs just issued).
      if (XF && j == (CO == 128 ? 6 : 2) && strip + 1 < s_end) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        xform(strip + 1, cur ^ 1);
      }
    }
    wh_dma_wait();
    __syncthreads();
    cur ^= 1;
  }

  // slab [z][a][tap][b] (k_wgrad_reduce sums the zper splits of a layer in a fixed order)
  const int h = lane >> 5, c32 = lane & 31;
  const int b = b0 + nh * 32 + c32;
#pragma unroll
  for (int i = 0; i < NA; i++)
#pragma unroll
    for (int k = 0; k < NK; k++) {
      if (k >= ntaps) continue;
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int a = a0 + (mp * NA + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        p.ws[(((long)bz * p.up + a) * 9 + tap0 + k) * p.vp + b] = acc[i][k][e];
      }
    }
#endif
}

// splits for a shape (0 = shape not covered by this kernel)
// 128-row dW tiles halve the operand traffic per FLOP; 64-row tiles halve the split-K slab bytes
// (measured at 256 -> 256 @ 14x14: 97 us with 128-row tiles, 104 us with 64-row tiles)
static bool wh_wide(int up) {
  const int lim = msml_opt().wgrad_halo_wide_min;
  return up % 128 == 0 && up >= lim;
}

static bool wh_pair7(const WgradShape& s) { return s.H == 7 && s.W == 7; }    // two 7 x 7 images per strip

// (image-pair strips: 64-row tiles only -- the 128-row instantiation of that variant spills)
int msml_wgrad_halo_variant(const WgradShape& s) {
  return wh_pair7(s) ? WGRAD_HALO_PAIR7 : wh_wide(s.up) ? WGRAD_HALO_128 : WGRAD_HALO_64;
}

// `group` layers of this shape share one launch: every layer gets 1 / group of the splits of a one-layer launch
int msml_wgrad_halo_applies(const WgradShape& s) {
  const bool off = msml_opt().no_halo_wgrad;
  if (off) return 0;
  if (s.R != 3 || s.S != 3 || s.stride != 1 || s.pad_h != 1 || s.pad_w != 1 || s.P != s.H || s.Q != s.W) return 0;
  if (s.up % 64 != 0 || s.vp % 64 != 0 || s.A != s.up || s.Breal != s.vp) return 0;
  if (wh_pair7(s) && s.bnin) return 0;               // (no in-LDS BatchNorm variant of the image-pair strips)
  const bool pair7 = wh_pair7(s) && !msml_opt().wgrad_halo_no_pair7;
  const long strips = pair7 ? (s.N + 1) / 2 : (long)s.N * cdiv(s.H, 7) * cdiv(s.W, 14);
  if ((long)s.N * s.H * s.W * 10 < strips * 112 * 7) return 0;     // < 70 % real k-values
  if ((long)s.N * s.H * s.W * s.up * 2 >= 0x70000000L || (long)s.N * s.H * s.W * s.vp * 2 >= 0x70000000L) return 0;
  const int tiles = s.up / (msml_wgrad_halo_variant(s) == WGRAD_HALO_128 ? 128 : 64) * (s.vp / 64);
  long splits = msml_num_cus() / tiles;                      // one resident workgroup per CU
  if (splits < 1) splits = 1;
  if (splits > strips) splits = strips;
  if (splits > WGRAD_MAXSPLITS) splits = WGRAD_MAXSPLITS;
  if (s.group < 1 || s.group > WGRAD_MAXGROUP) return 0;
  return (int)splits / s.group;
}

// (this family takes one completion only: V on the grid of U, stride 1, pad 1, every stored channel real)
int msml_wgrad_halo_max_splits(const WgradShape& s) {
  WgradShape h = s;
  h.H = s.P; h.W = s.Q; h.stride = h.pad_h = h.pad_w = 1; h.A = s.up; h.Breal = s.vp; h.group = 1; h.bnin = 0;
  return msml_wgrad_halo_applies(h);
}

template <int CO, bool XF, bool P7 = false>
static void wh_launch(const WgradHaloArgs& a, dim3 grid, hipStream_t st) {
  // two stages of (7 dY row blocks per 32 Cout + 10 X rows x 2 channel groups) KB (+ coefficient table)
  const size_t lds = 2 * (7 * (CO / 32) + 10 * 2) * 1024 + (XF ? 3 * 64 * sizeof(float) : 0);
  static std::once_flag attr_once;                     // (per template instantiation; launches come from
  std::call_once(attr_once, [&] {                      //  the forward thread AND the autograd thread)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wgrad_halo<CO, XF, P7>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  });
  k_wgrad_halo<CO, XF, P7><<<grid, dim3(512), lds, st>>>(a);
}

// slabs land in ws[(layer * splits + split)][up][9][vp]
void msml_wgrad_halo_launch(const WgradCall& c, const WgradPlan& p) {
  const bool no_remap = msml_opt().wgrad_halo_no_remap;
  const int up = c.up, vp = c.vp, N = c.N, H = c.H, W = c.W;
  WgradHaloArgs a;
  for (int i = 0; i < WGRAD_MAXGROUP; i++) {
    a.u[i] = (const unsigned short*)c.u[i < c.group ? i : 0];
    a.v[i] = (const unsigned short*)c.v[i < c.group ? i : 0];
  }
  a.up = up; a.u_bytes = (unsigned int)((long)N * H * W * up * 2);
  a.vp = vp; a.v_bytes = (unsigned int)((long)N * H * W * vp * 2);
  a.N = N; a.H = H; a.W = W; a.spy = cdiv(H, 7); a.spx = cdiv(W, 14);
  a.pair7 = p.variant == WGRAD_HALO_PAIR7 ? 1 : 0;
  a.nstrips = a.pair7 ? (N + 1) / 2 : N * a.spy * a.spx;
  a.chunk = cdiv(a.nstrips, p.splits);
  a.zper = p.splits;
  a.ws = c.ws;
  a.xin = BnIn{nullptr, nullptr, nullptr};
  if (c.xin) a.xin = *c.xin;
  const int gz = c.group * p.splits;
  const int co = p.variant == WGRAD_HALO_128 ? 128 : 64;
  a.remap = (!no_remap && (up / co) * (vp / 64) >= 4 && gz % 8 == 0) ? 1 : 0;
  const dim3 grid(up / co, vp / 64, gz);
  if (a.pair7) wh_launch<64, false, true>(a, grid, c.st);
  else if (co == 128 && c.xin) wh_launch<128, true>(a, grid, c.st);
  else if (co == 128) wh_launch<128, false>(a, grid, c.st);
  else if (c.xin) wh_launch<64, true>(a, grid, c.st);
  else wh_launch<64, false>(a, grid, c.st);
}
