// Device input pipeline: occlusion synthesis + flip + Gaussian light +
// normalisation on the GPU, producing (img, msk, ori) from decoded uint8 faces.
//
// Replaces the per-sample CPU work of FaceByRandOccMask.__getitem__ (datasets/load_dataset.py:101-139):
//   _get_occluded_face_and_mask  -> RandomRect (datasets/augment/rand_occ.py:103-139), RandomEllipse
//                                   (:148-203, analytic ellipse instead of cv2's rasteriser), RandomConnectedPolygon
//                                   (:217-322, even-odd point-in-polygon test instead of cv2.fillPoly), NoneOcc
//                                   (:80-90), RandomBlock (:43-72, evaluation)
//   random horizontal flip       -> load_dataset.py:119-123
//   _add_gauss_to_face           -> load_dataset.py:183-201 with _get_gauss :282-339 (Euclidean, radius 128)
//   Msk2Tenser / Normalize       -> mask 0 = occluded, 1 = clean (load_dataset.py:37); (x - 0.5) / 0.5
//   RandomGlasses / RandomGlassesList (rand_occ.py:337-428), RandomScarf (:431-517), RandomRealObject (:520-600):
//                                   texture occluders pasted from a CALLER-SUPPLIED RGBA atlas (the reference's PNGs are
//                                   read from the user's checkout at run time, msml_amd/data.py load_occluder_sets);
//                                   per sample: random entry, random rescale with PIL's bicubic resampling restated
//                                   bit for bit (premultiplied alpha, two fixed-point passes, coefficient tables built
//                                   on the host), placement rule of each class, alpha-keyed paste and mask
// Facial-mask samples (load_dataset.py:113,167-177 + _add_gauss_to_mask :203-280): the 3D-mask renders (mask_out.rec /
// mask.rec) are the caller's, as the occluder PNGs are; what is done with them runs here (k_occ_apply_mask below): Resize,
// flip, light, the <= 128 binarisation and the Gaussian light / Gaussian noise / block on the mask pixels.  Only the
// renderer itself is not part of this pipeline.
//
// Random draws come from a counter-based generator (splitmix64 of seed, image index, draw index): the
// same (seed, offset) gives the same batch on any launch geometry, and the CPU oracle regenerates it.
#include <hip/hip_fp16.h>

#include "common.h"

// every float expression below is restated operation by operation on the CPU (oracle/occ.py): no FMA
// contraction, so that truncations to int agree bit for bit
#pragma clang fp contract(off)

#define OCC_DESC 64      // int32 words per image
#define OCC_MAXV 24      // polygon vertices (at most 1 + 2 * 10)
enum { OCC_NONE = 0, OCC_RECT = 1, OCC_ELLIPSE = 2, OCC_BLOCK = 3, OCC_POLY = 4, OCC_GLASSES = 5, OCC_SCARF = 6, OCC_OBJECT = 7, OCC_MASK = 8 };
// desc: 0 kind | 1 x0 / cx | 2 y0 / cy | 3 w / aw | 4 h / ah | 5,6,7 r g b | 8 flip | 9 light cx (f32 bits)
//       10 light cy (f32 bits) | 11 light scale (f32 bits) | 12 polygon vertex count | 13 texture set | 14 texture entry
//       15 reserved | 16 + 2 v, 17 + 2 v: polygon vertex v (x, y)
// Mask samples (kind 8, msml_occ_draw_mask): words 1-7 and 12-15 stay 0 -- the apply kernels above the overlay index the
//   patch buffer with words 1-4 and treat such a descriptor as a clean sample -- and everything of the mask sits where a
//   polygon's vertices would: 16 type (0 Gaussian light, 1 Gaussian noise, 2 block) | 17 lx | 18 ly | 19 rx | 20 ry (the
//   rectangle in OUTPUT pixels, after the flip) | 21 sign (+1 / -1) | 22, 23, 24 colour-jitter bit of r, g, b | 25 light
//   centre x | 26 light centre y | 27 light radius (f32 bits) | 28, 29 the low and high half of the sample's noise key.
//   Draw indices: 46 flag, 47 type, 48-51 the rectangle's four offsets, 52 sign, 53 / 54 centre, 55 radius, 56-58 jitter
//   (0-13 and 16-45 belong to the other kinds).  Per-pixel normal variates come from a key domain of their own
//   (occ_mask_normal: seed + 0x6D61736B): img * 64 + k has no room.
// Texture kinds (5-7): 1, 2 = top-left corner of the paste, 3, 4 = resampled width / height of the occluder.
// Occluder sets: meta[set][OCC_META] int32 = 0 byte offset of the set in the atlas | 1 entries | 2 h0 | 3 w0 | 4 kind
//   | 5 wmin | 6 wmax | 7 hmin | 8 hmax (resampled sizes the tables cover) | 9 wdir | 10 hdir: dir[wdir + w' - wmin] is
//   the offset in rtab of the horizontal table w0 -> w' (w' rows of OCC_RT ints: first tap, taps, 8 fixed-point
//   coefficients), dir[hdir + h' - hmin] of the vertical one.
#define OCC_META 16
#define OCC_RT 10

__host__ __device__ inline unsigned long long occ_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
__host__ __device__ inline unsigned int occ_u32(unsigned long long seed, unsigned long long img, int k) {
  return (unsigned int)(occ_mix(occ_mix(seed) + img * 64ULL + (unsigned long long)k) >> 32);
}
// a mask sample's key of the per-pixel normal variates (occ_mask_normal below): a domain of its own, seed + "mask"
__host__ __device__ inline unsigned long long occ_mask_key(unsigned long long seed, unsigned long long img) {
  return occ_mix(occ_mix(seed + 0x6D61736BULL) + img);
}
// integer in [a, b) (np.random.randint(a, b)): multiply-shift, no rejection
__host__ __device__ inline int occ_randint(unsigned int u, int a, int b) {
  return a + (int)(((unsigned long long)u * (unsigned long long)(b - a)) >> 32);
}
// uniform f32 in [0, 1) with 24 bits
__host__ __device__ inline float occ_unif(unsigned int u) { return (float)(u >> 8) * (1.0f / 16777216.0f); }

// sin / cos for the polygon vertices, written out operation by operation (quadrant reduction + Taylor polynomials in
// f32, no FMA) so that the CPU oracle reproduces the truncated integer coordinates bit for bit; |error| < 2e-6
__host__ __device__ inline void occ_sincos(float a, float* s, float* c) {
  const int q = (int)(a * 0.63661977236758134f + 0.5f);            // nearest multiple of pi / 2 (a >= 0)
  const float r = (a - (float)q * 1.5707963705062866f) - (float)q * -4.371138828673793e-08f;
  const float r2 = r * r;
  float sp = -1.9841270114e-04f + r2 * 2.7557314297e-06f;
  sp = 8.3333337680e-03f + r2 * sp;
  sp = -1.6666667163e-01f + r2 * sp;
  sp = r + r * (r2 * sp);
  float cp = -1.3888889225e-03f + r2 * (2.4801587642e-05f + r2 * -2.7557314297e-07f);
  cp = 4.1666667908e-02f + r2 * cp;
  cp = -0.5f + r2 * cp;
  cp = 1.0f + r2 * cp;
  const int m = q & 3;
  *s = m == 0 ? sp : (m == 1 ? cp : (m == 2 ? -sp : -cp));
  *c = m == 0 ? cp : (m == 1 ? -sp : (m == 2 ? -cp : sp));
}

// mode 0: training mix -- kind uniform over {rect, ellipse, polygon, none}; mode 1: RandomRect only;
// mode 2: RandomBlock(lo, hi, 'black') (evaluation); mode 3: no occlusion; mode 4: RandomConnectedPolygon only.
// modes 5-9 need occluder sets: 5 = the reference's ms1m mix (load_dataset.py:155-157: uniform over rect, ellipse,
// polygon, glasses, scarf, real object, none), 6 = its casia mix (:158-163: none with probability 1/2, else uniform
// over the six occluders), 7 / 8 / 9 = glasses / scarf / real object only.
__device__ inline int occ_pick_set(const int* meta, int nsets, int kind, unsigned int u) {
  int cnt = 0;
  for (int s = 0; s < nsets; s++) cnt += meta[s * OCC_META + 4] == kind;
  if (cnt == 0) return -1;
  int want = occ_randint(u, 0, cnt);                    // RandomGlassesList: uniform over its folders
  for (int s = 0; s < nsets; s++)
    if (meta[s * OCC_META + 4] == kind && want-- == 0) return s;
  return -1;
}

__global__ void k_occ_draw(unsigned long long seed, unsigned long long offset, int N, int H, int W, int mode, int lo,
                           int hi, int flip_on, const int* __restrict__ meta, int nsets, int* __restrict__ desc,
                           int LH, int LW, float p_mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const unsigned long long img = offset + (unsigned long long)i;
  int d[OCC_DESC];
  for (int k = 0; k < OCC_DESC; k++) d[k] = 0;
  int kind = OCC_NONE;
  // load_dataset.py:113: a mask sample takes no occluder; its descriptor does not depend on p_mask
  const bool masked = p_mask > 0.f && occ_unif(occ_u32(seed, img, 46)) < p_mask;
  if (masked) {                                 // _add_gauss_to_mask :219-261, _get_gauss :302-316
    kind = OCC_MASK;
    const int tt = occ_randint(occ_u32(seed, img, 47), 0, 11);
    const int type = tt >= 7 ? 0 : (tt >= 5 ? 1 : 2);
    const int lx = 40 + occ_randint(occ_u32(seed, img, 48), -20, 21);
    const int rx = 100 + occ_randint(occ_u32(seed, img, 49), -20, 11);
    int ly = 1, ry = 111;
    if (type == 2) {
      ly = 40 + occ_randint(occ_u32(seed, img, 50), -20, 20);
      ry = 100 + occ_randint(occ_u32(seed, img, 51), -20, 10);
    }
    d[16] = type; d[17] = lx; d[18] = ly; d[19] = rx; d[20] = ry;
    d[21] = occ_randint(occ_u32(seed, img, 52), 0, 2) * 2 - 1;
    for (int c = 0; c < 3; c++) d[22 + c] = occ_randint(occ_u32(seed, img, 56 + c), 0, 2);
    const int rw = rx - lx, rh = ry - ly, edge = rw > rh ? rw : rh;
    const int rlo = (int)((double)edge / 1.5), rhi = (int)((double)edge * 1.5);
    d[25] = __float_as_int((float)lx + (float)rw * occ_unif(occ_u32(seed, img, 53)));
    d[26] = __float_as_int((float)ly + (float)rh * occ_unif(occ_u32(seed, img, 54)));
    d[27] = __float_as_int((float)rlo + (float)(rhi - rlo) * occ_unif(occ_u32(seed, img, 55)));
    const unsigned long long nk = occ_mask_key(seed, img);        // the sample's key of occ_mask_normal
    d[28] = (int)(unsigned int)(nk & 0xFFFFFFFFULL);
    d[29] = (int)(unsigned int)(nk >> 32);
  } else if (mode == 0) {
    const int pick = occ_randint(occ_u32(seed, img, 0), 0, 4);
    kind = pick == 0 ? OCC_RECT : (pick == 1 ? OCC_ELLIPSE : (pick == 2 ? OCC_POLY : OCC_NONE));
  } else if (mode == 1) kind = OCC_RECT;
  else if (mode == 2) kind = OCC_BLOCK;
  else if (mode == 4) kind = OCC_POLY;
  else if (mode == 5 || mode == 6) {
    const int six = mode == 5 ? occ_randint(occ_u32(seed, img, 0), 0, 7)
                              : (occ_randint(occ_u32(seed, img, 0), 0, 8) >= 4 ? occ_randint(occ_u32(seed, img, 13), 0, 6) : 6);
    kind = six == 0 ? OCC_RECT : six == 1 ? OCC_ELLIPSE : six == 2 ? OCC_POLY : six == 3 ? OCC_GLASSES
         : six == 4 ? OCC_SCARF : six == 5 ? OCC_OBJECT : OCC_NONE;
  } else if (mode >= 7 && mode <= 9) kind = OCC_GLASSES + (mode - 7);
  if (kind >= OCC_GLASSES && kind <= OCC_OBJECT) {
    const int set = occ_pick_set(meta, nsets, kind, occ_u32(seed, img, 1));
    if (set < 0) kind = OCC_NONE;
    else {
      const int* m = meta + set * OCC_META;
      const float w0 = (float)m[3], h0 = (float)m[2];
      const float u3 = occ_unif(occ_u32(seed, img, 3)), u4 = occ_unif(occ_u32(seed, img, 4));
      int ow, oh, x0, y0;
      if (kind == OCC_GLASSES) {                 // rand_occ.py:371-387
        const float bw = (float)W * (w0 / 120.0f), bh = (float)H * (h0 / 120.0f);
        const float lo_s = 1.0f / 1.1f;
        ow = (int)(bw * (lo_s + (1.1f - lo_s) * u3));
        oh = (int)(bh * (lo_s + (1.1f - lo_s) * u4));
        x0 = (int)((0.12f + (float)occ_randint(occ_u32(seed, img, 5), -5, 6) * 0.02f) * (float)W);
        y0 = (int)((0.3f + (float)occ_randint(occ_u32(seed, img, 6), -5, 6) * 0.01f) * (float)H);
      } else if (kind == OCC_SCARF) {            // :466-479 (both offsets scale with the image WIDTH)
        const float lo_s = 1.0f / 1.1f;
        ow = (int)(w0 * (lo_s + (1.0f - lo_s) * u3));
        oh = (int)(h0 * (lo_s + (1.0f - lo_s) * u4));
        x0 = (int)((0.1f + (float)occ_randint(occ_u32(seed, img, 5), -5, 5) * 0.01f) * (float)W);
        y0 = (int)((0.6f + (float)occ_randint(occ_u32(seed, img, 6), -5, 5) * 0.01f) * (float)W);
      } else {                                   // :563-575
        ow = (int)(w0 * (1.0f + (2.0f - 1.0f) * u3));
        oh = (int)(h0 * (1.0f + (2.0f - 1.0f) * u4));
        x0 = (int)(((float)occ_randint(occ_u32(seed, img, 5), 15, 51) * 0.01f) * (float)W);
        y0 = (int)(((float)occ_randint(occ_u32(seed, img, 6), 15, 51) * 0.01f) * (float)H);
      }
      ow = ow < m[5] ? m[5] : (ow > m[6] ? m[6] : ow);          // the tables cover [wmin, wmax] x [hmin, hmax]
      oh = oh < m[7] ? m[7] : (oh > m[8] ? m[8] : oh);
      d[1] = x0; d[2] = y0; d[3] = ow; d[4] = oh;
      d[13] = set;
      d[14] = occ_randint(occ_u32(seed, img, 2), 0, m[1]);
    }
  }
  if (kind == OCC_RECT) {                       // rand_occ.py:113-121
    const int pct = occ_randint(occ_u32(seed, img, 1), lo, hi);
    const float ratio = (float)pct * 0.01f;
    const int area = (int)((float)(W * H) * ratio);
    const int ow = occ_randint(occ_u32(seed, img, 2), (int)((float)W * ratio) + 1, W + 1);
    const int oh = area / ow;
    d[1] = occ_randint(occ_u32(seed, img, 3), 0, W - ow + 1);
    d[2] = occ_randint(occ_u32(seed, img, 4), 0, H - oh + 1);
    d[3] = ow;
    d[4] = oh;
    for (int c = 0; c < 3; c++) d[5 + c] = occ_randint(occ_u32(seed, img, 5 + c), 0, 256);
    if (oh == 0) kind = OCC_NONE;
  } else if (kind == OCC_ELLIPSE) {             // rand_occ.py:184-199
    const int ch = occ_randint(occ_u32(seed, img, 1), H / 5, 4 * H / 5);
    const int cw = occ_randint(occ_u32(seed, img, 2), W / 5, 4 * W / 5);
    const int mh = ch < H - ch ? ch : H - ch;
    const int ah = occ_randint(occ_u32(seed, img, 3), 20, mh > 20 ? mh : 21);
    const float ratio = 0.2f + (0.4f - 0.2f) * occ_unif(occ_u32(seed, img, 4));
    const int aw = (int)((float)(H * W) * ratio / (3.14f * (float)ah));
    d[1] = cw; d[2] = ch; d[3] = aw; d[4] = ah;
    for (int c = 0; c < 3; c++) d[5 + c] = occ_randint(occ_u32(seed, img, 5 + c), 1, 256);
  } else if (kind == OCC_POLY) {                // rand_occ.py:262-322: a star between a big and a small circle
    const int cnt = occ_randint(occ_u32(seed, img, 1), 4, 11);
    const int cx = occ_randint(occ_u32(seed, img, 2), H / 5, 4 * H / 5);
    const int cy = occ_randint(occ_u32(seed, img, 3), W / 5, 4 * W / 5);
    const int big = occ_randint(occ_u32(seed, img, 4), H / 5, (int)(1.3f * (float)H) / 5);
    const float small = (float)big / (1.3f + (2.6f - 1.3f) * occ_unif(occ_u32(seed, img, 12)));
    const float step = 6.2831854820251465f / (float)cnt;
    float ab = 0.f, as = 0.f, sn, cs;
    int nv = 0;
    d[16] = (int)((float)cx + (float)big);                 // angle 0 on the big circle
    d[17] = cy;
    nv = 1;
    for (int i = 0; i < cnt; i++) {
      ab = ab + step * (0.7f + (1.3f - 0.7f) * occ_unif(occ_u32(seed, img, 16 + 3 * i)));
      occ_sincos(ab, &sn, &cs);
      d[16 + 2 * nv] = (int)((float)cx + (float)big * cs);
      d[17 + 2 * nv] = (int)((float)cy + (float)big * sn);
      nv++;
      if (occ_unif(occ_u32(seed, img, 17 + 3 * i)) > 0.5f) {
        as = as + step * (0.6f + (1.4f - 0.6f) * occ_unif(occ_u32(seed, img, 18 + 3 * i)));
        occ_sincos(as, &sn, &cs);
        d[16 + 2 * nv] = (int)((float)cx + small * cs);
        d[17 + 2 * nv] = (int)((float)cy + small * sn);
        nv++;
      }
    }
    d[12] = nv;
    for (int c = 0; c < 3; c++) d[5 + c] = occ_randint(occ_u32(seed, img, 5 + c), 1, 256);
  } else if (kind == OCC_BLOCK) {               // rand_occ.py:36-70
    const int pct = occ_randint(occ_u32(seed, img, 1), lo, hi);
    const float ratio = (float)pct * 0.01f;
    const int bw = (int)sqrtf(ratio * (float)W * (float)W);
    if (pct == 0 || bw == 0) kind = OCC_NONE;
    else {
      d[1] = occ_randint(occ_u32(seed, img, 2), 0, W - bw + 1);
      d[2] = occ_randint(occ_u32(seed, img, 3), 0, W - bw + 1);
      d[3] = bw; d[4] = bw;
    }
  }
  d[0] = kind;
  d[8] = flip_on ? (occ_randint(occ_u32(seed, img, 8), 1, 11) >= 5 ? 1 : 0) : 0;    // load_dataset.py:120
  // _get_gauss :307-309: the light centre is uniform over the image the light is added to (LW x LH: the OUTPUT size,
  // load_dataset.py:183-201 runs after the resize; = W x H for msml_occ_draw[_tex])
  d[9] = __float_as_int((float)LW * occ_unif(occ_u32(seed, img, 9)));
  d[10] = __float_as_int((float)LH * occ_unif(occ_u32(seed, img, 10)));
  d[11] = __float_as_int(0.7f + (1.4f - 0.7f) * occ_unif(occ_u32(seed, img, 11)));  // :194
  for (int k = 0; k < OCC_DESC; k++) desc[i * OCC_DESC + k] = d[k];
}

__device__ __forceinline__ bool occ_inside(const int* d, int x, int y) {
  const int kind = d[0];
  if (kind == OCC_RECT || kind == OCC_BLOCK) return x >= d[1] && x < d[1] + d[3] && y >= d[2] && y < d[2] + d[4];
  if (kind == OCC_ELLIPSE) {
    const float dx = (float)(x - d[1]), dy = (float)(y - d[2]);
    const float aw = (float)d[3], ah = (float)d[4];
    return dx * dx * ah * ah + dy * dy * aw * aw <= aw * aw * ah * ah;
  }
  if (kind == OCC_POLY) {                       // even-odd rule on the integer lattice, exact integer arithmetic
    const int nv = d[12];
    bool in = false;
    for (int i = 0, j = nv - 1; i < nv; j = i++) {
      const int xi = d[16 + 2 * i], yi = d[17 + 2 * i], xj = d[16 + 2 * j], yj = d[17 + 2 * j];
      if ((yi > y) != (yj > y)) {
        const int dyv = yj - yi, lhs = (x - xi) * dyv, rhs = (xj - xi) * (y - yi);
        if (dyv > 0 ? lhs < rhs : lhs > rhs) in = !in;
      }
    }
    return in;
  }
  return false;
}

// One workgroup per image.  src: [N][H][W][3] uint8 (decoded RGB, HWC).  img / ori: [N][3][H][W] f32,
// msk: [N][H][W] int64.  light != 0: Gaussian light on img (not on ori, load_dataset.py:126-127).
// PIL's Image.resize of an RGBA image (the call rand_occ.py:375,466,562 makes), bit for bit: RGBA -> premultiplied
// RGBa (MULDIV255), horizontal then vertical pass with the precomputed 22-bit fixed-point bicubic coefficients
// (ImagingResample: ss = 1 << 21; ss += pixel * k; clip8(ss >> 22)), u8 intermediate, back to straight alpha
// (255 * c / a).  An unchanged size is a plain copy (Image.resize returns self.copy()), an unchanged axis skips its
// pass.  One workgroup per image; only texture kinds do anything.  patch: [N][pstride] bytes, rows of w' RGBA pixels.
__device__ __forceinline__ unsigned char occ_clip8(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ void __launch_bounds__(256) k_occ_resize(const unsigned char* __restrict__ atlas, const int* __restrict__ meta,
                                                    const int* __restrict__ dir, const int* __restrict__ rtab,
                                                    const int* __restrict__ desc, unsigned char* __restrict__ patch,
                                                    long pstride) {
  extern __shared__ unsigned char sm[];
  const int n = blockIdx.x, t = threadIdx.x;
  const int* d = desc + n * OCC_DESC;
  if (d[0] < OCC_GLASSES || d[0] > OCC_OBJECT) return;      // (a mask sample, kind 8, has no texture)
  const int* m = meta + d[13] * OCC_META;
  const int h0 = m[2], w0 = m[3], ow = d[3], oh = d[4];
  const unsigned char* e = atlas + (long)m[0] + (long)d[14] * h0 * w0 * 4;
  unsigned char* out = patch + (long)n * pstride;
  if (ow == w0 && oh == h0) {
    for (int i = t; i < h0 * w0 * 4; i += 256) out[i] = e[i];
    return;
  }
  unsigned char* A = sm;                       // [h0][w0][4] premultiplied
  unsigned char* B = sm + h0 * w0 * 4;         // [h0][ow][4] after the horizontal pass
  MSML_LDS_REGION(A, h0 * w0 * 4);
  MSML_LDS_REGION(B, h0 * ow * 4);
  for (int i = t; i < h0 * w0; i += 256) {
    const unsigned int a = e[i * 4 + 3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const unsigned int tmp = (unsigned int)e[i * 4 + c] * a + 128u;
      A[i * 4 + c] = (unsigned char)(((tmp >> 8) + tmp) >> 8);
    }
    A[i * 4 + 3] = (unsigned char)a;
  }
  __syncthreads();
  const unsigned char* Hsrc = A;
  if (ow != w0) {
    const int* tw = rtab + dir[m[9] + ow - m[5]];
    for (int i = t; i < h0 * ow; i += 256) {
      const int y = i / ow, xx = i - y * ow;
      const int* k = tw + xx * OCC_RT;
      const int xmin = k[0], cnt = k[1];
      int ss[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
      for (int j = 0; j < cnt; j++) {
        const unsigned char* px = A + (y * w0 + xmin + j) * 4;
        const int kk = k[2 + j];
#pragma unroll
        for (int c = 0; c < 4; c++) ss[c] += (int)px[c] * kk;
      }
#pragma unroll
      for (int c = 0; c < 4; c++) B[i * 4 + c] = occ_clip8(ss[c] >> 22);
    }
    __syncthreads();
    Hsrc = B;
  }
  const int* th = oh != h0 ? rtab + dir[m[10] + oh - m[7]] : nullptr;
  for (int i = t; i < oh * ow; i += 256) {
    const int yy = i / ow, xx = i - yy * ow;
    int v[4];
    if (th) {
      const int* k = th + yy * OCC_RT;
      const int ymin = k[0], cnt = k[1];
      int ss[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
      for (int j = 0; j < cnt; j++) {
        const unsigned char* px = Hsrc + ((ymin + j) * ow + xx) * 4;
        const int kk = k[2 + j];
#pragma unroll
        for (int c = 0; c < 4; c++) ss[c] += (int)px[c] * kk;
      }
#pragma unroll
      for (int c = 0; c < 4; c++) v[c] = occ_clip8(ss[c] >> 22);
    } else {
#pragma unroll
      for (int c = 0; c < 4; c++) v[c] = Hsrc[i * 4 + c];
    }
    const int a = v[3];
    if (a != 255 && a != 0) {
#pragma unroll
      for (int c = 0; c < 3; c++) v[c] = occ_clip8((255 * v[c]) / a);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) out[i * 4 + c] = (unsigned char)v[c];
  }
}

// _get_gauss at pixel (x, y) of the image the light is added to: integer-truncated offsets (astype(int16)), Euclidean
// distance, sigma 128, float16 map
__device__ __forceinline__ float occ_lightmap(int x, int y, float lcx, float lcy, float lscale) {
  const int ix = (int)((float)x - lcx), iy = (int)((float)y - lcy);
  const float dist = sqrtf((float)(ix * ix + iy * iy));
  const float g = expf(-0.5f * (dist * dist) / 16384.0f);
  const __half g16 = __float2half(g);
  const __half l16 = __float2half(__half2float(g16) * __half2float(__float2half(lscale)));
  return __half2float(l16);
}

__global__ void __launch_bounds__(256) k_occ_apply(const unsigned char* __restrict__ src, const int* __restrict__ desc,
                                                   float* __restrict__ img, long* __restrict__ msk,
                                                   float* __restrict__ ori, int H, int W, int light,
                                                   const unsigned char* __restrict__ patch, long pstride) {
  __shared__ int d[OCC_DESC];
  __shared__ float red[4];
  const int n = blockIdx.x, t = threadIdx.x;
  if (t < OCC_DESC) d[t] = desc[n * OCC_DESC + t];
  __syncthreads();
  const int HW = H * W;
  const unsigned char* s = src + (long)n * HW * 3;
  float* o = img + (long)n * 3 * HW;
  const bool flip = d[8] != 0;
  const float lcx = __int_as_float(d[9]), lcy = __int_as_float(d[10]), lscale = __int_as_float(d[11]);
  float vmax = 0.f;
  for (int p = t; p < HW; p += 256) {
    const int y = p / W, x = p - y * W;
    const int sx = flip ? W - 1 - x : x;          // occlude -> flip: tests run in source coordinates
    bool in = occ_inside(d, sx, y);
    const unsigned char* q = s + ((long)y * W + sx) * 3;
    // texture kinds: the resampled RGBA occluder at (d[1], d[2]); the paste is cropped at the image border
    // (rand_occ.py:486-489,582-585).  Pixel: glasses replace where alpha > 10 (:390), scarf / object where alpha != 0
    // (:495, :591); the mask marks alpha != 0 for all three (:400-401, :504-505, :600-601).
    const unsigned char* tp = nullptr;
    bool paste = false;
    if (d[0] >= OCC_GLASSES && patch != nullptr) {       // (no patch buffer: msml_occ_apply on texture descriptors = clean)
      const int px = sx - d[1], py = y - d[2];
      if (px >= 0 && px < d[3] && py >= 0 && py < d[4]) {
        tp = patch + (long)n * pstride + ((long)py * d[3] + px) * 4;
        in = tp[3] != 0;
        paste = d[0] == OCC_GLASSES ? tp[3] > 10 : tp[3] != 0;
      }
    }
    msk[(long)n * HW + p] = in ? 0 : 1;
    const float l = light ? occ_lightmap(x, y, lcx, lcy, lscale) : 1.f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float clean = (float)q[c] / 255.0f;                       // ToTensor
      if (ori) ori[((long)n * 3 + c) * HW + p] = (clean - 0.5f) / 0.5f;
      float v;
      if (d[0] >= OCC_GLASSES) v = paste ? (float)tp[c] / 255.0f : clean;
      else v = in ? (d[0] == OCC_BLOCK ? 0.f : (float)d[5 + c] / 255.0f) : clean;
      v *= l;
      o[(long)c * HW + p] = v;
      vmax = fmaxf(vmax, v);
    }
  }
  if (light) {                                    // out_img / out_img.max()  (load_dataset.py:199)
    vmax = wave_max(vmax);
    if ((t & 63) == 0) red[t >> 6] = vmax;
    __syncthreads();
    vmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
  }
  for (int p = t; p < 3 * HW; p += 256) {
    float v = o[p];
    if (light) v = v / vmax;
    o[p] = (v - 0.5f) / 0.5f;                      // Normalize(0.5, 0.5)
  }
}

// the k_occ_draw launch of the four draw entry points (LH x LW: the size the light is added at)
static int occ_draw_launch(const char* name, long seed, long offset, int N, int H, int W, int mode, int lo, int hi,
                           int flip, const int* meta, int nsets, int* desc, int LH, int LW, float p_mask, void* stream) {
  k_occ_draw<<<cdiv(N, 256), 256, 0, (hipStream_t)stream>>>((unsigned long long)seed, (unsigned long long)offset, N, H, W, mode, lo, hi, flip, meta, nsets, desc, LH, LW, p_mask);
  MSML_LAUNCH_OK(name);
  return MSML_OK;
}

extern "C" int msml_occ_draw(long seed, long offset, int N, int H, int W, int mode, int lo, int hi,
                             int flip, int* desc, void* stream) {
  MSML_CHECK(desc && N > 0 && H >= 32 && W >= 32 && mode >= 0 && mode <= 4 && lo >= 0 && hi > lo && hi <= 101,
             MSML_ERR_SHAPE, "occ_draw: bad arguments N=%d H=%d W=%d mode=%d lo=%d hi=%d", N, H, W, mode, lo, hi);
  return occ_draw_launch("occ_draw", seed, offset, N, H, W, mode, lo, hi, flip, nullptr, 0, desc, H, W, 0.f, stream);
}

extern "C" int msml_occ_draw_tex(long seed, long offset, int N, int H, int W, int mode, int lo, int hi, int flip,
                                 const int* meta, int nsets, int* desc, void* stream) {
  MSML_CHECK(desc && N > 0 && H >= 32 && W >= 32 && mode >= 0 && mode <= 9 && lo >= 0 && hi > lo && hi <= 101,
             MSML_ERR_SHAPE, "occ_draw_tex: bad arguments N=%d H=%d W=%d mode=%d lo=%d hi=%d", N, H, W, mode, lo, hi);
  MSML_CHECK(mode < 5 || (meta && nsets > 0 && nsets <= 16), MSML_ERR_SHAPE,
             "occ_draw_tex: modes 5-9 need 1..16 occluder sets (got %d)", nsets);
  return occ_draw_launch("occ_draw_tex", seed, offset, N, H, W, mode, lo, hi, flip, meta, nsets, desc, H, W, 0.f, stream);
}

extern "C" int msml_occ_resize(const unsigned char* atlas, const int* meta, const int* dir, const int* rtab,
                               const int* desc, unsigned char* patch, long patch_stride, int N, int lds_bytes,
                               void* stream) {
  MSML_CHECK(atlas && meta && dir && rtab && desc && patch && N > 0 && patch_stride > 0 && lds_bytes > 0 &&
                 lds_bytes <= 160 * 1024, MSML_ERR_SHAPE, "occ_resize: bad arguments");
  static int attr_lds = 0;
  if (lds_bytes > attr_lds) {                   // (monotonic; racing callers set the same or a larger value)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_occ_resize), hipFuncAttributeMaxDynamicSharedMemorySize,
                              lds_bytes);
    attr_lds = lds_bytes;
  }
  k_occ_resize<<<N, 256, lds_bytes, (hipStream_t)stream>>>(atlas, meta, dir, rtab, desc, patch, patch_stride);
  MSML_LAUNCH_OK("occ_resize");
  return MSML_OK;
}

extern "C" int msml_occ_apply(const unsigned char* src, const int* desc, float* img, long* msk, float* ori, int N,
                              int H, int W, int light, void* stream) {
  MSML_CHECK(src && desc && img && msk && N > 0 && H > 0 && W > 0, MSML_ERR_SHAPE, "occ_apply: bad arguments");
  k_occ_apply<<<N, 256, 0, (hipStream_t)stream>>>(src, desc, img, msk, ori, H, W, light, nullptr, 0);
  MSML_LAUNCH_OK("occ_apply");
  return MSML_OK;
}

extern "C" int msml_occ_apply_tex(const unsigned char* src, const int* desc, const unsigned char* patch,
                                  long patch_stride, float* img, long* msk, float* ori, int N, int H, int W, int light,
                                  void* stream) {
  MSML_CHECK(src && desc && patch && img && msk && N > 0 && H > 0 && W > 0, MSML_ERR_SHAPE, "occ_apply_tex: bad arguments");
  k_occ_apply<<<N, 256, 0, (hipStream_t)stream>>>(src, desc, img, msk, ori, H, W, light, patch, patch_stride);
  MSML_LAUNCH_OK("occ_apply_tex");
  return MSML_OK;
}

// ---------------------------------------------------------------- gray / resized / unnormalised output
// FaceByRandOccMask.__getitem__ with is_gray / out_size / use_norm (datasets/load_dataset.py:86-139,179,183-201; the
// LightCNN recipe config.py:99-102 sets gray, 128 x 128, no Normalize): occlude at the SOURCE size -> convert('L')
// (L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16) -> transforms.Resize of face, 0 / 255 mask and clean face
// (Image.resize(BILINEAR): Pillow's separable resampling with the triangle filter -- horizontal pass, uint8 intermediate,
// vertical pass, 22-bit fixed-point coefficients built on the host; an axis whose size does not change is skipped) ->
// flip -> ToTensor -> light at the OUTPUT size -> mask != 255 -> 0 else 1 -> Normalize only when asked.  The mask is
// interpolated as an image: every output pixel the filter mixes with an occluded one is occluded.
//
// One workgroup of 1024 threads per image, everything between the source read and the output stores in LDS:
//   raw  [H][W][3]   the decoded face, read once, 16 B per lane
//   Mk   [H][W]      0 (occluded) / 255 mask at source size
//   S    [H][W]      the plane being resampled (one colour plane of the occluded or of the clean face; L when gray)
//   Bh   [H][ow]     S after the horizontal pass (absent when ow == W)
//   O    [C][oh][ow] the occluded face after both passes and the flip: the light's  / max  needs every value of the
//                    image before the first one can be written, so img is kept here as uint8 and written ONCE
// Planes go through S / Bh one after the other (mask, C face planes, C clean planes), so RGB with a resize and ori fits:
// 136 960 B at 112 -> 128 RGB, 104 192 B gray.  Every global store is 16 B per lane (float4 / two int64); needs ow % 4 == 0.
#define OCC_OUT_T 1024
#define OCC_OUT_HDR 512          // desc[64] int32 + the 16 per-wave maxima
// The one LDS layout of k_occ_apply_out (mb = false) and of the mask overlay k_occ_apply_mask below (mb = true: plus
// MB [oh][ow], the binarised mask its last pass reads), for the host and for both kernels.
struct OccLds {
  long tabw, tabh, raw, mk, s, bh, o, mb, total;
};
__host__ __device__ constexpr long occ_r16(long b) { return (b + 15) & ~15L; }
__host__ __device__ constexpr OccLds occ_lds(int H, int W, int oh, int ow, int C, bool mb) {
  OccLds L{};
  long off = OCC_OUT_HDR;
  L.tabw = off; off += ow != W ? occ_r16((long)ow * OCC_RT * 4) : 0;
  L.tabh = off; off += oh != H ? occ_r16((long)oh * OCC_RT * 4) : 0;
  L.raw = off;  off += occ_r16((long)H * W * 3);
  L.mk = off;   off += occ_r16((long)H * W);
  L.s = off;    off += occ_r16((long)H * W);
  L.bh = off;   off += ow != W ? occ_r16((long)H * ow) : 0;
  L.o = off;    off += occ_r16((long)C * oh * ow);
  L.mb = off;   off += mb ? occ_r16((long)oh * ow) : 0;
  L.total = off;
  return L;
}
// the byte counts docs/KERNELS.md states: source -> output (oh, ow), channels
static_assert(occ_lds(112, 112, 128, 128, 1, false).total == 104192 && occ_lds(112, 112, 128, 128, 3, false).total == 136960 &&
              occ_lds(112, 112, 96, 96, 1, false).total == 90880 && occ_lds(112, 112, 112, 96, 3, false).total == 110080 &&
              occ_lds(112, 112, 144, 144, 3, false).total == 153088 && occ_lds(112, 112, 224, 224, 1, false).total == 156416 &&
              occ_lds(112, 112, 224, 224, 3, false).total == 256768, "k_occ_apply_out: LDS bytes");
static_assert(occ_lds(112, 112, 128, 128, 3, true).total == 153344 && occ_lds(112, 112, 128, 128, 1, true).total == 120576 &&
              occ_lds(112, 112, 112, 112, 3, true).total == 113408, "k_occ_apply_mask: LDS bytes");
__device__ __forceinline__ unsigned int occ_luma(unsigned int r, unsigned int g, unsigned int b) {
  return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;          // Pillow Convert.c L24 + rounding
}

// ---- what k_occ_apply_out and k_occ_apply_mask share.  None of these holds a barrier: the kernels place them.
// The descriptor of image n (to the head of the LDS) and the coefficient tables of the axes that change (has_w, has_h)
// -> LDS.
__device__ __forceinline__ void occ_stage_tables(unsigned char* sm, const OccLds& L, bool has_w, bool has_h,
                                                 const int* __restrict__ desc, const int* __restrict__ tabw,
                                                 const int* __restrict__ tabh, int n, int oh, int ow, int t) {
  if (t < OCC_DESC) reinterpret_cast<int*>(sm)[t] = desc[n * OCC_DESC + t];
  if (has_w) for (int i = t; i < ow * OCC_RT; i += OCC_OUT_T) reinterpret_cast<int*>(sm + L.tabw)[i] = tabw[i];
  if (has_h) for (int i = t; i < oh * OCC_RT; i += OCC_OUT_T) reinterpret_cast<int*>(sm + L.tabh)[i] = tabh[i];
}
// `bytes` bytes of a byte plane -> LDS (dst 16-byte aligned), 16 B per lane when the source allows it
__device__ __forceinline__ void occ_stage_bytes(unsigned char* dst, const unsigned char* __restrict__ s, int bytes, int t) {
  if (bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
    for (int i = t; i < bytes / 16; i += OCC_OUT_T)
      reinterpret_cast<u32x4*>(dst)[i] = reinterpret_cast<const u32x4*>(s)[i];
  } else {
    for (int i = t; i < bytes; i += OCC_OUT_T) dst[i] = s[i];
  }
}
// horizontal pass P [H][W] -> Bh [H][ow], four outputs per lane
__device__ __forceinline__ void occ_pass_h(const unsigned char* P, unsigned char* Bh, const int* tw, int H, int W, int ow,
                                           int t) {
  for (int i = t; i < H * ow / 4; i += OCC_OUT_T) {
    const int y = (i * 4) / ow, xx = i * 4 - y * ow;
    unsigned int pack = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int* k = tw + (xx + e) * OCC_RT;
      const unsigned char* row = P + y * W + k[0];
      int ss = 1 << 21;
      for (int j = 0; j < k[1]; j++) ss += (int)row[j] * k[2 + j];
      pack |= (unsigned int)occ_clip8(ss >> 22) << (8 * e);
    }
    reinterpret_cast<unsigned int*>(Bh)[i] = pack;
  }
}
// vertical pass (th null: the axis keeps its size) + flip of Q [.][ow] for output pixels (x .. x + 3, yy) -> v
__device__ __forceinline__ void occ_pass_v4(const unsigned char* Q, const int* th, int ow, int yy, int x, bool flip,
                                            int (&v)[4]) {
  const int base = flip ? ow - 4 - x : x;           // the four source columns, a 4-byte aligned word of every row
  if (th) {
    const int* k = th + yy * OCC_RT;
    int ss[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
    for (int j = 0; j < k[1]; j++) {
      const unsigned int wd = *reinterpret_cast<const unsigned int*>(Q + (k[0] + j) * ow + base);
      const int kk = k[2 + j];
#pragma unroll
      for (int e = 0; e < 4; e++) ss[e] += (int)((wd >> (8 * e)) & 255u) * kk;
    }
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = occ_clip8(ss[e] >> 22);
  } else {
    const unsigned int wd = *reinterpret_cast<const unsigned int*>(Q + yy * ow + base);
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = (int)((wd >> (8 * e)) & 255u);
  }
  if (flip) {
    int s0 = v[0], s1 = v[1];
    v[0] = v[3]; v[1] = v[2]; v[2] = s1; v[3] = s0;
  }
}
// The light's maximum (out_img.max(), load_dataset.py:199) over O [C][oh * ow], first half: this wave's maximum -> red.
// The kernel's barrier follows, then occ_light_max_fold gives every thread the workgroup's.
__device__ __forceinline__ void occ_light_max_waves(const unsigned char* O, int C, int ohow, int ow, float lcx, float lcy,
                                                    float lscale, float* red, int t) {
  float vmax = 0.f;
  for (int i = t; i < ohow / 4; i += OCC_OUT_T) {
    const int p = i * 4, y = p / ow, x = p - y * ow;
    float l[4];
#pragma unroll
    for (int e = 0; e < 4; e++) l[e] = occ_lightmap(x + e, y, lcx, lcy, lscale);
    for (int c = 0; c < C; c++) {
      const unsigned int wd = reinterpret_cast<const unsigned int*>(O + (long)c * ohow)[i];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float v = (float)((wd >> (8 * e)) & 255u) / 255.0f;
        v *= l[e];
        vmax = fmaxf(vmax, v);
      }
    }
  }
  vmax = wave_max(vmax);
  if ((t & 63) == 0) red[t >> 6] = vmax;
}
__device__ __forceinline__ float occ_light_max_fold(const float* red) {
  float vmax = red[0];
#pragma unroll
  for (int w = 1; w < OCC_OUT_T / 64; w++) vmax = fmaxf(vmax, red[w]);
  return vmax;
}

__global__ void __launch_bounds__(OCC_OUT_T) k_occ_apply_out(
    const unsigned char* __restrict__ src, const int* __restrict__ desc, const unsigned char* __restrict__ patch,
    long pstride, const int* __restrict__ tabw, const int* __restrict__ tabh, float* __restrict__ img,
    long* __restrict__ msk, float* __restrict__ ori, int H, int W, int oh, int ow, int gray, int norm, int light) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smo[];
  const int n = blockIdx.x, t = threadIdx.x;
  const int C = gray ? 1 : 3, HW = H * W, ohow = oh * ow;
  const OccLds L = occ_lds(H, W, oh, ow, C, false);
  int* d = reinterpret_cast<int*>(smo);
  float* red = reinterpret_cast<float*>(smo + OCC_DESC * 4);
  const int* tw = ow != W ? reinterpret_cast<const int*>(smo + L.tabw) : nullptr;
  const int* th = oh != H ? reinterpret_cast<const int*>(smo + L.tabh) : nullptr;
  unsigned char* raw = smo + L.raw;
  unsigned char* Mk = smo + L.mk;
  unsigned char* S = smo + L.s;
  unsigned char* Bh = smo + L.bh;
  unsigned char* O = smo + L.o;
  MSML_LDS_REGION(O, (long)C * ohow);
  occ_stage_tables(smo, L, tw != nullptr, th != nullptr, desc, tabw, tabh, n, oh, ow, t);
  occ_stage_bytes(raw, src + (long)n * HW * 3, HW * 3, t);
  __syncthreads();
  const int kind = d[0];
  const bool flip = d[8] != 0;
  const bool tex = kind >= OCC_GLASSES && patch != nullptr;     // (no patch buffer on texture descriptors = clean)
  const unsigned char* pt = tex ? patch + (long)n * pstride : nullptr;
  // the 0 / 255 mask at source size (occ_inside / alpha != 0 of the paste, as k_occ_apply)
  for (int p = t; p < HW; p += OCC_OUT_T) {
    const int y = p / W, x = p - y * W;
    bool in = occ_inside(d, x, y);
    if (tex) {
      const int px = x - d[1], py = y - d[2];
      if (px >= 0 && px < d[3] && py >= 0 && py < d[4]) in = pt[((long)py * d[3] + px) * 4 + 3] != 0;
    }
    Mk[p] = in ? 0 : 255;
  }
  __syncthreads();
  // planes: 0 = mask, 1 .. C = occluded face, C + 1 .. 2 C = clean face (ori)
  const int planes = ori ? 1 + 2 * C : 1 + C;
  for (int pl = 0; pl < planes; pl++) {
    const bool face = pl >= 1 && pl <= C;
    const int c = pl == 0 ? 0 : (pl - 1) % C;
    const unsigned char* P = Mk;
    if (pl > 0) {
      for (int p = t; p < HW; p += OCC_OUT_T) {
        const unsigned char* q = raw + p * 3;
        unsigned int r = q[0], g = q[1], b = q[2];
        if (face) {
          if (tex) {                                  // glasses replace where alpha > 10, scarf / object where alpha != 0
            const int y = p / W, x = p - y * W;
            const int px = x - d[1], py = y - d[2];
            if (px >= 0 && px < d[3] && py >= 0 && py < d[4]) {
              const unsigned char* tp = pt + ((long)py * d[3] + px) * 4;
              if (kind == OCC_GLASSES ? tp[3] > 10 : tp[3] != 0) { r = tp[0]; g = tp[1]; b = tp[2]; }
            }
          } else if (Mk[p] == 0) {
            if (kind == OCC_BLOCK) r = g = b = 0;
            else { r = (unsigned int)d[5]; g = (unsigned int)d[6]; b = (unsigned int)d[7]; }
          }
        }
        S[p] = (unsigned char)(gray ? occ_luma(r, g, b) : (c == 0 ? r : (c == 1 ? g : b)));
      }
      __syncthreads();
      P = S;
    }
    const unsigned char* Q = P;                       // [H][ow]
    if (tw) {
      occ_pass_h(P, Bh, tw, H, W, ow, t);
      __syncthreads();
      Q = Bh;
    }
    // vertical pass + flip, four outputs per lane: the mask and the clean face go to HBM, the occluded face to O
    for (int i = t; i < ohow / 4; i += OCC_OUT_T) {
      const int p = i * 4, yy = p / ow, x = p - yy * ow;
      int v[4];
      occ_pass_v4(Q, th, ow, yy, x, flip, v);
      if (pl == 0) {                                  // Msk2Tenser: != 255 -> 0, else 1
        longlong2 a, b;
        a.x = v[0] == 255; a.y = v[1] == 255; b.x = v[2] == 255; b.y = v[3] == 255;
        longlong2* o = reinterpret_cast<longlong2*>(msk + (long)n * ohow + p);
        o[0] = a;
        o[1] = b;
      } else if (face) {
        reinterpret_cast<unsigned int*>(O + (long)c * ohow)[i] =
            (unsigned int)v[0] | ((unsigned int)v[1] << 8) | ((unsigned int)v[2] << 16) | ((unsigned int)v[3] << 24);
      } else {
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float cl = (float)v[e] / 255.0f;      // ToTensor
          r[e] = norm ? (cl - 0.5f) / 0.5f : cl;
        }
        *reinterpret_cast<f32x4*>(ori + ((long)n * C + c) * ohow + p) = r;
      }
    }
    __syncthreads();                                  // S / Bh are rebuilt for the next plane; O is complete after the last
  }
  // ToTensor, light at the output size, / max, Normalize: img is written once
  const float lcx = __int_as_float(d[9]), lcy = __int_as_float(d[10]), lscale = __int_as_float(d[11]);
  float vmax = 0.f;
  if (light) {
    occ_light_max_waves(O, C, ohow, ow, lcx, lcy, lscale, red, t);
    __syncthreads();
    vmax = occ_light_max_fold(red);
  }
  for (int i = t; i < ohow / 4; i += OCC_OUT_T) {
    const int p = i * 4, y = p / ow, x = p - y * ow;
    float l[4];
#pragma unroll
    for (int e = 0; e < 4; e++) l[e] = light ? occ_lightmap(x + e, y, lcx, lcy, lscale) : 1.f;
    for (int c = 0; c < C; c++) {
      const unsigned int wd = reinterpret_cast<const unsigned int*>(O + (long)c * ohow)[i];
      f32x4 r;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float v = (float)((wd >> (8 * e)) & 255u) / 255.0f;
        v *= l[e];
        if (light) v = v / vmax;                      // out_img / out_img.max()  (load_dataset.py:199)
        r[e] = norm ? (v - 0.5f) / 0.5f : v;
      }
      *reinterpret_cast<f32x4*>(img + ((long)n * C + c) * ohow + p) = r;
    }
  }
}

extern "C" int msml_occ_draw_out(long seed, long offset, int N, int H, int W, int out_h, int out_w, int mode, int lo,
                                 int hi, int flip, const int* meta, int nsets, int* desc, void* stream) {
  MSML_CHECK(desc && N > 0 && H >= 32 && W >= 32 && out_h > 0 && out_w > 0 && mode >= 0 && mode <= 9 && lo >= 0 &&
                 hi > lo && hi <= 101, MSML_ERR_SHAPE,
             "occ_draw_out: bad arguments N=%d H=%d W=%d out=%dx%d mode=%d lo=%d hi=%d", N, H, W, out_h, out_w, mode, lo, hi);
  MSML_CHECK(mode < 5 || (meta && nsets > 0 && nsets <= 16), MSML_ERR_SHAPE,
             "occ_draw_out: modes 5-9 need 1..16 occluder sets (got %d)", nsets);
  return occ_draw_launch("occ_draw_out", seed, offset, N, H, W, mode, lo, hi, flip, mode < 5 ? nullptr : meta,
                         mode < 5 ? 0 : nsets, desc, out_h, out_w, 0.f, stream);
}

// What msml_occ_apply_out and msml_occ_apply_mask (mb) check after their own arguments, and the launch's LDS bytes, which
// `kernel` is allowed from here on; *attr_lds is the caller's record of what it has been allowed so far.
static int occ_out_setup(const char* name, const void* kernel, int* attr_lds, bool mb, const int* tabw, const int* tabh,
                         int H, int W, int out_h, int out_w, int gray, long* lds_bytes) {
  MSML_CHECK((out_w == W || tabw) && (out_h == H || tabh), MSML_ERR_SHAPE,
             "%s: %dx%d -> %dx%d needs the resampling table of every axis that changes", name, H, W, out_h, out_w);
  MSML_CHECK(out_w % 4 == 0, MSML_ERR_UNSUPPORTED,
             "%s: output width %d is not a multiple of 4 (16-byte stores)", name, out_w);
  const OccLds L = occ_lds(H, W, out_h, out_w, gray ? 1 : 3, mb);
  MSML_CHECK(L.total <= 160 * 1024, MSML_ERR_UNSUPPORTED,
             "%s: %dx%d -> %dx%d %s needs %ld bytes of LDS (163840 available)", name, H, W, out_h, out_w,
             gray ? "gray" : "RGB", L.total);
  if ((int)L.total > *attr_lds) {               // (monotonic; racing callers set the same or a larger value)
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total);
    *attr_lds = (int)L.total;
  }
  *lds_bytes = L.total;
  return MSML_OK;
}

extern "C" int msml_occ_apply_out(const unsigned char* src, const int* desc, const unsigned char* patch,
                                  long patch_stride, const int* tabw, const int* tabh, float* img, long* msk, float* ori,
                                  int N, int H, int W, int out_h, int out_w, int gray, int norm, int light, void* stream) {
  MSML_CHECK(src && desc && img && msk && N > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0 && H <= 4096 && W <= 4096 &&
                 out_h <= 4096 && out_w <= 4096 && (patch == nullptr || patch_stride > 0),
             MSML_ERR_SHAPE, "occ_apply_out: bad arguments N=%d H=%d W=%d out=%dx%d", N, H, W, out_h, out_w);
  static int attr_lds = 0;
  long lds = 0;
  const int rc = occ_out_setup("occ_apply_out", reinterpret_cast<const void*>(&k_occ_apply_out), &attr_lds, false, tabw,
                               tabh, H, W, out_h, out_w, gray, &lds);
  if (rc != MSML_OK) return rc;
  k_occ_apply_out<<<N, OCC_OUT_T, (size_t)lds, (hipStream_t)stream>>>(src, desc, patch, patch_stride, tabw, tabh, img, msk, ori, H, W, out_h, out_w, gray, norm, light);
  MSML_LAUNCH_OK("occ_apply_out");
  return MSML_OK;
}

// ---------------------------------------------------------------- facial-mask samples
// FaceByRandOccMask.__getitem__ with mask_flag (datasets/load_dataset.py:113-139,167-177) and _add_gauss_to_mask
// (:203-280) as an OVERLAY: launched after k_occ_apply / k_occ_apply_out, which wrote every sample -- a mask sample (kind 8,
// words 1-4 zero) as a clean one, and ori, the clean src face, for good.  A workgroup whose image is not a mask sample, or
// whose row is not one of the M the caller holds, returns before it reads anything else; the others rewrite img and msk:
//   masked[row] -> convert('L') when gray -> Resize (the two fixed-point passes of k_occ_apply_out) -> flip -> ToTensor
//   -> light at the output size, / max  (_add_gauss_to_face, unchanged)
//   mask[row]   -> Resize -> flip -> value <= 128 ? 0 (occluded) : 1  (:210-212, :278; NOT the != 255 of the occluders)
//   msk_light   =  float16 offset on the occluded pixels inside the rectangle (words 17-20, output pixels):
//       type 0  (exp(-0.5 d^2 / r^2) - 0.5) * 2 * 0.4 * sign, d from the int16-truncated  (x - lx) - cx,  (y - ly) - cy
//               (_get_gauss :319-323 subtracts the ABSOLUTE centre from the RELATIVE coordinate; restated as written),
//               r^2 = f32(r * r in f64) as numpy divides an f32 array by a Python float
//       type 1  a standard normal (occ_mask_normal)
//       type 2  sign (black or white block)
//     types 0 / 1: times the channel's jitter bit (:261); gray: (0.2989 l0 + 0.5870 l1 + 0.1140 l2) / 3 with every
//     operation rounded to float16 (:265-267)
//   img = face - msk_light in f32, not clamped (:271) -> Normalize only when asked.
// LDS as k_occ_apply_out without the clean planes, plus MB [oh][ow], the binarised mask the last pass reads
// (occ_lds with mb).
// The standard normal of output pixel (x, y) of image `img` (= offset + n), as a float16: a key domain of its own
// (seed + "mask"), keyed by the absolute pixel, so it depends on nothing else: r = mix(key + y * 65536 + x) with the image's
// key = mix(mix(seed + 0x6D61736B) + img), which k_occ_draw leaves in words 28 (low half) and 29 (high half).  Box-Muller
// in f32 from two 24-bit uniforms, the first in (0, 1]: u1 = ((r >> 40) + 1) / 2^24, u2 = ((r >> 8) & 0xFFFFFF) / 2^24,
// z = sqrt(-2 ln u1) * cos(2 pi u2).
__device__ __forceinline__ __half occ_mask_normal(unsigned long long key, int x, int y) {
  const unsigned long long r = occ_mix(key + (unsigned long long)(y * 65536 + x));
  const float u1 = (float)((unsigned int)(r >> 40) + 1u) * (1.0f / 16777216.0f);
  const float u2 = (float)((unsigned int)(r >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
  const float rad = sqrtf(-2.0f * logf(u1));
  const float ang = 6.2831854820251465f * u2;
  return __float2half(rad * cosf(ang));
}
__device__ __forceinline__ __half occ_hmul(__half a, __half b) { return __float2half(__half2float(a) * __half2float(b)); }
__device__ __forceinline__ __half occ_hadd(__half a, __half b) { return __float2half(__half2float(a) + __half2float(b)); }

__global__ void __launch_bounds__(OCC_OUT_T) k_occ_apply_mask(
    const unsigned char* __restrict__ masked, const unsigned char* __restrict__ mask, const int* __restrict__ rows, int M,
    const int* __restrict__ desc, const int* __restrict__ tabw, const int* __restrict__ tabh, float* __restrict__ img,
    long* __restrict__ msk, int H, int W, int oh, int ow, int gray, int norm, int light) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smm[];
  const int n = blockIdx.x, t = threadIdx.x;
  // both tests are uniform over the workgroup and come before the first barrier
  if (desc[n * OCC_DESC] != OCC_MASK) return;
  const int row = rows ? rows[n] : n;
  if (row < 0 || row >= M) return;               // no render for this sample: it stays the clean one
  const int C = gray ? 1 : 3, HW = H * W, ohow = oh * ow;
  const OccLds L = occ_lds(H, W, oh, ow, C, true);
  int* d = reinterpret_cast<int*>(smm);
  float* red = reinterpret_cast<float*>(smm + OCC_DESC * 4);
  const int* tw = ow != W ? reinterpret_cast<const int*>(smm + L.tabw) : nullptr;
  const int* th = oh != H ? reinterpret_cast<const int*>(smm + L.tabh) : nullptr;
  unsigned char* raw = smm + L.raw;
  unsigned char* Mk = smm + L.mk;
  unsigned char* S = smm + L.s;
  unsigned char* Bh = smm + L.bh;
  unsigned char* O = smm + L.o;
  unsigned char* MB = smm + L.mb;
  MSML_LDS_REGION(MB, (long)ohow);
  occ_stage_tables(smm, L, tw != nullptr, th != nullptr, desc, tabw, tabh, n, oh, ow, t);
  occ_stage_bytes(raw, masked + (long)row * HW * 3, HW * 3, t);
  occ_stage_bytes(Mk, mask + (long)row * HW, HW, t);
  __syncthreads();
  const bool flip = d[8] != 0;
  // planes: 0 = mask, 1 .. C = rendered face
  for (int pl = 0; pl <= C; pl++) {
    const int c = pl == 0 ? 0 : pl - 1;
    const unsigned char* P = Mk;
    if (pl > 0) {
      for (int p = t; p < HW; p += OCC_OUT_T) {
        const unsigned char* q = raw + p * 3;
        S[p] = (unsigned char)(gray ? occ_luma(q[0], q[1], q[2]) : q[c]);
      }
      __syncthreads();
      P = S;
    }
    const unsigned char* Q = P;                       // [H][ow]
    if (tw) {
      occ_pass_h(P, Bh, tw, H, W, ow, t);
      __syncthreads();
      Q = Bh;
    }
    // vertical pass + flip, four outputs per lane: the mask goes to HBM and, binarised, to MB; the face to O
    for (int i = t; i < ohow / 4; i += OCC_OUT_T) {
      const int p = i * 4, yy = p / ow, x = p - yy * ow;
      int v[4];
      occ_pass_v4(Q, th, ow, yy, x, flip, v);
      if (pl == 0) {                                  // :212: <= 128 -> 0 (occluded), else 255; :278: // 255
        longlong2 a, b;
        a.x = v[0] > 128; a.y = v[1] > 128; b.x = v[2] > 128; b.y = v[3] > 128;
        longlong2* o = reinterpret_cast<longlong2*>(msk + (long)n * ohow + p);
        o[0] = a;
        o[1] = b;
        reinterpret_cast<unsigned int*>(MB)[i] = (unsigned int)(v[0] > 128) | ((unsigned int)(v[1] > 128) << 8) |
                                                 ((unsigned int)(v[2] > 128) << 16) | ((unsigned int)(v[3] > 128) << 24);
      } else {
        reinterpret_cast<unsigned int*>(O + (long)c * ohow)[i] =
            (unsigned int)v[0] | ((unsigned int)v[1] << 8) | ((unsigned int)v[2] << 16) | ((unsigned int)v[3] << 24);
      }
    }
    __syncthreads();                                  // S / Bh are rebuilt for the next plane; O and MB are complete after the last
  }
  const float lcx = __int_as_float(d[9]), lcy = __int_as_float(d[10]), lscale = __int_as_float(d[11]);
  float vmax = 0.f;
  if (light) {
    occ_light_max_waves(O, C, ohow, ow, lcx, lcy, lscale, red, t);
    __syncthreads();
    vmax = occ_light_max_fold(red);
  }
  const int type = d[16], lx = d[17], ly = d[18], rx = d[19], ry = d[20];
  const float sgn = (float)d[21];
  const double mcx = (double)__int_as_float(d[25]), mcy = (double)__int_as_float(d[26]);
  const float mrad = __int_as_float(d[27]);
  const float r2 = (float)((double)mrad * (double)mrad);
  const unsigned long long nkey = ((unsigned long long)(unsigned int)d[29] << 32) | (unsigned long long)(unsigned int)d[28];
  const __half hzero = __float2half(0.f);
  // float16(0.2989), float16(0.5870), float16(0.1140), float16(3)
  const __half k0 = __float2half(0.298828125f), k1 = __float2half(0.5869140625f), k2 = __float2half(0.114013671875f);
  for (int i = t; i < ohow / 4; i += OCC_OUT_T) {
    const int p = i * 4, y = p / ow, x = p - y * ow;
    const unsigned int mb = reinterpret_cast<const unsigned int*>(MB)[i];
    float l[4];
    __half m16[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      l[e] = light ? occ_lightmap(x + e, y, lcx, lcy, lscale) : 1.f;
      const int X = x + e;
      m16[e] = hzero;
      if (((mb >> (8 * e)) & 255u) == 0u && X >= lx && X < rx && y >= ly && y < ry) {
        if (type == 0) {
          const int ix = (int)((double)(X - lx) - mcx), iy = (int)((double)(y - ly) - mcy);
          const float dist = sqrtf((float)(ix * ix + iy * iy));
          const float g = expf(-0.5f * (dist * dist) / r2);
          m16[e] = __float2half((g - 0.5f) * 2.0f * 0.4f * sgn);
        } else if (type == 1) {
          m16[e] = occ_mask_normal(nkey, X, y);
        } else {
          m16[e] = __float2half(sgn);
        }
      }
    }
    __half off[3][4];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int e = 0; e < 4; e++) off[c][e] = (type == 2 || d[22 + c] != 0) ? m16[e] : hzero;
    if (gray) {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const __half s = occ_hadd(occ_hadd(occ_hmul(k0, off[0][e]), occ_hmul(k1, off[1][e])), occ_hmul(k2, off[2][e]));
        off[0][e] = __float2half(__half2float(s) / 3.0f);
      }
    }
    for (int c = 0; c < C; c++) {
      const unsigned int wd = reinterpret_cast<const unsigned int*>(O + (long)c * ohow)[i];
      f32x4 r;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float v = (float)((wd >> (8 * e)) & 255u) / 255.0f;
        v *= l[e];
        if (light) v = v / vmax;                      // out_img / out_img.max()  (load_dataset.py:199)
        v = v - __half2float(c == 0 ? off[0][e] : (c == 1 ? off[1][e] : off[2][e]));      // :271
        r[e] = norm ? (v - 0.5f) / 0.5f : v;
      }
      *reinterpret_cast<f32x4*>(img + ((long)n * C + c) * ohow + p) = r;
    }
  }
}

extern "C" int msml_occ_draw_mask(long seed, long offset, int N, int H, int W, int out_h, int out_w, int mode, int lo,
                                  int hi, int flip, const int* meta, int nsets, float p_mask, int* desc, void* stream) {
  MSML_CHECK(desc && N > 0 && H >= 32 && W >= 32 && out_h > 0 && out_w > 0 && mode >= 0 && mode <= 9 && lo >= 0 &&
                 hi > lo && hi <= 101 && p_mask >= 0.f && p_mask <= 1.f, MSML_ERR_SHAPE,
             "occ_draw_mask: bad arguments N=%d H=%d W=%d out=%dx%d mode=%d lo=%d hi=%d p_mask=%g", N, H, W, out_h, out_w,
             mode, lo, hi, (double)p_mask);
  MSML_CHECK(mode < 5 || (meta && nsets > 0 && nsets <= 16), MSML_ERR_SHAPE,
             "occ_draw_mask: modes 5-9 need 1..16 occluder sets (got %d)", nsets);
  MSML_CHECK(p_mask == 0.f || (out_h >= 111 && out_w >= 110), MSML_ERR_SHAPE,
             "occ_draw_mask: the mask rectangle (up to x 110, y 111) does not fit an output of %dx%d", out_h, out_w);
  return occ_draw_launch("occ_draw_mask", seed, offset, N, H, W, mode, lo, hi, flip, mode < 5 ? nullptr : meta,
                         mode < 5 ? 0 : nsets, desc, out_h, out_w, p_mask, stream);
}

extern "C" int msml_occ_apply_mask(const unsigned char* masked, const unsigned char* mask, const int* rows, int M,
                                   const int* desc, const int* tabw, const int* tabh, float* img, long* msk, int N,
                                   int H, int W, int out_h, int out_w, int gray, int norm, int light, void* stream) {
  MSML_CHECK(masked && mask && desc && img && msk && N > 0 && M > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0 &&
                 H <= 4096 && W <= 4096 && out_h <= 4096 && out_w <= 4096 && (rows || M >= N),
             MSML_ERR_SHAPE, "occ_apply_mask: bad arguments N=%d M=%d H=%d W=%d out=%dx%d", N, M, H, W, out_h, out_w);
  static int attr_lds = 0;
  long lds = 0;
  const int rc = occ_out_setup("occ_apply_mask", reinterpret_cast<const void*>(&k_occ_apply_mask), &attr_lds, true, tabw,
                               tabh, H, W, out_h, out_w, gray, &lds);
  if (rc != MSML_OK) return rc;
  k_occ_apply_mask<<<N, OCC_OUT_T, (size_t)lds, (hipStream_t)stream>>>(masked, mask, rows, M, desc, tabw, tabh, img, msk, H, W, out_h, out_w, gray, norm, light);
  MSML_LAUNCH_OK("occ_apply_mask");
  return MSML_OK;
}
