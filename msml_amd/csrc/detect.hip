// MTCNN face detection on the device (eval/preprocess/mtcnn.py detect_faces and eval/preprocess/mtcnn_pytorch/src/
// {first_stage, box_utils, get_nets}.py): every step between the packed uint8 sources and the final boxes / landmarks.
//   k_det_resample   PIL Image.resize(BILINEAR) of a window of a source (the whole image for a pyramid level, a box with
//                    zeros outside the image for a 24 / 48 crop) + (x - 127.5) * 0.0078125, Pillow's 22-bit fixed-point
//                    coefficients computed in the kernel in f64 (boxes are device data; a pyramid shrink needs 12+ taps)
//   k_det_pnet       P-Net fused per 8 x 8 output tile: conv1 + PReLU + ceil-mode pool, conv2, conv3, the 1x1 heads; LDS
//   k_det_cand       the reference's softmax ALONG THE WIDTH of the class map, threshold, ordered compaction, boxes
//   k_det_nms        greedy NMS per segment in the reference's order (stable argsort from the end: ties -> higher index)
//   k_det_compact    rows gathered in pick order
//   k_det_refine     calibrate_box, convert_to_square, round, correct_bboxes WITH its in-place clipping, crop jobs
//   k_det_conv / k_det_pool / k_det_fc   R-Net and O-Net: direct f32 kernels, Flatten's transpose folded into the weight
//   k_det_select     class softmax, threshold, offsets / landmarks into the rows
// Box arithmetic is f64 with contraction off and is restated operation by operation in tests/mtcnn_cases.py; the nets
// are f32 FMA.  A row is DET_COLS doubles: x1 y1 x2 y2 score | image | offsets[4] or landmarks[10].
#include "common.h"

#pragma clang fp contract(off)

#define DET_COLS 16
#define DET_NMS_CAP 16384      // rows per NMS segment (one LDS byte each)
#define DET_TILE 8             // P-Net output cells per tile side
#define DET_IN (2 * DET_TILE + 10)
#define DET_P (DET_TILE + 4)   // pooled side
#define DET_C2 (DET_TILE + 2)  // conv2 output side
#define DET_MAX_SIDE 32768     // a crop window's side stays below this: the limit pack_images puts on an image's side
#define DET_KX 16              // horizontal taps kept in LDS per thread; more are recomputed

// ---------------------------------------------------------------------------------------------------------------------
// Pillow's Resample.c for one axis: bilinear (triangle, support 1) precompute_coeffs + normalize_coeffs_8bpc.
struct DetAxis {
  int xmin, cnt;
  double center, ss, ww;
};
__device__ __forceinline__ double det_tri(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
__device__ __forceinline__ DetAxis det_axis(int insz, int outsz, int xx) {
  DetAxis a;
  const double scale = (double)insz / (double)outsz;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * fs;
  a.center = ((double)xx + 0.5) * scale;
  a.ss = 1.0 / fs;
  int xmin = (int)(a.center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(a.center + support + 0.5);
  if (xmax > insz) xmax = insz;
  a.xmin = xmin;
  a.cnt = xmax - xmin;
  double ww = 0.0;
  for (int x = 0; x < a.cnt; ++x) ww += det_tri(((double)(x + xmin) - a.center + 0.5) * a.ss);
  a.ww = ww;
  return a;
}
__device__ __forceinline__ int det_coef(const DetAxis& a, int x) {
  double w = det_tri(((double)(x + a.xmin) - a.center + 0.5) * a.ss);
  if (a.ww != 0.0) w = w / a.ww;
  return (int)(0.5 + w * 4194304.0);          // the triangle filter has no negative lobe
}
__device__ __forceinline__ int det_clip8(int v) {
  v >>= 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// jobs[j] = {image, x0, y0, w, h, out_w, out_h, output offset in floats}; the output is planar [3][out_h][out_w].
// A job with w < 1 or h < 1 (a dropped box) is filled with the value of a black pixel.
__global__ void __launch_bounds__(256) k_det_resample(const unsigned char* __restrict__ src,
                                                      const long* __restrict__ meta, const long* __restrict__ jobs,
                                                      float* __restrict__ out, int chunks) {
  __shared__ int s_kx[DET_KX][256];
  const long j = blockIdx.x / chunks;
  const int chunk = blockIdx.x - (int)(j * chunks);
  const int t = threadIdx.x;
  const long* jb = jobs + j * 8;
  const int ow = (int)jb[5], oh = (int)jb[6];
  const long p = (long)chunk * 256 + t;
  if (p >= (long)ow * oh) return;
  const int oy = (int)(p / ow), ox = (int)(p - (long)oy * ow);
  const int x0 = (int)jb[1], y0 = (int)jb[2], bw = (int)jb[3], bh = (int)jb[4];
  float* o = out + jb[7] + (long)oy * ow + ox;
  const long plane = (long)ow * oh;
  if (bw < 1 || bh < 1) {
    o[0] = o[plane] = o[2 * plane] = (0.0f - 127.5f) * 0.0078125f;
    return;
  }
  const long* mt = meta + jb[0] * 4;
  const unsigned char* base = src + mt[0];
  const int H = (int)mt[1], W = (int)mt[2];
  const long pitch = mt[3];
  const DetAxis ax = det_axis(bw, ow, ox), ay = det_axis(bh, oh, oy);
  const bool cached = ax.cnt <= DET_KX;
  if (cached)
    for (int r = 0; r < ax.cnt; ++r) s_kx[r][t] = det_coef(ax, r);
  // only the taps inside the image are walked: a black pixel adds 0 to a row, and a black row (1 << 21 >> 22 = 0) adds 0
  const int gx0 = x0 + ax.xmin, gy0 = y0 + ay.xmin;
  const int rx_lo = gx0 < 0 ? -gx0 : 0, rx_hi = W - gx0 < ax.cnt ? W - gx0 : ax.cnt;
  const int ry_lo = gy0 < 0 ? -gy0 : 0, ry_hi = H - gy0 < ay.cnt ? H - gy0 : ay.cnt;
  int v0 = 1 << 21, v1 = 1 << 21, v2 = 1 << 21;
  for (int ry = ry_lo; ry < ry_hi; ++ry) {
    const int ky = det_coef(ay, ry);
    int h0 = 1 << 21, h1 = 1 << 21, h2 = 1 << 21;
    const unsigned char* row = base + (long)(gy0 + ry) * pitch;
    for (int rx = rx_lo; rx < rx_hi; ++rx) {
      const int kx = cached ? s_kx[rx][t] : det_coef(ax, rx);
      const unsigned char* px = row + (long)(gx0 + rx) * 3;
      h0 += (int)px[0] * kx;
      h1 += (int)px[1] * kx;
      h2 += (int)px[2] * kx;
    }
    v0 += det_clip8(h0) * ky;
    v1 += det_clip8(h1) * ky;
    v2 += det_clip8(h2) * ky;
  }
  o[0] = ((float)det_clip8(v0) - 127.5f) * 0.0078125f;
  o[plane] = ((float)det_clip8(v1) - 127.5f) * 0.0078125f;
  o[2 * plane] = ((float)det_clip8(v2) - 127.5f) * 0.0078125f;
}

// ---------------------------------------------------------------------------------------------------------------------
// P-Net.  Packed parameters (floats): conv1 w[10][3][3][3] b[10] a[10] | conv2 w[16][10][3][3] b[16] a[16] |
// conv3 w[32][16][3][3] b[32] a[32] | head w[6][32] b[6] (rows 0-1 conv4_1, rows 2-5 conv4_2).
#define PN_W1 0
#define PN_B1 270
#define PN_A1 280
#define PN_W2 290
#define PN_B2 1730
#define PN_A2 1746
#define PN_W3 1762
#define PN_B3 6370
#define PN_A3 6402
#define PN_W4 6434
#define PN_B4 6626
#define PN_TOTAL 6632

__device__ __forceinline__ float det_prelu(float x, float a) { return x > 0.f ? x : a * x; }

// levels[l] = {input offset (floats), H, W, output offset (floats), oh, ow}; tiles[i] = {level, ty, tx}.
// Input planar [3][H][W]; output planar [6][oh][ow] = class logits 0-1, box offsets 2-5.
// Wave w of the four owns a slice of the output channels in conv2 / conv3, so its weight addresses are wave-uniform.
__global__ void __launch_bounds__(256) k_det_pnet(const float* __restrict__ in, const long* __restrict__ levels,
                                                  const int* __restrict__ tiles, const float* __restrict__ prm,
                                                  float* __restrict__ out) {
  __shared__ float s_in[3][DET_IN][DET_IN + 1];
  __shared__ float s_p[10][DET_P][DET_P + 1];
  __shared__ float s_c2[16][DET_C2][DET_C2 + 1];
  __shared__ float s_c3[32][DET_TILE * DET_TILE + 1];
  const int t = threadIdx.x;
  const int* tl = tiles + (long)blockIdx.x * 3;
  const long* lv = levels + (long)tl[0] * 6;
  const int H = (int)lv[1], W = (int)lv[2], oh = (int)lv[4], ow = (int)lv[5];
  const int ty = tl[1], tx = tl[2];
  const float* src = in + lv[0];
  const int iy0 = 2 * DET_TILE * ty, ix0 = 2 * DET_TILE * tx;
  for (int i = t; i < 3 * DET_IN * DET_IN; i += 256) {
    const int c = i / (DET_IN * DET_IN), r = i - c * DET_IN * DET_IN;
    const int y = r / DET_IN, x = r - y * DET_IN;
    const int gy = iy0 + y, gx = ix0 + x;
    s_in[c][y][x] = (gy < H && gx < W) ? src[((long)c * H + gy) * W + gx] : 0.f;
  }
  __syncthreads();
  // conv1 + PReLU + 2x2 ceil-mode max-pool: a thread owns one pooled position, all 10 channels
  const int H1 = H - 2, W1 = W - 2;
  if (t < DET_P * DET_P) {
    const int py = t / DET_P, px = t - py * DET_P;
    float best[10];
#pragma unroll
    for (int c = 0; c < 10; ++c) best[c] = -INFINITY;
    bool any = false;
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx) {
        const int cy = 2 * py + dy, cx = 2 * px + dx;
        if (iy0 + cy >= H1 || ix0 + cx >= W1) continue;
        any = true;
        float v[27];
#pragma unroll
        for (int ci = 0; ci < 3; ++ci)
#pragma unroll
          for (int k = 0; k < 9; ++k) v[ci * 9 + k] = s_in[ci][cy + k / 3][cx + k % 3];
#pragma unroll
        for (int c = 0; c < 10; ++c) {
          float acc = prm[PN_B1 + c];
#pragma unroll
          for (int ci = 0; ci < 3; ++ci) {
            float part = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) part = fmaf(v[ci * 9 + k], prm[PN_W1 + (c * 3 + ci) * 9 + k], part);
            acc += part;
          }
          best[c] = fmaxf(best[c], det_prelu(acc, prm[PN_A1 + c]));
        }
      }
#pragma unroll
    for (int c = 0; c < 10; ++c) s_p[c][py][px] = any ? best[c] : 0.f;
  }
  __syncthreads();
  // conv2 10 -> 16 + PReLU: 128 position slots x 2 channel halves
  {
    const int pos = t & 127, co0 = (t >> 7) * 8;
    if (pos < DET_C2 * DET_C2) {
      const int y = pos / DET_C2, x = pos - y * DET_C2;
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = prm[PN_B2 + co0 + j];
      for (int ci = 0; ci < 10; ++ci) {
        float v[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = s_p[ci][y + k / 3][x + k % 3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float part = 0.f;
#pragma unroll
          for (int k = 0; k < 9; ++k) part = fmaf(v[k], prm[PN_W2 + ((co0 + j) * 10 + ci) * 9 + k], part);
          acc[j] += part;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s_c2[co0 + j][y][x] = det_prelu(acc[j], prm[PN_A2 + co0 + j]);
    }
  }
  __syncthreads();
  // conv3 16 -> 32 + PReLU: 64 positions x 4 channel quarters (one per wave)
  {
    const int pos = t & 63, co0 = (t >> 6) * 8;
    const int y = pos / DET_TILE, x = pos - y * DET_TILE;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = prm[PN_B3 + co0 + j];
    for (int ci = 0; ci < 16; ++ci) {
      float v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] = s_c2[ci][y + k / 3][x + k % 3];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float part = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) part = fmaf(v[k], prm[PN_W3 + ((co0 + j) * 16 + ci) * 9 + k], part);
        acc[j] += part;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_c3[co0 + j][pos] = det_prelu(acc[j], prm[PN_A3 + co0 + j]);
  }
  __syncthreads();
  // the 1x1 heads: 64 positions x 6 outputs
  for (int i = t; i < 6 * DET_TILE * DET_TILE; i += 256) {
    const int h = i / (DET_TILE * DET_TILE), pos = i - h * DET_TILE * DET_TILE;
    const int y = pos / DET_TILE, x = pos - y * DET_TILE;
    const int gy = DET_TILE * ty + y, gx = DET_TILE * tx + x;
    if (gy >= oh || gx >= ow) continue;
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < 32; ++c) acc = fmaf(s_c3[c][pos], prm[PN_W4 + h * 32 + c], acc);
    out[lv[3] + ((long)h * oh + gy) * ow + gx] = acc + prm[PN_B4 + h];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Candidates.  One wave per row of one level's class map.  The reference applies F.softmax(a, dim=-1) to [1][2][h][w]:
// a softmax over the WIDTH, per channel and row; channel 1 is the "probability" it thresholds.  write == 0: counts[row];
// write == 1: the rows at offs[row] in np.where's order (x ascending within the row).
__global__ void __launch_bounds__(64) k_det_cand(const float* __restrict__ maps, const long* __restrict__ levels,
                                                 const double* __restrict__ scales, const long* __restrict__ images,
                                                 const int* __restrict__ rowtab, float thr, int write,
                                                 long* __restrict__ counts, const long* __restrict__ offs,
                                                 double* __restrict__ rows) {
  const int lane = threadIdx.x;
  const int* rt = rowtab + (long)blockIdx.x * 2;
  const int l = rt[0], y = rt[1];
  const long* lv = levels + (long)l * 6;
  const int oh = (int)lv[4], ow = (int)lv[5];
  const float* a1 = maps + lv[3] + ((long)1 * oh + y) * ow;
  float m = -INFINITY;
  for (int x = lane; x < ow; x += 64) m = fmaxf(m, a1[x]);
  m = wave_max(m);
  float s = 0.f;
  for (int x = lane; x < ow; x += 64) s += expf(a1[x] - m);
  s = wave_sum(s);
  long n = write ? offs[blockIdx.x] : 0;
  const double scale = scales[l];
  for (int xb = 0; xb < ow; xb += 64) {
    const int x = xb + lane;
    float p = 0.f;
    bool hit = false;
    if (x < ow) {
      p = expf(a1[x] - m) / s;
      hit = p > thr;
    }
    const unsigned long long mask = __ballot(hit);
    if (hit && write) {
      double* r = rows + (n + __popcll(mask & ((1ull << lane) - 1ull))) * DET_COLS;
      r[0] = rint((2.0 * (double)x + 1.0) / scale);
      r[1] = rint((2.0 * (double)y + 1.0) / scale);
      r[2] = rint((2.0 * (double)x + 1.0 + 12.0) / scale);
      r[3] = rint((2.0 * (double)y + 1.0 + 12.0) / scale);
      r[4] = (double)p;
      r[5] = (double)images[l];
#pragma unroll
      for (int k = 0; k < 4; ++k) r[6 + k] = (double)maps[lv[3] + ((long)(2 + k) * oh + y) * ow + x];
#pragma unroll
      for (int k = 10; k < DET_COLS; ++k) r[k] = 0.0;
    }
    n += __popcll(mask);
  }
  if (!write && lane == 0) counts[blockIdx.x] = n;
}

// ---------------------------------------------------------------------------------------------------------------------
// NMS (box_utils.nms).  One workgroup per segment [seg_off[s], seg_off[s + 1]).  order = np.argsort(score) read from the
// end: descending score, the higher index first among equals.  Rows with valid[i] == 0 take no part.  keep receives the
// picked GLOBAL row indices in pick order at seg_off[s].., -1 behind them; keep_cnt[s] their number.
__device__ __forceinline__ bool det_overlaps(const double* a, const double* b, double thr, int mode_min) {
  const double area_a = (a[2] - a[0] + 1.0) * (a[3] - a[1] + 1.0);
  const double area_b = (b[2] - b[0] + 1.0) * (b[3] - b[1] + 1.0);
  const double ix1 = fmax(a[0], b[0]), iy1 = fmax(a[1], b[1]);
  const double ix2 = fmin(a[2], b[2]), iy2 = fmin(a[3], b[3]);
  const double w = fmax(0.0, ix2 - ix1 + 1.0), h = fmax(0.0, iy2 - iy1 + 1.0);
  const double inter = w * h;
  const double ov = mode_min ? inter / fmin(area_a, area_b) : inter / (area_a + area_b - inter);
  return ov > thr;
}

__global__ void __launch_bounds__(256) k_det_nms(const double* __restrict__ rows, const long* __restrict__ seg_off,
                                                 const unsigned char* __restrict__ valid, double thr, int mode_min,
                                                 int* __restrict__ order, int* __restrict__ keep,
                                                 int* __restrict__ keep_cnt) {
  __shared__ unsigned char s_sup[DET_NMS_CAP];
  __shared__ int s_nv;
  const int t = threadIdx.x;
  const long b0 = seg_off[blockIdx.x];
  const int n = (int)(seg_off[blockIdx.x + 1] - b0);
  if (n > DET_NMS_CAP) {                        // the host refuses this before the launch; never index past the flags
    if (t == 0) keep_cnt[blockIdx.x] = -1;
    return;
  }
  if (t == 0) s_nv = 0;
  int* ord = order + b0;
  for (int i = t; i < n; i += 256) {
    s_sup[i] = 0;
    keep[b0 + i] = -1;
    ord[i] = 0;                                 // NaN scores leave ranks unassigned: every entry stays an index < n
  }
  __syncthreads();
  for (int i = t; i < n; i += 256) {
    if (valid && !valid[b0 + i]) continue;
    const double si = rows[(b0 + i) * DET_COLS + 4];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      if (valid && !valid[b0 + j]) continue;
      const double sj = rows[(b0 + j) * DET_COLS + 4];
      rank += (sj > si || (sj == si && j > i)) ? 1 : 0;
    }
    ord[rank] = i;
    atomicAdd(&s_nv, 1);
  }
  __threadfence_block();
  __syncthreads();
  const int nv = s_nv;
  int cnt = 0;
  for (int k = 0; k < nv; ++k) {
    if (s_sup[k]) continue;                     // workgroup-uniform: final since the barrier of the last pick
    const int i = ord[k];
    if (t == 0) keep[b0 + cnt] = (int)(b0 + i);
    ++cnt;
    const double* bi = rows + (b0 + i) * DET_COLS;
    for (int m = k + 1 + t; m < nv; m += 256)
      if (!s_sup[m] && det_overlaps(bi, rows + (b0 + ord[m]) * DET_COLS, thr, mode_min)) s_sup[m] = 1;
    __syncthreads();
  }
  if (t == 0) keep_cnt[blockIdx.x] = cnt;
}

// out[new_off[s] + k] = rows[keep[seg_off[s] + k]] for k < keep_cnt[s]
__global__ void __launch_bounds__(256) k_det_compact(const double* __restrict__ rows, const int* __restrict__ keep,
                                                     const long* __restrict__ seg_off, const int* __restrict__ keep_cnt,
                                                     const long* __restrict__ new_off, double* __restrict__ out) {
  const long b0 = seg_off[blockIdx.x], d0 = new_off[blockIdx.x];
  const int cnt = keep_cnt[blockIdx.x];
  for (long i = threadIdx.x; i < (long)cnt * DET_COLS; i += 256) {
    const long k = i / DET_COLS, c = i - k * DET_COLS;
    out[(d0 + k) * DET_COLS + c] = rows[(long)keep[b0 + k] * DET_COLS + c];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// calibrate_box with the row's offsets, convert_to_square (which zeroes the score), np.round, then correct_bboxes: the
// crop window is the UNCLIPPED rounded box, and the row keeps the box CLIPPED to the image, as the reference's in-place
// views leave it.  valid[i] = 0 and an empty job for a box that has no pixel inside the image, or a side of DET_MAX_SIDE
// pixels or more.
__global__ void __launch_bounds__(256) k_det_refine(double* __restrict__ rows, const long* __restrict__ meta, long n,
                                                    int size, long* __restrict__ jobs,
                                                    unsigned char* __restrict__ valid) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double* r = rows + i * DET_COLS;
  double x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  {
    const double w = x2 - x1 + 1.0, h = y2 - y1 + 1.0;
    x1 = x1 + w * r[6];
    y1 = y1 + h * r[7];
    x2 = x2 + w * r[8];
    y2 = y2 + h * r[9];
  }
  {
    const double h = y2 - y1 + 1.0, w = x2 - x1 + 1.0;
    const double side = fmax(h, w);
    const double sx = x1 + w * 0.5 - side * 0.5, sy = y1 + h * 0.5 - side * 0.5;
    x2 = sx + side - 1.0;
    y2 = sy + side - 1.0;
    x1 = sx;
    y1 = sy;
  }
  x1 = rint(x1); y1 = rint(y1); x2 = rint(x2); y2 = rint(y2);
  const long img = (long)r[5];
  const double H = (double)meta[img * 4 + 1], W = (double)meta[img * 4 + 2];
  const double w = x2 - x1 + 1.0, h = y2 - y1 + 1.0;
  // a side of DET_MAX_SIDE or more (or a coordinate that is not finite) is refused: the taps of a crop grow with it
  const bool sane = fabs(x1) < 1e9 && fabs(y1) < 1e9 && w < (double)DET_MAX_SIDE && h < (double)DET_MAX_SIDE;
  const bool ok = sane && w >= 1.0 && h >= 1.0 && x2 >= 0.0 && y2 >= 0.0 && x1 <= W - 1.0 && y1 <= H - 1.0;
  long* jb = jobs + i * 8;
  jb[0] = img;
  jb[1] = ok ? (long)x1 : 0;
  jb[2] = ok ? (long)y1 : 0;
  jb[3] = ok ? (long)w : 0;
  jb[4] = ok ? (long)h : 0;
  jb[5] = size;
  jb[6] = size;
  jb[7] = i * 3 * size * size;
  valid[i] = ok ? 1 : 0;
  if (x2 > W - 1.0) x2 = W - 1.0;
  if (y2 > H - 1.0) y2 = H - 1.0;
  if (x1 < 0.0) x1 = 0.0;
  if (y1 < 0.0) y1 = 0.0;
  r[0] = x1; r[1] = y1; r[2] = x2; r[3] = y2;
  r[4] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------
// R-Net / O-Net.  Activations are NCHW f32.  A thread owns one output position and 4 output channels; blockIdx.y picks the
// channel group, so weight addresses are uniform.  Sums are blocked per input channel.
__global__ void __launch_bounds__(256) k_det_conv(const float* __restrict__ in, const float* __restrict__ w,
                                                  const float* __restrict__ b, const float* __restrict__ slope,
                                                  float* __restrict__ out, long total, int Ci, int H, int W, int Co,
                                                  int K) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int Ho = H - K + 1, Wo = W - K + 1;
  const int x = (int)(p % Wo);
  const long q = p / Wo;
  const int y = (int)(q % Ho);
  const long n = q / Ho;
  const int co0 = blockIdx.y * 4;
  float acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = b[co0 + j];
  const float* ip = in + ((n * Ci) * H + y) * W + x;
  const int KK = K * K;
  for (int ci = 0; ci < Ci; ++ci, ip += (long)H * W) {
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < K; ++ky)
      for (int kx = 0; kx < K; ++kx) {
        const float v = ip[ky * W + kx];
#pragma unroll
        for (int j = 0; j < 4; ++j) part[j] = fmaf(v, w[((long)(co0 + j) * Ci + ci) * KK + ky * K + kx], part[j]);
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += part[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    out[((n * Co + co0 + j) * Ho + y) * Wo + x] = det_prelu(acc[j], slope[co0 + j]);
}

// MaxPool2d(K, 2, ceil_mode=True) without padding: windows are cut at the border
__global__ void __launch_bounds__(256) k_det_pool(const float* __restrict__ in, float* __restrict__ out, long total,
                                                  int H, int W, int Ho, int Wo, int K) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int x = (int)(p % Wo);
  const long q = p / Wo;
  const int y = (int)(q % Ho);
  const long nc = q / Ho;
  const float* ip = in + nc * H * W;
  float m = -INFINITY;
  for (int ky = 0; ky < K; ++ky)
    for (int kx = 0; kx < K; ++kx) {
      const int sy = 2 * y + ky, sx = 2 * x + kx;
      if (sy < H && sx < W) m = fmaxf(m, ip[sy * W + sx]);
    }
  out[p] = m;
}

// out[n][o] = act(b[o] + sum_i in[n][i] * wt[i][o]); wt is [In][Out] (transposed at pack time), sums blocked by 32
__global__ void __launch_bounds__(256) k_det_fc(const float* __restrict__ in, const float* __restrict__ wt,
                                                const float* __restrict__ b, const float* __restrict__ slope,
                                                float* __restrict__ out, long total, int In, int Out, int out_pitch) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int o = (int)(p % Out);
  const long n = p / Out;
  const float* ip = in + n * In;
  float acc = b[o];
  for (int i0 = 0; i0 < In; i0 += 32) {
    float part = 0.f;
    const int i1 = i0 + 32 < In ? i0 + 32 : In;
    for (int i = i0; i < i1; ++i) part = fmaf(ip[i], wt[(long)i * Out + o], part);
    acc += part;
  }
  out[n * out_pitch + o] = slope ? det_prelu(acc, slope[o]) : acc;
}

// net[i] = 16 floats: class logits 0-1, offsets 2-5, landmarks 6-15 (O-Net).  valid[i] &= softmax(logits)[1] > thr (f32);
// the row takes the probability as its score.  R-Net (landmarks == 0): the offsets go into the row for the refine step.
// O-Net: landmarks xmin + width * l in f64, stored as f32 values, from the box as it came in; then calibrate_box.
__global__ void __launch_bounds__(256) k_det_select(double* __restrict__ rows, const float* __restrict__ net, long n,
                                                    float thr, int landmarks, unsigned char* __restrict__ valid) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* o = net + i * 16;
  const float m = fmaxf(o[0], o[1]);
  const float e0 = expf(o[0] - m), e1 = expf(o[1] - m);
  const float p = e1 / (e0 + e1);
  double* r = rows + i * DET_COLS;
  if (!(valid[i] && p > thr)) {
    valid[i] = 0;
    return;
  }
  r[4] = (double)p;
  if (!landmarks) {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[6 + k] = (double)o[2 + k];
    return;
  }
  const double x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  const double w = x2 - x1 + 1.0, h = y2 - y1 + 1.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    r[6 + k] = (double)(float)(x1 + w * (double)o[6 + k]);
    r[11 + k] = (double)(float)(y1 + h * (double)o[11 + k]);
  }
  r[0] = x1 + w * (double)o[2];
  r[1] = y1 + h * (double)o[3];
  r[2] = x2 + w * (double)o[4];
  r[3] = y2 + h * (double)o[5];
}

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int msml_det_resample(const unsigned char* src, const long* meta, const long* jobs, float* out, long njobs,
                                 long max_out_px, void* stream) {
  if (njobs == 0) return MSML_OK;
  MSML_CHECK(src && meta && jobs && out && njobs > 0 && max_out_px > 0, MSML_ERR_SHAPE,
             "det_resample: bad arguments (njobs=%ld, max_out_px=%ld)", njobs, max_out_px);
  MSML_CHECK(((uintptr_t)meta & 7) == 0 && ((uintptr_t)jobs & 7) == 0 && ((uintptr_t)out & 3) == 0, MSML_ERR_SHAPE,
             "det_resample: meta and jobs must be 8-byte, out 4-byte aligned");
  const long chunks = (max_out_px + 255) / 256;
  MSML_CHECK(njobs * chunks < 2147483647L, MSML_ERR_SHAPE, "det_resample: %ld jobs of %ld pixels are too many workgroups",
             njobs, max_out_px);
  k_det_resample<<<(unsigned)(njobs * chunks), 256, 0, (hipStream_t)stream>>>(src, meta, jobs, out, (int)chunks);
  MSML_LAUNCH_OK("det_resample");
  return MSML_OK;
}

extern "C" int msml_det_pnet_tile(void) { return DET_TILE; }
extern "C" int msml_det_pnet_params(void) { return PN_TOTAL; }
extern "C" int msml_det_nms_capacity(void) { return DET_NMS_CAP; }

extern "C" int msml_det_pnet(const float* in, const long* levels, const int* tiles, const float* params, float* out,
                             long ntiles, void* stream) {
  if (ntiles == 0) return MSML_OK;
  MSML_CHECK(in && levels && tiles && params && out && ntiles > 0 && ntiles < 2147483647L, MSML_ERR_SHAPE,
             "det_pnet: bad arguments (ntiles=%ld)", ntiles);
  k_det_pnet<<<(unsigned)ntiles, 256, 0, (hipStream_t)stream>>>(in, levels, tiles, params, out);
  MSML_LAUNCH_OK("det_pnet");
  return MSML_OK;
}

extern "C" int msml_det_candidates(const float* maps, const long* levels, const double* scales, const long* images,
                                   const int* rowtab, long nrows, float threshold, int write, long* counts,
                                   const long* offsets, double* rows, void* stream) {
  if (nrows == 0) return MSML_OK;
  MSML_CHECK(maps && levels && scales && images && rowtab && nrows > 0 && nrows < 2147483647L, MSML_ERR_SHAPE,
             "det_candidates: bad arguments (nrows=%ld)", nrows);
  MSML_CHECK(write ? (offsets && rows) : (counts != nullptr), MSML_ERR_SHAPE,
             "det_candidates: the %s pass needs its output", write ? "write" : "count");
  k_det_cand<<<(unsigned)nrows, 64, 0, (hipStream_t)stream>>>(maps, levels, scales, images, rowtab, threshold, write,
                                                              counts, offsets, rows);
  MSML_LAUNCH_OK("det_candidates");
  return MSML_OK;
}

extern "C" int msml_det_nms(const double* rows, const long* seg_off, const unsigned char* valid, long nseg, long max_n,
                            long capacity, double threshold, int mode_min, int* order, int* keep, int* keep_cnt,
                            void* stream) {
  MSML_CHECK(capacity >= 1 && capacity <= DET_NMS_CAP, MSML_ERR_SHAPE, "det_nms: capacity %ld outside 1..%d", capacity,
             DET_NMS_CAP);
  MSML_CHECK(max_n <= capacity, MSML_ERR_CAPACITY,
             "det_nms: a segment holds %ld candidates, more than the capacity of %ld", max_n, capacity);
  if (nseg == 0) return MSML_OK;
  MSML_CHECK(rows && seg_off && order && keep && keep_cnt && nseg > 0 && nseg < 2147483647L && max_n >= 0, MSML_ERR_SHAPE,
             "det_nms: bad arguments (nseg=%ld)", nseg);
  k_det_nms<<<(unsigned)nseg, 256, 0, (hipStream_t)stream>>>(rows, seg_off, valid, threshold, mode_min, order, keep,
                                                             keep_cnt);
  MSML_LAUNCH_OK("det_nms");
  return MSML_OK;
}

extern "C" int msml_det_compact(const double* rows, const int* keep, const long* seg_off, const int* keep_cnt,
                                const long* new_off, double* out, long nseg, void* stream) {
  if (nseg == 0) return MSML_OK;
  MSML_CHECK(rows && keep && seg_off && keep_cnt && new_off && out && nseg > 0 && nseg < 2147483647L, MSML_ERR_SHAPE,
             "det_compact: bad arguments (nseg=%ld)", nseg);
  k_det_compact<<<(unsigned)nseg, 256, 0, (hipStream_t)stream>>>(rows, keep, seg_off, keep_cnt, new_off, out);
  MSML_LAUNCH_OK("det_compact");
  return MSML_OK;
}

extern "C" int msml_det_refine(double* rows, const long* meta, long n, int size, long* jobs, unsigned char* valid,
                               void* stream) {
  if (n == 0) return MSML_OK;
  MSML_CHECK(rows && meta && jobs && valid && n > 0 && size > 0, MSML_ERR_SHAPE, "det_refine: bad arguments (n=%ld)", n);
  k_det_refine<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(rows, meta, n, size, jobs, valid);
  MSML_LAUNCH_OK("det_refine");
  return MSML_OK;
}

extern "C" int msml_det_select(double* rows, const float* net, long n, float threshold, int landmarks,
                               unsigned char* valid, void* stream) {
  if (n == 0) return MSML_OK;
  MSML_CHECK(rows && net && valid && n > 0, MSML_ERR_SHAPE, "det_select: bad arguments (n=%ld)", n);
  k_det_select<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(rows, net, n, threshold, landmarks, valid);
  MSML_LAUNCH_OK("det_select");
  return MSML_OK;
}

// One layer table per net: {kind (0 conv, 1 pool, 2 fc, 3 heads), Ci / In, Co / Out, K}.  Packed parameters follow the
// table in order: conv w[Co][Ci][K][K] b[Co] a[Co]; fc wt[In][Out] b[Out] a[Out]; heads wt[In][16] b[16].
struct DetLayer {
  int kind, ci, co, k;
};
static const DetLayer RNET[] = {{0, 3, 28, 3}, {1, 0, 0, 3}, {0, 28, 48, 3}, {1, 0, 0, 3}, {0, 48, 64, 2},
                                {2, 576, 128, 0}, {3, 128, 16, 0}};
static const DetLayer ONET[] = {{0, 3, 32, 3}, {1, 0, 0, 3}, {0, 32, 64, 3}, {1, 0, 0, 3}, {0, 64, 64, 3},
                                {1, 0, 0, 2}, {0, 64, 128, 2}, {2, 1152, 256, 0}, {3, 256, 16, 0}};

// floats of one ping-pong half of the workspace per crop (the largest activation: conv1's output)
static long det_net_half(int net) { return net == 0 ? 28L * 22 * 22 : 32L * 46 * 46; }

extern "C" long msml_det_net_workspace(int net, long n) { return 2 * det_net_half(net) * n * (long)sizeof(float); }

extern "C" long msml_det_net_params(int net) {
  const DetLayer* L = net == 0 ? RNET : ONET;
  const int nl = net == 0 ? 7 : 9;
  long total = 0;
  for (int i = 0; i < nl; ++i) {
    if (L[i].kind == 0) total += (long)L[i].co * L[i].ci * L[i].k * L[i].k + 2 * L[i].co;
    if (L[i].kind == 2) total += (long)L[i].ci * L[i].co + 2 * L[i].co;
    if (L[i].kind == 3) total += (long)L[i].ci * 16 + 16;
  }
  return total;
}

// net 0: R-Net on in [n][3][24][24]; net 1: O-Net on in [n][3][48][48].  out [n][16] as k_det_select reads it.
extern "C" int msml_det_net(int net, const float* in, const float* params, long n, float* ws, long ws_bytes, float* out,
                            void* stream) {
  MSML_CHECK(net == 0 || net == 1, MSML_ERR_UNSUPPORTED, "det_net: net %d is neither R-Net (0) nor O-Net (1)", net);
  if (n == 0) return MSML_OK;
  MSML_CHECK(in && params && ws && out && n > 0, MSML_ERR_SHAPE, "det_net: bad arguments (n=%ld)", n);
  MSML_CHECK(ws_bytes >= msml_det_net_workspace(net, n), MSML_ERR_WORKSPACE, "det_net: workspace %ld < %ld bytes", ws_bytes,
             msml_det_net_workspace(net, n));
  const DetLayer* L = net == 0 ? RNET : ONET;
  const int nl = net == 0 ? 7 : 9;
  int C = 3, H = net == 0 ? 24 : 48, W = H;
  const float* cur = in;
  float* half[2] = {ws, ws + det_net_half(net) * n};
  int which = 0;
  const float* p = params;
  for (int i = 0; i < nl; ++i) {
    const DetLayer& l = L[i];
    float* dst = half[which];
    if (l.kind == 0) {
      const int Ho = H - l.k + 1, Wo = W - l.k + 1;
      const long total = n * Ho * Wo;
      MSML_CHECK(total < 256L * 2147483647L, MSML_ERR_SHAPE, "det_net: n=%ld is too many workgroups", n);
      const float* w = p;
      const float* b = w + (long)l.co * l.ci * l.k * l.k;
      const float* a = b + l.co;
      p = a + l.co;
      k_det_conv<<<dim3((unsigned)cdiv(total, 256), l.co / 4), 256, 0, (hipStream_t)stream>>>(cur, w, b, a, dst, total, l.ci,
                                                                                            H, W, l.co, l.k);
      C = l.co; H = Ho; W = Wo;
    } else if (l.kind == 1) {
      const int Ho = (H - l.k + 1) / 2 + 1, Wo = (W - l.k + 1) / 2 + 1;      // ceil((H - K) / 2) + 1
      const long total = n * C * Ho * Wo;
      k_det_pool<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(cur, dst, total, H, W, Ho, Wo, l.k);
      H = Ho; W = Wo;
    } else if (l.kind == 2) {
      MSML_CHECK(C * H * W == l.ci, MSML_ERR_SHAPE, "det_net: flatten gives %d, the layer takes %d", C * H * W, l.ci);
      const float* w = p;
      const float* b = w + (long)l.ci * l.co;
      const float* a = b + l.co;
      p = a + l.co;
      const long total = n * l.co;
      k_det_fc<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(cur, w, b, a, dst, total, l.ci, l.co, l.co);
    } else {
      const float* w = p;
      const float* b = w + (long)l.ci * 16;
      p = b + 16;
      const long total = n * 16;
      k_det_fc<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(cur, w, b, nullptr, out, total, l.ci, 16, 16);
    }
    MSML_LAUNCH_OK("det_net");
    cur = dst;
    which ^= 1;
  }
  return MSML_OK;
}
