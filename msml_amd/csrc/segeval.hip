// Evaluation of the occlusion segmentation branch on the device: what the reference only looks at by eye (train.py:357-364
// saves _seg.jpg beside _gt_occ.jpg, eval/qeval_mxnet.py:350-363 _learned.jpg beside _truth.jpg).
//   k_seg_counts      confusion counts (tp, fp, fn, tn) of a predicted mask against the ground truth, one workgroup per
//                     image, 16-byte loads where the image's planes start on 16 bytes
//   k_seg_label       connected components of the occluded pixels (the `blobs` of tricks/consensus_loss.py:83), one workgroup
//                     per image, a union-find on an LDS parent plane, numbered in raster order of the first pixel
//   k_seg_blob_table  area, overlap with a second mask and bounding box of every component (LDS integer atomics)
// Integers only: no floating-point arithmetic beyond the b > a comparison of two logits, every run gives the same bits.
// tests/segeval_cases.py restates all of it in numpy.
#include <mutex>

#include "common.h"

#define SEG_MAX_SIDE 256         // largest H, W
#define SEG_LABEL_MAX 16384      // largest H * W of the labelling: the parent plane is 64 KiB of LDS
#define SEG_CAP_MAX 1024         // largest blob table
#define SEG_THREADS 1024
#define SEG_SLABS (SEG_LABEL_MAX / SEG_THREADS)      // pixels per thread of the labelling: pixel k * 1024 + t, k < 16
#define SEG_WAVES (SEG_THREADS / 64)

typedef __attribute__((ext_vector_type(2))) long i64x2;

// ---- the class rule --------------------------------------------------------------------------------------------
// logits: clean iff b > a in f32 (ties, NaN: occluded); index masks: 0 occluded.
__device__ __forceinline__ bool seg_logit_occ(float a, float b) { return !(b > a); }

// one pixel of image n, any kind (the labelling and the table: `kind` is uniform over the launch)
__device__ __forceinline__ bool seg_occ1(const void* p, int kind, long n, long HW, long i) {
  switch (kind) {
    case MSML_SEG_LOGITS_F32: {
      const float* q = reinterpret_cast<const float*>(p) + 2 * n * HW;
      return seg_logit_occ(q[i], q[HW + i]);
    }
    case MSML_SEG_LOGITS_BF16: {
      const unsigned short* q = reinterpret_cast<const unsigned short*>(p) + 2 * n * HW;
      return seg_logit_occ(bf2f(q[i]), bf2f(q[HW + i]));
    }
    case MSML_SEG_INDEX_U8:
      return reinterpret_cast<const unsigned char*>(p)[n * HW + i] == 0;
    default:
      return reinterpret_cast<const long*>(p)[n * HW + i] == 0;
  }
}

// Do the planes of image n start on 16 bytes (8 for the byte mask, which is read 8 bytes at a time)?
template <int KIND>
__device__ __forceinline__ bool seg_aligned(const void* p, long n, long HW) {
  if (KIND == MSML_SEG_LOGITS_F32) {
    const uintptr_t a = (uintptr_t)(reinterpret_cast<const float*>(p) + 2 * n * HW);
    return ((a | (a + (uintptr_t)HW * 4)) & 15) == 0;
  }
  if (KIND == MSML_SEG_LOGITS_BF16) {
    const uintptr_t a = (uintptr_t)(reinterpret_cast<const unsigned short*>(p) + 2 * n * HW);
    return ((a | (a + (uintptr_t)HW * 2)) & 15) == 0;
  }
  if (KIND == MSML_SEG_INDEX_U8) return ((uintptr_t)(reinterpret_cast<const unsigned char*>(p) + n * HW) & 7) == 0;
  return ((uintptr_t)(reinterpret_cast<const long*>(p) + n * HW) & 15) == 0;
}

// Pixels i .. i + 7 of image n (i % 8 == 0, seg_aligned): bit j set = pixel i + j occluded.
template <int KIND>
__device__ __forceinline__ unsigned int seg_occ8(const void* p, long n, long HW, long i) {
  unsigned int bits = 0;
  if (KIND == MSML_SEG_LOGITS_F32) {
    const float* q = reinterpret_cast<const float*>(p) + 2 * n * HW + i;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(q), a1 = *reinterpret_cast<const f32x4*>(q + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(q + HW), b1 = *reinterpret_cast<const f32x4*>(q + HW + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bits |= (unsigned int)seg_logit_occ(a0[j], b0[j]) << j;
      bits |= (unsigned int)seg_logit_occ(a1[j], b1[j]) << (4 + j);
    }
  } else if (KIND == MSML_SEG_LOGITS_BF16) {
    const unsigned short* q = reinterpret_cast<const unsigned short*>(p) + 2 * n * HW + i;
    const u32x4 a = *reinterpret_cast<const u32x4*>(q), b = *reinterpret_cast<const u32x4*>(q + HW);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bits |= (unsigned int)seg_logit_occ(__uint_as_float(a[j] << 16), __uint_as_float(b[j] << 16)) << (2 * j);
      bits |= (unsigned int)seg_logit_occ(__uint_as_float(a[j] & 0xffff0000u), __uint_as_float(b[j] & 0xffff0000u))
              << (2 * j + 1);
    }
  } else if (KIND == MSML_SEG_INDEX_U8) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned char*>(p) + n * HW + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) bits |= (unsigned int)(((v[j >> 2] >> (8 * (j & 3))) & 255u) == 0u) << j;
  } else {
    const long* q = reinterpret_cast<const long*>(p) + n * HW + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const i64x2 v = *reinterpret_cast<const i64x2*>(q + 2 * j);
      bits |= (unsigned int)(v[0] == 0) << (2 * j);
      bits |= (unsigned int)(v[1] == 0) << (2 * j + 1);
    }
  }
  return bits;
}

template <int KIND>
__device__ __forceinline__ bool seg_occ1k(const void* p, long n, long HW, long i) {
  return seg_occ1(p, KIND, n, HW, i);
}

__device__ __forceinline__ int seg_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- confusion counts ------------------------------------------------------------------------------------------
// One workgroup per image.  A thread counts (pred occluded and gt occluded, pred occluded, gt occluded) over its pixels;
// tp, fp, fn, tn follow from the three sums and H W.
template <int PK, int GK>
__global__ void __launch_bounds__(SEG_THREADS) k_seg_counts(const void* __restrict__ pred, const void* __restrict__ gt,
                                                            long* __restrict__ counts, long* __restrict__ total, int HW) {
  __shared__ int s_part[SEG_WAVES][3];
  const long n = blockIdx.x;
  const int t = threadIdx.x;
  const bool vec = seg_aligned<PK>(pred, n, HW) && seg_aligned<GK>(gt, n, HW);
  const int body = vec ? (HW & ~7) : 0;
  int both = 0, po = 0, go = 0;
#pragma unroll 2
  for (int i = t * 8; i < body; i += SEG_THREADS * 8) {
    const unsigned int p = seg_occ8<PK>(pred, n, HW, i), g = seg_occ8<GK>(gt, n, HW, i);
    both += __popc(p & g);
    po += __popc(p);
    go += __popc(g);
  }
  for (int i = body + t; i < HW; i += SEG_THREADS) {
    const bool p = seg_occ1k<PK>(pred, n, HW, i), g = seg_occ1k<GK>(gt, n, HW, i);
    both += p && g;
    po += p;
    go += g;
  }
  both = seg_wave_sum(both);
  po = seg_wave_sum(po);
  go = seg_wave_sum(go);
  if ((t & 63) == 0) {
    s_part[t >> 6][0] = both;
    s_part[t >> 6][1] = po;
    s_part[t >> 6][2] = go;
  }
  __syncthreads();
  if (t == 0) {
    long b = 0, p = 0, g = 0;
    for (int w = 0; w < SEG_WAVES; ++w) {
      b += s_part[w][0];
      p += s_part[w][1];
      g += s_part[w][2];
    }
    const long c[4] = {b, p - b, g - b, (long)HW - p - g + b};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      counts[n * 4 + k] = c[k];
      if (total) atomicAdd(reinterpret_cast<unsigned long long*>(total) + k, (unsigned long long)c[k]);
    }
  }
}

static bool seg_kind_ok(int kind) { return kind >= MSML_SEG_LOGITS_F32 && kind <= MSML_SEG_INDEX_I64; }
static bool seg_is_index(int kind) { return kind == MSML_SEG_INDEX_U8 || kind == MSML_SEG_INDEX_I64; }
// the weakest alignment a kind is read with on the scalar path
static uintptr_t seg_kind_align(int kind) {
  return kind == MSML_SEG_LOGITS_F32 ? 3 : kind == MSML_SEG_LOGITS_BF16 ? 1 : kind == MSML_SEG_INDEX_U8 ? 0 : 7;
}

#define SEG_CHECK_SIZE(who, N, H, W)                                                                              \
  MSML_CHECK((N) >= 1, MSML_ERR_UNSUPPORTED, who ": N=%d", (N));                                                   \
  MSML_CHECK((H) >= 1 && (H) <= SEG_MAX_SIDE && (W) >= 1 && (W) <= SEG_MAX_SIDE, MSML_ERR_UNSUPPORTED,             \
             who ": image %dx%d outside 1..%d", (H), (W), SEG_MAX_SIDE)

extern "C" int msml_seg_counts(const void* pred, int pred_kind, const void* gt, int gt_kind, long* counts, long* total,
                               int N, int H, int W, void* stream) {
  MSML_CHECK(pred && gt && counts, MSML_ERR_SHAPE, "seg_counts: null pointer");
  MSML_CHECK(seg_kind_ok(pred_kind), MSML_ERR_DTYPE, "seg_counts: pred kind %d (0 f32 logits, 1 bf16 logits, 2 uint8 index, "
             "3 int64 index)", pred_kind);
  MSML_CHECK(seg_is_index(gt_kind), MSML_ERR_DTYPE, "seg_counts: gt kind %d (2 uint8 index, 3 int64 index)", gt_kind);
  SEG_CHECK_SIZE("seg_counts", N, H, W);
  MSML_CHECK(((uintptr_t)pred & seg_kind_align(pred_kind)) == 0 && ((uintptr_t)gt & seg_kind_align(gt_kind)) == 0 &&
                 ((uintptr_t)counts & 7) == 0 && ((uintptr_t)total & 7) == 0,
             MSML_ERR_SHAPE, "seg_counts: pred / gt must be aligned to their element, counts / total to 8 bytes");
  const int HW = H * W;
  hipStream_t s = (hipStream_t)stream;
#define SEG_COUNTS_LAUNCH(PK, GK) k_seg_counts<PK, GK><<<N, SEG_THREADS, 0, s>>>(pred, gt, counts, total, HW)
#define SEG_COUNTS_GT(PK)                                                    \
  if (gt_kind == MSML_SEG_INDEX_U8) SEG_COUNTS_LAUNCH(PK, MSML_SEG_INDEX_U8); \
  else SEG_COUNTS_LAUNCH(PK, MSML_SEG_INDEX_I64)
  switch (pred_kind) {
    case MSML_SEG_LOGITS_F32: SEG_COUNTS_GT(MSML_SEG_LOGITS_F32); break;
    case MSML_SEG_LOGITS_BF16: SEG_COUNTS_GT(MSML_SEG_LOGITS_BF16); break;
    case MSML_SEG_INDEX_U8: SEG_COUNTS_GT(MSML_SEG_INDEX_U8); break;
    default: SEG_COUNTS_GT(MSML_SEG_INDEX_I64); break;
  }
#undef SEG_COUNTS_GT
#undef SEG_COUNTS_LAUNCH
  MSML_LAUNCH_OK("seg_counts");
  return MSML_OK;
}

// ---- connected components --------------------------------------------------------------------------------------
// P is the parent plane: -1 on clean pixels, else the index of another pixel of the same component with P[i] <= i.  Every
// write keeps P[i] <= i (the seeds point left, atomicMin only lowers), so a walk strictly descends and ends at a root
// (P[r] == r) within H W steps: the bounds below are never reached on a sound plane, and a thread that does reach one
// reports it instead of going on.
__device__ __forceinline__ bool seg_find(volatile int* P, int& a, int bound) {
  for (int s = 0; s <= bound; ++s) {
    const int p = P[a];
    if (p == a) return true;
    a = p;
  }
  return false;
}

// Merge the components of pixels a and b: link the larger root under the smaller with atomicMin.  When another thread
// has linked that root first (old != a), `old` is what it pointed to before, and is now to be merged with b: a + b falls
// in every round, so 2 H W rounds bound the loop.
__device__ __forceinline__ bool seg_unite(int* P, int a, int b, int bound) {
  for (int it = 0; it <= 2 * bound; ++it) {
    if (!seg_find(P, a, bound) || !seg_find(P, b, bound)) return false;
    if (a == b) return true;
    if (a < b) {
      const int x = a;
      a = b;
      b = x;
    }
    const int old = atomicMin(&P[a], b);
    if (old == a) return true;
    a = old;
  }
  return false;
}

// One workgroup = one image.  Thread t owns the pixels k * 1024 + t (k < 16): consecutive lanes touch consecutive LDS
// words.  Dynamic LDS: P[H W], then cnt[16 slabs][16 waves], then (total, failed).
__global__ void __launch_bounds__(SEG_THREADS) k_seg_label(const void* __restrict__ mask, int kind, int* __restrict__ labels,
                                                           int* __restrict__ count, int* __restrict__ status, int H, int W,
                                                           int conn) {
  extern __shared__ int s_seg[];
  const int HW = H * W;
  int* P = s_seg;
  int* s_cnt = s_seg + HW;
  int* s_flag = s_cnt + SEG_SLABS * SEG_WAVES;           // [0] the number of components, [1] a bound was reached
  MSML_LDS_REGION(s_seg, (size_t)(HW + SEG_SLABS * SEG_WAVES + 2) * sizeof(int));
  const long n = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < 2) s_flag[t] = 0;
  for (int i = t; i < HW; i += SEG_THREADS) P[i] = seg_occ1(mask, kind, n, HW, i) ? i : -1;
  __syncthreads();
  // 1. seeds: every occluded pixel points at the first pixel of its row run (at most W - 1 steps to the left)
  int reg[SEG_SLABS];
#pragma unroll
  for (int k = 0; k < SEG_SLABS; ++k) {
    const int i = k * SEG_THREADS + t;
    int s = -1;
    if (i < HW && P[i] >= 0) {
      s = i;
      for (int x = i % W; x > 0 && P[s - 1] >= 0; --x) --s;
    }
    reg[k] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SEG_SLABS; ++k)
    if (reg[k] >= 0) P[k * SEG_THREADS + t] = reg[k];
  __syncthreads();
  // 2. merges with the row above.  u / ul / ur / l: the pixel above, above left, above right, left is occluded.  A pixel
  // whose left neighbour has the same run above it leaves the merge to that neighbour (its run reaches it), and a
  // diagonal counts only where the pixel above is clean (otherwise the diagonal pixel is in the run of the pixel above).
  bool failed = false;
#pragma unroll 1
  for (int k = 0; k < SEG_SLABS; ++k) {
    const int i = k * SEG_THREADS + t;
    if (i >= HW || i < W || P[i] < 0) continue;
    const int x = i % W;
    const bool u = P[i - W] >= 0;
    const bool l = x > 0 && P[i - 1] >= 0;
    const bool ul = x > 0 && P[i - W - 1] >= 0;
    if (u && !(l && ul)) failed |= !seg_unite(P, i, i - W, HW);
    if (conn == 8 && !u) {
      if (ul && !l) failed |= !seg_unite(P, i, i - W - 1, HW);
      if (x < W - 1 && P[i - W + 1] >= 0) failed |= !seg_unite(P, i, i - W + 1, HW);
    }
  }
  if (failed) s_flag[1] = 1;
  __syncthreads();
  // 3. roots.  The root of a component is its smallest index, its first pixel in raster order: the rank of a root among
  // the roots is the component's number - 1.
  failed = false;
#pragma unroll
  for (int k = 0; k < SEG_SLABS; ++k) {
    const int i = k * SEG_THREADS + t;
    int r = -1;
    if (i < HW && P[i] >= 0) {
      r = i;
      failed |= !seg_find(P, r, HW);
    }
    reg[k] = r;
    const unsigned long long roots = __ballot(r == i && r >= 0);
    if (lane == 0) s_cnt[k * SEG_WAVES + wave] = __popcll(roots);
  }
  if (failed) s_flag[1] = 1;
  __syncthreads();
  if (wave == 0) {                                     // exclusive prefix sum of the 256 (slab, wave) counts
    int c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = s_cnt[lane * 4 + j];
      sum += c[j];
    }
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    int run = incl - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s_cnt[lane * 4 + j] = run;
      run += c[j];
    }
    if (lane == 63) s_flag[0] = incl;
  }
  __syncthreads();
  const bool bad = s_flag[1] != 0;
  if (!bad) {
#pragma unroll
    for (int k = 0; k < SEG_SLABS; ++k) {
      const int i = k * SEG_THREADS + t;
      const bool root = reg[k] == i && reg[k] >= 0;
      const unsigned long long roots = __ballot(root);
      if (root) P[i] = s_cnt[k * SEG_WAVES + wave] + __popcll(roots & ((1ULL << lane) - 1ULL)) + 1;
    }
  }
  __syncthreads();
  if (labels) {
#pragma unroll
    for (int k = 0; k < SEG_SLABS; ++k) {
      const int i = k * SEG_THREADS + t;
      if (i < HW) labels[n * HW + i] = (bad || reg[k] < 0) ? 0 : P[reg[k]];
    }
  }
  if (t == 0) {
    count[n] = bad ? 0 : s_flag[0];
    status[n] = bad ? 2 : 0;
  }
}

extern "C" int msml_seg_label(const void* mask, int kind, int* labels, int* count, int* status, int N, int H, int W,
                              int connectivity, void* stream) {
  MSML_CHECK(mask && count && status, MSML_ERR_SHAPE, "seg_label: null pointer");
  MSML_CHECK(seg_kind_ok(kind), MSML_ERR_DTYPE, "seg_label: mask kind %d (0 f32 logits, 1 bf16 logits, 2 uint8 index, "
             "3 int64 index)", kind);
  SEG_CHECK_SIZE("seg_label", N, H, W);
  MSML_CHECK(H * W <= SEG_LABEL_MAX, MSML_ERR_UNSUPPORTED, "seg_label: %dx%d = %d pixels, more than the %d whose parent "
             "plane fits in LDS", H, W, H * W, SEG_LABEL_MAX);
  MSML_CHECK(connectivity == 4 || connectivity == 8, MSML_ERR_UNSUPPORTED, "seg_label: connectivity %d is not 4 or 8",
             connectivity);
  MSML_CHECK(((uintptr_t)mask & seg_kind_align(kind)) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)count & 3) == 0 &&
                 ((uintptr_t)status & 3) == 0,
             MSML_ERR_SHAPE, "seg_label: mask must be aligned to its element, labels / count / status to 4 bytes");
  constexpr size_t lds_max = (size_t)(SEG_LABEL_MAX + SEG_SLABS * SEG_WAVES + 2) * sizeof(int);
  static std::once_flag once;
  std::call_once(once, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_seg_label), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_max);
  });
  const size_t lds = (size_t)(H * W + SEG_SLABS * SEG_WAVES + 2) * sizeof(int);
  k_seg_label<<<N, SEG_THREADS, lds, (hipStream_t)stream>>>(mask, kind, labels, count, status, H, W, connectivity);
  MSML_LAUNCH_OK("seg_label");
  return MSML_OK;
}

// ---- per-component statistics ----------------------------------------------------------------------------------
// One workgroup = one image; the table rows (area, hit, x0, y0, x1, y1) of its first min(count, cap) components sit in
// LDS and every labelled pixel adds itself with integer atomics.
__global__ void __launch_bounds__(SEG_THREADS) k_seg_blob_table(const int* __restrict__ labels, const int* __restrict__ count,
                                                                const void* __restrict__ b, int b_kind, int* __restrict__ table,
                                                                int H, int W, int cap) {
  __shared__ int s_tab[SEG_CAP_MAX * 6];
  const long n = blockIdx.x;
  const int t = threadIdx.x, HW = H * W;
  int rows = count[n];
  rows = rows < 0 ? 0 : (rows > cap ? cap : rows);
  for (int j = t; j < rows * 6; j += SEG_THREADS) {
    const int f = j % 6;
    s_tab[j] = (f == 2 || f == 3) ? 0x7fffffff : (f >= 4 ? -1 : 0);
  }
  __syncthreads();
  for (int i = t; i < HW; i += SEG_THREADS) {
    const int lab = labels[n * HW + i];
    if (lab < 1 || lab > rows) continue;
    int* row = s_tab + (lab - 1) * 6;
    const int y = i / W, x = i - y * W;
    atomicAdd(row + 0, 1);
    if (seg_occ1(b, b_kind, n, HW, i)) atomicAdd(row + 1, 1);
    atomicMin(row + 2, x);
    atomicMin(row + 3, y);
    atomicMax(row + 4, x);
    atomicMax(row + 5, y);
  }
  __syncthreads();
  for (int j = t; j < cap * 6; j += SEG_THREADS) table[n * cap * 6 + j] = j < rows * 6 ? s_tab[j] : 0;
}

extern "C" int msml_seg_blob_table(const int* labels, const int* count, const void* b, int b_kind, int* table, int N, int H,
                                   int W, int cap, void* stream) {
  MSML_CHECK(labels && count && b && table, MSML_ERR_SHAPE, "seg_blob_table: null pointer");
  MSML_CHECK(seg_kind_ok(b_kind), MSML_ERR_DTYPE, "seg_blob_table: mask kind %d (0 f32 logits, 1 bf16 logits, 2 uint8 index, "
             "3 int64 index)", b_kind);
  SEG_CHECK_SIZE("seg_blob_table", N, H, W);
  MSML_CHECK(cap >= 1 && cap <= SEG_CAP_MAX, MSML_ERR_UNSUPPORTED, "seg_blob_table: cap %d outside 1..%d", cap, SEG_CAP_MAX);
  MSML_CHECK(((uintptr_t)b & seg_kind_align(b_kind)) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)count & 3) == 0 &&
                 ((uintptr_t)table & 3) == 0,
             MSML_ERR_SHAPE, "seg_blob_table: b must be aligned to its element, labels / count / table to 4 bytes");
  k_seg_blob_table<<<N, SEG_THREADS, 0, (hipStream_t)stream>>>(labels, count, b, b_kind, table, H, W, cap);
  MSML_LAUNCH_OK("seg_blob_table");
  return MSML_OK;
}
