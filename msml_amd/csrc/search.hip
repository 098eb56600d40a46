// 1:N identification: for every probe row the k largest inner products with the gallery rows, without ever storing
// the P x G score matrix (msml_search_topk).  The lists the MegaFace / AR writers of the reference prepare
// (datasets/benchmarks/get_list.py:138-208, :100-135) and the IJB-C 1:N galleries are searched this way; the reference
// itself ships no evaluator for them.
//   k_search_tile<T>   one workgroup = one tile of SEARCH_TM probe rows x one split of the gallery columns.  It walks
//                      its split in tiles of SEARCH_TN columns; per tile the reduction over E runs on the 16x16x4 MFMA
//                      of T (f32 / f64) from two LDS stages, and the tile's scores go through LDS into the per-row
//                      sorted lists (k entries, also LDS).  At the end the lists are the split's partial result.
//   k_topk_merge<T>    merges the `splits` partial lists of a probe row.
// Order everywhere: descending score, ties by ascending gallery row (-0.0 == 0.0 tie); a filler is (-inf, -1) and
// loses against every real entry.  Every dot product is one MFMA accumulator chain over the channels in ascending
// order, the same instructions whatever the split or the tile position, there is no atomic and no workgroup waits
// for another: the result has the same bits for every `splits` and in every run.
#include <math.h>

#include "common.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;

#define SEARCH_TM 64          // probe rows of a workgroup: 4 waves x 16
#define SEARCH_TN 64          // gallery columns of a tile: 4 MFMA tiles of every wave
#define SEARCH_KMAX 32        // list length limit (one entry per lane of the lower wave half)
#define SEARCH_SP 65          // row pitch of the score tile in elements
#define SEARCH_MAX_SPLITS 65535

// The 16x16x4 MFMA of T.  A: lane l holds A[l & 15][k = l >> 4]; B: lane l holds B[k = l >> 4][l & 15], for both
// types.  C/D: column l & 15 for both, but the ROW of register r differs: f32 (l >> 4) * 4 + r, f64 (l >> 4) + 4 r.
// KSTEP: channels per LDS stage (128 bytes of a row for both types); PITCH: row pitch of a stage in elements, chosen
// so that the 32 lanes of a half wave (16 rows x 2 channels) read 32 different banks (f32, 4-byte banks modulo 32)
// or 32 different bank pairs (f64, modulo 64).
template <typename T>
struct Mma;
template <>
struct Mma<float> {
  typedef f32x4 Acc;
  static constexpr int KSTEP = 32, PITCH = 34;
  static __device__ __forceinline__ Acc mma(float a, float b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) * 4 + reg; }
};
template <>
struct Mma<double> {
  typedef f64x4 Acc;
  static constexpr int KSTEP = 16, PITCH = 18;
  static __device__ __forceinline__ Acc mma(double a, double b, Acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};

template <typename T>
__device__ __forceinline__ T neg_inf() { return (T)(-INFINITY); }

// (s, i) comes before (t, j) in the result order
template <typename T>
__device__ __forceinline__ bool before(T s, int i, T t, int j) {
  return s > t || (s == t && (unsigned)i < (unsigned)j);
}

// One wave, one probe row.  Lane j < k holds entry j of the row's sorted list in (ls, li); every lane offers one
// candidate (v, gi) when `valid`.  Candidates that come before the list's last entry are taken in ascending lane
// order, each one checked again against the last entry as it stands by then, and inserted at its place: the entries
// behind it move one lane up and the last one leaves.  Returns true when the list changed.
template <typename T>
__device__ __forceinline__ bool topk_insert(T v, int gi, bool valid, int k, int lane, T& ls, int& li) {
  T ts = __shfl(ls, k - 1, 64);
  int ti = __shfl(li, k - 1, 64);
  unsigned long long m = __ballot(valid && before(v, gi, ts, ti));
  bool changed = false;
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const T cs = __shfl(v, src, 64);
    const int ci = __shfl(gi, src, 64);
    if (!before(cs, ci, ts, ti)) continue;              // wave-uniform: the last entry has risen past it
    const int pos = __popcll(__ballot(lane < k && before(ls, li, cs, ci)));
    const T ps = __shfl_up(ls, 1, 64);
    const int pi = __shfl_up(li, 1, 64);
    if (lane > pos) { ls = ps; li = pi; }
    else if (lane == pos) { ls = cs; li = ci; }
    ts = __shfl(ls, k - 1, 64);
    ti = __shfl(li, k - 1, 64);
    changed = true;
  }
  return changed;
}

// 16 bytes at p (when `on`) or zeros
__device__ __forceinline__ u32x4 load_chunk(const char* p, bool on) {
  u32x4 z = {0u, 0u, 0u, 0u};
  return on ? *reinterpret_cast<const u32x4*>(p) : z;
}
// ... into a stage whose rows are only 8-byte aligned
__device__ __forceinline__ void store_chunk(char* p, u32x4 v) {
  u32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
  *reinterpret_cast<u32x2*>(p) = lo;
  *reinterpret_cast<u32x2*>(p + 8) = hi;
}

// grid (probe tiles, splits), 256 threads.  tiles_per_split: column tiles of a split (the last splits may be short or
// empty: they write fillers).  out_s / out_i: [splits][P][k].
template <typename T>
__global__ void __launch_bounds__(256) k_search_tile(const T* __restrict__ probe, long P, const T* __restrict__ gallery,
                                                     int G, int E, int k, int tiles_per_split, T* __restrict__ out_s,
                                                     int* __restrict__ out_i) {
  typedef Mma<T> M;
  typedef typename M::Acc Acc;
  constexpr int KSTEP = M::KSTEP, PITCH = M::PITCH;
  constexpr int EPC = 16 / (int)sizeof(T);                       // elements of a 16-byte chunk
  constexpr int STAGE = SEARCH_TM * PITCH;                       // elements of one operand of one stage
  static_assert(SEARCH_TM == SEARCH_TN && KSTEP * sizeof(T) == 128, "a stage row is 8 chunks for both operands");
  static_assert(4 * STAGE >= SEARCH_TM * SEARCH_SP, "the score tile lies over the stages");
  __shared__ __attribute__((aligned(16))) T s_stage[4 * STAGE];  // [buffer][A | B][row][PITCH]; the score tile over it
  __shared__ T s_ls[SEARCH_TM][SEARCH_KMAX];
  __shared__ int s_li[SEARCH_TM][SEARCH_KMAX];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long p0 = (long)blockIdx.x * SEARCH_TM;
  const int split = blockIdx.y;
  const int n_ct = (G + SEARCH_TN - 1) / SEARCH_TN;
  const int ct0 = split * tiles_per_split;
  const int ct1 = min(ct0 + tiles_per_split, n_ct);
  const int nk = (E + KSTEP - 1) / KSTEP;

  if (lane < SEARCH_KMAX) {
    for (int r = 0; r < 16; ++r) {
      s_ls[wave * 16 + r][lane] = neg_inf<T>();
      s_li[wave * 16 + r][lane] = -1;
    }
  }

  // staging: chunk c = tid + 256 i of an operand: row c >> 3, 16-byte chunk c & 7 of the stage's 128 bytes
  const int c_row[2] = {tid >> 3, (tid + 256) >> 3};
  const int c_ch = tid & 7;
  const size_t row_bytes = (size_t)E * sizeof(T);
  const char* a_ptr[2];
  bool a_on[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    a_on[i] = p0 + c_row[i] < P;
    a_ptr[i] = reinterpret_cast<const char*>(probe) + (size_t)(a_on[i] ? p0 + c_row[i] : 0) * row_bytes + c_ch * 16;
  }
  T* const s_score = s_stage + wave * 16 * SEARCH_SP;            // this wave's 16 rows of the score tile

  for (int ct = ct0; ct < ct1; ++ct) {
    const int g0 = ct * SEARCH_TN;
    const char* b_ptr[2];
    bool b_on[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      b_on[i] = g0 + c_row[i] < G;
      b_ptr[i] = reinterpret_cast<const char*>(gallery) + (size_t)(b_on[i] ? g0 + c_row[i] : 0) * row_bytes + c_ch * 16;
    }
    u32x4 ra[2], rb[2];
    {
      const bool kon = c_ch * EPC < E;                           // E % 4 == 0: a chunk is inside the row or outside
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ra[i] = load_chunk(a_ptr[i], a_on[i] && kon);
        rb[i] = load_chunk(b_ptr[i], b_on[i] && kon);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        store_chunk(reinterpret_cast<char*>(s_stage + c_row[i] * PITCH) + c_ch * 16, ra[i]);
        store_chunk(reinterpret_cast<char*>(s_stage + STAGE + c_row[i] * PITCH) + c_ch * 16, rb[i]);
      }
    }
    __syncthreads();

    Acc acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[n][r] = (T)0;

    for (int ks = 0; ks < nk; ++ks) {
      const bool more = ks + 1 < nk;
      if (more) {                                                // the next stage's loads fly behind the MFMAs
        const int kc = (ks + 1) * KSTEP + c_ch * EPC;
        const bool kon = kc < E;
        const size_t off = (size_t)(ks + 1) * KSTEP * sizeof(T);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          ra[i] = load_chunk(a_ptr[i] + off, a_on[i] && kon);
          rb[i] = load_chunk(b_ptr[i] + off, b_on[i] && kon);
        }
      }
      const T* sa = s_stage + (ks & 1) * 2 * STAGE + (wave * 16 + (lane & 15)) * PITCH + (lane >> 4);
      const T* sb = s_stage + (ks & 1) * 2 * STAGE + STAGE + (lane & 15) * PITCH + (lane >> 4);
#pragma unroll
      for (int kk = 0; kk < KSTEP / 4; ++kk) {                   // channels ascending: 4 kk + (lane >> 4)
        const T a = sa[kk * 4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = M::mma(a, sb[n * 16 * PITCH + kk * 4], acc[n]);
      }
      if (more) {
        T* dst = s_stage + ((ks + 1) & 1) * 2 * STAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          store_chunk(reinterpret_cast<char*>(dst + c_row[i] * PITCH) + c_ch * 16, ra[i]);
          store_chunk(reinterpret_cast<char*>(dst + STAGE + c_row[i] * PITCH) + c_ch * 16, rb[i]);
        }
      }
      __syncthreads();
    }

    // every wave has left the stages: the scores of this wave's 16 rows, column on the lane
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) s_score[M::row(lane, r) * SEARCH_SP + n * 16 + (lane & 15)] = acc[n][r];
    __syncthreads();

    const int gi = g0 + lane;
    const bool valid = gi < G;
    for (int r = 0; r < 16; ++r) {
      const int row = wave * 16 + r;
      if (p0 + row >= P) break;                                  // wave-uniform
      const T v = s_score[r * SEARCH_SP + lane];
      T ls = neg_inf<T>();
      int li = -1;
      if (lane < k) { ls = s_ls[row][lane]; li = s_li[row][lane]; }
      if (topk_insert<T>(v, gi, valid, k, lane, ls, li) && lane < k) {
        s_ls[row][lane] = ls;
        s_li[row][lane] = li;
      }
    }
    __syncthreads();                                             // the next tile's first stage overwrites the scores
  }

  __syncthreads();
  if (lane < k) {
    for (int r = 0; r < 16; ++r) {
      const long prow = p0 + wave * 16 + r;
      if (prow >= P) break;
      const size_t o = ((size_t)split * P + prow) * k + lane;
      out_s[o] = s_ls[wave * 16 + r][lane];
      out_i[o] = s_li[wave * 16 + r][lane];
    }
  }
}

// one wave per probe row: the list of split 0, then the entries of every further split offered to it
template <typename T>
__global__ void __launch_bounds__(256) k_topk_merge(const T* __restrict__ ws_s, const int* __restrict__ ws_i, long P,
                                                    int k, int splits, T* __restrict__ scores,
                                                    int* __restrict__ index) {
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;
  T ls = neg_inf<T>();
  int li = -1;
  if (lane < k) { ls = ws_s[(size_t)p * k + lane]; li = ws_i[(size_t)p * k + lane]; }
  for (int s = 1; s < splits; ++s) {
    T v = neg_inf<T>();
    int gi = -1;
    const size_t o = ((size_t)s * P + p) * k + lane;
    if (lane < k) { v = ws_s[o]; gi = ws_i[o]; }
    topk_insert<T>(v, gi, gi >= 0, k, lane, ls, li);
  }
  if (lane < k) {
    scores[(size_t)p * k + lane] = ls;
    index[(size_t)p * k + lane] = li;
  }
}

// ---------------------------------------------------------------------------------------------------------------
static int search_tiles_per_split(long G, int splits) {
  const int n_ct = cdiv(G, SEARCH_TN);
  return cdiv(n_ct, splits);
}

extern "C" int msml_search_topk_splits(long P, long G, int k) {
  (void)k;
  if (P < 1 || G < 1 || G >= 2147483647L) return 0;
  const long p_tiles = (P + SEARCH_TM - 1) / SEARCH_TM;
  const int n_ct = cdiv(G, SEARCH_TN);
  long want = (3 * 256 + p_tiles - 1) / p_tiles;                 // three workgroups for each of the 256 CUs
  if (want > n_ct) want = n_ct;
  if (want > 1024) want = 1024;
  if (want < 1) want = 1;
  return cdiv(n_ct, cdiv(n_ct, want));                           // no empty split
}

extern "C" size_t msml_search_topk_workspace(long P, int k, int splits) {
  if (P < 1 || k < 1 || splits < 2) return 0;                    // one split writes the result itself
  return (size_t)splits * (size_t)P * (size_t)k * (sizeof(double) + sizeof(int));
}

template <typename T>
static int search_launch(const void* probe, long P, const void* gallery, long G, int E, int k, int splits, void* scores,
                         int* index, void* workspace, hipStream_t st) {
  T* out_s = reinterpret_cast<T*>(scores);
  int* out_i = index;
  if (splits > 1) {
    out_s = reinterpret_cast<T*>(workspace);
    out_i = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + (size_t)splits * P * k * sizeof(double));
  }
  const dim3 grid((unsigned)cdiv(P, SEARCH_TM), (unsigned)splits);
  k_search_tile<T><<<grid, 256, 0, st>>>(reinterpret_cast<const T*>(probe), P, reinterpret_cast<const T*>(gallery),
                                         (int)G, E, k, search_tiles_per_split(G, splits), out_s, out_i);
  MSML_LAUNCH_OK("search_topk");
  if (splits > 1) {
    k_topk_merge<T><<<cdiv(P, 4), 256, 0, st>>>(out_s, out_i, P, k, splits, reinterpret_cast<T*>(scores), index);
    MSML_LAUNCH_OK("search_topk merge");
  }
  return MSML_OK;
}

extern "C" int msml_search_topk(const void* probe, long P, const void* gallery, long G, int E, int k, int splits,
                                int dtype, void* scores, int* index, void* workspace, size_t ws_bytes, void* stream) {
  MSML_CHECK(probe && gallery && scores && index, MSML_ERR_SHAPE, "search_topk: null pointer");
  MSML_CHECK(dtype == MSML_F32 || dtype == MSML_F64, MSML_ERR_SHAPE, "search_topk: dtype %d is not MSML_F32 or MSML_F64",
             dtype);
  MSML_CHECK(P >= 1 && P < 2147483647L && G >= 1 && G < 2147483647L, MSML_ERR_SHAPE,
             "search_topk: bad shape P=%ld G=%ld", P, G);
  MSML_CHECK(E >= 4 && E % 4 == 0, MSML_ERR_SHAPE, "search_topk: E=%d must be a positive multiple of 4 (16-byte loads)",
             E);
  MSML_CHECK(k >= 1 && k <= SEARCH_KMAX, MSML_ERR_SHAPE, "search_topk: k=%d outside 1..%d", k, SEARCH_KMAX);
  MSML_CHECK(k <= G, MSML_ERR_SHAPE, "search_topk: k=%d exceeds the %ld gallery rows", k, G);
  MSML_CHECK(splits >= 1 && splits <= SEARCH_MAX_SPLITS, MSML_ERR_SHAPE, "search_topk: splits=%d outside 1..%d", splits,
             SEARCH_MAX_SPLITS);
  MSML_CHECK(((uintptr_t)probe & 15) == 0 && ((uintptr_t)gallery & 15) == 0, MSML_ERR_SHAPE,
             "search_topk: probe and gallery must be 16-byte aligned");
  MSML_CHECK(((uintptr_t)scores & 7) == 0 && ((uintptr_t)index & 3) == 0, MSML_ERR_SHAPE,
             "search_topk: scores / index misaligned");
  if (splits > 1) {
    const size_t need = msml_search_topk_workspace(P, k, splits);
    MSML_CHECK(workspace && ((uintptr_t)workspace & 7) == 0, MSML_ERR_SHAPE,
               "search_topk: %d splits need an 8-byte aligned workspace", splits);
    MSML_CHECK(ws_bytes >= need, MSML_ERR_SHAPE, "search_topk: workspace holds %zu bytes, %d splits need %zu", ws_bytes,
               splits, need);
  }
  if (dtype == MSML_F64)
    return search_launch<double>(probe, P, gallery, G, E, k, splits, scores, index, workspace, (hipStream_t)stream);
  return search_launch<float>(probe, P, gallery, G, E, k, splits, scores, index, workspace, (hipStream_t)stream);
}
