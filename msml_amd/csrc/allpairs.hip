// All-pairs verification: exact TAR @ FAR over every probe x gallery comparison without ever storing the P x G score
// matrix (msml_allpairs_pass).  This is the second protocol the MegaFace list writer of the reference prepares
// (datasets/benchmarks/get_list.py:138-208: TAR at FAR = 1e-6 over all probe x gallery pairs); the reference ships no
// evaluator for it.  The threshold of a FAR target is an order statistic of the impostor scores, found by a radix
// select on order-preserving keys: msml_amd/allpairs.py walks the levels, this file is one pass over the tiles.
//   k_allpairs<T, MODE>  one workgroup = one tile of AP_TM probe rows x one split of the gallery columns, walked in
//                        tiles of AP_TN columns.  The reduction over E is that of k_search_tile (search.hip): the
//                        16x16x4 MFMA of T from two LDS stages, one accumulator chain per dot product from a zero
//                        accumulator, channels ascending, so a pair's score has the bits msml_search_topk gives it.
//                        The epilogue works on the accumulators: a pair is genuine when the two subject codes are
//                        equal, an impostor otherwise, and by MODE
//     AP_HIST      an impostor key inside one of the ranges counts into that range's 2^b bins (the key's next b bits):
//                  u32 per workgroup in LDS, flushed into the global u64 table
//     AP_COLLECT   an impostor score inside one of the ranges is appended to that range's part of `cand` through the
//                  range's global counter
//     AP_COUNT     every score is compared with the thresholds: 2 T u64 counters (genuine above, impostor above)
// Every result is an integer count or a set of scores whose order of arrival does not matter: the pass gives the same
// result for every `splits` and in every run although it uses atomics.
#include <math.h>

#include "common.h"

typedef __attribute__((ext_vector_type(4))) double ap_f64x4;
typedef unsigned long long u64;

#define AP_TM 64              // probe rows of a workgroup: 4 waves x 16
#define AP_TN 64              // gallery columns of a tile: 4 MFMA tiles of every wave
#define AP_MAX_RANGES 16      // one range per target at the most
#define AP_MAX_THR 16
#define AP_HBINS 8192         // bins of a workgroup's LDS histogram: n_ranges << bins_log2 at the most
#define AP_MAX_SPLITS 65535
#define AP_FLUSH_TILES (1 << 19)   // a tile adds at most 4096 to a bin: a u32 bin stays below 2^31 between two flushes
enum { AP_HIST = MSML_ALLPAIRS_HIST, AP_COLLECT = MSML_ALLPAIRS_COLLECT, AP_COUNT = MSML_ALLPAIRS_COUNT };

// The 16x16x4 MFMA of T and its LDS stage: lane maps, KSTEP and PITCH as Mma<T> of search.hip.
template <typename T>
struct ApMma;
template <>
struct ApMma<float> {
  typedef f32x4 Acc;
  typedef unsigned int Key;
  static constexpr int KSTEP = 32, PITCH = 34, W = 32;
  static __device__ __forceinline__ Acc mma(float a, float b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) * 4 + reg; }
  // order-preserving key: all bits of a negative flipped, the sign bit of a non-negative set
  static __device__ __forceinline__ Key key(float v) {
    const unsigned int b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
  }
};
template <>
struct ApMma<double> {
  typedef ap_f64x4 Acc;
  typedef u64 Key;
  static constexpr int KSTEP = 16, PITCH = 18, W = 64;
  static __device__ __forceinline__ Acc mma(double a, double b, Acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
  static __device__ __forceinline__ Key key(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    return b ^ ((b >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
  }
};

// kernel arguments by value: the ranges of a histogram / collecting pass, the thresholds of a count pass
struct ApRanges {
  u64 prefix[AP_MAX_RANGES];
  int bits[AP_MAX_RANGES];
  int n, bins_log2;
};
struct ApThr {
  double v[AP_MAX_THR];
  int n;
};

// 16 bytes at p (when `on`) or zeros
static __device__ __forceinline__ u32x4 ap_load_chunk(const char* p, bool on) {
  u32x4 z = {0u, 0u, 0u, 0u};
  return on ? *reinterpret_cast<const u32x4*>(p) : z;
}
// ... into a stage whose rows are only 8-byte aligned
static __device__ __forceinline__ void ap_store_chunk(char* p, u32x4 v) {
  u32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
  *reinterpret_cast<u32x2*>(p) = lo;
  *reinterpret_cast<u32x2*>(p + 8) = hi;
}

// key >> (W - bits) == prefix; bits == 0 is the whole key space
template <typename K, int W>
static __device__ __forceinline__ bool ap_in_range(K key, u64 prefix, int bits) {
  return bits == 0 ? true : (key >> (W - bits)) == (K)prefix;
}

// the workgroup's LDS bins into the global table, and back to zero; called by the whole workgroup
static __device__ __forceinline__ void ap_hist_flush(unsigned int* h, int nbins, u64* hist, int tid) {
  __syncthreads();
  for (int i = tid; i < nbins; i += 256) {
    const unsigned int c = h[i];
    if (c) {
      atomicAdd(&hist[i], (u64)c);
      h[i] = 0u;
    }
  }
  __syncthreads();
}

// grid (probe tiles, splits), 256 threads.  tiles_per_split: column tiles of a split (the last splits may be short or
// empty).  symmetric: gallery == probe, only the pairs (i, j) with i < j exist.  hist [rg.n][1 << rg.bins_log2],
// cand [rg.n][cand_cap] with cand_count [rg.n], counts [2][th.n] (genuine above, impostor above): the tables, the
// counters and counts are zero before the launch.
template <typename T, int MODE>
__global__ void __launch_bounds__(256) k_allpairs(const T* __restrict__ probe, long P, const int* __restrict__ pcode,
                                                  const T* __restrict__ gallery, int G, const int* __restrict__ gcode,
                                                  int E, int symmetric, int tiles_per_split, ApRanges rg, ApThr th,
                                                  u64* __restrict__ hist, T* __restrict__ cand,
                                                  u64* __restrict__ cand_count, u64 cand_cap, u64* __restrict__ counts) {
  typedef ApMma<T> M;
  typedef typename M::Acc Acc;
  typedef typename M::Key Key;
  constexpr int KSTEP = M::KSTEP, PITCH = M::PITCH, W = M::W;
  constexpr int EPC = 16 / (int)sizeof(T);                       // elements of a 16-byte chunk
  constexpr int STAGE = AP_TM * PITCH;                           // elements of one operand of one stage
  static_assert(AP_TM == AP_TN && KSTEP * sizeof(T) == 128, "a stage row is 8 chunks for both operands");
  __shared__ __attribute__((aligned(16))) T s_stage[4 * STAGE];  // [buffer][A | B][row][PITCH]
  __shared__ unsigned int s_hist[MODE == AP_HIST ? AP_HBINS : 1];
  __shared__ u64 s_cnt[MODE == AP_COUNT ? 2 * AP_MAX_THR : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long p0 = (long)blockIdx.x * AP_TM;
  const int n_ct = (G + AP_TN - 1) / AP_TN;
  int ct0 = blockIdx.y * tiles_per_split;
  const int ct1 = min(ct0 + tiles_per_split, n_ct);
  if (symmetric) ct0 = max(ct0, (int)blockIdx.x);                // the tiles before lie wholly on or below the diagonal
  const int nk = (E + KSTEP - 1) / KSTEP;
  const int nbins = MODE == AP_HIST ? rg.n << rg.bins_log2 : 0;  // <= AP_HBINS (checked by the caller)

  if (MODE == AP_HIST)
    for (int i = tid; i < nbins; i += 256) s_hist[i] = 0u;
  if (MODE == AP_COUNT && tid < 2 * AP_MAX_THR) s_cnt[tid] = 0ull;
  unsigned int n_gen[AP_MAX_THR], n_imp[AP_MAX_THR];             // AP_COUNT: this lane's counts (< 2^29: 16 per tile)
#pragma unroll
  for (int t = 0; t < AP_MAX_THR; ++t) n_gen[t] = n_imp[t] = 0u;

  // the subject codes and row numbers of the lane's four accumulator rows; -1: no such row
  int pc[4];
  long prow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    prow[r] = p0 + wave * 16 + M::row(lane, r);
    pc[r] = prow[r] < P ? pcode[prow[r]] : -1;
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

  int since_flush = 0;
  for (int ct = ct0; ct < ct1; ++ct) {
    const int g0 = ct * AP_TN;
    const char* b_ptr[2];
    bool b_on[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      b_on[i] = g0 + c_row[i] < G;
      b_ptr[i] = reinterpret_cast<const char*>(gallery) + (size_t)(b_on[i] ? g0 + c_row[i] : 0) * row_bytes + c_ch * 16;
    }
    // the codes of the lane's four accumulator columns; -2: no such column
    int gc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int gcol = g0 + n * 16 + (lane & 15);
      gc[n] = gcol < G ? gcode[gcol] : -2;
    }
    u32x4 ra[2], rb[2];
    {
      const bool kon = c_ch * EPC < E;                           // E % 4 == 0: a chunk is inside the row or outside
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ra[i] = ap_load_chunk(a_ptr[i], a_on[i] && kon);
        rb[i] = ap_load_chunk(b_ptr[i], b_on[i] && kon);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ap_store_chunk(reinterpret_cast<char*>(s_stage + c_row[i] * PITCH) + c_ch * 16, ra[i]);
        ap_store_chunk(reinterpret_cast<char*>(s_stage + STAGE + c_row[i] * PITCH) + c_ch * 16, rb[i]);
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
          ra[i] = ap_load_chunk(a_ptr[i] + off, a_on[i] && kon);
          rb[i] = ap_load_chunk(b_ptr[i] + off, b_on[i] && kon);
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
          ap_store_chunk(reinterpret_cast<char*>(dst + c_row[i] * PITCH) + c_ch * 16, ra[i]);
          ap_store_chunk(reinterpret_cast<char*>(dst + STAGE + c_row[i] * PITCH) + c_ch * 16, rb[i]);
        }
      }
      __syncthreads();                                           // after the last stage: the next tile may fill buffer 0
    }

    // the epilogue, straight from the accumulators: register r of tile n is (row prow[r], column g0 + 16 n + lane % 16)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const long gcol = g0 + n * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const T v = acc[n][r] + (T)0;                            // -0.0 counts as 0.0
        const bool pair = pc[r] >= 0 && gc[n] >= 0 && (!symmetric || gcol > prow[r]);
        const bool gen = pair && pc[r] == gc[n];
        const bool imp = pair && pc[r] != gc[n];
        if (MODE == AP_HIST) {
          const Key key = M::key(v);
          for (int q = 0; q < rg.n; ++q) {
            const int pb = rg.bits[q];
            const bool in = imp && ap_in_range<Key, W>(key, rg.prefix[q], pb);
            const unsigned int bin = (unsigned int)(key >> (W - pb - rg.bins_log2)) & ((1u << rg.bins_log2) - 1u);
            // impostor scores cluster and most lanes of a wave hit one bin; adding once per agreeing wave instead
            // was measured and is not faster (docs/KERNELS.md)
            if (in) atomicAdd(&s_hist[((unsigned int)q << rg.bins_log2) | bin], 1u);
          }
        } else if (MODE == AP_COLLECT) {
          const Key key = M::key(v);
          for (int q = 0; q < rg.n; ++q) {
            if (imp && ap_in_range<Key, W>(key, rg.prefix[q], rg.bits[q])) {
              const u64 pos = atomicAdd(&cand_count[q], 1ull);   // keeps counting past the capacity: the caller checks
              if (pos < cand_cap) cand[(u64)q * cand_cap + pos] = v;
            }
          }
        } else {
          const double s = (double)v;
#pragma unroll
          for (int t = 0; t < AP_MAX_THR; ++t) {
            const bool above = t < th.n && s > th.v[t];
            n_gen[t] += (above && gen) ? 1u : 0u;
            n_imp[t] += (above && imp) ? 1u : 0u;
          }
        }
      }
    }
    if (MODE == AP_HIST && ++since_flush == AP_FLUSH_TILES) {
      ap_hist_flush(s_hist, nbins, hist, tid);
      since_flush = 0;
    }
  }

  if (MODE == AP_HIST) ap_hist_flush(s_hist, nbins, hist, tid);
  if (MODE == AP_COUNT) {
    __syncthreads();                                             // s_cnt is zero
#pragma unroll
    for (int t = 0; t < AP_MAX_THR; ++t) {
      if (n_gen[t]) atomicAdd(&s_cnt[t], (u64)n_gen[t]);
      if (n_imp[t]) atomicAdd(&s_cnt[AP_MAX_THR + t], (u64)n_imp[t]);
    }
    __syncthreads();
    if (tid < 2 * AP_MAX_THR) {
      const int t = tid & (AP_MAX_THR - 1);
      const u64 c = s_cnt[tid];
      if (t < th.n && c) atomicAdd(&counts[(tid >> 4) * th.n + t], c);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
extern "C" int msml_allpairs_splits(long P, long G) {
  if (P < 1 || G < 1 || P >= 2147483647L || G >= 2147483647L) return 0;
  const long p_tiles = (P + AP_TM - 1) / AP_TM;
  const int n_ct = cdiv(G, AP_TN);
  long want = (3 * 256 + p_tiles - 1) / p_tiles;                 // three workgroups for each of the 256 CUs
  if (want > n_ct) want = n_ct;
  if (want > 1024) want = 1024;
  if (want < 1) want = 1;
  return cdiv(n_ct, cdiv(n_ct, want));                           // no empty split
}

template <typename T, int MODE>
static int allpairs_launch(const void* probe, long P, const int* pcode, const void* gallery, long G, const int* gcode,
                           int E, int symmetric, const ApRanges& rg, const ApThr& th, u64* hist, void* cand,
                           u64* cand_count, long cand_cap, u64* counts, int splits, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(P, AP_TM), (unsigned)splits);
  k_allpairs<T, MODE><<<grid, 256, 0, st>>>(reinterpret_cast<const T*>(probe), P, pcode,
                                            reinterpret_cast<const T*>(gallery), (int)G, gcode, E, symmetric,
                                            cdiv(cdiv(G, AP_TN), splits), rg, th, hist, reinterpret_cast<T*>(cand),
                                            cand_count, (u64)cand_cap, counts);
  MSML_LAUNCH_OK("allpairs_pass");
  return MSML_OK;
}

extern "C" int msml_allpairs_pass(const void* probe, long P, const int* probe_code, const void* gallery, long G,
                                  const int* gallery_code, int E, int dtype, int symmetric, int mode, int n_ranges,
                                  const unsigned long long* range_prefix, const int* range_bits, int bins_log2,
                                  unsigned long long* hist, void* cand, unsigned long long* cand_count, long cand_cap,
                                  const double* thresholds, int n_thr, unsigned long long* counts, int splits,
                                  void* stream) {
  MSML_CHECK(probe && gallery && probe_code && gallery_code, MSML_ERR_SHAPE, "allpairs_pass: null pointer");
  MSML_CHECK(dtype == MSML_F32 || dtype == MSML_F64, MSML_ERR_SHAPE,
             "allpairs_pass: dtype %d is not MSML_F32 or MSML_F64", dtype);
  MSML_CHECK(P >= 1 && P < 2147483647L && G >= 1 && G < 2147483647L, MSML_ERR_SHAPE,
             "allpairs_pass: bad shape P=%ld G=%ld", P, G);
  MSML_CHECK(E >= 4 && E % 4 == 0, MSML_ERR_SHAPE,
             "allpairs_pass: E=%d must be a positive multiple of 4 (16-byte loads)", E);
  MSML_CHECK(symmetric == 0 || (symmetric == 1 && gallery == probe && gallery_code == probe_code && G == P),
             MSML_ERR_SHAPE, "allpairs_pass: symmetric is 0, or 1 with the gallery being the probe set itself");
  MSML_CHECK(splits >= 1 && splits <= AP_MAX_SPLITS, MSML_ERR_SHAPE, "allpairs_pass: splits=%d outside 1..%d", splits,
             AP_MAX_SPLITS);
  MSML_CHECK(((uintptr_t)probe & 15) == 0 && ((uintptr_t)gallery & 15) == 0, MSML_ERR_SHAPE,
             "allpairs_pass: probe and gallery must be 16-byte aligned");
  MSML_CHECK(((uintptr_t)probe_code & 3) == 0 && ((uintptr_t)gallery_code & 3) == 0, MSML_ERR_SHAPE,
             "allpairs_pass: subject codes misaligned");
  const int W = dtype == MSML_F64 ? 64 : 32;
  ApRanges rg = {};
  ApThr th = {};
  if (mode == AP_HIST || mode == AP_COLLECT) {
    MSML_CHECK(range_prefix && range_bits, MSML_ERR_SHAPE, "allpairs_pass: null pointer (ranges)");
    MSML_CHECK(n_ranges >= 1 && n_ranges <= AP_MAX_RANGES, MSML_ERR_SHAPE, "allpairs_pass: %d ranges outside 1..%d",
               n_ranges, AP_MAX_RANGES);
    if (mode == AP_HIST) {
      MSML_CHECK(bins_log2 >= 1 && bins_log2 <= 13 && ((long)n_ranges << bins_log2) <= AP_HBINS, MSML_ERR_SHAPE,
                 "allpairs_pass: %d ranges of 2^%d bins exceed the %d bins of a pass", n_ranges, bins_log2, AP_HBINS);
      MSML_CHECK(hist && ((uintptr_t)hist & 7) == 0, MSML_ERR_SHAPE, "allpairs_pass: hist null or misaligned");
    } else {
      bins_log2 = 0;
      MSML_CHECK(cand && cand_count && ((uintptr_t)cand & 7) == 0 && ((uintptr_t)cand_count & 7) == 0, MSML_ERR_SHAPE,
                 "allpairs_pass: cand / cand_count null or misaligned");
      MSML_CHECK(cand_cap >= 1, MSML_ERR_SHAPE, "allpairs_pass: cand_cap=%ld", cand_cap);
    }
    for (int q = 0; q < n_ranges; ++q) {
      const int pb = range_bits[q];
      MSML_CHECK(pb >= 0 && pb + bins_log2 <= W, MSML_ERR_SHAPE,
                 "allpairs_pass: range %d: %d prefix bits + %d bin bits exceed the %d key bits", q, pb, bins_log2, W);
      MSML_CHECK(pb == 64 || (range_prefix[q] >> pb) == 0, MSML_ERR_SHAPE,
                 "allpairs_pass: range %d: the prefix does not fit its %d bits", q, pb);
      rg.prefix[q] = range_prefix[q];
      rg.bits[q] = pb;
    }
    rg.n = n_ranges;
    rg.bins_log2 = bins_log2;
  } else if (mode == AP_COUNT) {
    MSML_CHECK(thresholds && counts && ((uintptr_t)counts & 7) == 0, MSML_ERR_SHAPE,
               "allpairs_pass: thresholds / counts null or misaligned");
    MSML_CHECK(n_thr >= 1 && n_thr <= AP_MAX_THR, MSML_ERR_SHAPE, "allpairs_pass: %d thresholds outside 1..%d", n_thr,
               AP_MAX_THR);
    for (int t = 0; t < n_thr; ++t) {
      MSML_CHECK(!isnan(thresholds[t]), MSML_ERR_SHAPE, "allpairs_pass: threshold %d is NaN", t);
      th.v[t] = thresholds[t];
    }
    th.n = n_thr;
  } else {
    MSML_CHECK(false, MSML_ERR_SHAPE, "allpairs_pass: mode %d is not MSML_ALLPAIRS_HIST, _COLLECT or _COUNT", mode);
  }
  hipStream_t st = (hipStream_t)stream;
#define AP_GO(T, MODE)                                                                                              \
  return allpairs_launch<T, MODE>(probe, P, probe_code, gallery, G, gallery_code, E, symmetric, rg, th, hist, cand, \
                                  cand_count, cand_cap, counts, splits, st)
  if (dtype == MSML_F64) {
    if (mode == AP_HIST) AP_GO(double, AP_HIST);
    if (mode == AP_COLLECT) AP_GO(double, AP_COLLECT);
    AP_GO(double, AP_COUNT);
  }
  if (mode == AP_HIST) AP_GO(float, AP_HIST);
  if (mode == AP_COLLECT) AP_GO(float, AP_COLLECT);
  AP_GO(float, AP_COUNT);
#undef AP_GO
}
