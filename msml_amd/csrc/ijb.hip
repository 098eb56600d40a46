// Device side of the template (IJB-B / IJB-C) verification protocol of eval/qeval_ijbc.py and of the TAR @ FAR
// metrics of eval/qeval_mxnet.py:422-483 (Verification.start_verification):
//   k_template_pool     image2template_feature (:303-337) with the flip sum and the detector-score weighting of
//                       get_template_features (:484-502) folded into the one read of the image features
//   k_template_pair     verification (:343-369): cosine of every listed template pair
//   k_roc_block / k_roc_points / k_roc_reduce
//                       roc_curve + the TPR @ FPR table + auc (:565-585) on integer counts
//   k_pair_cosdist      cdist(..., 'cosine') of the normalised rows (qeval_mxnet.py:419,426-430)
//   k_rank_count        the two O(n^2) counting loops of :461-478 as rank queries on sorted distances
// Every floating-point sum runs in f64 in a fixed order and no kernel uses a floating-point atomic or waits on
// another workgroup: two runs give the same bits.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------
// Template pooling.  One workgroup per template, one wave per 256-column slab of E (a lane owns 4 consecutive
// columns: one 16-byte load per row), so a wave streams whole rows of its slab and keeps the media sum and the
// template sum of its 4 columns in registers.  order[] lists the image rows sorted by (template, media, row);
// media_start[m] .. media_start[m + 1] are the positions of media m in it, tmpl_media_start[t] ..
// tmpl_media_start[t + 1] the medias of template t.  launch[b] is the template workgroup b pools: the host lists
// the templates by falling row count, so the few templates with hundreds of images start first and the many
// one-image templates fill in behind them.
// ---------------------------------------------------------------------------------------------------------------
#define POOL_UNROLL 4

__global__ void __launch_bounds__(1024) k_template_pool(const float* __restrict__ feats, long ld, int E, int flip,
                                                        const float* __restrict__ faceness,
                                                        const int* __restrict__ order,
                                                        const int* __restrict__ media_start,
                                                        const int* __restrict__ tmpl_media_start,
                                                        const int* __restrict__ launch, double* __restrict__ out) {
  __shared__ double s_part[16];
  const int t = launch[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  const int m0 = tmpl_media_start[t], m1 = tmpl_media_start[t + 1];
  double* dst = out + (size_t)t * E;
  double ss = 0.0;                                   // this wave's sum of squares, slabs ascending
  for (int c = wave * 256 + lane * 4; c - lane * 4 < E; c += nwave * 256) {
    const bool on = c < E;
    double ts[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m = m0; m < m1; ++m) {
      const int r0 = media_start[m], r1 = media_start[m + 1];
      double ms[4] = {0.0, 0.0, 0.0, 0.0};
      for (int r = r0; r < r1; r += POOL_UNROLL) {
        float4 a[POOL_UNROLL], b[POOL_UNROLL];
        float w[POOL_UNROLL];
#pragma unroll
        for (int u = 0; u < POOL_UNROLL; ++u) {      // all loads first, the ordered f64 adds after them
          a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          b[u] = a[u];
          w[u] = 1.f;
          if (on && r + u < r1) {
            const int row = order[r + u];
            const float* p = feats + (size_t)row * ld + c;
            a[u] = *reinterpret_cast<const float4*>(p);
            if (flip) b[u] = *reinterpret_cast<const float4*>(p + E);
            if (faceness) w[u] = faceness[row];
          }
        }
#pragma unroll
        for (int u = 0; u < POOL_UNROLL; ++u) {
          if (r + u < r1) {
            const double wd = (double)w[u];
            ms[0] += ((double)a[u].x + (double)b[u].x) * wd;
            ms[1] += ((double)a[u].y + (double)b[u].y) * wd;
            ms[2] += ((double)a[u].z + (double)b[u].z) * wd;
            ms[3] += ((double)a[u].w + (double)b[u].w) * wd;
          }
        }
      }
      const double cnt = (double)(r1 - r0);          // np.mean: sum / count (a single row stays as it is)
#pragma unroll
      for (int k = 0; k < 4; ++k) ts[k] += ms[k] / cnt;
    }
    if (on) {
      *reinterpret_cast<double2*>(dst + c) = make_double2(ts[0], ts[1]);
      *reinterpret_cast<double2*>(dst + c + 2) = make_double2(ts[2], ts[3]);
      ss += ts[0] * ts[0] + ts[1] * ts[1] + ts[2] * ts[2] + ts[3] * ts[3];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) s_part[wave] = ss;
  __syncthreads();
  double tot = 0.0;
  for (int w = 0; w < nwave; ++w) tot += s_part[w];
  double nrm = sqrt(tot);
  if (nrm == 0.0) nrm = 1.0;                         // sklearn.preprocessing.normalize: a zero row stays zero
  // every thread re-reads only what it wrote itself
  for (int c = wave * 256 + lane * 4; c < E; c += nwave * 256) {
    double2 u = *reinterpret_cast<double2*>(dst + c), v = *reinterpret_cast<double2*>(dst + c + 2);
    u.x /= nrm; u.y /= nrm; v.x /= nrm; v.y /= nrm;
    *reinterpret_cast<double2*>(dst + c) = u;
    *reinterpret_cast<double2*>(dst + c + 2) = v;
  }
}

// score[i] = <Tn[r1[i]], Tn[r2[i]]>, one wave per pair, a lane owns 2 consecutive columns per 128-column step.
// The pair list repeats r1 in long runs, so that row comes from the L1 / L2 of the CU that has just read it.
__global__ void __launch_bounds__(256) k_template_pair(const double* __restrict__ tn, int T, int E,
                                                       const int* __restrict__ r1, const int* __restrict__ r2,
                                                       long P, double* __restrict__ score) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= P) return;
  const int ia = r1[i], ib = r2[i];
  if ((unsigned)ia >= (unsigned)T || (unsigned)ib >= (unsigned)T) {   // the host checks the ids; never read outside
    if (lane == 0) score[i] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  const double* a = tn + (size_t)ia * E;
  const double* b = tn + (size_t)ib * E;
  double s = 0.0;
  for (int c = lane * 2; c < E; c += 128) {
    const double2 x = *reinterpret_cast<const double2*>(a + c), y = *reinterpret_cast<const double2*>(b + c);
    s += x.x * y.x;
    s += x.y * y.y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) score[i] = s;
}

// 1 - a.b / (|a||b|) of the L2-normalised rows 2i, 2i+1: sklearn normalize (qeval_mxnet.py:419) then scipy's
// cosine (row norms of the NORMALISED rows, |cos| clipped to 1).
template <typename T>
__global__ void __launch_bounds__(256) k_pair_cosdist(const T* __restrict__ emb, int n_pairs, int E,
                                                      double* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= n_pairs) return;
  const T* a = emb + (size_t)(2 * pair) * E;
  const T* b = a + E;
  double sa = 0.0, sb = 0.0;
  for (int j = lane; j < E; j += 64) {
    const double x = a[j], y = b[j];
    sa += x * x;
    sb += y * y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sa += __shfl_xor(sa, o, 64);
    sb += __shfl_xor(sb, o, 64);
  }
  double na = sqrt(sa), nb = sqrt(sb);
  if (na == 0.0) na = 1.0;
  if (nb == 0.0) nb = 1.0;
  double d = 0.0, ua = 0.0, ub = 0.0;
  for (int j = lane; j < E; j += 64) {
    const double x = (double)a[j] / na, y = (double)b[j] / nb;
    d += x * y;
    ua += x * x;
    ub += y * y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    d += __shfl_xor(d, o, 64);
    ua += __shfl_xor(ua, o, 64);
    ub += __shfl_xor(ub, o, 64);
  }
  if (lane == 0) {
    double c = d / (sqrt(ua) * sqrt(ub));
    if (fabs(c) > 1.0) c = copysign(1.0, c);
    dist[pair] = 1.0 - c;
  }
}

// out[j] = number of sorted[i] < q[j] (strict) or <= q[j]; sorted ascending.
__global__ void __launch_bounds__(256) k_rank_count(const double* __restrict__ sorted, int n,
                                                    const double* __restrict__ q, int m, int strict,
                                                    int* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const double v = q[j];
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const bool left = strict ? (sorted[mid] < v) : (sorted[mid] <= v);
    if (left) lo = mid + 1;
    else hi = mid;
  }
  out[j] = lo;
}

// ---------------------------------------------------------------------------------------------------------------
// ROC on integer counts.  s[]: scores sorted descending, y[]: their 0/1 labels.  Position i ends a run of equal
// scores when i == n - 1 or s[i] != s[i + 1]; the curve has one point per run end: tps = positives among 0..i,
// fps = i + 1 - tps (_binary_clf_curve).  Two passes over blocks of ROC_BLOCK positions with the per-block table
// (positives, run ends) scanned on the host between them; nobody waits for another workgroup.
// ---------------------------------------------------------------------------------------------------------------
#define ROC_THREADS 256
#define ROC_PER 16
#define ROC_BLOCK (ROC_THREADS * ROC_PER)

// inclusive scan of (a, b) over the 256 threads of the block; total in (ta, tb)
__device__ __forceinline__ void block_scan2(int& a, int& b, int& ta, int& tb, int* s_a, int* s_b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int pa = __shfl_up(a, o, 64), pb = __shfl_up(b, o, 64);
    if (lane >= o) { a += pa; b += pb; }
  }
  if (lane == 63) { s_a[wave] = a; s_b[wave] = b; }
  __syncthreads();
  int oa = 0, ob = 0;
  ta = 0; tb = 0;
#pragma unroll
  for (int w = 0; w < ROC_THREADS / 64; ++w) {
    if (w < wave) { oa += s_a[w]; ob += s_b[w]; }
    ta += s_a[w]; tb += s_b[w];
  }
  a += oa; b += ob;
  __syncthreads();
}

__device__ __forceinline__ bool roc_run_end(const double* __restrict__ s, int i, int n) {
  return i == n - 1 || s[i] != s[i + 1];
}

// blk[b] = {positives, run ends} of block b
__global__ void __launch_bounds__(ROC_THREADS) k_roc_block(const double* __restrict__ s,
                                                           const unsigned char* __restrict__ y, int n,
                                                           int* __restrict__ blk) {
  __shared__ int s_a[ROC_THREADS / 64], s_b[ROC_THREADS / 64];
  const int base = blockIdx.x * ROC_BLOCK + threadIdx.x * ROC_PER;
  int pos = 0, ends = 0;
#pragma unroll
  for (int k = 0; k < ROC_PER; ++k) {
    const int i = base + k;
    if (i < n) {
      pos += y[i] ? 1 : 0;
      ends += roc_run_end(s, i, n) ? 1 : 0;
    }
  }
  int tp, te;
  block_scan2(pos, ends, tp, te, s_a, s_b);
  if (threadIdx.x == 0) {
    blk[2 * blockIdx.x] = tp;
    blk[2 * blockIdx.x + 1] = te;
  }
}

// off[b] = {positives, run ends} BEFORE block b (the host's exclusive scan of blk).  Writes tps[k], fps[k] of the
// k-th run end.
__global__ void __launch_bounds__(ROC_THREADS) k_roc_points(const double* __restrict__ s,
                                                            const unsigned char* __restrict__ y, int n,
                                                            const int* __restrict__ off, int* __restrict__ tps,
                                                            int* __restrict__ fps) {
  __shared__ int s_a[ROC_THREADS / 64], s_b[ROC_THREADS / 64];
  const int base = blockIdx.x * ROC_BLOCK + threadIdx.x * ROC_PER;
  int pos = 0, ends = 0;
  unsigned yb = 0, eb = 0;
#pragma unroll
  for (int k = 0; k < ROC_PER; ++k) {
    const int i = base + k;
    if (i < n) {
      if (y[i]) { yb |= 1u << k; ++pos; }
      if (roc_run_end(s, i, n)) { eb |= 1u << k; ++ends; }
    }
  }
  const int mypos = pos, myends = ends;
  int tp, te;
  block_scan2(pos, ends, tp, te, s_a, s_b);
  int cp = off[2 * blockIdx.x] + pos - mypos;        // positives before this thread's first position
  int ce = off[2 * blockIdx.x + 1] + ends - myends;  // run ends before it
#pragma unroll
  for (int k = 0; k < ROC_PER; ++k) {
    cp += (yb >> k) & 1u;
    if ((eb >> k) & 1u) {
      tps[ce] = cp;
      fps[ce] = base + k + 1 - cp;
      ++ce;
    }
  }
}

// Over the K curve points: keep[k] = the point survives roc_curve's drop_intermediate (first, last, or a non-zero
// second difference of fps or tps); per block the number kept, twice the trapezoid area of the block's segments
// (k - 1 -> k, point -1 = the origin roc_curve prepends; an exact integer, and dropping collinear points does not
// change it), and for each target the kept point nearest in |fps / n_neg - target|, ties to the larger k
// (min(zip(diff, index)) after flipud).  part[b] = {kept, area2, then per target: diff bits, k} as 64-bit words.
#define ROC_MAX_TARGETS 16
__global__ void __launch_bounds__(ROC_THREADS) k_roc_reduce(const int* __restrict__ tps, const int* __restrict__ fps,
                                                            int K, const double* __restrict__ target, int ntarget,
                                                            unsigned char* __restrict__ keep,
                                                            unsigned long long* __restrict__ part) {
  __shared__ unsigned long long s_kept[ROC_THREADS / 64], s_area[ROC_THREADS / 64];
  __shared__ double s_diff[ROC_THREADS / 64][ROC_MAX_TARGETS];
  __shared__ int s_idx[ROC_THREADS / 64][ROC_MAX_TARGETS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.x * ROC_THREADS + threadIdx.x;
  const double n_neg = (double)fps[K - 1];
  bool kp = false;
  unsigned long long area = 0;
  int f = 0;
  if (k < K) {
    f = fps[k];
    const int t = tps[k];
    const int fm = k > 0 ? fps[k - 1] : 0, tm = k > 0 ? tps[k - 1] : 0;
    kp = k == 0 || k == K - 1;
    if (!kp) {
      const int fn = fps[k + 1], tn = tps[k + 1];
      kp = (fn - f) != (f - fm) || (tn - t) != (t - tm);
    }
    keep[k] = kp ? 1 : 0;
    area = (unsigned long long)(f - fm) * (unsigned long long)(t + tm);
  }
  unsigned long long kept = kp ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kept += __shfl_xor(kept, o, 64);
    area += __shfl_xor(area, o, 64);
  }
  if (lane == 0) { s_kept[wave] = kept; s_area[wave] = area; }
  const double fpr = (double)f / n_neg;
  for (int j = 0; j < ntarget; ++j) {
    double d = kp ? fabs(fpr - target[j]) : __longlong_as_double(0x7ff0000000000000LL);
    int idx = kp ? k : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double od = __shfl_xor(d, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      if (od < d || (od == d && oi > idx)) { d = od; idx = oi; }
    }
    if (lane == 0) { s_diff[wave][j] = d; s_idx[wave][j] = idx; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* p = part + (size_t)blockIdx.x * (2 + 2 * ntarget);
    unsigned long long a = 0, c = 0;
    for (int w = 0; w < ROC_THREADS / 64; ++w) { c += s_kept[w]; a += s_area[w]; }
    p[0] = c;
    p[1] = a;
  }
  if (threadIdx.x < ntarget) {
    const int j = threadIdx.x;
    double d = s_diff[0][j];
    int idx = s_idx[0][j];
    for (int w = 1; w < ROC_THREADS / 64; ++w) {
      const double od = s_diff[w][j];
      const int oi = s_idx[w][j];
      if (od < d || (od == d && oi > idx)) { d = od; idx = oi; }
    }
    unsigned long long* p = part + (size_t)blockIdx.x * (2 + 2 * ntarget) + 2 + 2 * j;
    p[0] = (unsigned long long)__double_as_longlong(d);
    p[1] = (unsigned long long)(long long)idx;
  }
}

// ---------------------------------------------------------------------------------------------------------------
extern "C" int msml_template_pool(const float* feats, long n_rows, long ld, int E, int flip, const float* faceness,
                                  const int* order, const int* media_start, const int* tmpl_media_start,
                                  const int* launch, int n_templates, double* out, void* stream) {
  MSML_CHECK(feats && order && media_start && tmpl_media_start && launch && out, MSML_ERR_SHAPE,
             "template_pool: null pointer");
  MSML_CHECK(n_rows > 0 && n_rows < 2147483647L && n_templates > 0 && n_templates <= n_rows, MSML_ERR_SHAPE,
             "template_pool: bad shape n_rows=%ld n_templates=%d", n_rows, n_templates);
  MSML_CHECK(E > 0 && E % 4 == 0 && E <= 16 * 256 * 16, MSML_ERR_SHAPE,
             "template_pool: E=%d must be a positive multiple of 4 (16-byte loads)", E);
  MSML_CHECK(ld % 4 == 0 && ld >= (flip ? 2L * E : (long)E), MSML_ERR_SHAPE,
             "template_pool: row stride %ld does not hold %s of E=%d (multiple of 4)", ld,
             flip ? "both halves" : "one half", E);
  MSML_CHECK(((uintptr_t)feats & 15) == 0 && ((uintptr_t)out & 15) == 0, MSML_ERR_SHAPE,
             "template_pool: feats and out must be 16-byte aligned");
  int waves = cdiv(E, 256);
  if (waves > 16) waves = 16;
  k_template_pool<<<n_templates, 64 * waves, 0, (hipStream_t)stream>>>(feats, ld, E, flip, faceness, order,
                                                                        media_start, tmpl_media_start, launch, out);
  MSML_LAUNCH_OK("template_pool");
  return MSML_OK;
}

extern "C" int msml_template_pair_score(const double* tn, int n_templates, int E, const int* r1, const int* r2,
                                        long n_pairs, double* score, void* stream) {
  MSML_CHECK(tn && r1 && r2 && score && n_templates > 0 && n_pairs > 0 && n_pairs < 4L * 2147483647L, MSML_ERR_SHAPE,
             "template_pair_score: bad shape n_templates=%d n_pairs=%ld", n_templates, n_pairs);
  MSML_CHECK(E > 0 && E % 2 == 0 && ((uintptr_t)tn & 15) == 0, MSML_ERR_SHAPE,
             "template_pair_score: E=%d must be even and the features 16-byte aligned", E);
  k_template_pair<<<cdiv(n_pairs, 4), 256, 0, (hipStream_t)stream>>>(tn, n_templates, E, r1, r2, n_pairs, score);
  MSML_LAUNCH_OK("template_pair_score");
  return MSML_OK;
}

extern "C" int msml_pair_cosdist(const float* emb, int n_pairs, int E, double* dist, void* stream) {
  MSML_CHECK(emb && dist && n_pairs > 0 && E > 0, MSML_ERR_SHAPE, "pair_cosdist: bad shape n_pairs=%d E=%d", n_pairs, E);
  k_pair_cosdist<float><<<cdiv(n_pairs, 4), 256, 0, (hipStream_t)stream>>>(emb, n_pairs, E, dist);
  MSML_LAUNCH_OK("pair_cosdist");
  return MSML_OK;
}

extern "C" int msml_pair_cosdist_f64(const double* emb, int n_pairs, int E, double* dist, void* stream) {
  MSML_CHECK(emb && dist && n_pairs > 0 && E > 0, MSML_ERR_SHAPE, "pair_cosdist_f64: bad shape n_pairs=%d E=%d", n_pairs,
             E);
  k_pair_cosdist<double><<<cdiv(n_pairs, 4), 256, 0, (hipStream_t)stream>>>(emb, n_pairs, E, dist);
  MSML_LAUNCH_OK("pair_cosdist_f64");
  return MSML_OK;
}

extern "C" int msml_rank_count(const double* sorted, int n, const double* q, int m, int strict, int* out,
                               void* stream) {
  MSML_CHECK(sorted && q && out && n > 0 && m > 0, MSML_ERR_SHAPE, "rank_count: bad shape n=%d m=%d", n, m);
  k_rank_count<<<cdiv(m, 256), 256, 0, (hipStream_t)stream>>>(sorted, n, q, m, strict, out);
  MSML_LAUNCH_OK("rank_count");
  return MSML_OK;
}

extern "C" int msml_roc_blocks(int n) { return n > 0 ? cdiv(n, ROC_BLOCK) : 0; }

extern "C" int msml_roc_block_counts(const double* sorted, const unsigned char* label, int n, int* blk, void* stream) {
  MSML_CHECK(sorted && label && blk && n > 0, MSML_ERR_SHAPE, "roc_block_counts: bad shape n=%d", n);
  k_roc_block<<<cdiv(n, ROC_BLOCK), ROC_THREADS, 0, (hipStream_t)stream>>>(sorted, label, n, blk);
  MSML_LAUNCH_OK("roc_block_counts");
  return MSML_OK;
}

extern "C" int msml_roc_points(const double* sorted, const unsigned char* label, int n, const int* off, int* tps,
                               int* fps, void* stream) {
  MSML_CHECK(sorted && label && off && tps && fps && n > 0, MSML_ERR_SHAPE, "roc_points: bad shape n=%d", n);
  k_roc_points<<<cdiv(n, ROC_BLOCK), ROC_THREADS, 0, (hipStream_t)stream>>>(sorted, label, n, off, tps, fps);
  MSML_LAUNCH_OK("roc_points");
  return MSML_OK;
}

extern "C" int msml_roc_reduce_blocks(int n_points) { return n_points > 0 ? cdiv(n_points, ROC_THREADS) : 0; }

extern "C" int msml_roc_reduce(const int* tps, const int* fps, int n_points, const double* target, int n_targets,
                               unsigned char* keep, unsigned long long* part, void* stream) {
  MSML_CHECK(tps && fps && keep && part && n_points > 0, MSML_ERR_SHAPE, "roc_reduce: bad shape n_points=%d", n_points);
  MSML_CHECK(n_targets >= 0 && n_targets <= ROC_MAX_TARGETS && (target || n_targets == 0), MSML_ERR_SHAPE,
             "roc_reduce: n_targets=%d outside 0..%d", n_targets, ROC_MAX_TARGETS);
  k_roc_reduce<<<cdiv(n_points, ROC_THREADS), ROC_THREADS, 0, (hipStream_t)stream>>>(tps, fps, n_points, target,
                                                                                      n_targets, keep, part);
  MSML_LAUNCH_OK("roc_reduce");
  return MSML_OK;
}
