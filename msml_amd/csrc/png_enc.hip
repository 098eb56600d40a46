// PNG encoding on the device: files Pillow, zlib and msml_png_decode read back to exactly the source pixels (what
// PIL.Image.save writes for the .png names of eval/align_dataset.py:52-75 and the '.png' payloads of
// datasets/3d_tools/cvt_casia_webface.py:35).  The bytes are NOT Pillow's: PNG is lossless, and zlib's level-6 lazy
// matcher is a sequential algorithm.  The arithmetic is csrc/png_enc_core.h, shared with the host check.
//   k_png_enc_filter   one wavefront per row: the five filters' sums of abs((int8) byte), the adaptive choice (smallest
//                      sum, ties to the lowest filter number) or the forced filter, the filter byte and the row into
//                      the workspace.  Reads the packed source through img_rect_ok; writes status[n] (0, 1, 3).
//   k_png_enc_deflate  one wavefront per chunk of 65535 filtered bytes = one deflate block.  64 positions per step: every
//                      lane hashes the 4 bytes at its position, reads the last earlier position with that hash from an
//                      LDS table (then enters its own with an LDS max, so the table never depends on lane order), also
//                      tries the byte one row above, verifies and extends by byte compares; the lanes' overlapping
//                      matches become one greedy token sequence (a uniform walk over the lanes' lengths gives a 64-bit
//                      mask of token starts, a population count below the lane the token's index).  A chunk after the
//                      first enters the 32 KiB before its start into the table first: that is input, not output.
//                      Histograms in LDS; code lengths, code-length code and the bit costs of fixed / dynamic /
//                      dynamic with literals only on lane 0 (a parallel rank sort in front); the cheapest is written
//                      to the chunk's scratch from bit 0, 64 tokens per step through an LDS staging window (LDS OR).
//                      A chunk whose cheapest coding passes what a stored block costs writes nothing.
//   k_png_enc_emit     one workgroup per image: walks the chunks in order (bit offsets, stored or compressed by the
//                      exact cost at that offset, Adler-32 folded from the chunks' sums), shifts every chunk's bits to
//                      its offset or copies the stored bytes, then signature, IHDR, the one IDAT with its CRC-32
//                      (256 table CRCs over equal pieces, combined with x^(8 L) by repeated squaring), IEND, length[n].
// Integer arithmetic; the only atomics are LDS max / add / or, whose results do not depend on their order; one writer
// per byte of the output: two runs, and any batch composition, give the same bytes.
#include "common.h"
#include "png_enc_core.h"

struct PngeSlotOut {                                         // writes inside [0, cap) of the image's slot only
  unsigned char* slot;
  long cap;
  __device__ void put(long pos, int v) {
    if (pos >= 0 && pos < cap) slot[pos] = (unsigned char)v;
  }
};

__global__ void __launch_bounds__(64) k_png_enc_filter(const unsigned char* __restrict__ src, long src_bytes,
                                                       const long* __restrict__ meta, int channels, int swap_rb,
                                                       int filter, const int* __restrict__ desc,
                                                       unsigned char* __restrict__ ws, int* __restrict__ status) {
  const int n = blockIdx.y, y = blockIdx.x, lane = threadIdx.x;
  const int* d = desc + (long)n * PNGE_DESC_WORDS;
  const int H = d[PE_H], W = d[PE_W];
  if (!pnge_size_ok(H, W, channels)) {
    if (y == 0 && lane == 0) status[n] = PNGE_ERR_GEOMETRY;
    return;
  }
  PngeGeom G;
  pnge_geom(H, W, channels, G);
  const long* mt = meta + (long)n * 4;
  const bool ok = img_rect_ok(mt, H, W, G.rb, G.rb, src_bytes);
  if (y == 0 && lane == 0) status[n] = ok ? PNGE_OK : PNGE_ERR_SOURCE;
  if (!ok || y >= H) return;
  const long pitch = mt[3];
  const unsigned char* row = src + mt[0] + (long)y * pitch;
  const unsigned char* up = row - pitch;                     // read only where y > 0
  unsigned char* out = ws + (long)d[PE_WS] * PNGE_WS_ALIGN + G.o_filt + (long)y * G.stride;
  int f = filter;
  if (filter == PNGE_ADAPTIVE) {
    unsigned int sum[5] = {0, 0, 0, 0, 0};
    for (long j = lane; j < G.rb; j += 64) {
      const long js = pnge_src_index(j, channels, swap_rb);
      const int x = row[js], a = j >= channels ? row[js - channels] : 0, b = y ? up[js] : 0,
                c = (y && j >= channels) ? up[js - channels] : 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) sum[k] += pnge_abs8(pnge_filter(k, x, a, b, c));
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
      for (int o = 32; o; o >>= 1) sum[k] += __shfl_xor(sum[k], o);
    f = 0;
#pragma unroll
    for (int k = 1; k < 5; ++k)
      if (sum[k] < sum[f]) f = k;
  }
  if (lane == 0) out[0] = (unsigned char)f;
  for (long j = lane; j < G.rb; j += 64) {
    const long js = pnge_src_index(j, channels, swap_rb);
    const int x = row[js], a = j >= channels ? row[js - channels] : 0, b = y ? up[js] : 0,
              c = (y && j >= channels) ? up[js - channels] : 0;
    out[1 + j] = (unsigned char)pnge_filter(f, x, a, b, c);
  }
}

struct PngeLds {
  uint32_t hash[1 << PNGE_HASH_BITS];                        // position + 1 of the last entry, 0 = none
  uint32_t ll[PNGE_NLL + 2], dd[PNGE_ND + 2];                // counts of the token sequence
  uint32_t lit[PNGE_NLL + 2], nod[PNGE_ND + 2];              // counts of the literals-only coding (nod stays zero)
  uint16_t sorted[PNGE_NLL + 2];
  PngeScratch S;
  PngeBlockCode B[2];                                        // [0] fixed or dynamic, [1] dynamic with literals only
  uint32_t stage[128];
  unsigned long long red[64];
  uint32_t red32[64];
};

// symbols with a count, ascending by (count, symbol): a rank sort over the wavefront -> how many
__device__ inline int pnge_wave_sort(const uint32_t* cnt, int n, uint16_t* sorted, int lane) {
  int mine = 0;
  for (int s = lane; s < n; s += 64) {
    const uint32_t c = cnt[s];
    if (!c) continue;
    int r = 0;
    for (int t = 0; t < n; ++t) {
      const uint32_t ct = cnt[t];
      r += (ct != 0 && (ct < c || (ct == c && t < s))) ? 1 : 0;
    }
    sorted[r] = (uint16_t)s;
    ++mine;
  }
  for (int o = 32; o; o >>= 1) mine += __shfl_xor(mine, o);
  __syncthreads();
  return mine;
}

__device__ inline int pnge_match_len(const unsigned char* a, const unsigned char* b, int maxlen) {
  int l = 0;
  while (l < maxlen && a[l] == b[l]) ++l;
  return l;
}

// One step of the bit writer: every lane brings nb (0..48) bits v; they leave in lane order.  stage holds the pending
// bits (fill of them, fewer than 32, in stage[0]); whole words go to out[outw ...], never past capw.
__device__ inline void pnge_emit_step(uint64_t v, int nb, uint32_t* stage, uint32_t* out, long capw, int& fill, long& outw,
                                      int lane) {
  int incl = nb;
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o);
    if (lane >= o) incl += u;
  }
  const int sum = __shfl(incl, 63);
  const int off = fill + incl - nb;
  if (nb) {
    const int w = off >> 5, sh = off & 31;
    const uint64_t lo = v << sh;
    atomicOr(&stage[w], (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) atomicOr(&stage[w + 1], (uint32_t)(lo >> 32));
    if (sh && (uint32_t)(v >> (64 - sh))) atomicOr(&stage[w + 2], (uint32_t)(v >> (64 - sh)));
  }
  __syncthreads();
  const int tot = fill + sum, full = tot >> 5;               // at most 31 + 64 * 48 bits: 97 words
  for (int k = lane; k < full; k += 64)
    if (outw + k < capw) out[outw + k] = stage[k];
  const uint32_t keep = stage[full];
  __syncthreads();
  for (int k = lane; k < 128; k += 64) stage[k] = 0;
  __syncthreads();
  if (lane == 0) stage[0] = keep;
  __syncthreads();
  fill = tot & 31;
  outw += full;
}

__global__ void __launch_bounds__(64) k_png_enc_deflate(int channels, const int* __restrict__ desc,
                                                        unsigned char* __restrict__ ws, const int* __restrict__ status) {
  __shared__ PngeLds L;
  const int n = blockIdx.y, lane = threadIdx.x;
  if (status[n] != 0) return;
  const int* d = desc + (long)n * PNGE_DESC_WORDS;
  PngeGeom G;
  pnge_geom(d[PE_H], d[PE_W], channels, G);
  const long chunk = blockIdx.x;
  if (chunk >= G.nchunks) return;
  unsigned char* base = ws + (long)d[PE_WS] * PNGE_WS_ALIGN;
  const unsigned char* f = base + G.o_filt;
  const int ntot = (int)G.n, c0 = (int)(chunk * PNGE_CHUNK);
  const int len = ntot - c0 < PNGE_CHUNK ? ntot - c0 : PNGE_CHUNK, cend = c0 + len;
  const int stride = (int)(G.stride <= PNGE_WINDOW ? G.stride : 0);     // 0: the row above is out of reach
  uint32_t* tok = reinterpret_cast<uint32_t*>(base + G.o_tok) + c0;
  uint32_t* out = reinterpret_cast<uint32_t*>(base + G.o_bits + chunk * G.bits_stride);
  const long capw = G.bits_stride / 4;
  int* rec = reinterpret_cast<int*>(base + G.o_rec) + chunk * PNGE_REC_WORDS;

  for (int k = lane; k < (1 << PNGE_HASH_BITS); k += 64) L.hash[k] = 0;
  for (int k = lane; k < PNGE_NLL + 2; k += 64) L.ll[k] = 0, L.lit[k] = 0;
  if (lane < PNGE_ND + 2) L.dd[lane] = 0, L.nod[lane] = 0;
  for (int k = lane; k < 128; k += 64) L.stage[k] = 0;
  __syncthreads();
  for (int b0 = c0 > PNGE_WINDOW ? c0 - PNGE_WINDOW : 0; b0 < c0; b0 += 64) {   // the window before the chunk
    const int p = b0 + lane;
    if (p < c0 && p + 4 <= ntot) {
      const uint32_t v = f[p] | (f[p + 1] << 8) | (f[p + 2] << 16) | ((uint32_t)f[p + 3] << 24);
      atomicMax(&L.hash[pnge_hash(v)], (uint32_t)(p + 1));
    }
  }
  __syncthreads();

  int next = c0, ntok = 0;                                   // next: the first position no token covers yet
  uint32_t xbits = 0, sa = 0;
  unsigned long long sb = 0;
  for (int b0 = c0; b0 < cend; b0 += 64) {
    const int p = b0 + lane;
    const bool inb = p < cend, hashable = inb && p + 4 <= ntot;
    int x = 0;
    uint32_t hv = 0, cand = 0;
    if (inb) {
      x = f[p];
      atomicAdd(&L.lit[x], 1u);
      sa += (uint32_t)x;
      sb += (unsigned long long)(uint32_t)(cend - p) * (uint32_t)x;
    }
    if (hashable) {
      hv = pnge_hash(f[p] | (f[p + 1] << 8) | (f[p + 2] << 16) | ((uint32_t)f[p + 3] << 24));
      cand = L.hash[hv];
    }
    __syncthreads();
    if (hashable) atomicMax(&L.hash[hv], (uint32_t)(p + 1));
    int best = 0, bdist = 0;
    if (inb && p >= next) {
      const int maxlen = cend - p < PNGE_MAX_MATCH ? cend - p : PNGE_MAX_MATCH;
      if (maxlen >= PNGE_MIN_MATCH) {
        if (cand) {
          const int dist = p - (int)(cand - 1);
          if (dist >= 1 && dist <= PNGE_WINDOW) {
            best = pnge_match_len(f + p - dist, f + p, maxlen);
            bdist = dist;
          }
        }
        if (stride && p >= stride && stride != bdist) {
          const int l = pnge_match_len(f + p - stride, f + p, maxlen);
          if (l > best || (l == best && stride < bdist)) best = l, bdist = stride;
        }
      }
    }
    if (best < PNGE_MIN_MATCH) best = 0;
    unsigned long long taken = 0;
    const int lim = b0 + 64 < cend ? b0 + 64 : cend;
    int cur = next > b0 ? next : b0;
    while (cur < lim) {
      const int l = __shfl(best, cur - b0);
      taken |= 1ull << (cur - b0);
      cur += l ? l : 1;
    }
    next = cur;
    if ((taken >> lane) & 1) {
      const int idx = ntok + __popcll(taken & ((1ull << lane) - 1));
      if (best) {
        int ls, le, lx, ds, de, dx;
        pnge_len_symbol(best, ls, le, lx);
        pnge_dist_symbol(bdist, ds, de, dx);
        tok[idx] = pnge_match_token(best, bdist);
        atomicAdd(&L.ll[ls], 1u);
        atomicAdd(&L.dd[ds], 1u);
        xbits += (uint32_t)(le + de);
      } else {
        tok[idx] = (uint32_t)x;
        atomicAdd(&L.ll[x], 1u);
      }
    }
    ntok += __popcll(taken);
  }
  L.red[lane] = sb;
  L.red32[lane] = sa;
  __syncthreads();
  if (lane == 0) {
    unsigned long long b = 0, a = 0;
    for (int k = 0; k < 64; ++k) b += L.red[k] % PNGE_ADLER, a += L.red32[k];
    rec[2] = (int)(a % PNGE_ADLER);
    rec[3] = (int)(b % PNGE_ADLER);
    L.ll[256] = 1;
    L.lit[256] = 1;
  }
  L.red32[lane] = xbits;
  __syncthreads();
  long extra = 0;
  for (int k = 0; k < 64; ++k) extra += L.red32[k];
  __syncthreads();

  // the three candidates' costs (the 3 block bits included)
  long cost_fixed = 0;
  if (lane == 0) {
    pnge_fixed_code(L.ll, L.dd, L.B[0]);
    L.red[0] = (unsigned long long)L.B[0].body_bits;
  }
  __syncthreads();
  cost_fixed = 3 + (long)L.red[0] + extra;
  int m = pnge_wave_sort(L.ll, PNGE_NLL, L.sorted, lane);
  if (lane == 0) pnge_huff_lengths(L.ll, PNGE_NLL, L.sorted, m, 15, L.B[0].ll_len, L.S);
  __syncthreads();
  m = pnge_wave_sort(L.dd, PNGE_ND, L.sorted, lane);
  if (lane == 0) {
    pnge_huff_lengths(L.dd, PNGE_ND, L.sorted, m, 15, L.B[0].d_len, L.S);
    pnge_dynamic_header(L.ll, L.dd, L.B[0], L.S);
  }
  __syncthreads();
  const long cost_dyn = 3 + L.B[0].header_bits + L.B[0].body_bits + extra;
  m = pnge_wave_sort(L.lit, PNGE_NLL, L.sorted, lane);
  if (lane == 0) {
    pnge_huff_lengths(L.lit, PNGE_NLL, L.sorted, m, 15, L.B[1].ll_len, L.S);
    pnge_huff_lengths(L.nod, PNGE_ND, L.sorted, 0, 15, L.B[1].d_len, L.S);
    pnge_dynamic_header(L.lit, L.nod, L.B[1], L.S);
  }
  __syncthreads();
  const long cost_lit = 3 + L.B[1].header_bits + L.B[1].body_bits;
  int mode = PNGE_MODE_FIXED;
  long bits = cost_fixed;
  if (cost_dyn < bits) mode = PNGE_MODE_DYNAMIC, bits = cost_dyn;
  if (cost_lit < bits) mode = PNGE_MODE_LITERALS, bits = cost_lit;
  if (bits > pnge_stored_max_bits(len)) mode = PNGE_MODE_SKIPPED;
  if (lane == 0) {
    rec[0] = mode;
    rec[1] = mode == PNGE_MODE_SKIPPED ? 0 : (int)bits;
    if (mode == PNGE_MODE_FIXED) pnge_fixed_code(L.ll, L.dd, L.B[0]);
  }
  __syncthreads();
  if (mode == PNGE_MODE_SKIPPED) return;

  const PngeBlockCode& B = L.B[mode == PNGE_MODE_LITERALS ? 1 : 0];
  const int final_block = chunk + 1 == G.nchunks ? 1 : 0;
  const int nbody = mode == PNGE_MODE_LITERALS ? len : ntok;
  const int total = 1 + B.nitems + nbody + 1;                // block bits, header, tokens, end of block
  int fill = 0;
  long outw = 0;
  for (int i0 = 0; i0 < total; i0 += 64) {
    const int i = i0 + lane;
    uint64_t v = 0;
    int nb = 0;
    if (i == 0) {
      v = (uint64_t)(final_block | ((mode == PNGE_MODE_FIXED ? 1 : 2) << 1));
      nb = 3;
    } else if (i <= B.nitems) {
      v = B.items[i - 1] & 0xffffu;
      nb = (int)(B.items[i - 1] >> 16);
    } else if (i < total - 1) {
      const int k = i - 1 - B.nitems;
      const uint32_t t = mode == PNGE_MODE_LITERALS ? (uint32_t)f[c0 + k] : tok[k];
      nb = pnge_token_bits(t, B.ll_len, B.ll_code, B.d_len, B.d_code, v);
    } else if (i == total - 1) {
      v = B.ll_code[256];
      nb = B.ll_len[256];
    }
    pnge_emit_step(v, nb, L.stage, out, capw, fill, outw, lane);
  }
  if (lane == 0 && fill && outw < capw) out[outw] = L.stage[0];
}

__global__ void __launch_bounds__(256) k_png_enc_emit(int channels, const int* __restrict__ desc,
                                                      unsigned char* __restrict__ ws, unsigned char* __restrict__ dst,
                                                      long dst_bytes, const long* __restrict__ out_meta,
                                                      int* __restrict__ length, int* __restrict__ status) {
  __shared__ uint32_t s_tab[256], s_crc[256];
  __shared__ long s_bits;
  __shared__ uint32_t s_adler;
  __shared__ int s_ok;
  const int n = blockIdx.x, t = threadIdx.x;
  s_tab[t] = pnge_crc_entry((uint32_t)t);
  if (status[n] != 0) {
    if (t == 0) length[n] = 0;
    return;
  }
  const long off = out_meta[(long)n * 2], cap = out_meta[(long)n * 2 + 1];
  if (off < 0 || cap < 0 || off > dst_bytes || cap > dst_bytes - off) {
    if (t == 0) {
      length[n] = 0;
      status[n] = PNGE_ERR_SLOT;
    }
    return;
  }
  const int* d = desc + (long)n * PNGE_DESC_WORDS;
  PngeGeom G;
  pnge_geom(d[PE_H], d[PE_W], channels, G);
  unsigned char* base = ws + (long)d[PE_WS] * PNGE_WS_ALIGN;
  const unsigned char* f = base + G.o_filt;
  int* rec = reinterpret_cast<int*>(base + G.o_rec);
  long* rec64 = reinterpret_cast<long*>(base + G.o_rec);
  if (t == 0) {
    long bo = 16;                                            // behind the two bytes of the zlib header
    uint32_t a = 1, b = 0;
    for (long c = 0; c < G.nchunks; ++c) {
      int* r = rec + c * PNGE_REC_WORDS;
      const long c0 = c * PNGE_CHUNK, len = G.n - c0 < PNGE_CHUNK ? G.n - c0 : PNGE_CHUNK;
      const long se = pnge_stored_end(bo, len);
      const bool packed = r[0] != PNGE_MODE_SKIPPED && r[1] > 0 && bo + r[1] < se;
      rec64[c * (PNGE_REC_WORDS / 2) + 2] = bo;
      r[6] = packed ? 1 : 0;
      bo = packed ? bo + r[1] : se;
      pnge_adler_append(a, b, (uint32_t)r[2], (uint32_t)r[3], len);
    }
    s_bits = bo;
    s_adler = (b << 16) | a;
    const long total = PNGE_HEAD_BYTES + ((bo + 7) >> 3) + 4 + 16;
    s_ok = total <= cap && total <= 0x7fffffffL;
    if (!s_ok) {
      length[n] = 0;
      status[n] = PNGE_ERR_SLOT;
    }
  }
  __syncthreads();
  if (!s_ok) return;
  PngeSlotOut file = {dst + off, cap};
  PngeSlotOut z = {dst + off + PNGE_HEAD_BYTES, cap - PNGE_HEAD_BYTES};
  if (t == 0) z.put(0, 0x78), z.put(1, 0x01);
  int carry = 0;                                             // the bits of the byte a chunk shares with the next one
  for (long c = 0; c < G.nchunks; ++c) {
    const int* r = rec + c * PNGE_REC_WORDS;
    const long c0 = c * PNGE_CHUNK, len = G.n - c0 < PNGE_CHUNK ? G.n - c0 : PNGE_CHUNK;
    const long bo = rec64[c * (PNGE_REC_WORDS / 2) + 2];
    const int s = (int)(bo & 7);
    const long d0 = bo >> 3;
    const bool last = c + 1 == G.nchunks;
    if (r[6]) {
      const unsigned char* sp = base + G.o_bits + c * G.bits_stride;
      const long nb = r[1], nsrc = (nb + 7) >> 3, e = bo + nb, dl = (e - 1) >> 3;
      const bool whole = (e & 7) == 0 || last;
      const long nw = dl - d0 + (whole ? 1 : 0);
      for (long k = t; k < nw; k += 256) {
        const int lo = k < nsrc ? sp[k] : 0, hi = (k >= 1 && k - 1 < nsrc) ? sp[k - 1] : 0;
        z.put(d0 + k, (((lo << s) | (hi >> (8 - s))) & 255) | (k == 0 ? carry : 0));
      }
      if (!whole) {
        const long k = dl - d0;
        const int lo = k < nsrc ? sp[k] : 0, hi = (k >= 1 && k - 1 < nsrc) ? sp[k - 1] : 0;
        carry = (((lo << s) | (hi >> (8 - s))) & 255) | (k == 0 ? carry : 0);
      } else {
        carry = 0;
      }
    } else {
      const long a = (bo + 3 + 7) >> 3;                      // LEN starts here
      if (t == 0) {
        z.put(d0, carry | ((last ? 1 : 0) << s));
        for (long j = d0 + 1; j < a; ++j) z.put(j, 0);
        z.put(a, (int)(len & 255)), z.put(a + 1, (int)(len >> 8));
        z.put(a + 2, (int)(~len & 255)), z.put(a + 3, (int)((~len >> 8) & 255));
      }
      for (long k = t; k < len; k += 256) z.put(a + 4 + k, f[c0 + k]);
      carry = 0;
    }
  }
  const long zend = (s_bits + 7) >> 3, idat = zend + 4;
  if (t == 0) {
    for (int i = 0; i < 4; ++i) z.put(zend + i, (int)((s_adler >> (24 - 8 * i)) & 255));
    pnge_head(file, G.H, G.W, channels, idat, s_tab);
  }
  __syncthreads();
  // CRC-32 of "IDAT" + stream: M bytes from file offset 37, cut into 256 pieces of P bytes, zeros in front
  const long M = 4 + idat, P = (M + 255) / 256, pad = 256 * P - M;
  {
    const unsigned char* m = dst + off + 37;
    long v0 = (long)t * P - pad, v1 = v0 + P;
    if (v0 < 0) v0 = 0;
    uint32_t cr = 0;
    for (long v = v0; v < v1; ++v) cr = s_tab[(cr ^ m[v]) & 255] ^ (cr >> 8);
    s_crc[t] = cr;
  }
  __syncthreads();
  if (t == 0) {
    const uint32_t op = pnge_gf_x8n(P);
    uint32_t acc = 0;
    for (int i = 0; i < 256; ++i) acc = pnge_gf_mul(op, acc) ^ s_crc[i];
    pnge_tail(file, PNGE_HEAD_BYTES + idat, pnge_crc_finish(acc, M));
    length[n] = (int)(PNGE_HEAD_BYTES + idat + 16);
  }
}

extern "C" long msml_png_encode_ws_bytes(int* desc, int channels, int N) {
  if (!desc || N < 1 || channels < 1 || channels > 4) return 0;
  long units = 0;
  for (int n = 0; n < N; ++n) {
    int* d = desc + (long)n * PNGE_DESC_WORDS;
    d[PE_WS] = 0;
    if (units > 0x7fffffffL) return 0;
    d[PE_WS] = (int)units;
    if (!pnge_size_ok(d[PE_H], d[PE_W], channels)) continue;   // status 3 on the device, no workspace
    PngeGeom G;
    pnge_geom(d[PE_H], d[PE_W], channels, G);
    units += G.bytes / PNGE_WS_ALIGN;
  }
  return (units > 0 ? units : 1) * PNGE_WS_ALIGN;
}

extern "C" long msml_png_encode_bound(int H, int W, int channels) { return pnge_bound(H, W, channels); }

extern "C" int msml_png_encode(const unsigned char* src, long src_bytes, const long* meta, int channels, int swap_rb,
                               int filter, const int* desc, const int* desc_host, unsigned char* dst, long dst_bytes,
                               const long* out_meta, int* length, int* status, unsigned char* ws, long ws_bytes, int N,
                               void* stream) {
  MSML_CHECK(N >= 1 && N <= 65535, MSML_ERR_UNSUPPORTED, "png_encode: N=%d outside 1..65535", N);
  MSML_CHECK(channels >= 1 && channels <= 4, MSML_ERR_UNSUPPORTED, "png_encode: channels=%d (1..4)", channels);
  MSML_CHECK(filter >= 0 && filter <= PNGE_ADAPTIVE, MSML_ERR_UNSUPPORTED,
             "png_encode: filter=%d (0 none, 1 sub, 2 up, 3 average, 4 paeth, 5 adaptive)", filter);
  MSML_CHECK(swap_rb == 0 || channels >= 3, MSML_ERR_UNSUPPORTED, "png_encode: swap_rb with %d channels", channels);
  MSML_CHECK(src && meta && desc && desc_host && dst && out_meta && length && status && ws, MSML_ERR_SHAPE,
             "png_encode: null pointer");
  MSML_CHECK(((uintptr_t)desc & 3) == 0 && ((uintptr_t)length & 3) == 0 && ((uintptr_t)status & 3) == 0 &&
                 ((uintptr_t)meta & 7) == 0 && ((uintptr_t)out_meta & 7) == 0 && ((uintptr_t)ws & 15) == 0,
             MSML_ERR_SHAPE, "png_encode: desc, length, status must be 4-byte, meta, out_meta 8-byte, ws 16-byte aligned");
  MSML_CHECK(src_bytes >= 0 && dst_bytes >= 0 && ws_bytes >= 0, MSML_ERR_SHAPE,
             "png_encode: src_bytes=%ld dst_bytes=%ld ws_bytes=%ld", src_bytes, dst_bytes, ws_bytes);
  long units = 0, max_h = 1, max_chunks = 1;
  for (int n = 0; n < N; ++n) {
    const int* d = desc_host + (long)n * PNGE_DESC_WORDS;
    MSML_CHECK(d[PE_WS] == units, MSML_ERR_SHAPE, "png_encode: descriptor %d: workspace offset %d, not the %ld "
               "msml_png_encode_ws_bytes writes", n, d[PE_WS], units);
    if (!pnge_size_ok(d[PE_H], d[PE_W], channels)) continue;
    PngeGeom G;
    pnge_geom(d[PE_H], d[PE_W], channels, G);
    units += G.bytes / PNGE_WS_ALIGN;
    MSML_CHECK(units * PNGE_WS_ALIGN <= ws_bytes, MSML_ERR_WORKSPACE, "png_encode: workspace of %ld bytes is too small "
               "(image %d ends at %ld)", ws_bytes, n, units * PNGE_WS_ALIGN);
    max_h = G.H > max_h ? G.H : max_h;
    max_chunks = G.nchunks > max_chunks ? G.nchunks : max_chunks;
  }
  hipStream_t s = (hipStream_t)stream;
  k_png_enc_filter<<<dim3((unsigned)max_h, N), 64, 0, s>>>(src, src_bytes, meta, channels, swap_rb, filter, desc, ws, status);
  MSML_LAUNCH_OK("png_enc_filter");
  k_png_enc_deflate<<<dim3((unsigned)max_chunks, N), 64, 0, s>>>(channels, desc, ws, status);
  MSML_LAUNCH_OK("png_enc_deflate");
  k_png_enc_emit<<<N, 256, 0, s>>>(channels, desc, ws, dst, dst_bytes, out_meta, length, status);
  MSML_LAUNCH_OK("png_enc_emit");
  return MSML_OK;
}
