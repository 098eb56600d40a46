// Baseline JPEG encoding on the device, byte for byte what libjpeg writes for PIL.Image.save (eval/align_dataset.py:52-75)
// and, for the entropy-coded data, for mx.recordio.pack_img (datasets/3d_tools/cvt_casia_webface.py:57).  The arithmetic
// is csrc/jpeg_enc_core.h, shared with the host check; tests/jpeg_enc_cases.py restates it.
//   k_jpeg_enc_dct   one workgroup of 64 per tile (a run of MCUs of one MCU row): the source rows are staged through LDS
//                    as Y, Cb, Cr planes (consecutive lanes read consecutive pixels, edges replicated as libjpeg does),
//                    then one thread per 8 x 8 block downsamples, transforms and quantises; int16 coefficients in zigzag
//                    order, blocks in scan order, dummy blocks included.  Each thread also zeroes its block's share of
//                    the bit buffer.  Writes status[n] (the source rectangle is checked here).
//   k_jpeg_enc_size  one thread per block: the bits it will emit (its DC predecessor read from the coefficients)
//   k_jpeg_enc_scan  one workgroup per image: bit offset of every block in its restart interval (a segmented scan),
//                    byte offset of every interval
//   k_jpeg_enc_emit  one thread per block: its codes at its bit offset of the unstuffed bit buffer; whole words are
//                    OR-ed in (atomicOr on the zeroed buffer: the first and last word of a block are shared with its
//                    neighbours), the last block of an interval pads with 1 bits
//   k_jpeg_enc_pack  one workgroup per image: counts the FF bytes in front of every byte (a scan) and writes header,
//                    stuffed data, RSTn markers and EOI into the slot; writes length[n], and status[n] for a slot that
//                    is too small
// Integer arithmetic only; the only atomics are the integer ORs, whose result does not depend on their order: two runs
// give the same bytes.  An image whose status is not 0 is skipped by the later passes.
#include "common.h"
#include "jpeg_enc_core.h"

struct JpeAtomicWord {
  unsigned int* p;
  __device__ void merge(long w, uint32_t v) { atomicOr(p + w, v); }
};

// writes inside [0, cap) of the image's slot only
struct JpeSlotOut {
  unsigned char* slot;
  long cap;
  __device__ void put(long pos, int v) {
    if (pos >= 0 && pos < cap) slot[pos] = (unsigned char)v;
  }
};

__global__ void __launch_bounds__(64) k_jpeg_enc_dct(const unsigned char* __restrict__ src, long src_bytes,
                                                     const long* __restrict__ meta, int channels, int swap_rb,
                                                     const int* __restrict__ desc, const int* __restrict__ qtabs,
                                                     unsigned char* __restrict__ ws, int* __restrict__ status) {
  __shared__ unsigned char s_y[JPE_TILE_PIXELS], s_cb[JPE_TILE_PIXELS], s_cr[JPE_TILE_PIXELS];
  __shared__ uint32_t s_div[2][64], s_rcp[2][64];
  __shared__ int s_dc[64];
  const int n = blockIdx.y, t = threadIdx.x;
  const int* d = desc + (long)n * JPE_DESC_WORDS;
  JpeGeom G;
  jpe_geom(d, G);
  const long* mt = meta + (long)n * 4;
  const bool ok = jpe_source_ok(G, mt, channels, src_bytes);
  if (blockIdx.x == 0 && t == 0) status[n] = ok ? JPE_OK : JPE_ERR_SOURCE;
  const int tm = jpe_tile_mcus(G);
  const int tpr = (G.mcux + tm - 1) / tm;                    // tiles per MCU row
  if (!ok || blockIdx.x >= (unsigned)(tpr * G.mcuy)) return;
  const int my = blockIdx.x / tpr, mx0 = (blockIdx.x - my * tpr) * tm;
  for (int k = t; k < 128; k += 64) {
    const int tb = k >> 6, z = k & 63;
    const uint32_t dv = 8u * (uint32_t)qtabs[(long)d[JE_QT + tb] * 64 + img_zigzag(z)];
    s_div[tb][z] = dv;
    s_rcp[tb][z] = jpe_recip(dv < 8u ? 8u : dv);
  }
  jpe_stage(G, src + mt[0], mt[3], channels, swap_rb, my, mx0, s_y, s_cb, s_cr, t, 64);
  __syncthreads();
  const int mloc = t / G.bpm, j = t - mloc * G.bpm, mx = mx0 + mloc;
  const bool mine = t < tm * G.bpm && mx < G.mcux;
  int comp = 0, jx = 0, jy = 0;
  bool dummy = false;
  if (mine) jpe_block_place(G, my, mx, j, comp, jx, jy, dummy);
  const long b = ((long)my * G.mcux + mx) * G.bpm + j;
  uint4* out = reinterpret_cast<uint4*>(ws + (long)d[JE_WS] * JPE_WS_ALIGN) + b * 8;
  if (mine && !dummy) {
    int blk[64];
    jpe_block_samples(G, s_y, s_cb, s_cr, mloc, comp, jx, jy, blk);
    jpe_fdct(blk);
    const int tb = comp ? 1 : 0;
    unsigned int pk[32];
#pragma unroll
    for (int k = 0; k < 64; k += 2) {
      const int a = jpe_quant(blk[img_zigzag(k)], s_div[tb][k], s_rcp[tb][k], k ? 1023 : 1024);
      const int c = jpe_quant(blk[img_zigzag(k + 1)], s_div[tb][k + 1], s_rcp[tb][k + 1], 1023);
      if (k == 0) s_dc[t] = a;
      pk[k >> 1] = ((unsigned int)a & 0xffffu) | ((unsigned int)c << 16);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = make_uint4(pk[4 * k], pk[4 * k + 1], pk[4 * k + 2], pk[4 * k + 3]);
  }
  __syncthreads();
  if (mine && dummy) {
    // AC zero, DC that of the previous block of the MCU (jccoefct.c): of the nearest real one, since dummies copy it on
    int s = t - 1;
    for (;;) {
      int c2, x2, y2;
      bool d2;
      jpe_block_place(G, my, mx, s - mloc * G.bpm, c2, x2, y2, d2);
      if (!d2) break;
      --s;
    }
    out[0] = make_uint4((unsigned int)s_dc[s] & 0xffffu, 0u, 0u, 0u);
    for (int k = 1; k < 8; ++k) out[k] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (mine) {
    uint4* z = reinterpret_cast<uint4*>(ws + (long)d[JE_WS] * JPE_WS_ALIGN + G.o_ubuf) + b * (JPE_BLOCK_BYTES / 16);
    for (int k = 0; k < JPE_BLOCK_BYTES / 16; ++k) z[k] = make_uint4(0u, 0u, 0u, 0u);
  }
}

__global__ void __launch_bounds__(256) k_jpeg_enc_size(const int* __restrict__ desc, unsigned char* __restrict__ ws,
                                                       const int* __restrict__ status) {
  __shared__ uint32_t s_huff[JPE_HUFF_WORDS];
  const int n = blockIdx.y;
  if (status[n] != 0) return;
  const int* d = desc + (long)n * JPE_DESC_WORDS;
  JpeGeom G;
  jpe_geom(d, G);
  if ((long)blockIdx.x * 256 >= G.nblk) return;
  jpe_huff_zero(s_huff, threadIdx.x, 256);
  __syncthreads();
  jpe_huff_fill(s_huff, threadIdx.x, 256);
  __syncthreads();
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= G.nblk) return;
  unsigned char* base = ws + (long)d[JE_WS] * JPE_WS_ALIGN;
  const int16_t* coef = reinterpret_cast<const int16_t*>(base);
  const long pb = jpe_pred_block(G, b);
  const int tb = (int)(b % G.bpm) < G.ny ? 0 : 1;
  JpeCountSink cs = {0};
  jpe_block_code(coef + b * 64, pb < 0 ? 0 : (int)coef[pb * 64], s_huff + 16 * tb, s_huff + JPE_HUFF_AC + 256 * tb, cs);
  reinterpret_cast<long*>(base + G.o_boff)[b] = cs.bits;
}

// Inclusive scan over the 256 values of the workgroup, restarting at every element whose flag is set.  -> the value;
// f becomes whether a flag is set at or before this thread.
__device__ inline long jpe_wg_scan(long v, int& f, long* s_v, int* s_f) {
  const int t = threadIdx.x;
  s_v[t] = v;
  s_f[t] = f;
  __syncthreads();
  for (int dlt = 1; dlt < 256; dlt <<= 1) {
    long pv = 0;
    int pf = 0;
    if (t >= dlt) {
      pv = s_v[t - dlt];
      pf = s_f[t - dlt];
    }
    __syncthreads();
    if (t >= dlt) {
      if (!s_f[t]) s_v[t] += pv;
      s_f[t] |= pf;
    }
    __syncthreads();
  }
  v = s_v[t];
  f = s_f[t];
  __syncthreads();
  return v;
}

__global__ void __launch_bounds__(256) k_jpeg_enc_scan(const int* __restrict__ desc, unsigned char* __restrict__ ws,
                                                       const int* __restrict__ status) {
  __shared__ long s_v[256];
  __shared__ int s_f[256];
  __shared__ long s_carry;
  const int n = blockIdx.x, t = threadIdx.x;
  if (status[n] != 0) return;
  const int* d = desc + (long)n * JPE_DESC_WORDS;
  JpeGeom G;
  jpe_geom(d, G);
  unsigned char* base = ws + (long)d[JE_WS] * JPE_WS_ALIGN;
  long* boff = reinterpret_cast<long*>(base + G.o_boff);
  long* ioff = reinterpret_cast<long*>(base + G.o_ioff);
  const long per = G.ri > 0 ? (long)G.ri * G.bpm : G.nblk;   // blocks of a whole interval
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (long b0 = 0; b0 < G.nblk; b0 += 256) {
    const long b = b0 + t;
    const long v = b < G.nblk ? boff[b] : 0;
    int f = b < G.nblk && b % per == 0;
    long inc = jpe_wg_scan(v, f, s_v, s_f);
    if (!f) inc += s_carry;                                  // the interval began in an earlier round
    if (b < G.nblk) {
      boff[b] = inc - v;
      if (b + 1 == G.nblk || (b + 1) % per == 0) ioff[b / per] = (inc + 7) >> 3;
    }
    __syncthreads();
    if (t == 255) s_carry = inc;
    __syncthreads();
  }
  // every interval's bytes -> its offset among the image's unstuffed bytes; ioff[nint] = all of them
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (long i0 = 0; i0 < G.nint; i0 += 256) {
    const long i = i0 + t;
    const long v = i < G.nint ? ioff[i] : 0;
    int f = 0;
    const long inc = jpe_wg_scan(v, f, s_v, s_f) + s_carry;
    if (i < G.nint) ioff[i] = inc - v;
    if (i + 1 == G.nint) ioff[G.nint] = inc;
    __syncthreads();
    if (t == 255) s_carry = inc;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_jpeg_enc_emit(const int* __restrict__ desc, unsigned char* __restrict__ ws,
                                                       const int* __restrict__ status) {
  __shared__ uint32_t s_huff[JPE_HUFF_WORDS];
  const int n = blockIdx.y;
  if (status[n] != 0) return;
  const int* d = desc + (long)n * JPE_DESC_WORDS;
  JpeGeom G;
  jpe_geom(d, G);
  if ((long)blockIdx.x * 256 >= G.nblk) return;
  jpe_huff_zero(s_huff, threadIdx.x, 256);
  __syncthreads();
  jpe_huff_fill(s_huff, threadIdx.x, 256);
  __syncthreads();
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= G.nblk) return;
  unsigned char* base = ws + (long)d[JE_WS] * JPE_WS_ALIGN;
  const int16_t* coef = reinterpret_cast<const int16_t*>(base);
  const long* boff = reinterpret_cast<const long*>(base + G.o_boff);
  const long* ioff = reinterpret_cast<const long*>(base + G.o_ioff);
  const long per = G.ri > 0 ? (long)G.ri * G.bpm : G.nblk;
  const long pb = jpe_pred_block(G, b);
  const int tb = (int)(b % G.bpm) < G.ny ? 0 : 1;
  JpeBitSink<JpeAtomicWord> bs;
  bs.out.p = reinterpret_cast<unsigned int*>(base + G.o_ubuf);
  bs.nwords = G.nblk * (JPE_BLOCK_BYTES / 4);
  bs.begin(ioff[b / per] * 8 + boff[b]);
  jpe_block_code(coef + b * 64, pb < 0 ? 0 : (int)coef[pb * 64], s_huff + 16 * tb, s_huff + JPE_HUFF_AC + 256 * tb, bs);
  if (b + 1 == G.nblk || (b + 1) % per == 0) bs.pad();
  bs.end();
}

__global__ void __launch_bounds__(256) k_jpeg_enc_pack(const int* __restrict__ desc, const unsigned char* __restrict__ ws,
                                                       const unsigned char* __restrict__ headers,
                                                       unsigned char* __restrict__ dst, long dst_bytes,
                                                       const long* __restrict__ out_meta, int* __restrict__ length,
                                                       int* __restrict__ status) {
  __shared__ long s_v[256];
  __shared__ int s_f[256];
  __shared__ long s_carry;
  const int n = blockIdx.x, t = threadIdx.x;
  if (status[n] != 0) {
    if (t == 0) length[n] = 0;
    return;
  }
  const long off = out_meta[(long)n * 2], cap = out_meta[(long)n * 2 + 1];
  if (off < 0 || cap < 0 || off > dst_bytes || cap > dst_bytes - off) {
    if (t == 0) {
      length[n] = 0;
      status[n] = JPE_ERR_SLOT;
    }
    return;
  }
  const int* d = desc + (long)n * JPE_DESC_WORDS;
  JpeGeom G;
  jpe_geom(d, G);
  const unsigned char* base = ws + (long)d[JE_WS] * JPE_WS_ALIGN;
  const long* ioff = reinterpret_cast<const long*>(base + G.o_ioff);
  const unsigned char* ub = base + G.o_ubuf;
  long U = ioff[G.nint];
  U = U < 0 ? 0 : (U > G.nblk * JPE_BLOCK_BYTES ? G.nblk * JPE_BLOCK_BYTES : U);   // what the bit buffer holds at most
  const int hlen = d[JE_HLEN];
  JpeSlotOut out = {dst + off, cap};
  for (int i = t; i < hlen; i += 256) out.put(i, headers[d[JE_HOFF] + i]);
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (long c0 = 0; c0 < U; c0 += 1024) {
    const long j0 = c0 + (long)t * 4, j1 = j0 + 4 < U ? j0 + 4 : U;
    long cnt = 0;
    for (long j = j0; j < j1; ++j) cnt += ub[j] == 0xFF;
    int f = 0;
    const long inc = jpe_wg_scan(cnt, f, s_v, s_f) + s_carry;
    jpe_pack_bytes(ub, j0, j1, ioff, G.nint, inc - cnt, hlen, out);
    __syncthreads();
    if (t == 255) s_carry = inc;
    __syncthreads();
  }
  if (t == 0) {
    const long L = hlen + U + s_carry + 2 * (G.nint - 1) + 2;
    const bool fits = L <= cap && L <= 0x7fffffffL;
    if (fits) {
      out.put(L - 2, 0xFF);
      out.put(L - 1, 0xD9);
    }
    length[n] = fits ? (int)L : 0;
    if (!fits) status[n] = JPE_ERR_SLOT;
  }
}

extern "C" long msml_jpeg_encode_workspace(int* desc, int N) {
  if (!desc || N < 1) return 0;
  long units = 0;
  for (int n = 0; n < N; ++n) {
    int* d = desc + (long)n * JPE_DESC_WORDS;
    d[JE_WS] = 0;
    if (jpe_desc_ok(d, 0x7fffffff, 0x7fffffffffffL) != 1) return 0;
    if (units > 0x7fffffffL) return 0;
    JpeGeom G;
    jpe_geom(d, G);
    d[JE_WS] = (int)units;
    units += G.bytes / JPE_WS_ALIGN;
  }
  return units * JPE_WS_ALIGN;
}

extern "C" long msml_jpeg_encode_bound(int H, int W, int sampling, int restart, int header_bytes) {
  return jpe_bound(H, W, sampling, restart, header_bytes);
}

extern "C" int msml_jpeg_encode(const unsigned char* src, long src_bytes, const long* meta, int channels, int swap_rb,
                                const int* desc, const int* desc_host, const int* qtabs, int nq,
                                const unsigned char* headers, long header_bytes, unsigned char* dst, long dst_bytes,
                                const long* out_meta, int* length, int* status, unsigned char* ws, long ws_bytes, int N,
                                void* stream) {
  MSML_CHECK(N >= 1 && N <= 65535, MSML_ERR_UNSUPPORTED, "jpeg_encode: N=%d outside 1..65535", N);
  MSML_CHECK(channels == 1 || channels == 3, MSML_ERR_UNSUPPORTED, "jpeg_encode: channels=%d (1 or 3)", channels);
  MSML_CHECK(src && meta && desc && desc_host && qtabs && headers && dst && out_meta && length && status && ws,
             MSML_ERR_SHAPE, "jpeg_encode: null pointer");
  MSML_CHECK(((uintptr_t)desc & 3) == 0 && ((uintptr_t)qtabs & 3) == 0 && ((uintptr_t)length & 3) == 0 &&
                 ((uintptr_t)status & 3) == 0 && ((uintptr_t)meta & 7) == 0 && ((uintptr_t)out_meta & 7) == 0 &&
                 ((uintptr_t)ws & 15) == 0,
             MSML_ERR_SHAPE, "jpeg_encode: desc, qtabs, length, status must be 4-byte, meta, out_meta 8-byte, ws 16-byte "
                             "aligned");
  MSML_CHECK(src_bytes >= 0 && dst_bytes >= 0 && ws_bytes >= 0 && header_bytes >= 0 && nq >= 1, MSML_ERR_SHAPE,
             "jpeg_encode: src_bytes=%ld dst_bytes=%ld ws_bytes=%ld header_bytes=%ld nq=%d", src_bytes, dst_bytes,
             ws_bytes, header_bytes, nq);
  long units = 0, max_blk = 0, max_tiles = 0;
  for (int n = 0; n < N; ++n) {
    const int* d = desc_host + (long)n * JPE_DESC_WORDS;
    MSML_CHECK(d[JE_SAMP] >= 0 && d[JE_SAMP] <= 3, MSML_ERR_UNSUPPORTED,
               "jpeg_encode: image %d: sampling %d (0 gray, 1 4:4:4, 2 4:2:2, 3 4:2:0)", n, d[JE_SAMP]);
    MSML_CHECK(d[JE_H] >= 1 && d[JE_H] <= 32767 && d[JE_W] >= 1 && d[JE_W] <= 32767, MSML_ERR_UNSUPPORTED,
               "jpeg_encode: image %d: size %d x %d outside 1..32767", n, d[JE_H], d[JE_W]);
    MSML_CHECK(channels == 3 || d[JE_SAMP] == 0, MSML_ERR_UNSUPPORTED,
               "jpeg_encode: image %d has a colour sampling, channels=1 takes gray only", n);
    MSML_CHECK(jpe_desc_ok(d, nq, header_bytes) == 1, MSML_ERR_SHAPE, "jpeg_encode: descriptor %d is inconsistent", n);
    JpeGeom G;
    jpe_geom(d, G);
    MSML_CHECK(d[JE_WS] == units, MSML_ERR_SHAPE, "jpeg_encode: descriptor %d: workspace offset %d, not the %ld "
               "msml_jpeg_encode_workspace writes", n, d[JE_WS], units);
    units += G.bytes / JPE_WS_ALIGN;
    MSML_CHECK(units * JPE_WS_ALIGN <= ws_bytes, MSML_ERR_WORKSPACE, "jpeg_encode: workspace of %ld bytes is too small "
               "(image %d ends at %ld)", ws_bytes, n, units * JPE_WS_ALIGN);
    const int tm = jpe_tile_mcus(G);
    const long tiles = (long)((G.mcux + tm - 1) / tm) * G.mcuy;
    max_blk = G.nblk > max_blk ? G.nblk : max_blk;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
  }
  hipStream_t s = (hipStream_t)stream;
  k_jpeg_enc_dct<<<dim3((unsigned)max_tiles, N), 64, 0, s>>>(src, src_bytes, meta, channels, swap_rb, desc, qtabs, ws, status);
  MSML_LAUNCH_OK("jpeg_enc_dct");
  k_jpeg_enc_size<<<dim3(cdiv(max_blk, 256), N), 256, 0, s>>>(desc, ws, status);
  MSML_LAUNCH_OK("jpeg_enc_size");
  k_jpeg_enc_scan<<<N, 256, 0, s>>>(desc, ws, status);
  MSML_LAUNCH_OK("jpeg_enc_scan");
  k_jpeg_enc_emit<<<dim3(cdiv(max_blk, 256), N), 256, 0, s>>>(desc, ws, status);
  MSML_LAUNCH_OK("jpeg_enc_emit");
  k_jpeg_enc_pack<<<N, 256, 0, s>>>(desc, ws, headers, dst, dst_bytes, out_meta, length, status);
  MSML_LAUNCH_OK("jpeg_enc_pack");
  return MSML_OK;
}
