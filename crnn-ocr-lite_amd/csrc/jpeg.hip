// Baseline JPEG files -> grey pages in a page arena (pages.h).  The host reads the headers (crnn_jpeg_plan: no GPU call), the device does the rest
// in three launches: entropy decode (one lane per restart segment), dequantisation + IDCT (eight lanes per block), upsampling + colour + grey.
// Everything after the entropy decode is integer arithmetic restated from libjpeg (jidctint's islow IDCT, the "fancy" upsampling, the 16-bit
// fixed-point YCbCr -> RGB) and equals crnn_mi355x/jpeg.py jpeg_decode_host bit for bit; the grey value is float64 with explicit fma(), so
// nothing here may be contracted (the pragma below, as in ingest.hip).  The contract is in include/crnn_mi355x.h.
#include "pages.h"
#include <string.h>
#include <vector>
#pragma clang fp contract(off)

#define JPEG_THREADS 256
#define JPEG_ZIGZAG                                                                                                                        \
  0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, \
      50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63
static const unsigned char jpeg_zz_host[64] = {JPEG_ZIGZAG};            // natural index of zigzag position k
__device__ const unsigned char jpeg_zz_dev[64] = {JPEG_ZIGZAG};

// ---------------------------------------------------------------- the plan (host) ----------------------------------------------------------------

namespace {

struct JpegFrame {
  int rows = 0, cols = 0, ncomp = 0, id[4] = {0, 0, 0, 0}, hs[4] = {0, 0, 0, 0}, vs[4] = {0, 0, 0, 0}, tq[4] = {0, 0, 0, 0};
};

struct JpegTables {
  bool q_have[4] = {false, false, false, false}, q16[4] = {false, false, false, false}, h_have[2][4] = {{false, false, false, false}, {false, false, false, false}};
  int q[4][CRNN_JPEG_QUANT_INTS];
  int h[2][4][CRNN_JPEG_HUFF_INTS];
};

struct JpegPool {
  int* pool;
  long cap, used = 0;
  long recent[16], added = 0;           // a ring of the last 16 tables added
  int recent_len[16];
  // -> the table's offset in the pool (one of the 16 tables before it when equal), or -1 when the pool is full
  long add(const int* t, int len) {
    for (int k = 0; k < (added < 16 ? added : 16); ++k)
      if (recent_len[k] == len && memcmp(pool + recent[k], t, sizeof(int) * len) == 0) return recent[k];
    if (used + len > cap) return -1;
    memcpy(pool + used, t, sizeof(int) * len);
    recent[added % 16] = used;
    recent_len[added % 16] = len;
    ++added;
    used += len;
    return used - len;
  }
};

inline int be16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

// One file.  d[0 .. len): its bytes; base: its offset in the blob.  -> the status; fills what it learnt into *it (rows / cols as soon as a frame
// header is read).  `segs_needed` and the pool advance only for a supported file.  -1: the pool is full (the call's fault, not the file's).
int jpeg_plan_file(const unsigned char* d, long len, long base, crnn_jpeg_item* it, JpegPool& pool, crnn_jpeg_seg* segs, long seg_cap, long& nsegs, int index) {
  if (len < 2 || d[0] != 0xFF || d[1] != 0xD8) return CRNN_JPEG_UNSUPPORTED;        // not a JPEG file
  JpegFrame fr;
  JpegTables* tb = new JpegTables;
  struct Free { JpegTables* p; ~Free() { delete p; } } guard{tb};
  bool have_frame = false, jfif = false, adobe = false;
  int adobe_transform = -1, restart = 0;
  long p = 2;
  for (;;) {
    if (p >= len || d[p] != 0xFF) return CRNN_JPEG_CORRUPT;
    while (p < len && d[p] == 0xFF) ++p;                                           // fill bytes in front of a marker
    if (p >= len) return CRNN_JPEG_CORRUPT;
    const int m = d[p++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;                            // stand-alone markers
    if (m == 0xD9 || m == 0xD8 || m == 0x00) return CRNN_JPEG_CORRUPT;              // no scan / a second SOI / stuffed data outside a scan
    if (p + 2 > len) return CRNN_JPEG_CORRUPT;
    const int L = be16(d + p);
    if (L < 2 || p + L > len) return CRNN_JPEG_CORRUPT;
    const unsigned char* s = d + p + 2;
    const int n = L - 2;
    if (m == 0xDB) {                                                                // DQT
      int o = 0;
      while (o < n) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (pq > 1 || tq > 3 || o + 1 + 64 * (pq + 1) > n) return CRNN_JPEG_CORRUPT;
        for (int k = 0; k < 64; ++k) tb->q[tq][jpeg_zz_host[k]] = pq ? be16(s + o + 1 + 2 * k) : s[o + 1 + k];
        tb->q_have[tq] = true;
        tb->q16[tq] = pq != 0;
        o += 1 + 64 * (pq + 1);
      }
    } else if (m == 0xC4) {                                                         // DHT
      int o = 0;
      while (o < n) {
        if (o + 17 > n) return CRNN_JPEG_CORRUPT;
        const int tc = s[o] >> 4, th = s[o] & 15;
        if (tc > 1 || th > 3) return CRNN_JPEG_CORRUPT;
        int total = 0, code = 0, k = 0;
        int* h = tb->h[tc][th];
        h[0] = h[17] = -1;
        h[18] = h[35] = 0;
        for (int l = 1; l <= 16; ++l) {
          const int cnt = s[o + l];
          total += cnt;
          h[18 + l] = k - code;
          code += cnt;
          if (code > (1 << l)) return CRNN_JPEG_CORRUPT;                            // the counts overflow the code space
          h[l] = cnt ? code - 1 : -1;
          k += cnt;
          code <<= 1;
        }
        if (total > 256 || o + 17 + total > n) return CRNN_JPEG_CORRUPT;
        for (int v = 0; v < 256; ++v) h[36 + v] = v < total ? s[o + 17 + v] : 0;
        for (int pre = 0; pre < 256; ++pre) {                                       // the look-ahead: what the length search finds within 8 bits
          h[292 + pre] = 0;
          for (int l = 1; l <= 8; ++l)
            if ((pre >> (8 - l)) <= h[l]) {
              h[292 + pre] = (l << 8) | h[36 + ((h[18 + l] + (pre >> (8 - l))) & 255)];
              break;
            }
        }
        tb->h_have[tc][th] = true;
        o += 17 + total;
      }
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {                  // a frame header
      if (have_frame || n < 6) return CRNN_JPEG_CORRUPT;
      const int prec = s[0], nc = s[5];
      fr.rows = be16(s + 1);
      fr.cols = be16(s + 3);
      if (n != 6 + 3 * nc || fr.rows == 0 || fr.cols == 0 || nc == 0) return CRNN_JPEG_CORRUPT;
      it->rows = fr.rows;
      it->cols = fr.cols;
      it->ncomp = nc;
      if (m > 0xC1 || prec != 8 || (nc != 1 && nc != 3)) return CRNN_JPEG_UNSUPPORTED;   // progressive, lossless, arithmetic, 12-bit, CMYK
      fr.ncomp = nc;
      for (int c = 0; c < nc; ++c) {
        fr.id[c] = s[6 + 3 * c];
        fr.hs[c] = s[7 + 3 * c] >> 4;
        fr.vs[c] = s[7 + 3 * c] & 15;
        fr.tq[c] = s[8 + 3 * c];
        if (fr.hs[c] < 1 || fr.hs[c] > 4 || fr.vs[c] < 1 || fr.vs[c] > 4 || fr.tq[c] > 3) return CRNN_JPEG_CORRUPT;
      }
      have_frame = true;
    } else if (m == 0xDD) {                                                         // DRI
      if (n != 2) return CRNN_JPEG_CORRUPT;
      restart = be16(s);
    } else if (m == 0xE0) {
      if (n >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
    } else if (m == 0xDA) {                                                         // SOS: the one scan
      if (!have_frame || n < 1) return CRNN_JPEG_CORRUPT;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return CRNN_JPEG_CORRUPT;
      if (ns != fr.ncomp) return CRNN_JPEG_UNSUPPORTED;                             // not one interleaved scan of all components
      int td[3], ta[3];
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != fr.id[c]) return CRNN_JPEG_UNSUPPORTED;                 // components out of the frame's order
        td[c] = s[2 + 2 * c] >> 4;
        ta[c] = s[2 + 2 * c] & 15;
        if (td[c] > 3 || ta[c] > 3) return CRNN_JPEG_CORRUPT;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return CRNN_JPEG_UNSUPPORTED;
      if (fr.ncomp == 1) {
        fr.hs[0] = fr.vs[0] = 1;                                                    // a one-component scan is not interleaved: its factors do not matter
      } else {
        const bool luma_ok = (fr.hs[0] == 1 && fr.vs[0] == 1) || (fr.hs[0] == 2 && fr.vs[0] == 1) || (fr.hs[0] == 2 && fr.vs[0] == 2);
        if (!luma_ok || fr.hs[1] != 1 || fr.vs[1] != 1 || fr.hs[2] != 1 || fr.vs[2] != 1) return CRNN_JPEG_UNSUPPORTED;
        if (adobe ? adobe_transform == 0 : (!jfif && fr.id[0] == 'R' && fr.id[1] == 'G' && fr.id[2] == 'B')) return CRNN_JPEG_UNSUPPORTED;   // RGB, not YCbCr
      }
      for (int c = 0; c < fr.ncomp; ++c) {
        if (!tb->q_have[fr.tq[c]] || !tb->h_have[0][td[c]] || !tb->h_have[1][ta[c]]) return CRNN_JPEG_CORRUPT;   // a missing table
        if (tb->q16[fr.tq[c]]) return CRNN_JPEG_UNSUPPORTED;
      }
      // the entropy-coded data: up to the first marker that is no restart marker, cut at the restart markers
      const int hmax = fr.hs[0], vmax = fr.vs[0];
      const int mcux = (fr.cols + 8 * hmax - 1) / (8 * hmax), mcuy = (fr.rows + 8 * vmax - 1) / (8 * vmax);
      const long nmcu = (long)mcux * mcuy;
      const long expect = restart ? (nmcu + restart - 1) / restart : 1;
      if (expect > 0x7fffffffL || nsegs + expect > 0x7fffffffL) return CRNN_JPEG_UNSUPPORTED;
      const long scan_off = p + L;
      long q = scan_off, seg_begin = scan_off, scan_end = len, found = 0;
      int end_marker = -1;
      auto emit = [&](long b, long e) {
        if (found < expect) {
          if (nsegs + found < seg_cap) {
            crnn_jpeg_seg& sg = segs[nsegs + found];
            sg.begin = base + b;
            sg.end = base + e;
            sg.item = index;
            sg.mcu0 = (int)(found * restart);
            sg.nmcu = (int)(restart ? (nmcu - found * restart < restart ? nmcu - found * restart : restart) : nmcu);
            sg.pad = 0;
          }
          ++found;
        }
      };
      while (q < len) {
        const unsigned char* f = (const unsigned char*)memchr(d + q, 0xFF, (size_t)(len - q));
        if (!f) break;
        const long ff = f - d;                                                      // the first FF of a run
        q = ff;
        while (q + 1 < len && d[q + 1] == 0xFF) ++q;
        if (q + 1 >= len) { scan_end = ff; break; }                                 // the file ends inside a marker
        const int c = d[q + 1];
        q += 2;
        if (c == 0) continue;                                                       // a stuffed FF
        if (restart && c >= 0xD0 && c <= 0xD7) { emit(seg_begin, ff); seg_begin = q; continue; }
        scan_end = ff;
        end_marker = c;
        break;
      }
      if (end_marker != -1 && end_marker != 0xD9) return CRNN_JPEG_UNSUPPORTED;     // more after the scan than EOI: further scans or tables
      if (seg_begin > scan_end) seg_begin = scan_end;
      emit(seg_begin, scan_end);
      while (found < expect) emit(scan_end, scan_end);                             // segments the file never reached: empty, the device reports TRUNCATED
      it->ncomp = fr.ncomp;
      it->restart = restart;
      it->mcux = mcux;
      it->mcuy = mcuy;
      it->scan_off = base + scan_off;
      it->scan_end = base + scan_end;
      it->seg0 = (int)nsegs;
      it->nseg = (int)expect;
      for (int c = 0; c < fr.ncomp; ++c) {
        it->hs[c] = fr.hs[c];
        it->vs[c] = fr.vs[c];
        const long a = pool.add(tb->q[fr.tq[c]], CRNN_JPEG_QUANT_INTS), b = pool.add(tb->h[0][td[c]], CRNN_JPEG_HUFF_INTS),
                   e = pool.add(tb->h[1][ta[c]], CRNN_JPEG_HUFF_INTS);
        if (a < 0 || b < 0 || e < 0 || e > 0x7fffffffL) return -1;
        it->qt[c] = (int)a;
        it->dc[c] = (int)b;
        it->ac[c] = (int)e;
      }
      nsegs += expect;
      return CRNN_JPEG_OK;
    }
    p += L;                                                                         // every other segment is skipped by its length
  }
}

inline long jpeg_item_samples(const crnn_jpeg_item& t) {
  long s = 0;
  for (int c = 0; c < t.ncomp && c < 3; ++c) s += (long)t.mcux * t.hs[c] * 8 * ((long)t.mcuy * t.vs[c] * 8);
  return s;
}

}  // namespace

extern "C" int crnn_jpeg_plan(const void* blob, long blob_bytes, const long* offs, const long* lens, int n, crnn_jpeg_item* items, int* pool, long pool_cap,
                              crnn_jpeg_seg* segs, long seg_cap, long* totals) {
  if (!blob || !offs || !lens || !items || !pool || !totals || n < 1 || blob_bytes < 0 || pool_cap < 0 || seg_cap < 0 || (seg_cap > 0 && !segs)) return CRNN_ERR_ARG;
  for (int i = 0; i < n; ++i)
    if (offs[i] < 0 || lens[i] < 0 || offs[i] > blob_bytes || lens[i] > blob_bytes - offs[i]) return CRNN_ERR_ARG;
  JpegPool pl;
  pl.pool = pool;
  pl.cap = pool_cap;
  long nsegs = 0, arena = 0, samples = 0;
  for (int i = 0; i < n; ++i) {
    crnn_jpeg_item& it = items[i];
    memset(&it, 0, sizeof(it));
    it.data_off = offs[i];
    const int st = jpeg_plan_file((const unsigned char*)blob + offs[i], lens[i], offs[i], &it, pl, segs, seg_cap, nsegs, i);
    if (st < 0) return CRNN_ERR_ARG;
    it.status = st;
    it.samp_off = samples;
    it.page_off = arena;
    it.stride = it.cols;
    if (st == CRNN_JPEG_OK) {
      samples += jpeg_item_samples(it);
      arena += (long)page_up16((size_t)it.rows * it.cols);
    }
  }
  totals[0] = pl.used;
  totals[1] = nsegs;
  totals[2] = arena;
  totals[3] = samples;
  return nsegs > seg_cap ? CRNN_ERR_ARG : CRNN_OK;
}

// ---------------------------------------------------------------- 1: entropy decode ----------------------------------------------------------------

struct JpegBits {
  const unsigned char* d;
  long pos, end;
  unsigned long long acc;
  int cnt, pad;                        // cnt bits in acc, the lowest `pad` of them zeros from past the segment's end
  bool stuffed;                        // the byte before was the data byte FF: the next one (the stuffed 00) is skipped
  // four raw bytes at once -- the four loads do not depend on one another, and each lies inside the segment -- give 2 to 4 data bytes
  __device__ __forceinline__ void fill4() {
    unsigned raw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) raw[i] = pos + i < end ? d[pos + i] : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (stuffed) { stuffed = false; ++pos; continue; }
      unsigned b = 0;
      if (pos < end) {
        b = raw[i];
        ++pos;
        stuffed = b == 0xFF;           // FF xx: the data byte FF
      } else {
        pad += 8;
      }
      acc = (acc << 8) | b;
      cnt += 8;
    }
  }
  __device__ __forceinline__ unsigned peek16() {
    if (cnt < 16) fill4();             // two stuffed bytes at the most among four: at least 16 bits more
    return (unsigned)(acc >> (cnt - 16)) & 0xffffu;
  }
  // -> true when one of the n bits consumed came from past the end
  __device__ __forceinline__ bool skip(int n) {
    cnt -= n;
    if (cnt < pad) { pad = cnt; return true; }
    return false;
  }
};

// one Huffman symbol -> 0..255, or -1 when no code of up to 16 bits matches
__device__ __forceinline__ int jpeg_symbol(JpegBits& br, const int* __restrict__ tab, bool& trunc) {
  const int v = (int)br.peek16();
  const int e = tab[292 + (v >> 8)];   // codes of up to 8 bits: one load
  if (e) {
    trunc |= br.skip((e >> 8) & 15);
    return e & 255;
  }
  int l = 17;                          // 9..16 bits: the shortest length whose code is within maxcode; the eight loads do not depend on one another
#pragma unroll
  for (int k = 16; k >= 9; --k)
    if ((v >> (16 - k)) <= tab[k]) l = k;
  if (l > 16) return -1;
  trunc |= br.skip(l);
  return tab[36 + ((tab[18 + l] + (v >> (16 - l))) & 255)] & 255;
}

__device__ __forceinline__ int jpeg_receive_extend(JpegBits& br, int s, bool& trunc) {
  const int v = (int)(br.peek16() >> (16 - s));
  trunc |= br.skip(s);
  return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_entropy_kernel(const unsigned char* __restrict__ blob, long blob_bytes, const crnn_jpeg_item* __restrict__ items,
                                                                    int n, const crnn_jpeg_seg* __restrict__ segs, long nsegs, const int* __restrict__ pool,
                                                                    long pool_ints, short* __restrict__ coef, long samples, int* __restrict__ status) {
  __shared__ unsigned char zz[64];     // the zigzag order out of LDS: one dependent global load less per coefficient
  if (threadIdx.x < 64) zz[threadIdx.x] = jpeg_zz_dev[threadIdx.x];
  __syncthreads();
  const long t = (long)blockIdx.x * JPEG_THREADS + threadIdx.x;
  if (t < n) {
    const int st = items[t].status & ~CRNN_JPEG_SKIP;
    if (st) atomicOr(&status[t], st);
  }
  if (t >= nsegs) return;
  const crnn_jpeg_seg sg = segs[t];
  if (sg.item < 0 || sg.item >= n) return;
  const crnn_jpeg_item& it = items[sg.item];
  if (it.status != 0) return;
  const int ncomp = min(max(it.ncomp, 1), 3), mcux = max(it.mcux, 1);
  JpegBits br;
  br.d = blob;
  br.end = sg.end < 0 ? 0 : (sg.end > blob_bytes ? blob_bytes : sg.end);
  br.pos = sg.begin < 0 ? 0 : (sg.begin > br.end ? br.end : sg.begin);
  br.acc = 0;
  br.cnt = br.pad = 0;
  br.stuffed = false;
  unsigned pred[3] = {0u, 0u, 0u};
  bool trunc = false, bad = false;
  long comp_base[3];
  int hs[3], vs[3];
  const int *dct[3], *act[3];
  long base = it.samp_off;
  for (int c = 0; c < 3; ++c) {
    hs[c] = c < ncomp ? min(max(it.hs[c], 1), 2) : 0;
    vs[c] = c < ncomp ? min(max(it.vs[c], 1), 2) : 0;
    comp_base[c] = base;
    base += (long)mcux * hs[c] * 8 * ((long)it.mcuy * vs[c] * 8);
    const long lim = pool_ints - CRNN_JPEG_HUFF_INTS;
    dct[c] = pool + (c < ncomp ? min(max((long)it.dc[c], 0L), lim) : 0);
    act[c] = pool + (c < ncomp ? min(max((long)it.ac[c], 0L), lim) : 0);
  }
  for (int m = 0; m < sg.nmcu && !bad; ++m) {
    const int mcu = sg.mcu0 + m, my = mcu / mcux, mx = mcu - my * mcux;
    for (int c = 0; c < ncomp && !bad; ++c)
      for (int bv = 0; bv < vs[c] && !bad; ++bv)
        for (int bh = 0; bh < hs[c] && !bad; ++bh) {
          const long blk = (long)(my * vs[c] + bv) * (mcux * hs[c]) + (mx * hs[c] + bh);
          const long at = comp_base[c] + blk * 64;
          if (at < 0 || at + 64 > samples) { bad = true; break; }                  // (the host's checks make this unreachable)
          short* o = coef + at;
          const int s = jpeg_symbol(br, dct[c], trunc);
          if (s < 0 || s > 11) { bad = true; break; }
          if (s) pred[c] += (unsigned)jpeg_receive_extend(br, s, trunc);
          o[0] = (short)pred[c];
          for (int k = 1; k < 64; ++k) {
            const int rs = jpeg_symbol(br, act[c], trunc);
            if (rs < 0) { bad = true; break; }
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0 && r != 15) break;                                          // end of block
            if (k + r > 63) { bad = true; break; }                                 // a run past position 63
            k += r;
            if (sz) o[zz[k]] = (short)jpeg_receive_extend(br, sz, trunc);
          }
        }
  }
  const int flags = (bad ? CRNN_JPEG_CORRUPT : 0) | (trunc ? CRNN_JPEG_TRUNCATED : 0);
  if (flags) atomicOr(&status[sg.item], flags);
}

// ---------------------------------------------------------------- 2: dequantisation + IDCT ----------------------------------------------------------------

// the last file whose first sample is at or before s (files without samples share the offset of the file after them): at most 32 steps
__device__ __forceinline__ int jpeg_file_of(const crnn_jpeg_item* __restrict__ items, int n, long s) {
  int lo = 0, hi = n - 1;
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].samp_off <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// jidctint's 1-D pass on wrapped 32-bit values (unsigned: overflow of absurd coefficients is defined)
__device__ __forceinline__ void jpeg_idct8(const unsigned (&i)[8], unsigned (&o)[8]) {
  unsigned z1 = (i[2] + i[6]) * 4433u;
  const unsigned t2 = z1 - i[6] * 15137u, t3 = z1 + i[2] * 6270u;
  const unsigned t0 = (i[0] + i[4]) << 13, t1 = (i[0] - i[4]) << 13;
  const unsigned t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  unsigned a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  unsigned z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const unsigned z5 = (z3 + z4) * 9633u;
  a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
  z1 *= (unsigned)-7373; z2 *= (unsigned)-20995;
  z3 = z3 * (unsigned)-16069 + z5;
  z4 = z4 * (unsigned)-3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  o[0] = t10 + a3; o[1] = t11 + a2; o[2] = t12 + a1; o[3] = t13 + a0;
  o[4] = t13 - a0; o[5] = t12 - a1; o[6] = t11 - a2; o[7] = t10 - a3;
}

#define JPEG_TILE 72   // ints per block in LDS: rows of 9 (8 + 1 pad), so that the column and the row accesses of a wave's 8 blocks hit 64 banks

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const crnn_jpeg_item* __restrict__ items, int n, const int* __restrict__ pool, long pool_ints,
                                                                 const short* __restrict__ coef, unsigned char* __restrict__ planes, long samples,
                                                                 const int* __restrict__ status) {
  __shared__ unsigned tile[(JPEG_THREADS / 8) * JPEG_TILE];
  const int tid = threadIdx.x, lane = tid & 7, b = tid >> 3;
  const long g = (long)blockIdx.x * (JPEG_THREADS / 8) + b;        // the block, counted over the whole workspace
  unsigned* tl = tile + b * JPEG_TILE;
  bool live = g * 64 + 64 <= samples;
  long out = 0;
  int pw = 0;
  if (live) {
    const int f = jpeg_file_of(items, n, g * 64);
    const crnn_jpeg_item& it = items[f];
    live = it.status == 0 && status[f] == 0;
    if (live) {
      long lb = g - it.samp_off / 64, base = it.samp_off;
      const int ncomp = min(max(it.ncomp, 1), 3);
      int c = 0, bw = 1;
      for (; c < ncomp; ++c) {
        bw = max(it.mcux, 1) * min(max(it.hs[c], 1), 2);
        const long nb = (long)bw * (max(it.mcuy, 1) * min(max(it.vs[c], 1), 2));
        if (lb < nb) break;
        lb -= nb;
        base += nb * 64;
      }
      live = c < ncomp && lb >= 0;
      if (live) {
        const long by = lb / bw, bx = lb - by * bw;
        pw = bw * 8;
        out = base + (by * 8 + lane) * pw + bx * 8;
        live = out >= 0 && out + 8 <= samples;
        const int* q = pool + min(max((long)it.qt[c], 0L), pool_ints - CRNN_JPEG_QUANT_INTS) + lane * 8;
        const int4 raw = *reinterpret_cast<const int4*>(coef + g * 64 + lane * 8);        // row `lane` of the block: 8 int16
        const int w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          tl[lane * 9 + 2 * k] = (unsigned)(int)(short)(w[k] & 0xffff) * (unsigned)q[2 * k];
          tl[lane * 9 + 2 * k + 1] = (unsigned)(w[k] >> 16) * (unsigned)q[2 * k + 1];
        }
      }
    }
  }
  __syncthreads();
  unsigned in[8], o[8];
  if (live) {                                                      // column `lane`
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = tl[r * 9 + lane];
    jpeg_idct8(in, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) tl[r * 9 + lane] = (unsigned)((int)(o[r] + (1u << 10)) >> 11);
  }
  __syncthreads();
  if (live) {                                                      // row `lane`
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = tl[lane * 9 + k];
    jpeg_idct8(in, o);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int v = ((int)(o[k] + (1u << 17)) >> 18) + 128;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      if (k < 4) lo |= (unsigned)v << (8 * k); else hi |= (unsigned)v << (8 * (k - 4));
    }
    *reinterpret_cast<uint2*>(planes + out) = make_uint2(lo, hi);
  }
}

// ---------------------------------------------------------------- 3: upsampling + colour + grey ----------------------------------------------------------------

struct JpegPlane {
  const unsigned char* p;
  int pw, dw, dh;                                                  // the plane's row length, the component's columns and rows
  __device__ __forceinline__ int at(int r, int c) const { return p[(long)r * pw + c]; }
};

// the chroma sample at pixel (r, c) of a component at half the width (h2v1) or half the width and height (h2v2): libjpeg's "fancy" upsampling
__device__ __forceinline__ int jpeg_chroma(const JpegPlane& pl, int hs, int vs, int r, int c) {
  if (hs == 1) return pl.at(r, c);
  const int cc = c >> 1;
  if (vs == 1) {
    if (pl.dw <= 2 || c == 0 || c == 2 * pl.dw - 1) return pl.at(r, cc);
    return (c & 1) ? (3 * pl.at(r, cc) + pl.at(r, cc + 1) + 2) >> 2 : (3 * pl.at(r, cc) + pl.at(r, cc - 1) + 1) >> 2;
  }
  const int rr = r >> 1;
  if (pl.dw <= 2) return pl.at(rr, cc);
  int far = (r & 1) ? rr + 1 : rr - 1;
  far = far < 0 ? 0 : (far > pl.dh - 1 ? pl.dh - 1 : far);
  const int s = 3 * pl.at(rr, cc) + pl.at(far, cc);
  if (c == 0) return (4 * s + 8) >> 4;
  if (c == 2 * pl.dw - 1) return (4 * s + 7) >> 4;
  if (c & 1) return (3 * s + 3 * pl.at(rr, cc + 1) + pl.at(far, cc + 1) + 7) >> 4;
  return (3 * s + 3 * pl.at(rr, cc - 1) + pl.at(far, cc - 1) + 8) >> 4;
}

__device__ __forceinline__ int jpeg_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_grey_kernel(const crnn_jpeg_item* __restrict__ items, int n, const unsigned char* __restrict__ planes,
                                                                 long samples, const int* __restrict__ status, unsigned char* __restrict__ arena, long out_bytes) {
  for (int f = blockIdx.y; f < n; f += gridDim.y) {
    const crnn_jpeg_item& it = items[f];
    if (it.status != 0) continue;                                  // refused by the plan, or the caller's to decode: not written at all
    crnn_page_item pg;
    pg.page_off = it.page_off; pg.rows = it.rows; pg.cols = it.cols; pg.stride = it.stride;
    if (it.rows < 1 || it.cols < 1 || page_outside(pg, it.rows, it.cols, out_bytes, out_bytes)) continue;
    const long npix = (long)it.rows * it.cols;
    const bool zero = status[f] != 0;
    const int ncomp = min(max(it.ncomp, 1), 3), hs = ncomp == 3 ? min(max(it.hs[0], 1), 2) : 1, vs = ncomp == 3 ? min(max(it.vs[0], 1), 2) : 1;
    const int mcux = max(it.mcux, 1), mcuy = max(it.mcuy, 1);
    JpegPlane Y, Cb, Cr;
    Y.p = planes + it.samp_off; Y.pw = mcux * hs * 8; Y.dw = it.cols; Y.dh = it.rows;
    const long ysz = (long)Y.pw * (mcuy * vs * 8), csz = (long)mcux * 8 * (mcuy * 8);
    Cb.p = Y.p + ysz; Cb.pw = mcux * 8; Cb.dw = (it.cols + hs - 1) / hs; Cb.dh = (it.rows + vs - 1) / vs;
    Cr = Cb; Cr.p = Cb.p + csz;
    // every plane read stays inside the file's samples: rows < mcuy vs 8 and cols < pw follow from the MCU grid covering the image
    const bool fits = it.samp_off >= 0 && it.samp_off + ysz + (ncomp == 3 ? 2 * csz : 0) <= samples && (long)mcux * hs * 8 >= it.cols && (long)mcuy * vs * 8 >= it.rows;
    for (long px = (long)blockIdx.x * JPEG_THREADS + threadIdx.x; px < npix; px += (long)gridDim.x * JPEG_THREADS) {
      const int r = (int)(px / it.cols), c = (int)(px - (long)r * it.cols);
      int v = 0;
      if (!zero && fits) {
        const int y = Y.at(r, c);
        if (ncomp == 1) {
          v = y;
        } else {
          const int cb = jpeg_chroma(Cb, hs, vs, r, c) - 128, cr = jpeg_chroma(Cr, hs, vs, r, c) - 128;
          const int R = jpeg_clamp8(y + ((91881 * cr + 32768) >> 16));
          const int G = jpeg_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
          const int B = jpeg_clamp8(y + ((116130 * cb + 32768) >> 16));
          const double gy = floor(fma(0.114, (double)B, fma(0.587, (double)G, 0.299 * (double)R)) + 0.5);
          v = gy < 0.0 ? 0 : (gy > 255.0 ? 255 : (int)gy);
        }
      }
      arena[it.page_off + (long)r * it.stride + c] = (unsigned char)v;
    }
  }
}

// ---------------------------------------------------------------- the launcher ----------------------------------------------------------------

extern "C" size_t crnn_jpeg_workspace_bytes(long samples) {
  if (samples < 0) return 0;
  return page_up16((size_t)samples * 2) + page_up16((size_t)samples);
}

extern "C" int crnn_jpeg_decode(const void* blob_dev, long blob_bytes, const crnn_jpeg_item* items, const crnn_jpeg_item* items_dev, int n,
                                const crnn_jpeg_seg* segs, const crnn_jpeg_seg* segs_dev, long nsegs, const int* pool_dev, long pool_ints,
                                void* out_arena, long out_bytes, int* status_dev, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (!blob_dev || !items || !items_dev || !pool_dev || !out_arena || !status_dev || n < 1 || blob_bytes < 0 || nsegs < 0 || out_bytes < 0) return CRNN_ERR_ARG;
  if (nsegs > 0 && (!segs || !segs_dev)) return CRNN_ERR_ARG;
  if (pool_ints < 0 || nsegs > 0x7fffffffL) return CRNN_ERR_ARG;
  long samples = 0, max_pix = 0, live_segs = 0;
  for (int i = 0; i < n; ++i) {
    const crnn_jpeg_item& t = items[i];
    if (t.samp_off != samples) return CRNN_ERR_ARG;                // the files' samples follow one another in index order
    if (t.status != 0) continue;
    if ((t.ncomp != 1 && t.ncomp != 3) || t.mcux < 1 || t.mcuy < 1 || t.rows > 65535 || t.cols > 65535) return CRNN_ERR_ARG;
    CRNN_TRY(page_check(t.page_off, t.rows, t.cols, t.stride, 0, -1, out_bytes));
    for (int c = 0; c < t.ncomp; ++c) {
      const bool luma2 = t.ncomp == 3 && c == 0;
      if (t.hs[c] < 1 || t.vs[c] < 1 || t.hs[c] > (luma2 ? 2 : 1) || t.vs[c] > (luma2 ? t.hs[c] : 1)) return CRNN_ERR_ARG;
      if (t.qt[c] < 0 || t.qt[c] > pool_ints - CRNN_JPEG_QUANT_INTS || t.dc[c] < 0 || t.dc[c] > pool_ints - CRNN_JPEG_HUFF_INTS || t.ac[c] < 0 ||
          t.ac[c] > pool_ints - CRNN_JPEG_HUFF_INTS)
        return CRNN_ERR_ARG;
    }
    if ((long)t.mcux * t.hs[0] * 8 < t.cols || (long)t.mcuy * t.vs[0] * 8 < t.rows || (long)t.mcux * t.hs[0] * 8 > 65535 + 16 || (long)t.mcuy * t.vs[0] * 8 > 65535 + 16)
      return CRNN_ERR_ARG;
    if (t.nseg < 1 || t.seg0 < 0 || (long)t.seg0 + t.nseg > nsegs) return CRNN_ERR_ARG;
    samples += jpeg_item_samples(t);
    if (samples > 0x7fffffffL) return CRNN_ERR_UNSUPPORTED;
    const long pix = (long)t.rows * t.cols;
    max_pix = pix > max_pix ? pix : max_pix;
    live_segs += t.nseg;
  }
  for (long s = 0; s < nsegs; ++s) {
    const crnn_jpeg_seg& sg = segs[s];
    if (sg.item < 0 || sg.item >= n || sg.begin < 0 || sg.begin > sg.end || sg.end > blob_bytes || sg.mcu0 < 0 || sg.nmcu < 0) return CRNN_ERR_ARG;
    const crnn_jpeg_item& t = items[sg.item];
    if (t.status == 0 && (long)sg.mcu0 + sg.nmcu > (long)t.mcux * t.mcuy) return CRNN_ERR_ARG;
  }
  const size_t coef_bytes = page_up16((size_t)samples * 2);
  if (samples > 0 && (!ws || ((uintptr_t)ws & 15) || ws_bytes < crnn_jpeg_workspace_bytes(samples))) return CRNN_ERR_ARG;
  short* coef = (short*)ws;
  unsigned char* planes = (unsigned char*)ws + coef_bytes;
  hipError_t e = hipMemsetAsync(status_dev, 0, sizeof(int) * (size_t)n, stream);
  if (e != hipSuccess) return (int)e;
  if (samples > 0) {
    e = hipMemsetAsync(coef, 0, coef_bytes, stream);
    if (e != hipSuccess) return (int)e;
  }
  const long lanes = nsegs > n ? nsegs : n;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(cdiv(lanes, JPEG_THREADS)), dim3(JPEG_THREADS), 0, stream, (const unsigned char*)blob_dev, blob_bytes, items_dev, n,
                     segs_dev, nsegs, pool_dev, pool_ints, coef, samples, status_dev);
  CRNN_LAUNCH_CHECK();
  if (samples == 0 || live_segs == 0) return CRNN_OK;              // nothing for the device to decode
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(cdiv(samples / 64, JPEG_THREADS / 8)), dim3(JPEG_THREADS), 0, stream, items_dev, n, pool_dev, pool_ints,
                     (const short*)coef, planes, samples, (const int*)status_dev);
  CRNN_LAUNCH_CHECK();
  const long gx = cdiv(max_pix, JPEG_THREADS);
  hipLaunchKernelGGL(jpeg_grey_kernel, dim3((unsigned)(gx > 16384 ? 16384 : gx), (unsigned)(n > 65535 ? 65535 : n)), dim3(JPEG_THREADS), 0, stream, items_dev, n,
                     (const unsigned char*)planes, samples, (const int*)status_dev, (unsigned char*)out_arena, out_bytes);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
