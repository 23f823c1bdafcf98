// Adaptive (Sauvola) binarisation of page images on the device: uint8 pages in an arena (pages.h defines it) -> 0 (ink) / 255 pages in an
// arena of the same layout.  Integer-only (the rule: include/crnn_mi355x.h; the same rule in NumPy: crnn_mi355x/binarize.py): the window sums
// S = sum v and Q = sum v^2 over the (2 r + 1)^2 window clipped to the page, D = n Q - S^2, sd = floor(sqrt(D)) made exact by two correction
// loops, and one int64 comparison.  No float decision, no atomics: two calls agree bit for bit and equal the host.
//
// One launch, grid (strips, bands, pages), 256 threads.  A workgroup writes CRNN_BINARIZE_STRIP_C = 192 columns of CRNN_BINARIZE_BAND_R = 64
// rows; lane t owns the loaded column C0 - 32 + t (32 >= r columns of halo either side), so every row access is one coalesced byte load per lane.
// The box filter is separable and costs O(1) per pixel:
//   vertical first, in registers: each lane keeps the running sums of v and v^2 of its column over the rows i - r .. i + r (the row entering
//     r below is added, the row leaving r + 1 above is read again -- an L2 hit, the workgroup read it 2 r + 1 rows ago -- and subtracted).
//     Nothing is scanned for the leaving row and no ring of row sums is kept: the column sums are linear, so one scan of them per OUTPUT row
//     gives what the scans of the entering and the leaving row would give.  Rows and columns outside the page count 0, which is the clipping.
//   horizontal second: an inclusive prefix sum of the 256 column sums (<= 63 * 255 * 256 < 2^23 for v, <= 63 * 255^2 * 256 < 2^31 for v^2):
//     six DPP steps inside each wavefront, the wave-local prefixes and the four wave totals through LDS, one barrier per row (the LDS rows are
//     double-buffered on the row's parity); a window sum is the difference of two prefixes fewer than 64 lanes apart, so it needs one wave
//     total at most.  The 192 decisions of a row are made by the first three wavefronts, whole (lane t decides column C0 + t from the prefixes
//     at LDS positions t + 32 + r and t + 32 - r - 1), not by the middle 192 lanes of four.
// 32-bit arithmetic up to S, Q, v n^2 and S n (all < 2^32); 64-bit for D, sd and the comparison.  Stores are plain byte stores.
#include "pages.h"
#pragma clang fp contract(off)

#define BIN_THREADS 256
#define BIN_WAVES (BIN_THREADS / 64)
#define BIN_STRIP_C CRNN_BINARIZE_STRIP_C
#define BIN_BAND_R CRNN_BINARIZE_BAND_R
#define BIN_HALO ((BIN_THREADS - BIN_STRIP_C) / 2)
#define BIN_MAX_RADIUS 31
static_assert(BIN_STRIP_C + 2 * BIN_HALO == BIN_THREADS && BIN_HALO > BIN_MAX_RADIUS, "one loaded column per lane, the halo wider than any radius");

// The byte of row y of a column of the page (`col`: the column's first byte, the column clamped into the page).  The load is unconditional --
// the row is clamped into the page, and the kernel has checked once that the page lies inside the arena -- so that the loads of a row are
// issued together and ahead of their use, with no branch and no wait between them; bin_value then makes v of it, 0 outside the page.
__device__ __forceinline__ unsigned bin_load(const unsigned char* col, int stride, int rows, int y) {
  return col[(long)page_clampi(y, 0, rows - 1) * stride];
}
__device__ __forceinline__ unsigned bin_value(unsigned p, bool in, bool light) { return in ? (light ? 255u - p : p) : 0u; }

// inclusive prefix sum over the 64 lanes of a wavefront: row_shr 1 2 4 8 inside the rows of 16 lanes, then row_bcast 15 into rows 1 and 3 and
// row_bcast 31 into rows 2 and 3; a lane without a source adds 0 (`old`)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned bin_dpp_add(unsigned v) {
  return v + (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ unsigned bin_wave_scan(unsigned v) {
  v = bin_dpp_add<0x111, 0xf>(v);
  v = bin_dpp_add<0x112, 0xf>(v);
  v = bin_dpp_add<0x114, 0xf>(v);
  v = bin_dpp_add<0x118, 0xf>(v);
  v = bin_dpp_add<0x142, 0xa>(v);
  v = bin_dpp_add<0x143, 0xc>(v);
  return v;
}

// floor(sqrt(D)), D < 2^40 (exact in a double).  The double-precision root is the hardware's own (v_sqrt_f64, good to about 2^-23 relative:
// within 1 of the answer, which is below 2^20) instead of the library's correctly rounded one, 20 double-precision operations: the two
// correction loops of the rule make the result exact either way, and each takes a step at most.
__device__ __forceinline__ unsigned bin_isqrt(unsigned long long D) {
  unsigned s = (unsigned)__builtin_amdgcn_sqrt((double)D);
  while ((unsigned long long)s * s > D) --s;
  while ((unsigned long long)(s + 1) * (s + 1) <= D) ++s;
  return s;
}

__global__ __launch_bounds__(BIN_THREADS) void bin_sauvola_kernel(const unsigned char* __restrict__ arena, long arena_bytes,
                                                                  const crnn_page_item* __restrict__ pages, int radius, int k256, int polarity,
                                                                  unsigned char* __restrict__ out, long out_bytes) {
  __shared__ unsigned pS[2][BIN_THREADS], pQ[2][BIN_THREADS];   // wave-local inclusive prefixes of the column sums, by row parity
  __shared__ unsigned tS[2][BIN_WAVES], tQ[2][BIN_WAVES];       // and each wavefront's total
  const crnn_page_item pg = pages[blockIdx.z];
  const int rows = page_clampi(pg.rows, 0, PAGE_MAX_DIM), cols = page_clampi(pg.cols, 0, PAGE_MAX_DIM);
  const int C0 = (int)blockIdx.x * BIN_STRIP_C, R0 = (int)blockIdx.y * BIN_BAND_R;
  if (C0 >= cols || R0 >= rows) return;                         // (uniform over the workgroup)
  if (page_outside(pg, rows, cols, arena_bytes, out_bytes)) return;   // (uniform; pages.h: no load or store below needs a check of its own)
  const int r = page_clampi(radius, 1, BIN_MAX_RADIUS);
  const unsigned k = (unsigned)page_clampi(k256, 0, 255);
  const bool light = polarity == 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // two roles per lane: it SUMS the loaded column c = C0 - 32 + tid, and (the first 192 lanes, three whole wavefronts) it DECIDES the pixel of
  // column cw = C0 + tid from the prefixes at the loaded columns cw + r and cw - r - 1, which sit at hi and lo in the LDS row
  const int c = C0 - BIN_HALO + tid, cw = C0 + tid;
  const bool col_in = c >= 0 && c < cols;
  const bool writes = tid < BIN_STRIP_C && cw < cols;
  const int hi = tid + BIN_HALO + r, lo = tid + BIN_HALO - r - 1;      // 0 <= lo < hi <= 254, hi - lo < 64: at most one wavefront apart
  const bool split = (hi >> 6) != (lo >> 6);
  const int nc = (cw + r < cols - 1 ? cw + r : cols - 1) - (cw - r > 0 ? cw - r : 0) + 1;
  const int rend = R0 + BIN_BAND_R < rows ? R0 + BIN_BAND_R : rows;
  const unsigned char* col = arena + pg.page_off + page_clampi(c, 0, cols - 1);
  const unsigned char* colw = arena + pg.page_off + page_clampi(cw, 0, cols - 1);

  unsigned cs = 0, cq = 0;                                      // column c's sums over the rows of the window
  const int y1 = R0 + r < rows ? R0 + r : rows;
  for (int y = R0 - r > 0 ? R0 - r : 0; y < y1; y += 4) {       // the rows above row R0's entering one, four loads in flight
    unsigned p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = bin_load(col, pg.stride, rows, y + q);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned v = bin_value(p[q], col_in && y + q < y1, light);
      cs += v;
      cq += v * v;
    }
  }
  // the bytes of the entering row and the leaving row of column c and of this row of column cw, loaded one row ahead of their use
  unsigned pe = bin_load(col, pg.stride, rows, R0 + r), pl = bin_load(col, pg.stride, rows, R0 - r), pc = bin_load(colw, pg.stride, rows, R0);
  for (int i = R0; i < rend; ++i) {                             // i counts up to rend (uniform: every lane meets every barrier)
    const unsigned ve = bin_value(pe, col_in && i + r < rows, light), vl = bin_value(pl, col_in && i - r >= 0, light), v = bin_value(pc, true, light);
    pe = bin_load(col, pg.stride, rows, i + 1 + r);
    pl = bin_load(col, pg.stride, rows, i + 1 - r);
    pc = bin_load(colw, pg.stride, rows, i + 1);
    cs += ve;
    cq += ve * ve;
    const int b = i & 1;
    const unsigned ps = bin_wave_scan(cs), pq = bin_wave_scan(cq);
    pS[b][tid] = ps;
    pQ[b][tid] = pq;
    if (lane == 63) { tS[b][wave] = ps; tQ[b][wave] = pq; }
    __syncthreads();
    if (writes) {
      // inclusive prefix at x = its wave-local one + the totals of the wavefronts before x's: the difference of two needs lo's wavefront's total at most
      const unsigned S = pS[b][hi] - pS[b][lo] + (split ? tS[b][lo >> 6] : 0u);
      const unsigned Q = pQ[b][hi] - pQ[b][lo] + (split ? tQ[b][lo >> 6] : 0u);
      const unsigned n = (unsigned)(((i + r < rows - 1 ? i + r : rows - 1) - (i - r > 0 ? i - r : 0) + 1) * nc);
      const unsigned long long D = (unsigned long long)n * Q - (unsigned long long)S * S;
      const unsigned sd = bin_isqrt(D);
      const unsigned long long lhs = (unsigned long long)(v * n * n) << 15;                      // v n^2 < 2^32
      const unsigned long long rhs = (unsigned long long)(S * n) * (128u * (256u - k)) + (unsigned long long)(S * k) * sd;   // S n < 2^32
      out[pg.page_off + (long)i * pg.stride + cw] = lhs < rhs ? 0 : 255;
    }
    cs -= vl;
    cq -= vl * vl;
  }
}

// ---- entry point ---------------------------------------------------------------------------------------------------------------------------
extern "C" int crnn_binarize_pages(const void* arena, long arena_bytes, const crnn_page_item* pages, const crnn_page_item* pages_dev, int P,
                                   const crnn_binarize_params* prm, void* out_arena, long out_bytes, hipStream_t stream) {
  if (P < 0 || !prm || prm->radius < 1 || prm->radius > BIN_MAX_RADIUS || prm->k256 < 0 || prm->k256 > 255 || prm->polarity < 1 || prm->polarity > 2)
    return CRNN_ERR_ARG;
  if (P == 0) return CRNN_OK;
  if (!arena || arena_bytes < 1 || !pages || !pages_dev || !out_arena || out_bytes < 1) return CRNN_ERR_ARG;
  if (page_ranges_overlap(arena, arena_bytes, out_arena, out_bytes)) return CRNN_ERR_ARG;
  int max_rows = 0, max_cols = 0;
  CRNN_TRY(page_check_table(pages, P, CRNN_ERR_ARG, arena_bytes, out_bytes, [&](const crnn_page_item& g) {   // (pages.h; a page above the limit is CRNN_ERR_ARG here)
    if (g.rows > max_rows) max_rows = g.rows;
    if (g.cols > max_cols) max_cols = g.cols;
  }));
  if (P > 65535) return CRNN_ERR_UNSUPPORTED;                   // the page is the grid's z
  hipLaunchKernelGGL(bin_sauvola_kernel, dim3(cdiv(max_cols, BIN_STRIP_C), cdiv(max_rows, BIN_BAND_R), P), dim3(BIN_THREADS), 0, stream,
                     (const unsigned char*)arena, arena_bytes, pages_dev, prm->radius, prm->k256, prm->polarity, (unsigned char*)out_arena, out_bytes);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
