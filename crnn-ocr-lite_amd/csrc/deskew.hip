// Page deskew on the device: the skew of uint8 pages (the arena pages.h defines) by sheared projection profiles, and the pages resampled
// by that angle into an arena of the same layout.  Integer-only (the rules: include/crnn_mi355x.h; the same rules in NumPy:
// crnn_mi355x/deskew.py) apart from Otsu's fixed-order float64 score, which is the detector's own code (otsu.h).
//
// The estimate: five launches behind one memset of the histograms and profiles, one workspace:
//   otsu_hist_kernel      the page's 256-bin histogram (otsu.h, the detector's launch).
//   dsk_threshold_kernel  one workgroup per page: the threshold and polarity (otsu.h, as det_threshold_kernel) and the page's sanitised geometry
//                         and the offset of its profiles in the workspace (DskPage) -- the later kernels read only that record.
//   dsk_profile_kernel    grid (groups of DSK_STRIPS 64-column strips, bands of DSK_BAND_R rows, pages).  The ink of a strip is one 64-bit ballot
//                         word per row in LDS (as det_tile_kernel builds them), DSK_PADW zero words either side.  Over the 64 DSK_STRIPS columns
//                         of the workgroup a candidate's off takes at most 16 DSK_STRIPS + 1 consecutive values, so the band's ink falls into at
//                         most DSK_BAND_R + 16 DSK_STRIPS = 256 bins: lane t owns bin R0 - max off + t.  Within a strip off takes at most 17
//                         values, each on a segment of consecutive columns; the segment's mask is a ballot (off == value), and the lane adds
//                         popcount(word[bin + off] & mask).  One integer atomicAdd per non-zero (workgroup, candidate, bin) into the page's
//                         [candidate][bin] int32 profile: DSK_STRIPS times fewer than one per (strip, candidate, bin), and none per pixel.
//   dsk_score_kernel      grid (candidates, pages): sum of squares of a profile in int64.
//   dsk_pick_kernel       one workgroup per page: the candidate of the greatest score; the smallest |a|, then the negative one, among equals.
// Integer adds commute, so nothing depends on arrival order: two calls agree bit for bit.  No workgroup waits for another inside a launch;
// everything one workgroup must see from another crosses a kernel boundary.
//
// The rotation: one gather launch, grid (64-column strips, bands of DSK_ROT_R rows, pages); a wavefront writes 64 consecutive bytes of a row
// and reads, for slopes up to 0.25, from at most 17 source rows.  No atomics.
#include "pages.h"
#pragma clang fp contract(off)
#include "otsu.h"                           // the histogram and the threshold decision, shared with detect.hip
#include <math.h>

#define DSK_THREADS 256
#define DSK_WAVES (DSK_THREADS / 64)
#define DSK_STRIPS CRNN_DESKEW_STRIPS
#define DSK_BAND_R CRNN_DESKEW_BAND_R
#define DSK_PADW (16 * DSK_STRIPS)          // the most that off can differ between two columns of a workgroup: 64 DSK_STRIPS - 1 columns at 0.25
#define DSK_WORDS (DSK_BAND_R + 2 * DSK_PADW)
#define DSK_ROT_R 16
#define DSK_MAX_STEPS 64
#define DSK_MAX_SLOPE_STEP 1024
#define DSK_MAX_SLOPE 16384                 // steps * slope_step: 0.25 in units of 2^-16
static_assert(DSK_THREADS == OTSU_THREADS, "otsu.h's workgroups are the estimate's");
static_assert(DSK_BAND_R + DSK_PADW == DSK_THREADS, "one bin of the band per lane");
static_assert((64 * DSK_STRIPS - 1) * DSK_MAX_SLOPE / 65536 + 1 <= DSK_PADW, "off differs by at most DSK_PADW inside a workgroup");

struct DskPage {
  long off;                                 // byte offset of the page in the arena
  long prof;                                // offset of the page's profiles in their workspace section, in words
  int rows, cols, stride, pad;              // rows = 0: the page is skipped; pad: bin b sits at word b + pad of a profile
  int nbins, t, dark, pad0;                 // t = -1: no ink
  long pad1, pad2;
};
static_assert(sizeof(DskPage) == 64, "DskPage is one 64-byte record");
struct DskTable { int c[2 * DSK_MAX_STEPS + 1], s[2 * DSK_MAX_STEPS + 1]; };   // 65536 (cos, sin) of candidate a at a + steps

// |off| <= (cols / 2 + 1) * 0.25 + 1: the bins of a page are -pad .. rows - 1 + pad
__host__ __device__ __forceinline__ int dsk_pad(int cols) { return ((((cols >> 1) + 1) * DSK_MAX_SLOPE) >> 16) + 2; }
// (c - half) * s: |c - half| < 4096 + 64 DSK_STRIPS, |s| <= 2^14: below 2^27
__device__ __forceinline__ int dsk_off(int c, int half, int s) { return ((c - half) * s + 32768) >> 16; }

__global__ __launch_bounds__(DSK_THREADS) void dsk_threshold_kernel(const crnn_page_item* __restrict__ pages, const int* __restrict__ hist,
                                                                    DskPage* __restrict__ meta, int threshold, int polarity, int ncand,
                                                                    long total_words) {
  const int p = blockIdx.x, tid = threadIdx.x;
  int t = -1, dark = 0;
  otsu_decide(hist + (long)p * 256, threshold, polarity, t, dark);   // (otsu.h: the answer is thread 0's)
  if (tid != 0) return;
  // this page's place in the workspace: the sums over the pages before it, from the same table the host validated
  long prof = 0;
  for (int q = 0; q < p; ++q) {                                 // q counts up to p
    const int r = page_clampi(pages[q].rows, 0, PAGE_MAX_DIM), c = page_clampi(pages[q].cols, 0, PAGE_MAX_DIM);
    prof += (long)ncand * (r + 2 * dsk_pad(c));
  }
  const crnn_page_item pg = pages[p];
  int rows = page_clampi(pg.rows, 0, PAGE_MAX_DIM);
  const int cols = page_clampi(pg.cols, 0, PAGE_MAX_DIM);
  const int nbins = rows + 2 * dsk_pad(cols);
  if (cols == 0 || prof + (long)ncand * nbins > total_words) rows = 0;
  DskPage m;
  m.off = pg.page_off; m.prof = prof;
  m.rows = rows; m.cols = cols; m.stride = pg.stride; m.pad = dsk_pad(cols);
  m.nbins = nbins; m.t = t; m.dark = dark; m.pad0 = 0; m.pad1 = 0; m.pad2 = 0;
  meta[p] = m;
}

__global__ __launch_bounds__(DSK_THREADS) void dsk_profile_kernel(const unsigned char* __restrict__ arena, long arena_bytes,
                                                                  const DskPage* __restrict__ meta, int steps, int slope_step,
                                                                  int* __restrict__ prof) {
  __shared__ unsigned long long W[DSK_STRIPS][DSK_WORDS];       // word DSK_PADW + lr of strip k: the ink of row R0 + lr; zero words around
  const DskPage m = meta[blockIdx.z];
  const int rows = m.rows, cols = m.cols;
  const int C0 = (int)blockIdx.x * 64 * DSK_STRIPS, R0 = (int)blockIdx.y * DSK_BAND_R;
  if (rows < 1 || m.t < 0 || C0 >= cols || R0 >= rows) return;  // (uniform over the workgroup) no ink: the profiles stay 0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  steps = page_clampi(steps, 0, DSK_MAX_STEPS);
  slope_step = page_clampi(slope_step, 1, DSK_MAX_SLOPE / (steps > 0 ? steps : 1));
  for (int i = tid; i < DSK_STRIPS * DSK_WORDS; i += DSK_THREADS) (&W[0][0])[i] = 0;   // i grows by DSK_THREADS
  __syncthreads();
  // 1. ink words: one (row, strip) per wavefront pass, the four wavefronts on 256 consecutive bytes of a row
  for (int q = wave; q < DSK_BAND_R * DSK_STRIPS; q += DSK_WAVES) {   // q grows by DSK_WAVES
    const int lr = q / DSK_STRIPS, k = q % DSK_STRIPS;
    const int r = R0 + lr, c = C0 + 64 * k + lane;
    bool ink = false;
    if (r < rows && c < cols) ink = ((page_pixel(arena, arena_bytes, m.off, m.stride, r, c) <= m.t) ? 1 : 0) == m.dark;
    const unsigned long long M = __ballot(ink);
    if (lane == 0) W[k][DSK_PADW + lr] = M;
  }
  __syncthreads();
  // 2. every candidate: lane tid owns bin R0 - omax + tid, omax the greatest off of the workgroup's columns (off is monotonic in the column)
  const int half = cols >> 1;
  int* mine = prof + m.prof;
  for (int a = -steps; a <= steps; ++a) {                       // a counts up to steps
    const int s = a * slope_step;
    const int w0 = dsk_off(C0, half, s), w1 = dsk_off(C0 + 64 * DSK_STRIPS - 1, half, s);
    const int omax = w0 > w1 ? w0 : w1;                         // omax - (the least off of the workgroup) <= DSK_PADW
    int acc = 0;
#pragma unroll
    for (int k = 0; k < DSK_STRIPS; ++k) {
      const int ca = C0 + 64 * k;
      const int k0 = dsk_off(ca, half, s), k1 = dsk_off(ca + 63, half, s);
      const int kmin = k0 < k1 ? k0 : k1, span = k0 < k1 ? k1 - k0 : k0 - k1;   // span <= 16
      const int my = dsk_off(ca + lane, half, s);
      // the row of bin b at off o is b + o: word DSK_PADW + tid - (omax - o), in 0 .. DSK_WORDS - 1 because 0 <= omax - o <= DSK_PADW
      const unsigned long long* w = &W[k][DSK_PADW + tid - (omax - kmin)];
      for (int o = 0; o <= span; ++o) {                         // o counts up to span (uniform: every lane is in the ballot)
        const unsigned long long seg = __ballot(my == kmin + o);
        acc += __popcll(w[o] & seg);
      }
    }
    const int bin = R0 - omax + tid + m.pad;
    if (acc != 0 && bin >= 0 && bin < m.nbins) atomicAdd(&mine[(long)(a + steps) * m.nbins + bin], acc);
  }
}

__global__ __launch_bounds__(DSK_THREADS) void dsk_score_kernel(const DskPage* __restrict__ meta, const int* __restrict__ prof, int ncand,
                                                                long long* __restrict__ scores) {
  __shared__ long long red[DSK_THREADS];
  const DskPage m = meta[blockIdx.y];
  const int a = blockIdx.x, tid = threadIdx.x;
  long long sum = 0;
  if (m.rows > 0 && m.t >= 0) {
    const int* mine = prof + m.prof + (long)a * m.nbins;
    for (int i = tid; i < m.nbins; i += DSK_THREADS) {          // i grows by DSK_THREADS
      const long long v = mine[i];
      sum += v * v;
    }
  }
  red[tid] = sum;
  __syncthreads();
  for (int o = DSK_THREADS / 2; o > 0; o >>= 1) {               // o halves down to 0 (exact integers: any order gives the same sum)
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) scores[(long)blockIdx.y * ncand + a] = red[0];
}

__global__ __launch_bounds__(DSK_THREADS) void dsk_pick_kernel(const long long* __restrict__ scores, int steps, int* __restrict__ index) {
  __shared__ long long sc[2 * DSK_MAX_STEPS + 1];
  steps = page_clampi(steps, 0, DSK_MAX_STEPS);
  const int ncand = 2 * steps + 1, tid = threadIdx.x;
  if (tid < ncand) sc[tid] = scores[(long)blockIdx.x * ncand + tid];
  __syncthreads();
  if (tid != 0) return;
  int best = 0;
  for (int d = 1; d <= steps; ++d) {                            // 0, -1, 1, -2, 2, ...: the first of the greatest score wins
    if (sc[steps - d] > sc[steps + best]) best = -d;
    if (sc[steps + d] > sc[steps + best]) best = d;
  }
  index[blockIdx.x] = best;
}

// The coordinates fit int32 with room: |dc|, |dr| <= 4095, C <= 2^16 and |S| <= 15895 (0.25 / sqrt(1.0625) * 2^16), so |C d| < 2^28,
// |S d| < 2^26, (n - 1) << 16 < 2^28 and |X|, |Y| < 2^28 + 2^26 + 2^28 < 2^30.  The weighted sum is at most 2^16 * 255 + 2^15 < 2^24.
__global__ __launch_bounds__(DSK_THREADS) void dsk_rotate_kernel(const unsigned char* __restrict__ arena, long arena_bytes,
                                                                 const crnn_page_item* __restrict__ pages, const int* __restrict__ index,
                                                                 DskTable tab, int steps, int fill, unsigned char* __restrict__ out,
                                                                 long out_bytes) {
  const crnn_page_item pg = pages[blockIdx.z];
  const int rows = page_clampi(pg.rows, 0, PAGE_MAX_DIM), cols = page_clampi(pg.cols, 0, PAGE_MAX_DIM);
  const int C0 = (int)blockIdx.x * 64, R0 = (int)blockIdx.y * DSK_ROT_R;
  if (C0 >= cols || R0 >= rows) return;                         // (uniform over the workgroup)
  if (page_outside(pg, rows, cols, arena_bytes, out_bytes)) return;   // (uniform; pages.h: no load or store below needs a check of its own)
  steps = page_clampi(steps, 0, DSK_MAX_STEPS);
  int a = __builtin_amdgcn_readfirstlane(index[blockIdx.z]);   // (uniform: one page per workgroup)
  if (a < -steps || a > steps) a = 0;
  const int C = tab.c[a + steps], S = tab.s[a + steps];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = C0 + lane;
  if (c >= cols) return;
  const unsigned char* src = arena + pg.page_off;
  const int dc = 2 * c - (cols - 1);
  for (int r = R0 + wave; r < R0 + DSK_ROT_R && r < rows; r += DSK_WAVES) {   // r grows by DSK_WAVES
    const int dr = 2 * r - (rows - 1);
    const int X = C * dc - S * dr + ((cols - 1) << 16), Y = S * dc + C * dr + ((rows - 1) << 16);
    const int c0 = X >> 17, r0 = Y >> 17, fx = (X >> 9) & 255, fy = (Y >> 9) & 255;
    const int ra = page_clampi(r0, 0, rows - 1), rb = page_clampi(r0 + 1, 0, rows - 1);
    const int ca = page_clampi(c0, 0, cols - 1), cb = page_clampi(c0 + 1, 0, cols - 1);
    int p00 = src[(long)ra * pg.stride + ca], p01 = src[(long)ra * pg.stride + cb];
    int p10 = src[(long)rb * pg.stride + ca], p11 = src[(long)rb * pg.stride + cb];
    if (fill >= 0) {                                            // a sample outside the page is `fill`, not the clamped pixel
      const bool ia = ra == r0, ib = rb == r0 + 1, ja = ca == c0, jb = cb == c0 + 1;
      if (!(ia && ja)) p00 = fill;
      if (!(ia && jb)) p01 = fill;
      if (!(ib && ja)) p10 = fill;
      if (!(ib && jb)) p11 = fill;
    }
    const int v = ((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p01 + (256 - fx) * fy * p10 + fx * fy * p11 + 32768) >> 16;
    out[pg.page_off + (long)r * pg.stride + c] = (unsigned char)v;
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------------
struct DskTotals { long words; int max_rows, max_cols, max_pix; };

static bool dsk_params_ok(const crnn_deskew_params* p) {
  return p->threshold >= -1 && p->threshold <= 254 && p->polarity >= 0 && p->polarity <= 2 && p->steps >= 0 && p->steps <= DSK_MAX_STEPS &&
         p->slope_step >= 1 && p->slope_step <= DSK_MAX_SLOPE_STEP && p->steps * p->slope_step <= DSK_MAX_SLOPE && p->fill >= -1 && p->fill <= 255;
}

// the host table's checks (pages.h; arena_bytes / out_bytes < 0: no such arena to fit) and the launches' totals: 0, or CRNN_ERR_ARG / CRNN_ERR_UNSUPPORTED
static int dsk_totals(const crnn_page_item* pages, int P, int ncand, long arena_bytes, long out_bytes, DskTotals& t) {
  t = DskTotals{0, 0, 0, 0};
  return page_check_table(pages, P, CRNN_ERR_UNSUPPORTED, arena_bytes, out_bytes, [&t, ncand](const crnn_page_item& g) {
    t.words += (long)ncand * (g.rows + 2 * dsk_pad(g.cols));
    if (g.rows > t.max_rows) t.max_rows = g.rows;
    if (g.cols > t.max_cols) t.max_cols = g.cols;
    if (g.rows * g.cols > t.max_pix) t.max_pix = g.rows * g.cols;
  });
}

static inline size_t dsk_meta_bytes(int P) { return (size_t)P * sizeof(DskPage); }

extern "C" size_t crnn_deskew_workspace_bytes(const crnn_page_item* pages, int P, const crnn_deskew_params* prm) {
  DskTotals t;
  if (!pages || !prm || P < 1 || P > 65535 || !dsk_params_ok(prm) || dsk_totals(pages, P, 2 * prm->steps + 1, -1, -1, t) != 0) return 0;
  return otsu_hist_bytes(P) + page_up16((size_t)t.words * sizeof(int)) + dsk_meta_bytes(P);
}

extern "C" int crnn_deskew_estimate(const void* arena, long arena_bytes, const crnn_page_item* pages, const crnn_page_item* pages_dev, int P,
                                    const crnn_deskew_params* prm, int* index, long long* scores, void* ws, size_t ws_bytes,
                                    hipStream_t stream) {
  if (P < 0 || !prm || !dsk_params_ok(prm)) return CRNN_ERR_ARG;
  if (P == 0) return CRNN_OK;
  if (!arena || arena_bytes < 1 || !pages || !pages_dev || !index || !scores || !ws) return CRNN_ERR_ARG;
  const int ncand = 2 * prm->steps + 1;
  DskTotals t;
  CRNN_TRY(dsk_totals(pages, P, ncand, arena_bytes, -1, t));
  if (P > 65535) return CRNN_ERR_UNSUPPORTED;                   // the page is the grid's y or z
  if (ws_bytes < crnn_deskew_workspace_bytes(pages, P, prm) || ((uintptr_t)ws & 15)) return CRNN_ERR_ARG;
  unsigned char* w = (unsigned char*)ws;
  int* hist = (int*)w;                      w += otsu_hist_bytes(P);
  int* prof = (int*)w;                      w += page_up16((size_t)t.words * sizeof(int));
  DskPage* meta = (DskPage*)w;
  const unsigned char* a = (const unsigned char*)arena;
  const hipError_t e = hipMemsetAsync(hist, 0, otsu_hist_bytes(P) + page_up16((size_t)t.words * sizeof(int)), stream);   // histograms and profiles
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(otsu_hist_kernel, dim3(cdiv(t.max_pix, OTSU_HIST_CHUNK), P), dim3(DSK_THREADS), 0, stream, a, arena_bytes, pages_dev, hist);
  CRNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsk_threshold_kernel, dim3(P), dim3(DSK_THREADS), 0, stream, pages_dev, (const int*)hist, meta, prm->threshold,
                     prm->polarity, ncand, t.words);
  CRNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsk_profile_kernel, dim3(cdiv(t.max_cols, 64 * DSK_STRIPS), cdiv(t.max_rows, DSK_BAND_R), P), dim3(DSK_THREADS), 0, stream,
                     a, arena_bytes, (const DskPage*)meta, prm->steps, prm->slope_step, prof);
  CRNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsk_score_kernel, dim3(ncand, P), dim3(DSK_THREADS), 0, stream, (const DskPage*)meta, (const int*)prof, ncand, scores);
  CRNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsk_pick_kernel, dim3(P), dim3(DSK_THREADS), 0, stream, (const long long*)scores, prm->steps, index);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

extern "C" int crnn_rotate_pages(const void* arena, long arena_bytes, const crnn_page_item* pages, const crnn_page_item* pages_dev, int P,
                                 const int* index_dev, const crnn_deskew_params* prm, void* out_arena, long out_bytes, hipStream_t stream) {
  if (P < 0 || !prm || !dsk_params_ok(prm)) return CRNN_ERR_ARG;
  if (P == 0) return CRNN_OK;
  if (!arena || arena_bytes < 1 || !pages || !pages_dev || !index_dev || !out_arena || out_bytes < 1) return CRNN_ERR_ARG;
  if (page_ranges_overlap(arena, arena_bytes, out_arena, out_bytes)) return CRNN_ERR_ARG;
  DskTotals t;
  CRNN_TRY(dsk_totals(pages, P, 0, arena_bytes, out_bytes, t));
  if (P > 65535) return CRNN_ERR_UNSUPPORTED;                   // the page is the grid's z
  // 65536 (cos, sin) of every candidate's angle, in IEEE double: sqrt and / are correctly rounded, rint rounds to nearest (ties to even)
  DskTable tab;
  for (int a = -prm->steps; a <= prm->steps; ++a) {
    const int s = a * prm->slope_step;
    const double tt = (double)s / 65536.0;
    const double root = sqrt(1.0 + tt * tt);
    tab.c[a + prm->steps] = (int)rint(65536.0 / root);
    tab.s[a + prm->steps] = (int)rint((double)s / root);
  }
  for (int i = 2 * prm->steps + 1; i < 2 * DSK_MAX_STEPS + 1; ++i) { tab.c[i] = 65536; tab.s[i] = 0; }
  hipLaunchKernelGGL(dsk_rotate_kernel, dim3(cdiv(t.max_cols, 64), cdiv(t.max_rows, DSK_ROT_R), P), dim3(DSK_THREADS), 0, stream,
                     (const unsigned char*)arena, arena_bytes, pages_dev, index_dev, tab, prm->steps, prm->fill, (unsigned char*)out_arena,
                     out_bytes);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
