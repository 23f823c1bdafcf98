// Word detection: page images (uint8, the arena pages.h defines) -> word boxes, on the device.  Classical, deterministic, integer-only
// except for Otsu's fixed-order float64 score: a global threshold, run-length smearing so that the letters of a word touch, 8-connected
// component labelling, box extraction with a size filter (the rule: include/crnn_mi355x.h; the same rule in NumPy: crnn_mi355x/detect.py).
//
// Seven launches behind one memset of the histograms, one workspace:
//   otsu_hist_kernel      grid (chunks of 64 Ki pixels, P): the page's 256-bin histogram, privatised in LDS, non-empty bins added to hist[p].
//   det_threshold_kernel  one workgroup per page: Otsu (or the given threshold), the polarity, and the page's sanitised geometry and offsets into
//                         the workspace (DetPage) -- the later kernels read only that record, never the caller's table.
//   det_tile_kernel       one workgroup per DET_TILE_R x DET_TILE_C tile.  A wavefront's ballot over 64 pixels is one 64-bit row word (score.hip);
//                         three of them (the tile's columns and 64 either side: gap_x <= 64) give the horizontal smear of a row by two
//                         count-leading/trailing-zero distances per pixel; gap_y halo rows above and below get the same horizontal smear, then the
//                         vertical smear looks up and down the LDS row words.  Labelling in LDS: a pixel starts at the first pixel of its row run,
//                         runs are united with the row above (atomicMin union-find on LDS words).  The tile writes per pixel the page index of its
//                         tile-local root (the component's minimum index inside the tile; -1 for background) and per tile-local component one
//                         record (extent, ink count, root) at the root's slot: slot (r / 2, c / 2) of the page is unique per root, because two
//                         roots in one 2 x 2 block would be 8-adjacent.  Extents and ink are reduced in LDS per row run, not per pixel.
//   det_border_kernel     one thread per pixel on a tile's first row / first column: unites it with its set neighbours in the adjacent tile(s).
//                         The only launch where workgroups touch each other's words: atomicMin on label words, every read of a label word a
//                         relaxed agent-scope atomic load (the XCDs' L2s are not coherent for plain loads).
//   det_merge_kernel      one thread per slot: a tile-local record whose root is not a global root sends its five values to the global root's
//                         record: integer min / max / add, one set per (tile, component).  Labels are read-only here (plain loads).
//   det_count_kernel      one workgroup per slot row: how many global roots in each of its two pixel rows pass the filter (plain stores).
//   det_emit_kernel       one workgroup per slot row: its rank = the sum of the counts of the rows before it; the passing roots of its two pixel
//                         rows go out in column order by a ballot prefix count (lexicon_nearest.hip's compaction) while rank < cap.  The
//                         workgroup of slot row 0 also writes info and the -1 tail.
// Roots are minimum row-major indices, so nothing depends on arrival order: two calls agree bit for bit.  No workgroup waits for another inside a
// launch; everything one workgroup must see from another crosses a kernel boundary.
#include "pages.h"
#pragma clang fp contract(off)
#include "otsu.h"                           // the histogram and the threshold decision, shared with deskew.hip

#define DET_THREADS 256
#define DET_WAVES (DET_THREADS / 64)
#define DET_TILE_R CRNN_DETECT_TILE_R
#define DET_TILE_C CRNN_DETECT_TILE_C       // 64: one ballot word
static_assert(DET_TILE_C == 64 && DET_TILE_R % 2 == 0 && DET_TILE_R % (DET_THREADS / 64) == 0, "the tile is 64 columns wide: one ballot word per row");
#define DET_MAX_GAP_X 64                    // <= DET_TILE_C: one halo word either side
#define DET_MAX_GAP_Y 16
static_assert(DET_THREADS == OTSU_THREADS, "otsu.h's workgroups are the detector's");
#define DET_REC 6                           // r0 r1 c0 c1 ink root
#define DET_TILE_SLOTS ((DET_TILE_R / 2) * (DET_TILE_C / 2))
#define DET_INT_MAX 0x7fffffff

struct DetPage {
  long off;                                 // byte offset of the page in the arena
  long pix, slot, row;                      // offsets of the page's labels, records and row counts in their workspace sections
  int rows, cols, stride, scols;            // rows = 0: the page is skipped (the device table disagrees with the validated one)
  int t, dark, pad0, pad1;                  // t = -1: no ink
};
static_assert(sizeof(DetPage) == 64, "DetPage is one 64-byte record");

__device__ __forceinline__ int det_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int det_lds_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__global__ __launch_bounds__(DET_THREADS) void det_threshold_kernel(const crnn_page_item* __restrict__ pages, const int* __restrict__ hist,
                                                                    DetPage* __restrict__ meta, int threshold, int polarity, long total_pix,
                                                                    long total_slots, long total_rows) {
  const int p = blockIdx.x, tid = threadIdx.x;
  int t = -1, dark = 0;
  otsu_decide(hist + (long)p * 256, threshold, polarity, t, dark);   // (otsu.h: the answer is thread 0's)
  if (tid != 0) return;
  // this page's place in the workspace: the sums over the pages before it, from the same table the host validated
  long pix = 0, slot = 0, row = 0;
  for (int q = 0; q < p; ++q) {                                 // q counts up to p
    const int r = page_clampi(pages[q].rows, 0, PAGE_MAX_DIM), c = page_clampi(pages[q].cols, 0, PAGE_MAX_DIM);
    pix += (long)r * c;
    slot += (long)((r + 1) >> 1) * ((c + 1) >> 1);
    row += 2 * ((r + 1) >> 1);
  }
  const crnn_page_item pg = pages[p];
  int rows = page_clampi(pg.rows, 0, PAGE_MAX_DIM), cols = page_clampi(pg.cols, 0, PAGE_MAX_DIM);
  const long srows = (rows + 1) >> 1, scols = (cols + 1) >> 1;
  if (cols == 0 || pix + (long)rows * cols > total_pix || slot + srows * scols > total_slots || row + 2 * srows > total_rows) rows = 0;
  DetPage m;
  m.off = pg.page_off; m.pix = pix; m.slot = slot; m.row = row;
  m.rows = rows; m.cols = cols; m.stride = pg.stride; m.scols = (int)scols;
  m.t = t; m.dark = dark; m.pad0 = 0; m.pad1 = 0;
  meta[p] = m;
}

// LDS union-find of the tile: a label is the local index of an earlier pixel of the same component, or the pixel's own index at a root
__device__ __forceinline__ int det_lds_find(const int* lab, int x) {
  for (;;) {                                                    // a label is strictly below the index it sits at, except at a root
    const int q = det_lds_ld(lab + x);
    if ((unsigned)q >= (unsigned)x) return x;
    x = q;
  }
}
__device__ __forceinline__ void det_lds_union(int* lab, int a, int b) {
  for (;;) {                                                    // every pass returns or goes on from a strictly smaller label of b's chain
    a = det_lds_find(lab, a);
    b = det_lds_find(lab, b);
    if (a == b) return;
    if (a > b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(&lab[b], a);
    if (old == b) return;
    b = old;
  }
}

__global__ __launch_bounds__(DET_THREADS) void det_tile_kernel(const unsigned char* __restrict__ arena, long arena_bytes,
                                                               const DetPage* __restrict__ meta, int gap_x, int gap_y, int* __restrict__ labels,
                                                               int* __restrict__ recs) {
  __shared__ unsigned long long Hw[DET_TILE_R + 2 * DET_MAX_GAP_Y];   // horizontally smeared rows, halo rows included
  __shared__ unsigned long long Ow[DET_TILE_R], Vw[DET_TILE_R];       // original ink and the smeared mask of the tile's rows
  __shared__ int lab[DET_TILE_R * DET_TILE_C];
  __shared__ int rec[DET_TILE_SLOTS * DET_REC];
  const DetPage m = meta[blockIdx.y];
  const int rows = m.rows, cols = m.cols;
  const int tiles_c = (cols + DET_TILE_C - 1) / DET_TILE_C;
  const int tiles = ((rows + DET_TILE_R - 1) / DET_TILE_R) * tiles_c;
  if ((int)blockIdx.x >= tiles) return;
  const int R0 = ((int)blockIdx.x / tiles_c) * DET_TILE_R, C0 = ((int)blockIdx.x % tiles_c) * DET_TILE_C;
  const int tid = threadIdx.x, b = tid & 63, wave = tid >> 6;
  gap_x = page_clampi(gap_x, 0, DET_MAX_GAP_X);
  gap_y = page_clampi(gap_y, 0, DET_MAX_GAP_Y);
  const unsigned long long below = (1ull << b) - 1;             // the bits of the columns left of this lane's

  for (int i = tid; i < DET_TILE_SLOTS; i += DET_THREADS) {     // i grows by DET_THREADS
    int* r = rec + i * DET_REC;
    r[0] = DET_INT_MAX; r[1] = 0; r[2] = DET_INT_MAX; r[3] = 0; r[4] = 0; r[5] = -1;
  }
  // 1. ink words and the horizontal smear, one row per wavefront pass
  for (int hr = wave; hr < DET_TILE_R + 2 * gap_y; hr += DET_WAVES) {   // hr grows by DET_WAVES
    const int r = R0 - gap_y + hr;
    const bool row_in = r >= 0 && r < rows && m.t >= 0;         // (wave-uniform)
    bool ink0 = false, ink1 = false, ink2 = false;
    if (row_in) {
      const int c = C0 + b;
      if (c < cols) ink1 = ((page_pixel(arena, arena_bytes, m.off, m.stride, r, c) <= m.t) ? 1 : 0) == m.dark;
      if (gap_x > 0) {                                          // the halo words either side
        if (c - 64 >= 0) ink0 = ((page_pixel(arena, arena_bytes, m.off, m.stride, r, c - 64) <= m.t) ? 1 : 0) == m.dark;
        if (c + 64 < cols) ink2 = ((page_pixel(arena, arena_bytes, m.off, m.stride, r, c + 64) <= m.t) ? 1 : 0) == m.dark;
      }
    }
    const unsigned long long M0 = __ballot(ink0), M1 = __ballot(ink1), M2 = __ballot(ink2);
    bool fill = false;
    if (!ink1 && gap_x > 0) {
      // distances to the nearest ink left and right in this row (0 = none within 64 columns); the run between them is dl + dr - 1 long
      const unsigned long long lowm = M1 & below, him = b == 63 ? 0ull : (M1 >> (b + 1));
      int dl = 0, dr = 0;
      if (lowm) dl = b - (63 - __clzll(lowm));
      else if (M0) dl = b + 1 + __clzll(M0);
      if (him) dr = __ffsll((long long)him);
      else if (M2) dr = 63 - b + __ffsll((long long)M2);
      fill = dl > 0 && dr > 0 && dl + dr - 1 <= gap_x;
    }
    const unsigned long long H = __ballot(ink1 || fill);
    if (b == 0) {
      Hw[hr] = H;
      if (hr >= gap_y && hr < gap_y + DET_TILE_R) Ow[hr - gap_y] = M1;
    }
  }
  __syncthreads();
  // 2. the vertical smear of the tile's rows over the horizontally smeared ones
  for (int lr = wave; lr < DET_TILE_R; lr += DET_WAVES) {       // lr grows by DET_WAVES
    const int hr = lr + gap_y;
    const bool set = (Hw[hr] >> b) & 1;
    bool fill = false;
    if (!set && gap_y > 0) {
      int du = 0, dd = 0;
      for (int k = 1; k <= gap_y && !du; ++k)                   // k counts up to gap_y
        if ((Hw[hr - k] >> b) & 1) du = k;
      for (int k = 1; k <= gap_y && !dd; ++k)                   // k counts up to gap_y
        if ((Hw[hr + k] >> b) & 1) dd = k;
      fill = du > 0 && dd > 0 && du + dd - 1 <= gap_y;
    }
    const unsigned long long V = __ballot(set || fill);
    if (b == 0) Vw[lr] = V;
  }
  __syncthreads();
  // 3. labels: every pixel starts at the first pixel of its row run
  for (int lr = wave; lr < DET_TILE_R; lr += DET_WAVES) {       // lr grows by DET_WAVES
    const unsigned long long V = Vw[lr];
    if ((V >> b) & 1) {
      const unsigned long long z = ~V & below;
      lab[lr * 64 + b] = lr * 64 + (z ? 64 - __clzll(z) : 0);
    }
  }
  __syncthreads();
  // runs are united with the row above: N when set (NW and NE then belong to N's run), else NW and NE; a union that the left or right
  // neighbour's already implies is left out
  for (int lr = wave + DET_WAVES * (wave == 0); lr < DET_TILE_R; lr += DET_WAVES) {   // lr grows by DET_WAVES (row 0 has no row above)
    const unsigned long long V = Vw[lr], U = Vw[lr - 1];
    if (!((V >> b) & 1)) continue;
    const int p = lr * 64 + b, q = p - 64;
    const bool w = b > 0 && ((V >> (b - 1)) & 1), e = b < 63 && ((V >> (b + 1)) & 1);
    const bool n = (U >> b) & 1, nw = b > 0 && ((U >> (b - 1)) & 1), ne = b < 63 && ((U >> (b + 1)) & 1);
    if (n) {
      if (!(w && nw)) det_lds_union(lab, p, q);
    } else {
      if (nw && !w) det_lds_union(lab, p, q - 1);
      if (ne && !e) det_lds_union(lab, p, q + 1);
    }
  }
  __syncthreads();
  // 4. provisional labels out; extents and ink per row run into the root's record
  for (int lr = wave; lr < DET_TILE_R; lr += DET_WAVES) {       // lr grows by DET_WAVES
    const int r = R0 + lr, c = C0 + b;
    if (r >= rows || c >= cols) continue;
    const unsigned long long V = Vw[lr];
    int out = -1;
    if ((V >> b) & 1) {
      const int p = lr * 64 + b;
      const int root = det_lds_find(lab, p);
      const int rr = root >> 6, rc = root & 63;
      out = (R0 + rr) * cols + C0 + rc;
      int* rs = rec + ((rr >> 1) * (DET_TILE_C / 2) + (rc >> 1)) * DET_REC;
      if (root == p) rs[5] = out;
      if (b == 0 || !((V >> (b - 1)) & 1)) {                    // the first pixel of a run speaks for the run
        const unsigned long long z = ~V >> b;                   // bit 0 is clear: this pixel is set
        const int len = z ? __ffsll((long long)z) - 1 : 64 - b;
        const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1)) << b;
        atomicMin(&rs[0], r); atomicMax(&rs[1], r + 1);
        atomicMin(&rs[2], c); atomicMax(&rs[3], c + len);
        atomicAdd(&rs[4], __popcll(Ow[lr] & run));
      }
    }
    labels[m.pix + (long)r * cols + c] = out;
  }
  __syncthreads();
  for (int i = tid; i < DET_TILE_SLOTS; i += DET_THREADS) {     // i grows by DET_THREADS
    const int sr = (R0 >> 1) + i / (DET_TILE_C / 2), scol = (C0 >> 1) + i % (DET_TILE_C / 2);
    if (sr >= ((rows + 1) >> 1) || scol >= m.scols) continue;
    int* g = recs + (m.slot + (long)sr * m.scols + scol) * DET_REC;
    const int* r = rec + i * DET_REC;
    for (int k = 0; k < DET_REC; ++k) g[k] = r[k];              // six words
  }
}

// global union-find over the page's label words (det_border_kernel only): every read of a word another workgroup may atomicMin is an atomic load
__device__ __forceinline__ int det_find(const int* L, int x) {
  for (;;) {                                                    // a label is strictly below the index it sits at, except at a root
    const int q = det_ld(L + x);
    if ((unsigned)q >= (unsigned)x) return x;
    x = q;
  }
}
__device__ __forceinline__ void det_union(int* L, int a, int b) {
  for (;;) {                                                    // every pass returns or goes on from a strictly smaller label of b's chain
    a = det_find(L, a);
    b = det_find(L, b);
    if (a == b) return;
    if (a > b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(&L[b], a);
    if (old == b) return;
    b = old;
  }
}

__global__ __launch_bounds__(DET_THREADS) void det_border_kernel(const DetPage* __restrict__ meta, int* __restrict__ labels) {
  const DetPage m = meta[blockIdx.y];
  const int rows = m.rows, cols = m.cols;
  if (rows < 1) return;
  const long nh = (long)((rows - 1) / DET_TILE_R) * cols, nv = (long)((cols - 1) / DET_TILE_C) * rows;
  const long i = (long)blockIdx.x * DET_THREADS + threadIdx.x;
  if (i >= nh + nv) return;
  int* L = labels + m.pix;
  int r, c, nr[3], nc[3];
  if (i < nh) {                                                 // first row of a tile row: the three pixels above
    r = (int)(i / cols + 1) * DET_TILE_R; c = (int)(i % cols);
    for (int k = 0; k < 3; ++k) { nr[k] = r - 1; nc[k] = c - 1 + k; }
  } else {                                                      // first column of a tile column: the three pixels to the left
    const long j = i - nh;
    c = (int)(j / rows + 1) * DET_TILE_C; r = (int)(j % rows);
    for (int k = 0; k < 3; ++k) { nr[k] = r - 1 + k; nc[k] = c - 1; }
  }
  const int me = r * cols + c;
  if (det_ld(L + me) < 0) return;
  for (int k = 0; k < 3; ++k) {                                 // three neighbours
    if (nr[k] < 0 || nr[k] >= rows || nc[k] < 0 || nc[k] >= cols) continue;
    const int other = nr[k] * cols + nc[k];
    if (det_ld(L + other) >= 0) det_union(L, other, me);
  }
}

__global__ __launch_bounds__(DET_THREADS) void det_merge_kernel(const DetPage* __restrict__ meta, const int* __restrict__ labels,
                                                                int* __restrict__ recs) {
  const DetPage m = meta[blockIdx.y];
  const long nslots = (long)((m.rows + 1) >> 1) * m.scols;
  const long i = (long)blockIdx.x * DET_THREADS + threadIdx.x;
  if (m.rows < 1 || i >= nslots) return;
  const int* mine = recs + (m.slot + i) * DET_REC;
  const int root = mine[5], npix = m.rows * m.cols;
  if (root < 0 || root >= npix) return;
  const int* L = labels + m.pix;
  int g = root;
  for (;;) {                                                    // a label is strictly below the index it sits at, except at a root
    const int q = L[g];
    if ((unsigned)q >= (unsigned)g) break;
    g = q;
  }
  if (g == root) return;                                        // a global root keeps its record in place; the others add to it
  const int gr = g / m.cols, gc = g - gr * m.cols;
  int* dst = recs + (m.slot + (long)(gr >> 1) * m.scols + (gc >> 1)) * DET_REC;
  atomicMin(&dst[0], mine[0]); atomicMax(&dst[1], mine[1]);
  atomicMin(&dst[2], mine[2]); atomicMax(&dst[3], mine[3]);
  atomicAdd(&dst[4], mine[4]);
}

// the record of slot i when it holds a global root that passes the filter: -> the parity of the root's pixel row, else -1
__device__ __forceinline__ int det_passes(const DetPage& m, const int* __restrict__ labels, const int* __restrict__ rec,
                                          const crnn_detect_params& prm) {
  const int root = rec[5];
  if (root < 0 || root >= m.rows * m.cols || labels[m.pix + root] != root) return -1;
  const int h = rec[1] - rec[0], w = rec[3] - rec[2], ink = rec[4];
  if (w < prm.min_w || h < prm.min_h || ink < prm.min_ink) return -1;
  if ((prm.max_w > 0 && w > prm.max_w) || (prm.max_h > 0 && h > prm.max_h)) return -1;
  return (root / m.cols) & 1;
}

__global__ __launch_bounds__(DET_THREADS) void det_count_kernel(const DetPage* __restrict__ meta, const int* __restrict__ labels,
                                                                const int* __restrict__ recs, int* __restrict__ rowcnt,
                                                                crnn_detect_params prm) {
  __shared__ int cnt[2];
  const DetPage m = meta[blockIdx.y];
  const int R = blockIdx.x, tid = threadIdx.x;
  if (R >= ((m.rows + 1) >> 1)) return;
  if (tid < 2) cnt[tid] = 0;
  __syncthreads();
  int mine[2] = {0, 0};
  for (int s = tid; s < m.scols; s += DET_THREADS) {            // s grows by DET_THREADS
    const int par = det_passes(m, labels, recs + (m.slot + (long)R * m.scols + s) * DET_REC, prm);
    if (par >= 0) ++mine[par];
  }
  if (mine[0]) atomicAdd(&cnt[0], mine[0]);
  if (mine[1]) atomicAdd(&cnt[1], mine[1]);
  __syncthreads();
  if (tid < 2) rowcnt[m.row + 2 * R + tid] = cnt[tid];
}

__global__ __launch_bounds__(DET_THREADS) void det_emit_kernel(const DetPage* __restrict__ meta, const int* __restrict__ labels,
                                                               const int* __restrict__ recs, const int* __restrict__ rowcnt,
                                                               crnn_detect_params prm, int* __restrict__ rects, int* __restrict__ info) {
  __shared__ int sums[2];
  __shared__ int wt[2][DET_WAVES];
  const DetPage m = meta[blockIdx.y];
  const int R = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int srows = (m.rows + 1) >> 1, cap = prm.cap;
  int* out = rects + (long)blockIdx.y * cap * 5;
  if (R >= srows && R > 0) return;
  if (tid < 2) sums[tid] = 0;
  __syncthreads();
  int before = 0, all = 0;
  for (int i = tid; i < 2 * srows; i += DET_THREADS) {          // i grows by DET_THREADS
    const int v = rowcnt[m.row + i];
    all += v;
    if (i < 2 * R) before += v;
  }
  if (before) atomicAdd(&sums[0], before);
  if (all) atomicAdd(&sums[1], all);
  __syncthreads();
  const int rank0 = sums[0], found = sums[1];
  if (R == 0) {                                                 // the page's summary and the unused rows
    const int kept = found < cap ? found : cap;
    if (tid == 0) {
      int* o = info + (long)blockIdx.y * 4;
      o[0] = found; o[1] = kept; o[2] = m.t; o[3] = m.dark;
    }
    for (long i = (long)kept * 5 + tid; i < (long)cap * 5; i += DET_THREADS) out[i] = -1;   // i grows by DET_THREADS
  }
  if (R >= srows || rank0 >= cap) return;
  int rank = rank0, it = 0;
  for (int par = 0; par < 2; ++par) {                           // the even pixel row's roots come before the odd one's
    for (int s0 = 0; s0 < m.scols && rank < cap; s0 += DET_THREADS, ++it) {   // s0 grows by DET_THREADS
      const int s = s0 + tid;
      const int* rec = recs + (m.slot + (long)R * m.scols + (s < m.scols ? s : 0)) * DET_REC;
      const bool hit = s < m.scols && det_passes(m, labels, rec, prm) == par;
      const unsigned long long mask = __ballot(hit);
      if (lane == 0) wt[it & 1][wave] = __popcll(mask);
      __syncthreads();
      int pre = 0, tot = 0;
      for (int q = 0; q < DET_WAVES; ++q) {                     // four waves
        const int t = wt[it & 1][q];
        if (q < wave) pre += t;
        tot += t;
      }
      const int pos = rank + pre + __popcll(mask & ((1ull << lane) - 1));
      if (hit && pos < cap) {
        int* o = out + (long)pos * 5;
        for (int k = 0; k < 5; ++k) o[k] = rec[k];              // r0 r1 c0 c1 ink
      }
      rank += tot;
    }
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------------
struct DetTotals { long pix, slots, rows; int max_pix, max_tiles, max_border, max_slots, max_srows; };

// the host table's checks (pages.h; arena_bytes < 0: no arena to fit) and the launch sequence's totals: 0, or CRNN_ERR_ARG / CRNN_ERR_UNSUPPORTED
static int det_totals(const crnn_page_item* pages, int P, long arena_bytes, DetTotals& t) {
  t = DetTotals{0, 0, 0, 0, 0, 0, 0, 0};
  CRNN_TRY(page_check_table(pages, P, CRNN_ERR_UNSUPPORTED, arena_bytes, -1, [&t](const crnn_page_item& g) {
    const int sr = (g.rows + 1) >> 1, sc = (g.cols + 1) >> 1;
    const int pix = g.rows * g.cols;
    t.pix += pix; t.slots += (long)sr * sc; t.rows += 2 * sr;
    const int tiles = cdiv(g.rows, DET_TILE_R) * cdiv(g.cols, DET_TILE_C);
    const int border = ((g.rows - 1) / DET_TILE_R) * g.cols + ((g.cols - 1) / DET_TILE_C) * g.rows;
    if (pix > t.max_pix) t.max_pix = pix;
    if (tiles > t.max_tiles) t.max_tiles = tiles;
    if (border > t.max_border) t.max_border = border;
    if (sr * sc > t.max_slots) t.max_slots = sr * sc;
    if (sr > t.max_srows) t.max_srows = sr;
  }));
  if (t.pix > (1L << 31)) return CRNN_ERR_UNSUPPORTED;
  return 0;
}

static bool det_params_ok(const crnn_detect_params* p) {
  return p->threshold >= -1 && p->threshold <= 254 && p->polarity >= 0 && p->polarity <= 2 && p->gap_x >= 0 && p->gap_x <= DET_MAX_GAP_X &&
         p->gap_y >= 0 && p->gap_y <= DET_MAX_GAP_Y && p->min_w >= 0 && p->min_h >= 0 && p->min_ink >= 0 && p->max_w >= 0 && p->max_h >= 0 &&
         p->cap >= 1;
}

static inline size_t det_meta_bytes(int P) { return (size_t)P * sizeof(DetPage); }

extern "C" size_t crnn_detect_workspace_bytes(const crnn_page_item* pages, int P, const crnn_detect_params* prm) {
  DetTotals t;
  if (!pages || !prm || P < 1 || P > 65535 || !det_params_ok(prm) || det_totals(pages, P, -1, t) != 0) return 0;
  return otsu_hist_bytes(P) + det_meta_bytes(P) + page_up16((size_t)t.pix * sizeof(int)) + page_up16((size_t)t.slots * DET_REC * sizeof(int)) +
         page_up16((size_t)t.rows * sizeof(int));
}

extern "C" int crnn_detect_words(const void* arena, long arena_bytes, const crnn_page_item* pages, const crnn_page_item* pages_dev, int P,
                                 const crnn_detect_params* prm, int* rects, int* info, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (P < 0 || !prm || !det_params_ok(prm)) return CRNN_ERR_ARG;
  if (P == 0) return CRNN_OK;
  if (!arena || arena_bytes < 1 || !pages || !pages_dev || !rects || !info || !ws) return CRNN_ERR_ARG;
  DetTotals t;
  CRNN_TRY(det_totals(pages, P, arena_bytes, t));
  if (P > 65535) return CRNN_ERR_UNSUPPORTED;                   // the page is the grid's y
  if (ws_bytes < crnn_detect_workspace_bytes(pages, P, prm) || ((uintptr_t)ws & 15)) return CRNN_ERR_ARG;
  unsigned char* w = (unsigned char*)ws;
  int* hist = (int*)w;                      w += otsu_hist_bytes(P);
  DetPage* meta = (DetPage*)w;              w += det_meta_bytes(P);
  int* labels = (int*)w;                    w += page_up16((size_t)t.pix * sizeof(int));
  int* recs = (int*)w;                      w += page_up16((size_t)t.slots * DET_REC * sizeof(int));
  int* rowcnt = (int*)w;
  const unsigned char* a = (const unsigned char*)arena;
  const hipError_t e = hipMemsetAsync(hist, 0, otsu_hist_bytes(P), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(otsu_hist_kernel, dim3(cdiv(t.max_pix, OTSU_HIST_CHUNK), P), dim3(DET_THREADS), 0, stream, a, arena_bytes, pages_dev, hist);
  CRNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(det_threshold_kernel, dim3(P), dim3(DET_THREADS), 0, stream, pages_dev, (const int*)hist, meta, prm->threshold, prm->polarity,
                     t.pix, t.slots, t.rows);
  CRNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(det_tile_kernel, dim3(t.max_tiles, P), dim3(DET_THREADS), 0, stream, a, arena_bytes, (const DetPage*)meta, prm->gap_x,
                     prm->gap_y, labels, recs);
  CRNN_LAUNCH_CHECK();
  if (t.max_border > 0) {
    hipLaunchKernelGGL(det_border_kernel, dim3(cdiv(t.max_border, DET_THREADS), P), dim3(DET_THREADS), 0, stream, (const DetPage*)meta, labels);
    CRNN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(det_merge_kernel, dim3(cdiv(t.max_slots, DET_THREADS), P), dim3(DET_THREADS), 0, stream, (const DetPage*)meta,
                     (const int*)labels, recs);
  CRNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(det_count_kernel, dim3(t.max_srows, P), dim3(DET_THREADS), 0, stream, (const DetPage*)meta, (const int*)labels,
                     (const int*)recs, rowcnt, *prm);
  CRNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(det_emit_kernel, dim3(t.max_srows, P), dim3(DET_THREADS), 0, stream, (const DetPage*)meta, (const int*)labels,
                     (const int*)recs, (const int*)rowcnt, *prm, rects, info);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
