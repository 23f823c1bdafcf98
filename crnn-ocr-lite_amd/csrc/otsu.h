// What is ink on a page, shared by the word detector (detect.hip) and the skew estimate (deskew.hip): the page's 256-bin histogram and the
// threshold / polarity decision of the rule in include/crnn_mi355x.h (crnn_detect_words: THRESHOLD, POLARITY).  One definition, so that the
// two translation units cannot come to disagree about a page's ink.  The arena the pages lie in is pages.h's.
#pragma once
#include "pages.h"
#pragma clang fp contract(off)              // Otsu's score is four float64 operations in a fixed order

#define OTSU_THREADS 256                    // one thread per histogram bin
#define OTSU_HIST_CHUNK 65536               // pixels per workgroup of the histogram launch

static inline size_t otsu_hist_bytes(int P) { return (size_t)P * 256 * sizeof(int); }

// The histogram launch, grid (chunks of OTSU_HIST_CHUNK pixels, P), OTSU_THREADS threads: the chunk's histogram, privatised in LDS, non-empty
// bins added to hist[p] (integer atomics: any order gives the same sums).  static: each translation unit that includes this launches its own.
static __global__ __launch_bounds__(OTSU_THREADS) void otsu_hist_kernel(const unsigned char* __restrict__ arena, long arena_bytes,
                                                                        const crnn_page_item* __restrict__ pages, int* __restrict__ hist) {
  __shared__ int bins[256];
  const int p = blockIdx.y, tid = threadIdx.x;
  const crnn_page_item pg = pages[p];
  const int rows = page_clampi(pg.rows, 0, PAGE_MAX_DIM), cols = page_clampi(pg.cols, 0, PAGE_MAX_DIM);
  const long n = (long)rows * cols, lo = (long)blockIdx.x * OTSU_HIST_CHUNK;
  if (lo >= n) return;
  const long hi = lo + OTSU_HIST_CHUNK < n ? lo + OTSU_HIST_CHUNK : n;
  bins[tid] = 0;
  __syncthreads();
  for (long i = lo + tid; i < hi; i += OTSU_THREADS) {         // i grows by OTSU_THREADS up to hi
    const int r = (int)(i / cols), c = (int)(i - (long)r * cols);
    atomicAdd(&bins[page_pixel(arena, arena_bytes, pg.page_off, pg.stride, r, c)], 1);
  }
  __syncthreads();
  if (bins[tid]) atomicAdd(&hist[(long)p * 256 + tid], bins[tid]);
}

// The decision, by the OTSU_THREADS threads of one workgroup over the page's histogram h[256]: every thread calls it (it holds barriers);
// thread 0 receives t (-1: no ink) and ink_is_dark, the other threads receive nothing.
__device__ __forceinline__ void otsu_decide(const int* __restrict__ h256, int threshold, int polarity, int& t_out, int& dark_out) {
  __shared__ long long sw[2][256], ss[2][256];
  __shared__ double sc[256];
  __shared__ int st[256];
  const int tid = threadIdx.x;
  // inclusive prefix sums of h and v * h (Hillis-Steele, exact integers: any order gives the same sums)
  const long long h = h256[tid];
  sw[0][tid] = h;
  ss[0][tid] = h * tid;
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < 256; o <<= 1) {                           // o doubles up to 256
    sw[cur ^ 1][tid] = sw[cur][tid] + (tid >= o ? sw[cur][tid - o] : 0);
    ss[cur ^ 1][tid] = ss[cur][tid] + (tid >= o ? ss[cur][tid - o] : 0);
    cur ^= 1;
    __syncthreads();
  }
  const long long N = sw[cur][255], S = ss[cur][255];
  const long long w0 = sw[cur][tid], s0 = ss[cur][tid], w1 = N - w0;
  double score = -1.0;                                          // not admissible
  if (tid < 255 && w0 > 0 && w1 > 0) {
    const long long d = s0 * w1 - (S - s0) * w0;
    const double a = (double)d / (double)w0;
    const double b = (double)d / (double)w1;
    score = a * b;
  }
  sc[tid] = score;
  st[tid] = tid;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                           // o halves down to 0; the first t of the strictly greatest score
    if (tid < o) {
      const double s2 = sc[tid + o];
      const int t2 = st[tid + o];
      if (s2 > sc[tid] || (s2 == sc[tid] && t2 < st[tid])) { sc[tid] = s2; st[tid] = t2; }
    }
    __syncthreads();
  }
  if (tid != 0) return;
  int t = threshold;
  if (threshold < 0) t = sc[0] >= 0.0 ? st[0] : -1;
  t = page_clampi(t, -1, 254);
  int dark = polarity != 2;
  if (t >= 0 && polarity == 0) dark = sw[cur][t] <= N - sw[cur][t];
  t_out = t;
  dark_out = dark;
}
