// The page arena, stated once for ingest.hip, detect.hip, binarize.hip, deskew.hip and otsu.h (in Python: crnn_mi355x/pages.py).  An arena is one
// range of uint8 bytes; a crnn_page_item (include/crnn_mi355x.h) places a page of rows x cols pixels in it at byte page_off with row stride `stride`.
// Here: the size limit, the clamped pixel read, the kernels' guard of a device entry, the host's checks of an entry and of a table, "ranges overlap".
#pragma once
#include "common.h"

#define PAGE_MAX_DIM 4096                   // rows and cols of a page the detector, the binarisation and the deskew take

__host__ __device__ __forceinline__ int page_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static inline size_t page_up16(size_t n) { return (n + 15) & ~(size_t)15; }

// the page's pixel, every read inside the arena whatever the table holds
__device__ __forceinline__ int page_pixel(const unsigned char* arena, long arena_bytes, long off, int stride, int r, int c) {
  long a = off + (long)r * stride + c;
  a = a < 0 ? 0 : (a > arena_bytes - 1 ? arena_bytes - 1 : a);
  return arena[a];
}

// The device entry must fit both arenas, as the host's copy of it did; a page whose entry does not is left alone.  Checked once per workgroup:
// after it, rows and columns are clamped into the page and no load or store needs a check of its own.  rows, cols: clamped to PAGE_MAX_DIM.
__device__ __forceinline__ bool page_outside(const crnn_page_item& pg, int rows, int cols, long arena_bytes, long out_bytes) {
  const long span = (long)(rows - 1) * pg.stride + cols;
  return pg.page_off < 0 || pg.stride < cols || pg.page_off > arena_bytes - span || pg.page_off > out_bytes - span;
}

// Host: one entry -> 0 or the code of its first fault, in this order: the basic shape (CRNN_ERR_ARG), the size limit (`over`), the fit into the input
// arena and into the output arena (CRNN_ERR_ARG).  `over` is the caller's code for a page above PAGE_MAX_DIM, and the difference is the
// documented ABI (include/crnn_mi355x.h), not an accident: CRNN_ERR_UNSUPPORTED from crnn_detect_* and crnn_deskew_* / crnn_rotate_pages,
// CRNN_ERR_ARG from crnn_binarize_pages, 0 for no limit (crnn_ingest_crops).  arena_bytes / out_bytes < 0: there is no such arena to fit.
static inline int page_check(long page_off, int rows, int cols, int stride, int over, long arena_bytes, long out_bytes) {
  if (rows < 1 || cols < 1 || stride < cols || page_off < 0) return CRNN_ERR_ARG;
  if (over != 0 && (rows > PAGE_MAX_DIM || cols > PAGE_MAX_DIM)) return over;
  const long span = (long)(rows - 1) * stride + cols;
  if (arena_bytes >= 0 && (page_off > arena_bytes || span > arena_bytes - page_off)) return CRNN_ERR_ARG;
  if (out_bytes >= 0 && (page_off > out_bytes || span > out_bytes - page_off)) return CRNN_ERR_ARG;
  return 0;
}

// A table: the first faulty entry in index order decides; each(entry) takes a good entry into the caller's totals.  A limit on P itself
// (the page is a grid dimension) is the caller's, judged after the table.
template <class Each>
static inline int page_check_table(const crnn_page_item* pages, int P, int over, long arena_bytes, long out_bytes, Each&& each) {
  for (int i = 0; i < P; ++i) {
    CRNN_TRY(page_check(pages[i].page_off, pages[i].rows, pages[i].cols, pages[i].stride, over, arena_bytes, out_bytes));
    each(pages[i]);
  }
  return 0;
}

static inline bool page_ranges_overlap(const void* a, long a_bytes, const void* b, long b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}
