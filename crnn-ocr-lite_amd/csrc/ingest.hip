// Word-crop ingest: page images (uint8, one arena: pages.h) + a box table -> the normalised (B, imgh, imgw, 1) fp32 batch the forward reads.
// One workgroup builds one output image; one launch per batch.
//
// Restates crnn_mi355x/data.py open_img (rotate, modal fill value, optional 1.5x up-scale rounded to uint8, modal-value padding, inversion
// of bright-background images, bilinear squash to (imgh, imgw)) followed by norm(), bit for bit: resize_linear's float64 arithmetic is kept
// operation by operation, so nothing here may be contracted into fused multiply-adds (the pragma below; hipcc contracts by default).  The
// random choices of the padding are NOT made here: the host draws them (ingest.plan_crop) and passes the content offset / padded size.
#include "pages.h"
#pragma clang fp contract(off)

#define INGEST_THREADS 256
#define INGEST_LDS_BUDGET (48 * 1024)   // up-scaled content staged in LDS: int(imgh/2 * 1.5) * int(imgw/2 * 1.5) bytes (75 x 24 at 100 x 32)

// np: pos = (i + 0.5) * scale - 0.5; lo = floor(pos); frac = pos - lo, zeroed where lo < 0 or lo >= n_in - 1; lo and lo + 1 clipped
__device__ __forceinline__ void ingest_taps(int i, double scale, int n_in, int& lo, int& hi, double& f) {
  const double pos = ((double)i + 0.5) * scale - 0.5;
  const double fl = floor(pos);
  const int l = (int)fmin(fmax(fl, -1.0), (double)n_in);   // every decision below only asks where l lies against 0 and n_in - 1
  f = pos - fl;
  if (l < 0 || l >= n_in - 1) f = 0.0;
  lo = l < 0 ? 0 : (l > n_in - 1 ? n_in - 1 : l);
  hi = l + 1 < 0 ? 0 : (l + 1 > n_in - 1 ? n_in - 1 : l + 1);
}

// np: top = a*(1-fx) + b*fx; bot = c*(1-fx) + d*fx; out = top*(1-fy) + bot*fy; clip(floor(out + 0.5), 0, 255)
__device__ __forceinline__ int ingest_blend(int a, int b, int c, int d, double fx, double fy) {
  const double gx = 1.0 - fx, gy = 1.0 - fy;
  const double top = (double)a * gx + (double)b * fx;
  const double bot = (double)c * gx + (double)d * fx;
  const double o = top * gy + bot * fy;
  const double r = floor(o + 0.5);
  return r < 0.0 ? 0 : (r > 255.0 ? 255 : (int)r);
}

struct IngestPage {
  const unsigned char* arena;
  long arena_bytes, off;
  int rows, cols, stride, r0, c0, hc;
  // the rotated crop rot(i, j) = page[r0 + hc - 1 - j, c0 + i]; every read stays inside the page and inside the arena whatever the table holds
  __device__ __forceinline__ int at(int r, int c) const {
    return page_pixel(arena, arena_bytes, off, stride, page_clampi(r, 0, rows - 1), page_clampi(c, 0, cols - 1));
  }
  __device__ __forceinline__ int rot(int i, int j) const { return at(r0 + hc - 1 - j, c0 + i); }
};

__global__ __launch_bounds__(INGEST_THREADS) void ingest_crops_kernel(const unsigned char* __restrict__ arena, long arena_bytes,
                                                                      const crnn_crop_item* __restrict__ items, int n, int T0, int T1, int up_cap,
                                                                      const float* __restrict__ table, float* __restrict__ out,
                                                                      unsigned char* __restrict__ out_u8) {
  extern __shared__ unsigned char up[];          // up_cap bytes: the up-scaled content, row-major (s0, s1)
  __shared__ unsigned hist[256];
  __shared__ unsigned long long best;
  __shared__ unsigned bright;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int npx = T0 * T1;
  float* o32 = out + (long)b * npx;
  unsigned char* o8 = out_u8 ? out_u8 + (long)b * npx : nullptr;
  if (b >= n) {                                  // rows past n: zeros
    for (int o = tid; o < npx; o += INGEST_THREADS) {
      o32[o] = 0.f;
      if (o8) o8[o] = 0;
    }
    return;
  }
  const crnn_crop_item it = items[b];
  IngestPage pg;
  pg.arena = arena; pg.arena_bytes = arena_bytes; pg.off = it.page_off;
  pg.rows = it.rows; pg.cols = it.cols; pg.stride = it.stride; pg.r0 = it.r0; pg.c0 = it.c0;
  const int hc = it.r1 - it.r0, wc = it.c1 - it.c0;   // the rotated crop is (wc, hc): axis 0 = time
  pg.hc = hc;

  hist[tid] = 0;
  if (tid == 0) { best = 0; bright = 0; }
  __syncthreads();
  for (int r = tid >> 6; r < hc; r += INGEST_THREADS / 64)
    for (int c = tid & 63; c < wc; c += 64) atomicAdd(&hist[pg.at(it.r0 + r, it.c0 + c)], 1u);
  __syncthreads();
  // the smallest of the most frequent grey values: largest (count, 255 - value)
  atomicMax(&best, ((unsigned long long)hist[tid] << 8) | (unsigned)(255 - tid));

  int s0 = wc, s1 = hc;
  const bool do_up = it.upscale && wc <= T0 / 2 && hc <= T1 / 2 && ((3 * wc) >> 1) * ((3 * hc) >> 1) <= up_cap;
  if (do_up) {
    s0 = (3 * wc) >> 1;    // int(wc * 1.5)
    s1 = (3 * hc) >> 1;
    unsigned mine = 0;
    for (int idx = tid; idx < s0 * s1; idx += INGEST_THREADS) {
      const int i = idx / s1, j = idx - i * s1;
      int y0, y1, x0, x1;
      double fy, fx;
      ingest_taps(i, it.up_scale0, wc, y0, y1, fy);
      ingest_taps(j, it.up_scale1, hc, x0, x1, fx);
      const int v = ingest_blend(pg.rot(y0, x0), pg.rot(y0, x1), pg.rot(y1, x0), pg.rot(y1, x1), fx, fy);
      up[idx] = (unsigned char)v;
      mine += v > 127;
    }
    if (mine) atomicAdd(&bright, mine);
  } else if (tid >= 128 && hist[tid]) {
    atomicAdd(&bright, hist[tid]);
  }
  __syncthreads();

  const int fill = 255 - (int)(best & 255);
  // invert when values > 127 strictly outnumber the others over the whole padded image: the pad area is (p0*p1 - s0*s1) copies of fill
  const long total = (long)it.p0 * it.p1, content = (long)s0 * s1;
  const long hi_n = (long)bright + (fill > 127 ? total - content : 0);
  const bool inv = hi_n > total - hi_n;

  auto padded = [&](int i, int j) -> int {
    const int ci = i - it.b0, cj = j - it.b1;
    int v = fill;
    if (ci >= 0 && ci < s0 && cj >= 0 && cj < s1) v = do_up ? (int)up[ci * s1 + cj] : pg.rot(ci, cj);
    return inv ? 255 - v : v;
  };
  for (int o = tid; o < npx; o += INGEST_THREADS) {
    const int y = o / T1, x = o - y * T1;
    int y0, y1, x0, x1;
    double fy, fx;
    ingest_taps(y, it.out_scale0, it.p0, y0, y1, fy);
    ingest_taps(x, it.out_scale1, it.p1, x0, x1, fx);
    const int v = ingest_blend(padded(y0, x0), padded(y0, x1), padded(y1, x0), padded(y1, x1), fx, fy);
    o32[o] = table[v];
    if (o8) o8[o] = (unsigned char)v;
  }
}

static bool ingest_scale_ok(double s) { return s > 0.0 && s < 1e12; }   // (false for NaN)

extern "C" int crnn_ingest_crops(const void* arena, long arena_bytes, const crnn_crop_item* items, const crnn_crop_item* items_dev, int n, int batch,
                                 int imgh, int imgw, const float* table, float* out, void* out_u8, hipStream_t stream) {
  if (n < 0 || batch < 1 || n > batch || imgh < 1 || imgw < 1 || !table || !out) return CRNN_ERR_ARG;
  if ((long)batch * imgh * imgw > 0x7fffffffL || (long)imgh * imgw > (1L << 24)) return CRNN_ERR_ARG;
  if (n > 0 && (!arena || arena_bytes < 1 || !items || !items_dev)) return CRNN_ERR_ARG;
  const long up_cap = (long)((3 * (imgh / 2)) >> 1) * ((3 * (imgw / 2)) >> 1);
  if (up_cap > INGEST_LDS_BUDGET) return CRNN_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i) {
    const crnn_crop_item& t = items[i];
    CRNN_TRY(page_check(t.page_off, t.rows, t.cols, t.stride, 0, arena_bytes, -1));                       // (pages.h; no size limit here)
    if (t.r0 < 0 || t.r0 >= t.r1 || t.r1 > t.rows || t.c0 < 0 || t.c0 >= t.c1 || t.c1 > t.cols) return CRNN_ERR_ARG;   // empty box / outside its page
    const int hc = t.r1 - t.r0, wc = t.c1 - t.c0;
    const bool small = wc <= imgh / 2 && hc <= imgw / 2;
    if ((t.upscale != 0) != small) return CRNN_ERR_ARG;
    const long s0 = small ? (3L * wc) >> 1 : wc, s1 = small ? (3L * hc) >> 1 : hc;
    if (t.b0 < 0 || t.b1 < 0 || t.p0 < 1 || t.p1 < 1 || t.b0 + s0 > t.p0 || t.b1 + s1 > t.p1) return CRNN_ERR_ARG;
    if (!ingest_scale_ok(t.out_scale0) || !ingest_scale_ok(t.out_scale1)) return CRNN_ERR_ARG;
    if (small && (!ingest_scale_ok(t.up_scale0) || !ingest_scale_ok(t.up_scale1))) return CRNN_ERR_ARG;
  }
  hipLaunchKernelGGL(ingest_crops_kernel, dim3(batch), dim3(INGEST_THREADS), (size_t)(up_cap > 16 ? up_cap : 16), stream, (const unsigned char*)arena,
                     arena_bytes, items_dev, n, imgh, imgw, (int)up_cap, table, out, (unsigned char*)out_u8);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
