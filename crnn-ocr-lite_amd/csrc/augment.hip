// Training augmentation of the ingest's uint8 batch: warp, stroke width, blur, tone, noise, then the ingest's grey -> fp32 table.  The rule is
// stated in include/crnn_mi355x.h (crnn_augment_batch) and restated in NumPy by crnn_mi355x/augment.py augment_host; both give the same bytes.
// One workgroup per image, one launch per batch: the image goes from global memory into LDS once (16-byte loads), the stages that are switched
// on run between two LDS buffers, and the last pass writes the fp32 row (and the optional uint8 row) in pixel order.  Integers only before the
// table lookup; the random decisions are the host's (AugmentPolicy.draw), the items are uniform over a workgroup.
#include "pages.h"

#define AUG_THREADS 256
#define AUG_MAX_PIXELS 16384               // imgh * imgw: two 16 KiB LDS buffers
#define AUG_MAX_COEF 262144

__global__ __launch_bounds__(AUG_THREADS) void augment_batch_kernel(const unsigned char* __restrict__ in, const crnn_augment_item* __restrict__ items,
                                                                    int n, int T0, int T1, const float* __restrict__ table, float* __restrict__ out,
                                                                    unsigned char* __restrict__ out_u8) {
  __shared__ __attribute__((aligned(16))) unsigned char buf0[AUG_MAX_PIXELS + 16];
  __shared__ __attribute__((aligned(16))) unsigned char buf1[AUG_MAX_PIXELS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int npx = T0 * T1;
  if (npx < 1 || npx > AUG_MAX_PIXELS) return;   // (the host refuses these; uniform)
  float* o32 = out + (long)b * npx;
  unsigned char* o8 = out_u8 ? out_u8 + (long)b * npx : nullptr;
  if (b >= n) {                                  // rows past n: zeros
    for (int o = tid; o < npx; o += AUG_THREADS) {
      o32[o] = 0.f;
      if (o8) o8[o] = 0;
    }
    return;
  }
  const crnn_augment_item it = items[b];

  // The image starts at any byte of the batch: pixel o lives at cur[o] with cur shifted by the source's misalignment, so that every 16-byte chunk
  // of global memory lands on a 16-byte boundary of LDS.  Head and tail bytes go one by one; nothing outside the image's npx bytes is read.
  const unsigned char* src = in + (long)b * npx;
  const int shift = (int)((uintptr_t)src & 15);
  unsigned char* cur = buf0 + shift;
  unsigned char* nxt = buf1;
  const int head = min(npx, (16 - shift) & 15);
  const int nvec = (npx - head) >> 4;
  for (int o = tid; o < head; o += AUG_THREADS) cur[o] = src[o];
  for (int k = tid; k < nvec; k += AUG_THREADS) *(uint4*)(cur + head + 16 * k) = *(const uint4*)(src + head + 16 * k);
  for (int o = head + 16 * nvec + tid; o < npx; o += AUG_THREADS) cur[o] = src[o];
  __syncthreads();

  auto swap = [&]() {
    __syncthreads();
    unsigned char* t = cur; cur = nxt; nxt = t;
  };

  // 1 warp
  if (it.a00 != 65536 || it.a01 != 0 || it.a10 != 0 || it.a11 != 65536 || it.t0 != 0 || it.t1 != 0) {
    const long a00 = it.a00, a01 = it.a01, a10 = it.a10, a11 = it.a11;
    const long y_off = (long)it.t0 + ((long)(T0 - 1) << 16), x_off = (long)it.t1 + ((long)(T1 - 1) << 16);
    const int fill = it.fill;
    for (int o = tid; o < npx; o += AUG_THREADS) {
      const int i = o / T1, j = o - i * T1;
      const long di = 2 * i - (T0 - 1), dj = 2 * j - (T1 - 1);
      const long Y = a00 * di + a01 * dj + y_off, X = a10 * di + a11 * dj + x_off;
      const long yl = Y >> 17, xl = X >> 17;
      // every row at or below -2 reads what row -2 reads, every row at or above T0 what row T0 reads: both taps are outside on the same side
      const int i0 = (int)(yl < -2 ? -2 : (yl > T0 ? T0 : yl)), j0 = (int)(xl < -2 ? -2 : (xl > T1 ? T1 : xl));
      const int fy = (int)((Y >> 9) & 255), fx = (int)((X >> 9) & 255);
      const int ia = page_clampi(i0, 0, T0 - 1), ib = page_clampi(i0 + 1, 0, T0 - 1);
      const int ja = page_clampi(j0, 0, T1 - 1), jb = page_clampi(j0 + 1, 0, T1 - 1);
      int p00 = cur[ia * T1 + ja], p01 = cur[ia * T1 + jb], p10 = cur[ib * T1 + ja], p11 = cur[ib * T1 + jb];
      if (fill >= 0) {                           // a tap outside the image is `fill`, not the clamped pixel
        const bool ra = ia == i0, rb = ib == i0 + 1, ca = ja == j0, cb = jb == j0 + 1;
        if (!(ra && ca)) p00 = fill;
        if (!(ra && cb)) p01 = fill;
        if (!(rb && ca)) p10 = fill;
        if (!(rb && cb)) p11 = fill;
      }
      const int v = ((256 - fy) * (256 - fx) * p00 + (256 - fy) * fx * p01 + fy * (256 - fx) * p10 + fy * fx * p11 + 32768) >> 16;
      nxt[o] = (unsigned char)page_clampi(v, 0, 255);   // (v is within 0..255 for every fill the host lets through)
    }
    swap();
  }

  // 2 stroke width: max / min over the window clipped to the image = over clamped indices, which repeat window pixels only
  if (it.morph != 0) {
    const int r = page_clampi(it.morph < 0 ? -it.morph : it.morph, 1, 2);
    const bool dilate = it.morph > 0;
    for (int o = tid; o < npx; o += AUG_THREADS) {
      const int i = o / T1, j = o - i * T1;
      int v = cur[o];
      for (int a = -r; a <= r; ++a) {
        const unsigned char* row = cur + page_clampi(i + a, 0, T0 - 1) * T1;
        for (int c = -r; c <= r; ++c) {
          const int p = row[page_clampi(j + c, 0, T1 - 1)];
          v = dilate ? max(v, p) : min(v, p);
        }
      }
      nxt[o] = (unsigned char)v;
    }
    swap();
  }

  // 3 blur: the two 1-2-1 passes of one binomial pass as its nine taps (h does not fit a byte), edge replication = clamped indices
  for (int pass = 0; pass < page_clampi(it.blur, 0, 2); ++pass) {
    for (int o = tid; o < npx; o += AUG_THREADS) {
      const int i = o / T1, j = o - i * T1;
      const int jl = max(j - 1, 0), jr = min(j + 1, T1 - 1);
      const unsigned char* r0 = cur + max(i - 1, 0) * T1;
      const unsigned char* r1 = cur + i * T1;
      const unsigned char* r2 = cur + min(i + 1, T0 - 1) * T1;
      const int h0 = r0[jl] + 2 * r0[j] + r0[jr], h1 = r1[jl] + 2 * r1[j] + r1[jr], h2 = r2[jl] + 2 * r2[j] + r2[jr];
      nxt[o] = (unsigned char)((h0 + 2 * h1 + h2 + 8) >> 4);
    }
    swap();
  }

  // 4 tone, 5 noise, 6 output
  const bool tone = it.gain != 256 || it.bias != 0;
  const int tone_off = (128 + it.bias) * 256 + 128;
  for (int o = tid; o < npx; o += AUG_THREADS) {
    int v = cur[o];
    if (tone) v = page_clampi(((v - 128) * it.gain + tone_off) >> 8, 0, 255);
    if (it.noise != 0) {
      const unsigned h = crnn_mix32(it.seed ^ ((unsigned)o * 0x9E3779B9u));
      const int s = (int)((h & 255u) + ((h >> 8) & 255u) + ((h >> 16) & 255u) + (h >> 24)) - 510;
      v = page_clampi(v + ((s * it.noise) >> 8), 0, 255);
    }
    o32[o] = table[v];
    if (o8) o8[o] = (unsigned char)v;
  }
}

static bool aug_item_ok(const crnn_augment_item& t, int imgh, int imgw) {
  auto within = [](long v, long m) { return v >= -m && v <= m; };
  return within(t.a00, AUG_MAX_COEF) && within(t.a01, AUG_MAX_COEF) && within(t.a10, AUG_MAX_COEF) && within(t.a11, AUG_MAX_COEF)
         && within(t.t0, (long)imgh << 17) && within(t.t1, (long)imgw << 17) && t.fill >= -1 && t.fill <= 255 && within(t.morph, 2)
         && t.blur >= 0 && t.blur <= 2 && t.gain >= 0 && t.gain <= 1024 && within(t.bias, 255) && t.noise >= 0 && t.noise <= 64;
}

extern "C" int crnn_augment_batch(const void* in_u8, const crnn_augment_item* items, const crnn_augment_item* items_dev, int n, int batch, int imgh,
                                  int imgw, const float* table, float* out, void* out_u8, hipStream_t stream) {
  if (n < 0 || batch < 1 || n > batch || imgh < 1 || imgw < 1 || !in_u8 || !table || !out) return CRNN_ERR_ARG;
  if (n > 0 && (!items || !items_dev)) return CRNN_ERR_ARG;
  if ((long)imgh * imgw > AUG_MAX_PIXELS) return CRNN_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (!aug_item_ok(items[i], imgh, imgw)) return CRNN_ERR_ARG;
  const long bytes = (long)batch * imgh * imgw;
  if (out_u8 && page_ranges_overlap(in_u8, bytes, out_u8, bytes)) return CRNN_ERR_ARG;
  hipLaunchKernelGGL(augment_batch_kernel, dim3(batch), dim3(AUG_THREADS), 0, stream, (const unsigned char*)in_u8, items_dev, n, imgh, imgw, table, out,
                     (unsigned char*)out_u8);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
