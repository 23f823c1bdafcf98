// Synthetic training words: a glyph atlas and glyph codes -> the uint8 batch the ingest writes and its fp32 table[v].  The rule is stated in
// include/crnn_mi355x.h (crnn_synth_words) and restated in NumPy by crnn_mi355x/synth.py synth_host; both give the same bytes.
// One workgroup per image, one launch per batch: wave 0 turns the word's advances into pens with a wave prefix sum and leaves the glyph boxes
// (ink origin, size, arena offset) in LDS; every thread then takes runs of output pixels in memory order (j fastest), finds the glyphs that
// overlap the run's text column once -- a 64-bit mask, recomputed only when i changes -- and gathers the four taps of each pixel straight from
// the atlas (tens of KB per face: it stays in L2).  No composed line is stored, so the design adds no size limit.  Integers only before the
// table lookup; the random decisions are the host's (SynthPolicy.draw), the items are uniform over a workgroup.
#include "pages.h"

#define SYN_THREADS 256
#define SYN_MAX_LEN 64
#define SYN_MAX_PIXELS 16384               // imgh * imgw: crnn_augment_batch's limit, so the two launches compose
#define SYN_MAX_DIM 64                     // w, h, top + h, |left| of a glyph
#define SYN_MAX_ADVANCE 128
#define SYN_MIN_SCALE 16384
#define SYN_MAX_SCALE 262144
#define SYN_MAX_OFFSET (1 << 28)

// P = pixels per thread and step: 16 (npx a multiple of 16, both outputs on 16-byte boundaries: 16-byte stores) or 1.
template <int P>
__global__ __launch_bounds__(SYN_THREADS) void synth_words_kernel(const unsigned char* __restrict__ atlas, long atlas_bytes,
                                                                  const crnn_glyph* __restrict__ glyphs, int nfaces, int nglyphs,
                                                                  const int* __restrict__ codes, const crnn_synth_item* __restrict__ items, int n, int Lmax,
                                                                  int T0, int T1, const float* __restrict__ table, float* __restrict__ out,
                                                                  unsigned char* __restrict__ out_u8) {
  __shared__ int s_xlo[SYN_MAX_LEN], s_w[SYN_MAX_LEN], s_ylo[SYN_MAX_LEN], s_h[SYN_MAX_LEN];
  __shared__ long s_off[SYN_MAX_LEN];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int npx = T0 * T1;
  if (npx < 1 || npx > SYN_MAX_PIXELS || nfaces < 1 || nglyphs < 1 || atlas_bytes < 1) return;   // (the host refuses these; uniform)
  float* o32 = out + (long)b * npx;
  unsigned char* o8 = out_u8 ? out_u8 + (long)b * npx : nullptr;
  if (b >= n) {                                  // rows past n: zeros
    for (int o = tid * P; o < npx; o += SYN_THREADS * P) {
      if (P == 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) *(float4*)(o32 + o + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o8) *(uint4*)(o8 + o) = make_uint4(0u, 0u, 0u, 0u);
      } else {
        o32[o] = 0.f;
        if (o8) o8[o] = 0;
      }
    }
    return;
  }
  const crnn_synth_item it = items[b];
  // every field is clamped into its range again: the host judged its own copy of the tables, the kernel trusts neither copy with an address
  const int len = page_clampi(it.len, 0, min(Lmax, SYN_MAX_LEN));

  if (tid < 64) {                                // wave 0: lane k holds glyph k; pens = the exclusive prefix sum of advance + track
    int adv = 0, left = 0, top = 0, w = 0, h = 0;
    long off = 0;
    if (tid < len) {
      const int code = page_clampi(codes[(long)b * Lmax + tid], 0, nglyphs - 1);
      const crnn_glyph g = glyphs[(long)page_clampi(it.face, 0, nfaces - 1) * nglyphs + code];
      adv = page_clampi(g.advance, 0, SYN_MAX_ADVANCE) + page_clampi(it.track, -8, 32);
      left = page_clampi(g.left, -SYN_MAX_DIM, SYN_MAX_DIM);
      top = page_clampi(g.top, 0, SYN_MAX_DIM);
      w = page_clampi(g.w, 0, SYN_MAX_DIM);
      h = page_clampi(g.h, 0, SYN_MAX_DIM);
      off = g.off;
    }
    int sum = adv;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(sum, d, 64);
      if (tid >= d) sum += t;
    }
    const int jitter = page_clampi(it.jitter, 0, 8);
    const unsigned hash = crnn_mix32(it.seed ^ ((unsigned)tid * 0x9E3779B9u));
    const int dy = (int)(((hash & 0xffffu) * (unsigned)(2 * jitter + 1)) >> 16) - jitter;
    if (tid < len) {
      s_xlo[tid] = sum - adv + left;
      s_w[tid] = w;
      s_ylo[tid] = top + dy;
      s_h[tid] = h;
      s_off[tid] = off;
    }
  }
  __syncthreads();

  const long sx = it.sx, sy = it.sy, ox = it.ox, oy = it.oy;
  const int fg = page_clampi(it.fg, 0, 255), bg = page_clampi(it.bg, 0, 255);
  auto ink = [&](long a) -> int { return atlas[a < 0 ? 0 : (a > atlas_bytes - 1 ? atlas_bytes - 1 : a)]; };   // every read inside the arena
  int cur_i = -1, x0 = 0, fx = 0;
  unsigned long long cand = 0;                   // the glyphs whose columns reach x0 or x0 + 1
  auto pixel = [&](int o) -> int {
    const int i = o / T1, j = o - i * T1;
    if (i != cur_i) {
      cur_i = i;
      const long X = sx * i + ox;
      x0 = (int)(X >> 16);                       // |X| < 2^46: fits
      fx = (int)((X >> 8) & 255);
      cand = 0;
      for (int k = 0; k < len; ++k) {
        const int xl = s_xlo[k];
        if (x0 + 1 >= xl && x0 < xl + s_w[k]) cand |= 1ull << k;
      }
    }
    const long Y = sy * (T1 - 1 - j) + oy;
    const int y0 = (int)(Y >> 16), fy = (int)((Y >> 8) & 255);
    int c00 = 0, c01 = 0, c10 = 0, c11 = 0;
    for (unsigned long long m = cand; m; m &= m - 1) {
      const int k = __ffsll((long long)m) - 1;
      const int w = s_w[k], h = s_h[k], cx = x0 - s_xlo[k], cy = y0 - s_ylo[k];
      const bool ra = (unsigned)cy < (unsigned)h, rb = (unsigned)(cy + 1) < (unsigned)h;
      if (!(ra || rb)) continue;
      const bool ca = (unsigned)cx < (unsigned)w, cb = (unsigned)(cx + 1) < (unsigned)w;
      const long a = s_off[k] + (long)cy * w + cx;
      if (ra && ca) c00 = max(c00, ink(a));
      if (ra && cb) c01 = max(c01, ink(a + 1));
      if (rb && ca) c10 = max(c10, ink(a + w));
      if (rb && cb) c11 = max(c11, ink(a + w + 1));
    }
    const int c = ((256 - fy) * (256 - fx) * c00 + (256 - fy) * fx * c01 + fy * (256 - fx) * c10 + fy * fx * c11 + 32768) >> 16;
    return (bg * (255 - c) + fg * c + 127) / 255;
  };

  for (int o = tid * P; o < npx; o += SYN_THREADS * P) {
    if (P == 16) {
      unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {
        const int v0 = pixel(o + 4 * q), v1 = pixel(o + 4 * q + 1), v2 = pixel(o + 4 * q + 2), v3 = pixel(o + 4 * q + 3);
        *(float4*)(o32 + o + 4 * q) = make_float4(table[v0], table[v1], table[v2], table[v3]);
        const unsigned word = (unsigned)v0 | ((unsigned)v1 << 8) | ((unsigned)v2 << 16) | ((unsigned)v3 << 24);
        w0 = q == 0 ? word : w0;
        w1 = q == 1 ? word : w1;
        w2 = q == 2 ? word : w2;
        w3 = q == 3 ? word : w3;
      }
      if (o8) *(uint4*)(o8 + o) = make_uint4(w0, w1, w2, w3);
    } else {
      const int v = pixel(o);
      o32[o] = table[v];
      if (o8) o8[o] = (unsigned char)v;
    }
  }
}

static bool syn_glyph_ok(const crnn_glyph& g, long atlas_bytes) {
  if (g.w < 0 || g.h < 0 || g.w > SYN_MAX_DIM || g.h > SYN_MAX_DIM || (g.w == 0) != (g.h == 0) || g.top < 0 || g.top + g.h > SYN_MAX_DIM
      || g.left < -SYN_MAX_DIM || g.left > SYN_MAX_DIM || g.advance < 0 || g.advance > SYN_MAX_ADVANCE)
    return false;
  return g.w == 0 || (g.off >= 0 && g.off <= atlas_bytes - (long)g.w * g.h);      // a glyph without ink reads nothing: its off is not judged
}

static bool syn_item_ok(const crnn_synth_item& t, const int* codes, int nfaces, int nglyphs, int Lmax) {
  if (t.face < 0 || t.face >= nfaces || t.len < 0 || t.len > Lmax || t.track < -8 || t.track > 32 || t.jitter < 0 || t.jitter > 8
      || t.sx < SYN_MIN_SCALE || t.sx > SYN_MAX_SCALE || t.sy < SYN_MIN_SCALE || t.sy > SYN_MAX_SCALE || t.ox < -SYN_MAX_OFFSET
      || t.ox > SYN_MAX_OFFSET || t.oy < -SYN_MAX_OFFSET || t.oy > SYN_MAX_OFFSET || t.fg < 0 || t.fg > 255 || t.bg < 0 || t.bg > 255)
    return false;
  for (int k = 0; k < t.len; ++k)
    if (codes[k] < 0 || codes[k] >= nglyphs) return false;
  return true;
}

extern "C" int crnn_synth_words(const void* atlas, long atlas_bytes, const crnn_glyph* glyphs, const crnn_glyph* glyphs_dev, int nfaces, int nglyphs,
                                const int* codes, const int* codes_dev, const crnn_synth_item* items, const crnn_synth_item* items_dev, int n, int batch,
                                int Lmax, int imgh, int imgw, const float* table, float* out, void* out_u8, hipStream_t stream) {
  if (n < 0 || batch < 1 || n > batch || imgh < 1 || imgw < 1 || nfaces < 1 || nglyphs < 1 || Lmax < 1 || Lmax > SYN_MAX_LEN || atlas_bytes < 1
      || !atlas || !glyphs || !glyphs_dev || !table || !out)
    return CRNN_ERR_ARG;
  if (n > 0 && (!codes || !codes_dev || !items || !items_dev)) return CRNN_ERR_ARG;
  if ((long)imgh * imgw > SYN_MAX_PIXELS) return CRNN_ERR_UNSUPPORTED;
  for (long g = 0; g < (long)nfaces * nglyphs; ++g)
    if (!syn_glyph_ok(glyphs[g], atlas_bytes)) return CRNN_ERR_ARG;
  for (int i = 0; i < n; ++i)
    if (!syn_item_ok(items[i], codes + (long)i * Lmax, nfaces, nglyphs, Lmax)) return CRNN_ERR_ARG;
  const bool wide = (imgh * imgw) % 16 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)out_u8 & 15) == 0;
  if (wide)
    hipLaunchKernelGGL(synth_words_kernel<16>, dim3(batch), dim3(SYN_THREADS), 0, stream, (const unsigned char*)atlas, atlas_bytes, glyphs_dev, nfaces,
                       nglyphs, codes_dev, items_dev, n, Lmax, imgh, imgw, table, out, (unsigned char*)out_u8);
  else
    hipLaunchKernelGGL(synth_words_kernel<1>, dim3(batch), dim3(SYN_THREADS), 0, stream, (const unsigned char*)atlas, atlas_bytes, glyphs_dev, nfaces,
                       nglyphs, codes_dev, items_dev, n, Lmax, imgh, imgw, table, out, (unsigned char*)out_u8);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
