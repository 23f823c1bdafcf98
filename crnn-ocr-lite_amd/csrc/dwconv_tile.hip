// Depthwise 3x3 'same' on the halo tile (utils.py:43-56, 64-70), NHWC: forward, data gradient (the same kernel with flipped taps) and weight gradient.
//   The (TH+2) x (TW+2) halo tile of one 128-byte channel slab is staged in LDS with 16-byte loads, each thread produces 3 adjacent pixels from one 3x5
//   window, and the BatchNorm batch statistics (or the 9 tap gradients) leave as a deterministic per-tile partial; maps whose channel count is no whole
//   slab (the C = 1 first block) take the one-thread-per-element fallback.
// HBM-bandwidth bound.  The row-stream forms of the same stage are dwconv_stream.hip / dwconv_bwd_stream.hip.
#include "common.h"
#include "conv_vec.h"

constexpr int DW_NT = 256;   // threads per depthwise workgroup

// ---------------------------------------------------------------------------------------------
// depthwise 3x3, C % 32 == 0 : LDS halo tile
// grid.x = C/32, grid.y = B * ceil(H/TH); block 256 = 8 channel-quads x 32 pixel threads
// mode 0: out = conv(x, k) (flip=1 -> taps flipped = data gradient), optional stats partials
// mode 1: weight gradient partials: dk[tap][c] += x[shifted] * g[center]
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void widen(const float4& v, float (&f)[4]) { f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w; }
__device__ __forceinline__ void widen(const uint2& u, float (&f)[4]) {
  f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
  f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
}
__device__ __forceinline__ void zerov(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void zerov(uint2& v) { v = make_uint2(0u, 0u); }
__device__ __forceinline__ void narrow_store(float* p, const float (&f)[4]) { st4(p, make_float4(f[0], f[1], f[2], f[3])); }
__device__ __forceinline__ void narrow_store(bf16_t* p, const float (&f)[4]) { st4(p, make_float4(f[0], f[1], f[2], f[3])); }
// sum over the pixel-threads of a wave that share a channel lane (lanes l, l^CL, l^2CL, ...), fixed order
template <int CL>
__device__ __forceinline__ float pixlane_sum(float v) {
#pragma unroll
  for (int o = CL; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// A workgroup handles TH rows x full width x one 128-BYTE channel slab (32 fp32 or 64 bf16 channels): every
// pixel's slab is one full 128-B HBM segment in either storage type (CL lanes x sizeof(V) bytes).
// Each thread produces PXB horizontally adjacent pixels per step: the 3 x (PXB+2) window is read from LDS and widened
// once and feeds all PXB outputs (5 LDS vectors per output at PXB = 3 instead of 9).
#define DW_PXB 3   // fp32 storage; bf16 storage (8 channels per lane, 72 weight registers) uses 2
template <int MODE, int NT, typename T>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(3))) void dwconv_tile_kernel(const T* __restrict__ x, const float* __restrict__ k,
                                                          const T* __restrict__ g, T* __restrict__ out,
                                                          float* __restrict__ partials, int B, int H, int W, int C,
                                                          int TH, int TW, int flip, const float* __restrict__ bnstate) {
  // MODE 0: out = conv (+ statistics partials)   MODE 1: weight-gradient partials
  // MODE 2: out = ReLU6(conv * scale + shift) with bnstate = [mean|var|scale|shift] (inference: BatchNorm folded in)
  constexpr bool FWD = (MODE != 1);
  typedef typename RawV<T>::type V;
  constexpr int VN = RawV<T>::N;              // channels per lane
  constexpr int CL = 128 / sizeof(V);         // lanes per pixel (the 128-B slab)
  constexpr int PT = NT / CL;                 // pixel threads
  constexpr int MAXLD = 49152 / (NT * sizeof(V));   // loads per thread for a full 48 KiB tile
  extern __shared__ __attribute__((aligned(16))) float smem[];
  V* tile = reinterpret_cast<V*>(smem);
  const int tid = threadIdx.x, c4 = tid & (CL - 1), pt = tid / CL;
  const int cc0 = blockIdx.x * (VN * CL);
  const int nHb = (H + TH - 1) / TH, nWb = (W + TW - 1) / TW;
  const int wb = blockIdx.y % nWb, hb = (blockIdx.y / nWb) % nHb, b = blockIdx.y / (nWb * nHb);
  const int h0 = hb * TH, w0 = wb * TW;
  const int Wt = TW + 2;
  // halo-tile fill with 16-byte loads (8 lanes per pixel slab, whatever the compute vector is); all of this thread's
  // loads are issued before the first LDS write (one HBM latency per workgroup).  32-bit offsets inside the image,
  // (fy, fx) stepped without division or branches.
  {
    constexpr int FL = 8, FPT = NT / FL;                  // fill lanes per pixel, fill pixel-threads
    constexpr int FMAX = 49152 / (NT * 16);               // loads per thread for a full 48 KiB tile
    constexpr int FE = 16 / sizeof(T);                    // elements per 16-byte load
    uint4* tile16 = reinterpret_cast<uint4*>(smem);
    const T* xb = x + (long)b * H * W * C + cc0 + FE * (tid & (FL - 1));
    const int n16 = (TH + 2) * Wt * FL;
    const int dfy = FPT / Wt, dfx = FPT - dfy * Wt;
    for (int base = tid; base < n16; base += FMAX * NT) {
      uint4 v[FMAX];
      int pix0 = base / FL;
      int fy = pix0 / Wt, fx = pix0 - fy * Wt;
#pragma unroll
      for (int uu = 0; uu < FMAX; ++uu) {
        int i = base + uu * NT;
        int gh = h0 + fy - 1, gw = w0 + fx - 1;
        v[uu] = make_uint4(0u, 0u, 0u, 0u);
        if (i < n16 && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W)
          v[uu] = *reinterpret_cast<const uint4*>(xb + (gh * W + gw) * C);
        fx += dfx; fy += dfy;
        if (fx >= Wt) { fx -= Wt; ++fy; }
      }
#pragma unroll
      for (int uu = 0; uu < FMAX; ++uu) {
        int i = base + uu * NT;
        if (i < n16) tile16[i] = v[uu];
      }
    }
  }
  float kw[9][VN];
  if (FWD) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      int ts = flip ? 8 - t : t;
      VecF<VN> w = vload<VN>(&k[ts * C + cc0 + VN * c4]);
#pragma unroll
      for (int e = 0; e < VN; ++e) kw[t][e] = w.v[e];
    }
  }
  float bsc[VN], bsh[VN];
  if (MODE == 2) {
    VecF<VN> v1 = vload<VN>(&bnstate[2 * C + cc0 + VN * c4]), v2 = vload<VN>(&bnstate[3 * C + cc0 + VN * c4]);
#pragma unroll
    for (int e = 0; e < VN; ++e) { bsc[e] = v1.v[e]; bsh[e] = v2.v[e]; }
  }
  __syncthreads();
  float s[VN], ss[VN], dk[9][VN];
#pragma unroll
  for (int e = 0; e < VN; ++e) { s[e] = 0.f; ss[e] = 0.f; }
  if (MODE == 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < VN; ++e) dk[t][e] = 0.f;
  }
  constexpr int PXB = DW_PXB;
  const int gpr = (TW + PXB - 1) / PXB;        // pixel groups per tile row
  const int npg = TH * gpr;
  const int dly = PT / gpr, dlg = PT - dly * gpr;
  int ly = pt / gpr, lg = pt - ly * gpr;       // stepped incrementally below
  const T* gb = g + (long)b * H * W * C + cc0 + VN * c4;
  T* ob = out + (long)b * H * W * C + cc0 + VN * c4;
  for (int pg = pt; pg < npg; pg += PT) {
    const int lx = lg * PXB;
    const int gh = h0 + ly;
    if (gh >= H) break;
    const int o = (gh * W + w0 + lx) * C;
    float gv[PXB][VN];
    bool pv[PXB];                                // pixel e of this group exists (the last group of a row may be ragged)
#pragma unroll
    for (int e = 0; e < PXB; ++e) pv[e] = (lx + e < TW) && (w0 + lx + e < W);
    if (MODE == 1) {
#pragma unroll
      for (int e = 0; e < PXB; ++e) {
        V gr; zerov(gr);
        if (pv[e]) gr = ldraw<V>(gb + o + e * C);
        widen(gr, gv[e]);
      }
    }
    float a[PXB][VN];
#pragma unroll
    for (int e = 0; e < PXB; ++e)
#pragma unroll
      for (int c = 0; c < VN; ++c) a[e][c] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      float r[PXB + 2][VN];   // (the last group of a ragged row reads past the row end: those outputs are discarded)
#pragma unroll
      for (int j = 0; j < PXB + 2; ++j) widen(tile[((ly + i) * Wt + lx + j) * CL + c4], r[j]);
#pragma unroll
      for (int e = 0; e < PXB; ++e)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int c = 0; c < VN; ++c) {
            if (FWD) a[e][c] = fmaf(r[e + j][c], kw[i * 3 + j][c], a[e][c]);
            else if (pv[e]) dk[i * 3 + j][c] = fmaf(r[e + j][c], gv[e][c], dk[i * 3 + j][c]);   // (a ragged group's window may hold LDS garbage: 0 * NaN)
          }
      __builtin_amdgcn_sched_barrier(0);   // one window row at a time: keeps the live set under the 3-waves/SIMD budget
    }
    if (FWD) {
#pragma unroll
      for (int e = 0; e < PXB; ++e)
        if (pv[e]) {
          if (MODE == 2) {
#pragma unroll
            for (int c = 0; c < VN; ++c) a[e][c] = relu6f(fmaf(a[e][c], bsc[c], bsh[c]));
          }
          narrow_store(ob + o + e * C, a[e]);
          if (partials != nullptr) {
#pragma unroll
            for (int c = 0; c < VN; ++c) { s[c] += a[e][c]; ss[c] = fmaf(a[e][c], a[e][c], ss[c]); }
          }
        }
    }
    lg += dlg; ly += dly;
    if (lg >= gpr) { lg -= gpr; ++ly; }
  }
  if (partials == nullptr || MODE == 2) return;
  // per-tile partials: the 8 pixel-threads of each wave are combined with lane shuffles, the NT/64 waves through LDS
  __syncthreads();  // tile no longer needed
  constexpr int NW = NT / 64, NV = FWD ? 2 : 9;
  float* red = smem;   // [NW][NV][CL][VN]
  const int wave = tid >> 6, lane = tid & 63;
  if (FWD) {
#pragma unroll
    for (int e = 0; e < VN; ++e) { s[e] = pixlane_sum<CL>(s[e]); ss[e] = pixlane_sum<CL>(ss[e]); }
    if (lane < CL) {
#pragma unroll
      for (int e = 0; e < VN; ++e) { red[((wave * NV + 0) * CL + c4) * VN + e] = s[e]; red[((wave * NV + 1) * CL + c4) * VN + e] = ss[e]; }
    }
  } else {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < VN; ++e) dk[t][e] = pixlane_sum<CL>(dk[t][e]);
    if (lane < CL) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < VN; ++e) red[((wave * NV + t) * CL + c4) * VN + e] = dk[t][e];
    }
  }
  __syncthreads();
  for (int i = tid; i < NV * CL * VN; i += NT) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) a += red[w * NV * CL * VN + i];
    int v = i / (CL * VN), cch = i % (CL * VN);
    partials[((long)blockIdx.y * NV + v) * C + cc0 + cch] = a;
  }
}

// generic fallback (any C, e.g. the C=1 first block): one thread per output element
template <int MODE>
__global__ void dwconv_naive_kernel(const float* __restrict__ x, const float* __restrict__ k, const float* __restrict__ g,
                                    float* __restrict__ out, int B, int H, int W, int C, int flip) {
  if (MODE == 0) {
    long total = (long)B * H * W * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      int c = (int)(i % C); long pix = i / C;
      int w = (int)(pix % W); long r = pix / W; int h = (int)(r % H); long b = r / H;
      float a = 0.f;
      for (int ii = 0; ii < 3; ++ii)
        for (int j = 0; j < 3; ++j) {
          int gh = h + ii - 1, gw = w + j - 1;
          if (gh >= 0 && gh < H && gw >= 0 && gw < W) {
            int t = ii * 3 + j; if (flip) t = 8 - t;
            a = fmaf(x[((b * H + gh) * W + gw) * C + c], k[t * C + c], a);
          }
        }
      out[i] = a;
    }
  } else {
    // weight gradient, tiny tensors only: one block per (tap, channel), block-wide reduction
    int t = blockIdx.x / C, c = blockIdx.x % C;
    int ii = t / 3, j = t % 3;
    float a = 0.f;
    long npix = (long)B * H * W;
    for (long p = threadIdx.x; p < npix; p += blockDim.x) {
      int w = (int)(p % W); long r = p / W; int h = (int)(r % H); long b = r / H;
      int gh = h + ii - 1, gw = w + j - 1;
      if (gh >= 0 && gh < H && gw >= 0 && gw < W) a = fmaf(x[((b * H + gh) * W + gw) * C + c], g[p * C + c], a);
    }
    __shared__ float red[256];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) out[t * C + c] = red[0];
  }
}

// single-channel weight gradient: partials[blk][9]
__global__ __launch_bounds__(256) void dwconv_wgrad_c1_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                              float* __restrict__ partials, int B, int H, int W) {
  __shared__ float red[9][256];
  float acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.f;
  const long npix = (long)B * H * W;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256L) {
    int w = (int)(p % W); long r = p / W; int h = (int)(r % H);
    float gv = g[p];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        int gh = h + i - 1, gw = w + j - 1;
        if (gh >= 0 && gh < H && gw >= 0 && gw < W) acc[i * 3 + j] = fmaf(x[p + (long)(i - 1) * W + (j - 1)], gv, acc[i * 3 + j]);
      }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) red[t][threadIdx.x] = acc[t];
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if (threadIdx.x < s2)
#pragma unroll
      for (int t = 0; t < 9; ++t) red[t][threadIdx.x] += red[t][threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x < 9) partials[(long)blockIdx.x * 9 + threadIdx.x] = red[threadIdx.x][0];
}

// Tile = TH rows x TW columns of one 128-byte channel slab.  TW splits W into ceil(W/64) equal column tiles (the CRNN
// maps are at most 36 wide: full-width tiles), TH is as tall as a 48 KiB halo tile allows (3 workgroups per CU) and
// then balanced over the bands of H.
struct DwTile { int TH, TW, nHb, nWb; size_t lds; };
static DwTile dw_pick_tile(int H, int W) {
  DwTile t;
  t.nWb = cdiv(W, 64);
  t.TW = cdiv(W, t.nWb);
  t.nWb = cdiv(W, t.TW);
  const int lds_budget = 49152;                                                          // halo-tile budget in bytes
  int thmax = (int)((size_t)lds_budget / ((size_t)(t.TW + 2) * 128)) - 2;
  if (thmax < 1) thmax = 1;
  if (thmax > H) thmax = H;
  int nb = cdiv(H, thmax);
  t.TH = cdiv(H, nb);
  t.nHb = cdiv(H, t.TH);
  const size_t red = (size_t)(DW_NT / 64) * 9 * 64 * 4;  // weight-grad cross-wave reduction scratch (<= 64 channels per slab)
  size_t tile = (size_t)(t.TH + 2) * (t.TW + 2) * 128 + 128 * DW_PXB;   // + slack for the ragged last pixel group
  t.lds = tile > red ? tile : red;
  return t;
}

// number of tiles (= partial rows) the tiled kernels produce for a (B,H,W) map
extern "C" int crnn_dwconv_num_tiles(int B, int H, int W) {
  DwTile t = dw_pick_tile(H, W);
  return B * t.nHb * t.nWb;
}

// out = dwconv3x3(x, k[9][C]); flip=1 gives the data gradient.  If `stat_partials` != null (C%32==0
// only) it receives [num_tiles][2][C] (sum, sumsq) partial BatchNorm statistics of `out`.
// dtype: storage of x/out (CRNN_F32 | CRNN_BF16); arithmetic and statistics are fp32 either way.
template <typename T>
static int dwconv_fwd_launch(const T* x, const float* k, T* out, float* stat_partials, int B, int H, int W, int C, int flip,
                             hipStream_t stream, const float* bnstate = nullptr) {
  DwTile t = dw_pick_tile(H, W);
  if (t.lds > 160 * 1024) return CRNN_ERR_UNSUPPORTED;
  if (t.lds > 48 * 1024) {   // more dynamic LDS than the default launch limit: raise it to exactly what this tile needs
    hipError_t e = hipFuncSetAttribute((const void*)dwconv_tile_kernel<0, DW_NT, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds);
    if (e != hipSuccess) return (int)e;
    if (bnstate) { e = hipFuncSetAttribute((const void*)dwconv_tile_kernel<2, DW_NT, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds); if (e != hipSuccess) return (int)e; }
  }
  const int slab = 128 / (int)sizeof(T);   // channels per workgroup: 32 (fp32) or 64 (bf16)
  if (C % slab) return CRNN_ERR_UNSUPPORTED;
  dim3 grid(C / slab, B * t.nHb * t.nWb);
  if (bnstate) hipLaunchKernelGGL((dwconv_tile_kernel<2, DW_NT, T>), grid, dim3(DW_NT), t.lds, stream, x, k, (const T*)nullptr, out, (float*)nullptr, B, H, W, C, t.TH, t.TW, flip, bnstate);
  else hipLaunchKernelGGL((dwconv_tile_kernel<0, DW_NT, T>), grid, dim3(DW_NT), t.lds, stream, x, k, (const T*)nullptr, out, stat_partials, B, H, W, C, t.TH, t.TW, flip, (const float*)nullptr);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

extern "C" int crnn_dwconv3x3_fwd_ex(const void* x, const float* k, void* out, float* stat_partials, int B, int H, int W,
                                     int C, int flip, int dtype, hipStream_t stream) {
  if (C % 32 == 0) {
    if (dtype == CRNN_BF16) return dwconv_fwd_launch<bf16_t>((const bf16_t*)x, k, (bf16_t*)out, stat_partials, B, H, W, C, flip, stream);
    return dwconv_fwd_launch<float>((const float*)x, k, (float*)out, stat_partials, B, H, W, C, flip, stream);
  }
  if (stat_partials || dtype != CRNN_F32) return CRNN_ERR_UNSUPPORTED;
  long total = (long)B * H * W * C;
  int blocks = cdiv(total, 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dwconv_naive_kernel<0>, dim3(blocks), dim3(256), 0, stream, (const float*)x, k, nullptr, (float*)out, B, H, W, C, flip);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
// Inference form: out = ReLU6(BatchNorm(dwconv3x3(x, k))) with the normalisation folded into the conv's epilogue
// (bnstate = [mean|var|scale|shift] from crnn_bn_infer_state); C % (128 / sizeof(storage)) == 0 only.
extern "C" int crnn_dwconv3x3_bn_relu6_fwd(const void* x, const float* k, const float* bnstate, void* out, int B, int H, int W, int C,
                                           int dtype, hipStream_t stream) {
  if (!bnstate) return CRNN_ERR_ARG;
  if (dtype == CRNN_BF16) return dwconv_fwd_launch<bf16_t>((const bf16_t*)x, k, (bf16_t*)out, nullptr, B, H, W, C, 0, stream, bnstate);
  return dwconv_fwd_launch<float>((const float*)x, k, (float*)out, nullptr, B, H, W, C, 0, stream, bnstate);
}

// weight gradient of the depthwise conv: dk[9][C] = sum x[shifted] * g.  scratch: [num_tiles][9][C]
template <typename T>
static int dwconv_wgrad_launch(const T* x, const T* g, float* dk, float* scratch, int B, int H, int W, int C, hipStream_t stream) {
  DwTile t = dw_pick_tile(H, W);
  if (t.lds > 160 * 1024) return CRNN_ERR_UNSUPPORTED;
  if (t.lds > 48 * 1024) {   // more dynamic LDS than the default launch limit: raise it to exactly what this tile needs
    hipError_t e = hipFuncSetAttribute((const void*)dwconv_tile_kernel<1, DW_NT, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds);
    if (e != hipSuccess) return (int)e;
  }
  int ntiles = B * t.nHb * t.nWb;
  const int slab = 128 / (int)sizeof(T);
  if (C % slab) return CRNN_ERR_UNSUPPORTED;
  dim3 grid(C / slab, ntiles);
  hipLaunchKernelGGL((dwconv_tile_kernel<1, DW_NT, T>), grid, dim3(DW_NT), t.lds, stream, x, (const float*)nullptr, g, (T*)nullptr, scratch, B, H, W, C, t.TH, t.TW, 0, (const float*)nullptr);
  CRNN_LAUNCH_CHECK();
  return crnn_partials_sum(scratch, ntiles, 9 * C, dk, 1.f, stream);
}

extern "C" int crnn_dwconv3x3_wgrad_ex(const void* x, const void* g, float* dk, float* scratch, int B, int H, int W, int C,
                                       int dtype, hipStream_t stream) {
  if (C % 32 == 0) {
    if (dtype == CRNN_BF16) return dwconv_wgrad_launch<bf16_t>((const bf16_t*)x, (const bf16_t*)g, dk, scratch, B, H, W, C, stream);
    return dwconv_wgrad_launch<float>((const float*)x, (const float*)g, dk, scratch, B, H, W, C, stream);
  }
  if (dtype != CRNN_F32) return CRNN_ERR_UNSUPPORTED;
  if (C == 1) {  // first block: one channel, B*H*W pixels -> per-block partials [nblk][9], then the 2nd stage
    long npix = (long)B * H * W;
    int nblk = cdiv(npix, 2048); if (nblk > 1024) nblk = 1024;
    hipLaunchKernelGGL(dwconv_wgrad_c1_kernel, dim3(nblk), dim3(256), 0, stream, (const float*)x, (const float*)g, scratch, B, H, W);
    CRNN_LAUNCH_CHECK();
    return crnn_partials_sum(scratch, nblk, 9, dk, 1.f, stream);
  }
  hipLaunchKernelGGL(dwconv_naive_kernel<1>, dim3(9 * C), dim3(256), 0, stream, (const float*)x, nullptr, (const float*)g, dk, B, H, W, C, 0);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
