// fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact f32, == an fmaf chain).
//
// One kernel template serves every matmul-shaped op of the CRNN hot path:
//   NN  C[M,N] = A[M,K]  * B[K,N]      pointwise 1x1 conv fwd (utils.py:47), Dense fwd (utils.py:74,85,253,256),
//                                      RNN input GEMM, STN im2col convs (utils.py:249,251)
//   NT  C[M,N] = A[M,K]  * Bt[N,K]^T   data gradients (dX = dY * W^T)
//   TN  C[M,N] = At[K,M]^T * B[K,N]    weight gradients (dW = X^T * dY), reduction over the huge row
//                                      dimension split across workgroups (deterministic 2-stage sum)
// 128 x {128,64} x 32 block tile, 4 waves (64 lanes each), each wave owns 2x2 / 1x2 MFMA 32x32
// accumulators.  Operands are staged through LDS; "row-major-in-k" operands are stored
// [rows][BK+4] and read as ds_read_b128 (conflict-free: 144-B row stride), "k-major" operands are
// stored [BK][rows] and read as ds_read_b32.  The k order inside a BK chunk is permuted
// (k = 8*kk8 + 4*half + e) identically for A and B so one b128 read feeds four MFMAs.
// Workgroup ids are remapped so that tiles sharing the same A rows run on the same XCD (L2).
//
// This file also holds the second stages of a split reduction and the extern "C" entry points of the tile GEMM (all but crnn_split3_planes,
// which sits beside its kernel in gemm_planes.hip): an entry point describes its product as a TileGemm (gemm_tile.h) and the launcher of the
// product's kernel (here, gemm_bf16.hip, gemm_planes.hip) runs it.
#include "gemm_tile.h"

#define GBK 32
#define GLDM (GBK + 4)

template <bool KM, int ROWS>
__device__ __forceinline__ void load_tile(const float* __restrict__ X, int ld, int row0, int nrows_total,
                                          int k0, int kend, int vec, int tid, float4 (&r)[ROWS / 32]) {
  // ROWS x GBK tile -> ROWS*8 float4 -> ROWS/32 per thread (256 threads)
#pragma unroll
  for (int it = 0; it < ROWS / 32; ++it) {
    int idx = tid + it * 256;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!KM) {
      int row = idx >> 3, k4 = idx & 7;
      int gr = row0 + row, gk = k0 + 4 * k4;
      if (gr < nrows_total && gk < kend) {
        const float* p = X + (long)gr * ld + gk;
        if (vec) v = *reinterpret_cast<const float4*>(p);
        else {
          v.x = p[0];
          if (gk + 1 < kend) v.y = p[1];
          if (gk + 2 < kend) v.z = p[2];
          if (gk + 3 < kend) v.w = p[3];
        }
      }
    } else {
      int krow = idx / (ROWS / 4), c4 = idx % (ROWS / 4);
      int gk = k0 + krow, gc = row0 + 4 * c4;
      if (gk < kend && gc < nrows_total) {
        const float* p = X + (long)gk * ld + gc;
        if (vec) v = *reinterpret_cast<const float4*>(p);
        else {
          v.x = p[0];
          if (gc + 1 < nrows_total) v.y = p[1];
          if (gc + 2 < nrows_total) v.z = p[2];
          if (gc + 3 < nrows_total) v.w = p[3];
        }
      }
    }
    r[it] = v;
  }
}

template <bool KM, int ROWS>
__device__ __forceinline__ void store_tile(float* Xs, int tid, const float4 (&r)[ROWS / 32]) {
#pragma unroll
  for (int it = 0; it < ROWS / 32; ++it) {
    int idx = tid + it * 256;
    if (!KM) {
      int row = idx >> 3, k4 = idx & 7;
      *reinterpret_cast<float4*>(&Xs[row * GLDM + 4 * k4]) = r[it];
    } else {
      int krow = idx / (ROWS / 4), c4 = idx % (ROWS / 4);
      *reinterpret_cast<float4*>(&Xs[krow * ROWS + 4 * c4]) = r[it];
    }
  }
}

template <bool KM, int ROWS>
__device__ __forceinline__ void read_frag(const float* Xs, int r0, int kk8, int half, int l31, float (&f)[4]) {
  if (!KM) {
    float4 v = *reinterpret_cast<const float4*>(&Xs[(r0 + l31) * GLDM + kk8 * 8 + 4 * half]);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = Xs[(kk8 * 8 + 4 * half + e) * ROWS + r0 + l31];
  }
}

template <int BN, bool A_KM, bool B_KM>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmParams p) {
  constexpr int BM = 128;
  constexpr int WAVES_N = (BN == 128) ? 2 : 1;
  constexpr int WM = (BN == 128) ? 64 : 32;  // rows per wave
  constexpr int TM = WM / 32, TN = 2;        // MFMA tiles per wave (wave covers WM x 64)
  __shared__ __attribute__((aligned(16))) float smem[(BM + BN) * GLDM];
  float* As = smem;
  float* Bs = smem + BM * GLDM;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * 64;

  // XCD-aware bijective remap of the tile id (blocks b, b+8, ... share an L2)
  int nwg = gridDim.x, bid = blockIdx.x;
  int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
  int lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  const int tm = lid / p.tilesN, tn = lid % p.tilesN;
  const int m0 = tm * BM, n0 = tn * BN;

  const int kbeg = blockIdx.y * p.klen;
  const int kend = min(p.K, kbeg + p.klen);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  float4 ra[BM / 32], rb[BN / 32];
  load_tile<A_KM, BM>(p.A, p.lda, m0, p.M, kbeg, kend, p.vecA, tid, ra);
  load_tile<B_KM, BN>(p.B, p.ldb, n0, p.N, kbeg, kend, p.vecB, tid, rb);

  for (int k0 = kbeg; k0 < kend; k0 += GBK) {
    store_tile<A_KM, BM>(As, tid, ra);
    store_tile<B_KM, BN>(Bs, tid, rb);
    __syncthreads();
    if (k0 + GBK < kend) {  // prefetch the next chunk; in flight during the MFMAs below
      load_tile<A_KM, BM>(p.A, p.lda, m0, p.M, k0 + GBK, kend, p.vecA, tid, ra);
      load_tile<B_KM, BN>(p.B, p.ldb, n0, p.N, k0 + GBK, kend, p.vecB, tid, rb);
    }
#pragma unroll
    for (int kk8 = 0; kk8 < 4; ++kk8) {
      float fa[TM][4], fb[TN][4];
#pragma unroll
      for (int i = 0; i < TM; ++i) read_frag<A_KM, BM>(As, wm0 + i * 32, kk8, half, l31, fa[i]);
#pragma unroll
      for (int j = 0; j < TN; ++j) read_frag<B_KM, BN>(Bs, wn0 + j * 32, kk8, half, l31, fb[j]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  const bool split = gridDim.y > 1;
  float* Cout = split ? p.C + (long)blockIdx.y * p.M * p.N : p.C;
  const int ldc = split ? p.N : p.ldc;
  const int Q = p.permP ? p.M / p.permP : 0;
  // ---- epilogue: stage the accumulators through LDS (two 64-row halves) so that every lane stores 16
  // contiguous bytes (512 B per output row per wave) instead of 64 separate 4-byte-per-lane stores.
  constexpr int CLD = BN + 4;                      // padded row stride of the staged C half-tile
  constexpr int ROWS_PER_IT = 256 / (BN / 4);      // rows covered by the 256 threads per store iteration
  const bool vecC = p.vecC && !((ldc & 3) | (n0 & 3));
  float st_sum[TN], st_sq[TN];
  if (p.stats) tile_stats_regs<TM, TN>(acc, m0 + wm0, p.M, CRNN_F32, half, st_sum, st_sq);
#pragma unroll
  for (int hp = 0; hp < 2; ++hp) {
    if (wm0 >= 64 * hp && wm0 < 64 * hp + 64) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            smem[(wm0 - 64 * hp + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * half) * CLD + wn0 + j * 32 + l31] = acc[i][j][e];
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 64 / ROWS_PER_IT; ++it) {
      const int rl = it * ROWS_PER_IT + tid / (BN / 4), c4 = tid % (BN / 4);
      const int gm = m0 + 64 * hp + rl, gn = n0 + 4 * c4;
      if (gm < p.M && gn < p.N) {
        float4 v = *reinterpret_cast<const float4*>(&smem[rl * CLD + 4 * c4]);
        int orow = gm;
        if (!split && p.permP) orow = (gm % p.permP) * Q + gm / p.permP;
        float* dst = Cout + (long)orow * ldc + gn;
        float vv[4] = {v.x, v.y, v.z, v.w};
        if (!split) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (gn + e < p.N) {
              if (p.bias) vv[e] += p.bias[gn + e];
              if (p.act == 1) vv[e] = fmaxf(vv[e], 0.f);
              if (p.cscale) vv[e] = relu6f(fmaf(vv[e], p.cscale[gn + e], p.cshift[gn + e]));
            }
        }
        if (vecC && gn + 3 < p.N) {
          float4 o = make_float4(vv[0], vv[1], vv[2], vv[3]);
          if (!split && p.accumulate) { float4 c = *reinterpret_cast<const float4*>(dst); o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w; }
          *reinterpret_cast<float4*>(dst) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (gn + e < p.N) dst[e] = vv[e] + ((!split && p.accumulate) ? dst[e] : 0.f);
        }
      }
    }
    __syncthreads();
  }
  if (p.stats) tile_stats_finish<BN, TN, 4 / WAVES_N>(smem, p.stats, tm, n0, p.N, tid, wave / WAVES_N, wn0, half, l31, st_sum, st_sq);
}

// second stage of a split reduction: C = act(sum_z part[z] + bias) (+ C); fixed summation order (deterministic).
template <int LY>
__global__ __launch_bounds__(32 * LY) void gemm_splitk_reduce_kernel(const float* __restrict__ part, int nsplit, GemmParams p) {
  // blockDim (32, LY): 32 consecutive outputs x LY split-lanes (8 for short split lists, 32 for long ones), four
  // independent loads in flight per lane
  __shared__ float red[LY][33];
  const long total = (long)p.M * p.N;
  const long i = (long)blockIdx.x * 32 + threadIdx.x;
  float s = 0.f;
  if (i < total) {
    int z = threadIdx.y;
    for (; z + 3 * LY < nsplit; z += 4 * LY) {
      float v0 = part[(long)z * total + i], v1 = part[(long)(z + LY) * total + i];
      float v2 = part[(long)(z + 2 * LY) * total + i], v3 = part[(long)(z + 3 * LY) * total + i];
      s += (v0 + v1) + (v2 + v3);
    }
    for (; z < nsplit; z += LY) s += part[(long)z * total + i];
  }
  red[threadIdx.y][threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.y == 0 && i < total) {
    s = 0.f;
#pragma unroll
    for (int r = 0; r < LY; r += 4)
      s += (red[r][threadIdx.x] + red[r + 1][threadIdx.x]) + (red[r + 2][threadIdx.x] + red[r + 3][threadIdx.x]);
    int m = (int)(i / p.N), n = (int)(i % p.N);
    if (p.bias) s += p.bias[n];
    if (p.act == 1) s = fmaxf(s, 0.f);
    int orow = m;
    if (p.permP) orow = (m % p.permP) * (p.M / p.permP) + m / p.permP;
    if (p.dtC == CRNN_BF16) {
      bf16_t* dst = reinterpret_cast<bf16_t*>(p.C) + (long)orow * p.ldc + n;
      if (p.accumulate) s += ld1(dst);
      st1(dst, s);
    } else {
      float* dst = p.C + (long)orow * p.ldc + n;
      if (p.accumulate) s += *dst;
      *dst = s;
    }
  }
}
// The same second stage for the common case -- at most 8 partial results, fp32 result, N % 4 == 0 and 16-byte aligned rows: one thread sums
// four consecutive outputs over the splits in registers (the partial lists are 7 - 55 MB: the LDS-combining form above moved 32 outputs
// per 256-thread workgroup and ran dense1's forward reduction at a quarter of the memory bandwidth).  Fixed order: ((p0+p1)+(p2+p3)) +
// ((p4+p5)+(p6+p7)), absent partials count as zero.
__global__ __launch_bounds__(256) void gemm_splitk_reduce8_kernel(const float* __restrict__ part, int nsplit, GemmParams p) {
  const long total4 = ((long)p.M * p.N) >> 2;
  const long i4 = (long)blockIdx.x * 256 + threadIdx.x;
  if (i4 >= total4) return;
  const float4* src = reinterpret_cast<const float4*>(part);
  float4 v[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) v[z] = z < nsplit ? src[(long)z * total4 + i4] : make_float4(0.f, 0.f, 0.f, 0.f);
  float s[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float a0 = (&v[0].x)[e], a1 = (&v[1].x)[e], a2 = (&v[2].x)[e], a3 = (&v[3].x)[e];
    const float a4 = (&v[4].x)[e], a5 = (&v[5].x)[e], a6 = (&v[6].x)[e], a7 = (&v[7].x)[e];
    s[e] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
  }
  const long i = i4 << 2;
  const int m = (int)(i / p.N), n = (int)(i % p.N);
  if (p.bias) { const float4 b = *reinterpret_cast<const float4*>(p.bias + n); s[0] += b.x; s[1] += b.y; s[2] += b.z; s[3] += b.w; }
  if (p.act == 1) { s[0] = fmaxf(s[0], 0.f); s[1] = fmaxf(s[1], 0.f); s[2] = fmaxf(s[2], 0.f); s[3] = fmaxf(s[3], 0.f); }
  int orow = m;
  if (p.permP) orow = (m % p.permP) * (p.M / p.permP) + m / p.permP;
  float4* dst = reinterpret_cast<float4*>(p.C + (long)orow * p.ldc + n);
  if (p.accumulate) { const float4 c = *dst; s[0] += c.x; s[1] += c.y; s[2] += c.z; s[3] += c.w; }
  *dst = make_float4(s[0], s[1], s[2], s[3]);
}

namespace crnn_tile {

// launches the matching second stage
void launch_splitk_reduce(const float* scratch, int nsplit, const GemmParams& p, hipStream_t stream) {
  const long total = (long)p.M * p.N;
  const bool vec = nsplit <= 8 && p.dtC == CRNN_F32 && (p.N & 3) == 0 && (p.ldc & 3) == 0 && !(((uintptr_t)p.C | (uintptr_t)scratch) & 15) &&
                   (!p.bias || !((uintptr_t)p.bias & 15));
  if (vec) hipLaunchKernelGGL(gemm_splitk_reduce8_kernel, dim3(cdiv(total >> 2, 256)), dim3(256), 0, stream, scratch, nsplit, p);
  else if (nsplit > 32) hipLaunchKernelGGL(gemm_splitk_reduce_kernel<32>, dim3(cdiv(total, 32)), dim3(32, 32), 0, stream, scratch, nsplit, p);
  else hipLaunchKernelGGL(gemm_splitk_reduce_kernel<8>, dim3(cdiv(total, 32)), dim3(32, 8), 0, stream, scratch, nsplit, p);
}

// (BN, mode) -> the instantiation
template <int BN>
static void (*f32_kernel(int mode))(GemmParams) {
  return mode == 0 ? gemm_f32_kernel<BN, false, true> : mode == 1 ? gemm_f32_kernel<BN, false, false> : gemm_f32_kernel<BN, true, true>;
}
// fp32 tensors only, no prologue; a split stays a 2-D grid (the kernel has no XCD-pinned form)
int gemm_tile_f32(const TileGemm& g) {
  if (g.dtA != CRNN_F32 || g.dtB != CRNN_F32 || g.dtC != CRNN_F32 || g.ascale || g.ashift || g.bnb) return CRNN_ERR_ARG;
  TilePlan t;
  CRNN_TRY(plan_tile_gemm(g, GBK, kSplitWorkgroups, false, false, t));
  hipLaunchKernelGGL(t.BN == 128 ? f32_kernel<128>(g.mode) : f32_kernel<64>(g.mode), t.grid, dim3(256), 0, g.stream, t.pk);
  return finish_tile_gemm(g, t);
}

}  // namespace crnn_tile

using crnn_tile::TileGemm;
using crnn_tile::gemm_tile;

// operands and shapes of a product; everything else an entry point sets by name
static TileGemm tile_gemm(crnn_tile::Product product, int mode, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                          hipStream_t stream) {
  TileGemm g;
  g.product = product; g.mode = mode; g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.stream = stream;
  return g;
}
// the epilogue options and the scratch of crnn_gemm_f32's argument list (shared by the crnn_gemm_* entry points)
static int gemm_with_options(TileGemm g, const float* bias, int act, int accumulate, int permP, float* scratch, size_t scratch_bytes) {
  g.bias = bias; g.act = act; g.accumulate = accumulate; g.permP = permP; g.scratch = scratch; g.scratch_bytes = scratch_bytes;
  return gemm_tile(g);
}

// mode: 0 = NN, 1 = NT, 2 = TN.  `scratch` (scratch_bytes) is needed only when the reduction is split
// (mode 2 with few output tiles); pass nullptr/0 to forbid splitting.
extern "C" int crnn_gemm_f32(int mode, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb,
                             int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                             size_t scratch_bytes, hipStream_t stream) {
  return gemm_with_options(tile_gemm(crnn_tile::PRODUCT_F32, mode, A, B, C, M, N, K, lda, ldb, ldc, stream), bias, act, accumulate, permP, scratch, scratch_bytes);
}
// Same contract (include/crnn_mi355x.h); products in bf16, accumulation in fp32.  dtA/dtB/dtC give
// the storage of A, B and C (CRNN_F32 | CRNN_BF16); leading dimensions are in elements of the respective type.
extern "C" int crnn_gemm_bf16_ex(int mode, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb,
                                 int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                                 size_t scratch_bytes, int dtA, int dtB, int dtC, hipStream_t stream) {
  TileGemm g = tile_gemm(crnn_tile::PRODUCT_BF16, mode, A, B, C, M, N, K, lda, ldb, ldc, stream);
  g.dtA = dtA; g.dtB = dtB; g.dtC = dtC;
  return gemm_with_options(g, bias, act, accumulate, permP, scratch, scratch_bytes);
}
extern "C" int crnn_gemm_bf16(int mode, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb,
                              int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                              size_t scratch_bytes, hipStream_t stream) {
  return crnn_gemm_bf16_ex(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, accumulate, permP, scratch, scratch_bytes, CRNN_F32, CRNN_F32,
                           CRNN_F32, stream);
}
// fp32 in, fp32 out, fp32-accurate products from three bf16 planes per operand (six bf16 MFMAs per k-step instead of the eight four-times
// slower fp32 ones): the contract of crnn_gemm_f32 with results equal to it to fp32 round-off (not bit for bit) -- the conv-stack / dense /
// RNN-projection GEMMs of the parity mode (unless crnn_config.flags has CRNN_FLAG_F32_MFMA_GEMMS).
extern "C" int crnn_gemm_f32x3(int mode, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb,
                               int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                               size_t scratch_bytes, hipStream_t stream) {
  return gemm_with_options(tile_gemm(crnn_tile::PRODUCT_PLANES3, mode, A, B, C, M, N, K, lda, ldb, ldc, stream), bias, act, accumulate, permP, scratch, scratch_bytes);
}
// crnn_gemm_f32x3 with two planes per operand (hi*hi + hi*mid + mid*hi: 16 significant bits per factor): same contract
extern "C" int crnn_gemm_f32x2(int mode, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb,
                               int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                               size_t scratch_bytes, hipStream_t stream) {
  return gemm_with_options(tile_gemm(crnn_tile::PRODUCT_PLANES2, mode, A, B, C, M, N, K, lda, ldb, ldc, stream), bias, act, accumulate, permP, scratch, scratch_bytes);
}
// crnn_gemm_f32x3 mode 1 for the data gradient da = dq . W^T of a depthwise-separable block in the parity mode (utils.py:45-49 backwards) that also takes
// the statistics pass of the BatchNorm in front of the pointwise convolution: stat_partials [M / 128][2][N] = per-tile column sums of gy and gy * xhat,
// gy = da where 0 < d * scale + shift < 6, xhat = (d - mean) / sqrt(var + eps); d [M][N] fp32 = that BatchNorm's input, bnstate = [mean|var|scale|shift] x N.
// Feed the partials to crnn_bn_bwd_finalize_folded, apply with crnn_bn_bwd_apply_ex.  Whole tiles only (M % 128 == 0, N % 64 == 0, K % 64 == 0,
// 16-byte aligned operands): -3 otherwise (run crnn_bn_bwd_ex).  da equals crnn_gemm_f32x3's bit for bit; the sums are those of the stand-alone pass in another order.
extern "C" int crnn_gemm_f32x3_bnstats_supported(long M, int N, int K) {
  return (M > 0 && M <= 0x7fffffffL && M % 128 == 0 && N % 64 == 0 && (N <= 64 || N % 128 == 0) && K % HBK == 0) ? CRNN_OK : CRNN_ERR_UNSUPPORTED;
}
extern "C" int crnn_gemm_f32x3_bnstats_rows(long M) { return (int)(M / 128); }
static int gemm_planes_bnstats(crnn_tile::Product product, const float* dq, const float* W, float* da, long M, int N, int K, const float* d, const float* bnstate,
                               float* stat_partials, hipStream_t stream) {
  CRNN_TRY(crnn_gemm_f32x3_bnstats_supported(M, N, K));
  // the query is the whole shape rule (dense operands, no scratch: every tile and chunk whole, one reduction range); the unguarded epilogue's 16-byte accesses are the other
  if (N <= 0 || K <= 0 || !d || !bnstate || !stat_partials) return CRNN_ERR_ARG;
  if ((((uintptr_t)dq | (uintptr_t)W | (uintptr_t)da | (uintptr_t)d | (uintptr_t)bnstate) & 15)) return CRNN_ERR_UNSUPPORTED;
  const crnn_tile::BnBwdEpilogue e{d, N, bnstate, stat_partials};
  TileGemm g = tile_gemm(product, 1, dq, W, da, (int)M, N, K, K, K, N, stream);
  g.bnb = &e;
  return gemm_tile(g);
}
extern "C" int crnn_gemm_f32x3_bnstats(const float* dq, const float* W, float* da, long M, int N, int K, const float* d, const float* bnstate,
                                       float* stat_partials, hipStream_t stream) {
  return gemm_planes_bnstats(crnn_tile::PRODUCT_PLANES3, dq, W, da, M, N, K, d, bnstate, stat_partials, stream);
}
// Two-plane form of crnn_gemm_f32x3_bnstats: operands split into two bf16 planes, products hi*hi + hi*mid + mid*hi (16 significant bits per factor,
// fp32 accumulation; relative error of a product <= 3 * 2^-18): half the MFMA work.  The parity mode's default for the BACKWARD GEMMs of the conv stack.
extern "C" int crnn_gemm_f32x2_bnstats(const float* dq, const float* W, float* da, long M, int N, int K, const float* d, const float* bnstate,
                                       float* stat_partials, hipStream_t stream) {
  return gemm_planes_bnstats(crnn_tile::PRODUCT_PLANES2, dq, W, da, M, N, K, d, bnstate, stat_partials, stream);
}

// ---- pointwise 1x1 convolution = GEMM over the pixels, with the next BatchNorm's statistics from the epilogue
extern "C" int crnn_pwconv_stat_rows(long M) { return cdiv(M, 128); }
extern "C" int crnn_pwconv_fwd(const void* a, const void* w, void* q, long M, int N, int K, float* stat_partials,
                               const float* out_bnstate, int bf16_products, int dt_a, int dt_w, int dt_q, int w_transposed,
                               hipStream_t stream) {
  if (M <= 0 || M > 0x7fffffffL) return CRNN_ERR_ARG;
  // bf16_products: 0 = fp32 MFMA; 1 = bf16; fp32 tensors only: 2 = fp32-accurate three-plane bf16 products (crnn_gemm_f32x3), 3 = two planes (crnn_gemm_f32x2)
  const crnn_tile::Product product = bf16_products == 2 ? crnn_tile::PRODUCT_PLANES3 : bf16_products == 3 ? crnn_tile::PRODUCT_PLANES2
                                     : bf16_products ? crnn_tile::PRODUCT_BF16 : crnn_tile::PRODUCT_F32;
  if (product == crnn_tile::PRODUCT_F32 && (dt_a != CRNN_F32 || dt_w != CRNN_F32 || dt_q != CRNN_F32)) return CRNN_ERR_ARG;
  // w_transposed: the weights are given as W^T [N][K] (both operands then contiguous along the reduction: the staging
  // needs no k-pair interleave and the fragments are single 16-byte LDS reads)
  TileGemm g = tile_gemm(product, w_transposed ? 1 : 0, a, w, q, (int)M, N, K, K, w_transposed ? K : N, N, stream);
  g.dtA = dt_a; g.dtB = dt_w; g.dtC = dt_q;
  g.stats = stat_partials;
  // out_bnstate ([mean|var|scale|shift] of the BatchNorm after the conv, inference): q = ReLU6(product * scale + shift)
  if (out_bnstate) { g.cscale = out_bnstate + 2L * N; g.cshift = out_bnstate + 3L * N; }
  return gemm_tile(g);
}

// The same convolution fed by the PRE-BatchNorm depthwise output d: the operand is ReLU6(BN(d)) (utils.py:45-46), formed per element
// while the tile is staged (GemmParams::ascale/ashift), so the activated tensor is never written.  in_bnstate = [mean|var|scale|shift] x K.
// forward: q [M][N] = ReLU6(BN(d [M][K])) . w;  weight gradient: dw [K][N] = ReLU6(BN(d))^T [K][M] . g [M][N] (fp32 result)
static int pwconv_bnrelu6_fwd(crnn_tile::Product product, int dt, const void* d, const float* in_bnstate, const void* w, void* q, long M, int N, int K,
                              float* stat_partials, int dt_q, int w_transposed, hipStream_t stream) {
  if (M <= 0 || M > 0x7fffffffL || !in_bnstate) return CRNN_ERR_ARG;
  TileGemm g = tile_gemm(product, w_transposed ? 1 : 0, d, w, q, (int)M, N, K, K, w_transposed ? K : N, N, stream);
  g.dtA = g.dtB = dt; g.dtC = dt_q;
  g.stats = stat_partials;
  g.ascale = in_bnstate + 2L * K; g.ashift = in_bnstate + 3L * K;
  return gemm_tile(g);
}
static int pwconv_bnrelu6_wgrad(crnn_tile::Product product, int dt, const void* d, const float* in_bnstate, const void* gy, float* dw, long M, int N, int K,
                                float* scratch, size_t scratch_bytes, hipStream_t stream) {
  if (M <= 0 || M > 0x7fffffffL || !in_bnstate) return CRNN_ERR_ARG;
  TileGemm g = tile_gemm(product, 2, d, gy, dw, K, N, (int)M, K, N, N, stream);
  g.dtA = g.dtB = dt;
  g.scratch = scratch; g.scratch_bytes = scratch_bytes;
  g.ascale = in_bnstate + 2L * K; g.ashift = in_bnstate + 3L * K;
  return gemm_tile(g);
}
// bf16 tensors d, w, g (the bf16 kernel's prologue)
extern "C" int crnn_pwconv_bnrelu6_fwd(const void* d, const float* in_bnstate, const void* w, void* q, long M, int N, int K,
                                       float* stat_partials, int dt_q, int w_transposed, hipStream_t stream) {
  return pwconv_bnrelu6_fwd(crnn_tile::PRODUCT_BF16, CRNN_BF16, d, in_bnstate, w, q, M, N, K, stat_partials, dt_q, w_transposed, stream);
}
extern "C" int crnn_pwconv_bnrelu6_wgrad(const void* d, const float* in_bnstate, const void* g, float* dw, long M, int N, int K,
                                         float* scratch, size_t scratch_bytes, hipStream_t stream) {
  return pwconv_bnrelu6_wgrad(crnn_tile::PRODUCT_BF16, CRNN_BF16, d, in_bnstate, g, dw, M, N, K, scratch, scratch_bytes, stream);
}
// Parity mode (fp32 tensors, plane products): the staging waves of the plane kernel apply ReLU6(d * scale[ch] + shift[ch]) (the arithmetic of
// crnn_bn_act_pool_drop_ex, bit for bit) to the raw items before the plane split.  Results equal crnn_bn_act_pool_drop_ex + crnn_pwconv_fwd(bf16_products = 2 | 3) /
// crnn_gemm_f32x3 | crnn_gemm_f32x2 mode 2 bit for bit.  w [K][N] fp32 (K <= 512); -3 for shapes outside the kernel's rules.
// f32x2: two planes (hi*hi + hi*mid + mid*hi: 16 significant bits per factor; crnn_gemm_f32x2_bnstats)
extern "C" int crnn_pwconv_bnrelu6_fwd_f32x3(const float* d, const float* in_bnstate, const float* w, float* q, long M, int N, int K,
                                             float* stat_partials, hipStream_t stream) {
  return pwconv_bnrelu6_fwd(crnn_tile::PRODUCT_PLANES3, CRNN_F32, d, in_bnstate, w, q, M, N, K, stat_partials, CRNN_F32, 0, stream);
}
extern "C" int crnn_pwconv_bnrelu6_fwd_f32x2(const float* d, const float* in_bnstate, const float* w, float* q, long M, int N, int K,
                                             float* stat_partials, hipStream_t stream) {
  return pwconv_bnrelu6_fwd(crnn_tile::PRODUCT_PLANES2, CRNN_F32, d, in_bnstate, w, q, M, N, K, stat_partials, CRNN_F32, 0, stream);
}
extern "C" int crnn_pwconv_bnrelu6_wgrad_f32x3(const float* d, const float* in_bnstate, const float* g, float* dw, long M, int N, int K,
                                               float* scratch, size_t scratch_bytes, hipStream_t stream) {
  return pwconv_bnrelu6_wgrad(crnn_tile::PRODUCT_PLANES3, CRNN_F32, d, in_bnstate, g, dw, M, N, K, scratch, scratch_bytes, stream);
}
extern "C" int crnn_pwconv_bnrelu6_wgrad_f32x2(const float* d, const float* in_bnstate, const float* g, float* dw, long M, int N, int K,
                                               float* scratch, size_t scratch_bytes, hipStream_t stream) {
  return pwconv_bnrelu6_wgrad(crnn_tile::PRODUCT_PLANES2, CRNN_F32, d, in_bnstate, g, dw, M, N, K, scratch, scratch_bytes, stream);
}
