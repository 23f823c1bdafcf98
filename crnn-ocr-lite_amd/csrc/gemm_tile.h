// The tile GEMM's shared part: what one launch is (TileGemm), how it is cut into workgroups (plan_tile_gemm), the kernel parameter block
// (GemmParams) and the device helpers the tile kernels have in common -- statistics and tile epilogues, the workgroup-id mapping, the
// bf16 fragment read.  Three translation units build on it:
//   gemm.hip         fp32 MFMA kernel (the parity reference), the split-reduction second stages, the extern "C" entry points that dispatch
//   gemm_bf16.hip    bf16 MFMA kernel with its loaders and the producer prologue
//   gemm_planes.hip  products from two / three bf16 planes on producer waves, crnn_split3_planes
#pragma once
#include "common.h"
#include "stream_ops.h"

#define HBK 64                 // fp32 k per chunk of the bf16-family kernels
#define HLD (HBK + 8)          // bf16 row stride of the row-major-in-k layout (144 B)
#define KLD(ROWS) ((ROWS) + 32)   // bf16 row stride of the k-major layout (pad 32 = 64 B: the transposing fragment reads stay conflict-free)
#define TR_TAB 512             // channels the prologue's LDS table holds (K <= 512 in modes 0/1; the 128 tile rows in mode 2)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct GemmParams {
  const float* A; const float* B; float* C;
  int M, N, K;
  int lda, ldb, ldc;
  const float* bias;
  int act;         // 0 none, 1 relu
  int accumulate;  // C += result
  int permP;       // 0: none; else out_row = (m % P) * (M / P) + m / P
  int klen;        // K range per split (blockIdx.y); nsplit = gridDim.y
  int vecA, vecB;  // 16-byte vector loads legal for the operand
  int vecC;        // 16-byte stores legal for C (and the split scratch)
  int dtA, dtB, dtC;  // storage of the operands / result (CRNN_F32 | CRNN_BF16); the fp32 kernel requires all CRNN_F32
  int tilesN;
  int xsplit;      // > 0: 1-D grid of tiles * xsplit workgroups, K split xsplit-fold with split s on XCD s % 8 (all tiles of one K range
                   // share an L2): id -> xcd = id & 7, tile = (id >> 3) % tiles, split = ((id >> 3) / tiles) * 8 + xcd.  0: 2-D grid (tile, split)
  float* stats;    // optional [tilesM][2][N]: per-tile column sums / sums of squares of the result as stored (BatchNorm statistics)
  const float* cscale; const float* cshift;   // optional per-column epilogue  C = ReLU6(C * cscale[n] + cshift[n])  (inference BatchNorm folded in)
  // optional producer prologue on A (bf16 kernel, bf16 A): the operand the MFMA sees is ReLU6(A * ascale[ch] + ashift[ch])
  // rounded to bf16, ch = the reduction index (modes 0/1) or the A row (mode 2): the BatchNorm + ReLU6 between a depthwise
  // and a pointwise convolution, applied while the tile is staged instead of in a pass of its own
  const float* ascale; const float* ashift;
  // optional BatchNorm-BACKWARD statistics from the epilogue (bf16-family tile kernels, fp32 result, whole tiles): C is the gradient da that arrives at
  // a ReLU6(BatchNorm(d)); bnpart [tilesM][2][N] = per-tile column sums of gy and gy * xhat, gy = C where 0 < d * scale + shift < 6,
  // xhat = (d - mean) / sqrt(var + eps); bnD [M][ldd] fp32 = d, bnstate = [mean | var | scale | shift] x N
  const float* bnD; int ldd; const float* bnstate; float* bnpart;
};

// ---- statistics epilogue: per-tile column sums / sums of squares of the result as it will be stored, taken straight
// from the MFMA accumulators (a lane owns one column of each 32x32 block: 16 rows x TM blocks per column block), then
// combined across the two lane halves (shuffle) and the waves stacked along M (LDS), all in a fixed order.
typedef float f32x16_stats __attribute__((ext_vector_type(16)));
template <int TM, int TN>
__device__ __forceinline__ void tile_stats_regs(const f32x16_stats (&acc)[TM][TN], int row_base, int M, int dtC, int half,
                                                float (&ssum)[TN], float (&ssq)[TN]) {
  const bool full = row_base + TM * 32 <= M;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    float s0 = 0.f, s1 = 0.f, q0 = 0.f, q1 = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float v = acc[i][j][e];
        if (dtC == CRNN_BF16) v = __uint_as_float(pack2_bf16(v, 0.f) << 16);   // the value the consumer reads back
        if (!full && row_base + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * half >= M) v = 0.f;
        if (e & 1) { s1 += v; q1 = fmaf(v, v, q1); } else { s0 += v; q0 = fmaf(v, v, q0); }
      }
    float sv = s0 + s1, qv = q0 + q1;
    sv += __shfl_xor(sv, 32, 64); qv += __shfl_xor(qv, 32, 64);
    ssum[j] = sv; ssq[j] = qv;
  }
}
// smem: [2][WAVES_M][BN]; lanes of half 0 deposit their wave's column sums, then one thread per (stat, column) adds the waves
template <int BN, int TN, int WAVES_M>
__device__ __forceinline__ void tile_stats_finish(float* smem, float* stats, int tm, int n0, int N, int tid, int wmi, int wn0,
                                                  int half, int l31, const float (&ssum)[TN], const float (&ssq)[TN]) {
  if (half == 0) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      smem[(0 * WAVES_M + wmi) * BN + wn0 + j * 32 + l31] = ssum[j];
      smem[(1 * WAVES_M + wmi) * BN + wn0 + j * 32 + l31] = ssq[j];
    }
  }
  __syncthreads();
  if (tid < 2 * BN) {
    const int v = tid / BN, c = tid % BN;
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < WAVES_M; ++q) a += smem[(v * WAVES_M + q) * BN + c];
    if (n0 + c < N) stats[((long)tm * 2 + v) * N + n0 + c] = a;
  }
}

// ---- workgroup id -> (tile row, tile column, K range) of the bf16-family kernels.  Unsplit or 2-D split (xsplit == 0): an XCD-aware
// bijective remap of the tile id (blocks b, b+8, ... share an L2), K range = blockIdx.y.  xsplit > 0: split reduction over a huge K
// (weight gradients): every K range lives on ONE XCD, where all output tiles of that range run together and share the operand rows
// through its L2 (the rows are read from HBM once instead of once per tile row / column).
struct TileCoord { int tm, tn, ksplit; };
__device__ __forceinline__ TileCoord gemm_tile_coord(const GemmParams& p) {
  int lid, ksplit;
  if (p.xsplit > 0) {
    const int bid = blockIdx.x, ntile = gridDim.x / p.xsplit, rest = bid >> 3;
    lid = rest % ntile; ksplit = (rest / ntile) * 8 + (bid & 7);
  } else {
    int nwg = gridDim.x, bid = blockIdx.x;
    int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
    lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    ksplit = blockIdx.y;
  }
  return {lid / p.tilesN, lid % p.tilesN, ksplit};
}

// fragment = the 8 bf16 (k = 16*ks + 8*half .. +7) of row r0 + l31
template <bool KM, int ROWS>
__device__ __forceinline__ bf16x8 read_frag_h(const void* Xs, int r0, int ks, int half, int l31) {
  uint4 w;
  if (!KM) {
    w = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(Xs) + (r0 + l31) * HLD + ks * 16 + 8 * half);
  } else {
    // 16-lane group (l31 >> 4, half): lane li supplies the address of 4 of the group's 16 rows at k-row li >> 2 and receives the
    // 4 k of row li after the transpose (ds_read_b64_tr_b16); two reads = the fragment's 8 k
    const int li = l31 & 15;
    const unsigned short* X = reinterpret_cast<const unsigned short*>(Xs) + (ks * 16 + 8 * half + (li >> 2)) * KLD(ROWS) + r0 + (l31 & 16) + (li & 3) * 4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)X);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(X + 4 * KLD(ROWS)));
    const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
    w = make_uint4(a.x, a.y, b.x, b.y);
  }
  return __builtin_bit_cast(bf16x8, w);
}

// ---- epilogue shared by the tile kernels of this file: the accumulators of the workgroup's 128 x BN tile (4 MFMA waves = threads 0..255,
// wave w at rows wm0, columns wn0) go through LDS and leave as 16-byte stores with bias / ReLU / folded BatchNorm / row permutation /
// accumulate, or as a split-reduction partial; optional per-tile BatchNorm statistics.  Callers: every thread of the four MFMA waves.
template <int BN, int TM, int TN, bool FULL, bool BNB = false>
__device__ __forceinline__ void gemm_tile_epilogue(const GemmParams& p, f32x16 (&acc)[TM][TN], unsigned char* smem_raw, int tid, int m0, int n0, int tm,
                                                   int wm0, int wn0, int ksplit) {
  constexpr int WAVES_N = (BN == 128) ? 2 : 1;
  const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  // ---- epilogue (same as gemm.hip): stage through LDS, 16-byte stores
  float* smem = reinterpret_cast<float*>(smem_raw);
  const bool split = gridDim.y > 1 || p.xsplit > 1;
  float* Cout = split ? p.C + (long)ksplit * p.M * p.N : p.C;
  const int ldc = split ? p.N : p.ldc;
  const int Q = p.permP ? p.M / p.permP : 0;
  constexpr int CLD = BN + 4;
  constexpr int ROWS_PER_IT = 256 / (BN / 4);
  const bool vecC = p.vecC && !((ldc & 3) | (n0 & 3));
  float st_sum[TN], st_sq[TN];
  if (p.stats) tile_stats_regs<TM, TN>(acc, m0 + wm0, p.M, p.dtC, half, st_sum, st_sq);
  // FULL: the per-column epilogue operands of this thread's columns (fixed over its rows), loaded once
  const bool path8 = !split && p.dtC == CRNN_BF16 && vecC;
  float4 hb[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)}, hs[2] = {hb[0], hb[0]}, hh[2] = {hb[0], hb[0]};
  if constexpr (FULL) {
    const int gnf = path8 ? n0 + 8 * (tid % (BN / 8)) : n0 + 4 * (tid % (BN / 4));
    if (!split && p.bias) { hb[0] = *reinterpret_cast<const float4*>(p.bias + gnf); if (path8) hb[1] = *reinterpret_cast<const float4*>(p.bias + gnf + 4); }
    if (!split && p.cscale) {
      hs[0] = *reinterpret_cast<const float4*>(p.cscale + gnf); hh[0] = *reinterpret_cast<const float4*>(p.cshift + gnf);
      if (path8) { hs[1] = *reinterpret_cast<const float4*>(p.cscale + gnf + 4); hh[1] = *reinterpret_cast<const float4*>(p.cshift + gnf + 4); }
    }
  }
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
    if (path8) {   // bf16 result, 8 columns (one 16-byte store) per thread
      constexpr int RPI8 = 256 / (BN / 8);
#pragma unroll
      for (int it = 0; it < 64 / RPI8; ++it) {
        const int rl = it * RPI8 + tid / (BN / 8), c8 = tid % (BN / 8);
        const int gm = m0 + 64 * hp + rl, gn = n0 + 8 * c8;
        if (FULL || (gm < p.M && gn < p.N)) {
          float8 v;
          v.lo = *reinterpret_cast<const float4*>(&smem[rl * CLD + 8 * c8]);
          v.hi = *reinterpret_cast<const float4*>(&smem[rl * CLD + 8 * c8 + 4]);
          if (p.bias) {
            float4 b0 = hb[0], b1 = hb[1];
            if constexpr (!FULL) { b0 = *reinterpret_cast<const float4*>(p.bias + gn); b1 = *reinterpret_cast<const float4*>(p.bias + gn + 4); }
            v.lo.x += b0.x; v.lo.y += b0.y; v.lo.z += b0.z; v.lo.w += b0.w; v.hi.x += b1.x; v.hi.y += b1.y; v.hi.z += b1.z; v.hi.w += b1.w;
          }
          if (p.act == 1) {
            v.lo.x = fmaxf(v.lo.x, 0.f); v.lo.y = fmaxf(v.lo.y, 0.f); v.lo.z = fmaxf(v.lo.z, 0.f); v.lo.w = fmaxf(v.lo.w, 0.f);
            v.hi.x = fmaxf(v.hi.x, 0.f); v.hi.y = fmaxf(v.hi.y, 0.f); v.hi.z = fmaxf(v.hi.z, 0.f); v.hi.w = fmaxf(v.hi.w, 0.f);
          }
          if (p.cscale) {   // inference BatchNorm + ReLU6 folded into the epilogue
            float4 s0 = hs[0], s1 = hs[1], h0 = hh[0], h1 = hh[1];
            if constexpr (!FULL) {
              s0 = *reinterpret_cast<const float4*>(p.cscale + gn); s1 = *reinterpret_cast<const float4*>(p.cscale + gn + 4);
              h0 = *reinterpret_cast<const float4*>(p.cshift + gn); h1 = *reinterpret_cast<const float4*>(p.cshift + gn + 4);
            }
            v.lo.x = relu6f(fmaf(v.lo.x, s0.x, h0.x)); v.lo.y = relu6f(fmaf(v.lo.y, s0.y, h0.y)); v.lo.z = relu6f(fmaf(v.lo.z, s0.z, h0.z)); v.lo.w = relu6f(fmaf(v.lo.w, s0.w, h0.w));
            v.hi.x = relu6f(fmaf(v.hi.x, s1.x, h1.x)); v.hi.y = relu6f(fmaf(v.hi.y, s1.y, h1.y)); v.hi.z = relu6f(fmaf(v.hi.z, s1.z, h1.z)); v.hi.w = relu6f(fmaf(v.hi.w, s1.w, h1.w));
          }
          const int orow = p.permP ? (gm % p.permP) * Q + gm / p.permP : gm;
          bf16_t* dst = reinterpret_cast<bf16_t*>(Cout) + (long)orow * ldc + gn;
          if (p.accumulate) {
            float8 c = ld8(dst);
            v.lo.x += c.lo.x; v.lo.y += c.lo.y; v.lo.z += c.lo.z; v.lo.w += c.lo.w; v.hi.x += c.hi.x; v.hi.y += c.hi.y; v.hi.z += c.hi.z; v.hi.w += c.hi.w;
          }
          st8(dst, v);
        }
      }
    } else
#pragma unroll
    for (int it = 0; it < 64 / ROWS_PER_IT; ++it) {
      const int rl = it * ROWS_PER_IT + tid / (BN / 4), c4 = tid % (BN / 4);
      const int gm = m0 + 64 * hp + rl, gn = n0 + 4 * c4;
      if constexpr (FULL) {   // whole tile, 16-byte accesses, the column operands already in registers; same arithmetic as below
        float4 v = *reinterpret_cast<const float4*>(&smem[rl * CLD + 4 * c4]);
        int orow = gm;
        if (!split && p.permP) orow = (gm % p.permP) * Q + gm / p.permP;
        if (!split) {
          if (p.bias) { v.x += hb[0].x; v.y += hb[0].y; v.z += hb[0].z; v.w += hb[0].w; }
          if (p.act == 1) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
          if (p.cscale) {
            v.x = relu6f(fmaf(v.x, hs[0].x, hh[0].x)); v.y = relu6f(fmaf(v.y, hs[0].y, hh[0].y));
            v.z = relu6f(fmaf(v.z, hs[0].z, hh[0].z)); v.w = relu6f(fmaf(v.w, hs[0].w, hh[0].w));
          }
        }
        if (!split && p.dtC == CRNN_BF16) {
          bf16_t* dst = reinterpret_cast<bf16_t*>(Cout) + (long)orow * ldc + gn;
          if (p.accumulate) { float4 c = ld4(dst); v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w; }
          st4(dst, v);
        } else {
          float* dst = Cout + (long)orow * ldc + gn;
          if (!split && p.accumulate) { float4 c = *reinterpret_cast<const float4*>(dst); v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w; }
          *reinterpret_cast<float4*>(dst) = v;
        }
      } else
      if (gm < p.M && gn < p.N) {
        float4 v = *reinterpret_cast<const float4*>(&smem[rl * CLD + 4 * c4]);
        int orow = gm;
        if (!split && p.permP) orow = (gm % p.permP) * Q + gm / p.permP;
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
        if (!split && p.dtC == CRNN_BF16) {      // bf16 result tensor
          bf16_t* dst = reinterpret_cast<bf16_t*>(Cout) + (long)orow * ldc + gn;
          if (vecC && gn + 3 < p.N) {
            float4 o = make_float4(vv[0], vv[1], vv[2], vv[3]);
            if (p.accumulate) { float4 c = ld4(dst); o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w; }
            st4(dst, o);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (gn + e < p.N) st1(dst + e, vv[e] + (p.accumulate ? ld1(dst + e) : 0.f));
          }
        } else {
          float* dst = Cout + (long)orow * ldc + gn;
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
    }
    __syncthreads();
  }
  if (p.stats) tile_stats_finish<BN, TN, 4 / WAVES_N>(smem, p.stats, tm, n0, p.N, tid, wave / WAVES_N, wn0, half, l31, st_sum, st_sq);
  if constexpr (BNB) {
    // BatchNorm-backward statistics of the tile just stored (FULL fp32 result, no split, checked by the launcher): a second pass over this thread's
    // own rows -- its stores, read back through the cache -- so that nothing of it is live while the accumulators are (the kernel is held to 128
    // VGPRs).  The arithmetic of bn_bwd_kernel<1> (no pooling, no dropout); [thread row][2][BN] partial sums through the (free) staging tile, then
    // one fixed-order sum per column: one partial row per tile row.
    constexpr int RPI = 256 / (BN / 4), RT = RPI;
    const int tr = tid / (BN / 4), c4 = tid % (BN / 4), gnb = n0 + 4 * c4;
    const float4 mu = *reinterpret_cast<const float4*>(p.bnstate + gnb), va = *reinterpret_cast<const float4*>(p.bnstate + p.N + gnb);
    const float4 sc = *reinterpret_cast<const float4*>(p.bnstate + 2 * p.N + gnb), sh = *reinterpret_cast<const float4*>(p.bnstate + 3 * p.N + gnb);
    const float bmu[4] = {mu.x, mu.y, mu.z, mu.w}, bsc[4] = {sc.x, sc.y, sc.z, sc.w}, bsh[4] = {sh.x, sh.y, sh.z, sh.w};
    const float binv[4] = {1.0f / sqrtf(va.x + BN_EPS), 1.0f / sqrtf(va.y + BN_EPS), 1.0f / sqrtf(va.z + BN_EPS), 1.0f / sqrtf(va.w + BN_EPS)};
    float bs[4] = {0.f, 0.f, 0.f, 0.f}, bq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int it = 0; it < 128 / RPI; ++it) {
      const long gm = m0 + it * RPI + tr;
      const float4 v = *reinterpret_cast<const float4*>(p.C + gm * p.ldc + gnb);
      const float4 dv = *reinterpret_cast<const float4*>(p.bnD + gm * p.ldd + gnb);
      const float de[4] = {dv.x, dv.y, dv.z, dv.w}, ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = fmaf(de[e], bsc[e], bsh[e]);
        const float gy = (t > 0.f && t < 6.f) ? ve[e] : 0.f;
        bs[e] += gy; bq[e] = fmaf(gy, (de[e] - bmu[e]) * binv[e], bq[e]);
      }
    }
    *reinterpret_cast<float4*>(&smem[(tr * 2 + 0) * BN + 4 * c4]) = make_float4(bs[0], bs[1], bs[2], bs[3]);
    *reinterpret_cast<float4*>(&smem[(tr * 2 + 1) * BN + 4 * c4]) = make_float4(bq[0], bq[1], bq[2], bq[3]);
    __syncthreads();
    if (tid < 2 * BN) {
      const int which = tid / BN, col = tid % BN;
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < RT; ++r) a += smem[(r * 2 + which) * BN + col];
      p.bnpart[((long)tm * 2 + which) * p.N + n0 + col] = a;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
namespace crnn_tile {

enum Product { PRODUCT_F32, PRODUCT_BF16, PRODUCT_PLANES2, PRODUCT_PLANES3 };   // fp32 MFMA | bf16 MFMA | two / three bf16 planes per fp32 operand
struct BnBwdEpilogue { const float* d; int ldd; const float* bnstate; float* partials; };   // GemmParams::bnD .. bnpart

// One tile GEMM.  mode: 0 = NN, 1 = NT, 2 = TN (crnn_gemm_f32's contract, include/crnn_mi355x.h); an entry point names what it uses.
struct TileGemm {
  Product product = PRODUCT_F32;
  int mode = 0;
  const void* A = nullptr; const void* B = nullptr; void* C = nullptr;
  int M = 0, N = 0, K = 0;
  int lda = 0, ldb = 0, ldc = 0;                              // in elements of the operand's storage type
  int dtA = CRNN_F32, dtB = CRNN_F32, dtC = CRNN_F32;         // storage (CRNN_F32 | CRNN_BF16)
  const float* bias = nullptr; int act = 0, accumulate = 0, permP = 0;
  float* scratch = nullptr; size_t scratch_bytes = 0;         // allows a split reduction (nullptr / 0 forbids it)
  float* stats = nullptr;                                     // GemmParams::stats
  const float* cscale = nullptr; const float* cshift = nullptr;   // folded inference BatchNorm
  const float* ascale = nullptr; const float* ashift = nullptr;   // producer prologue on A
  const BnBwdEpilogue* bnb = nullptr;                         // BatchNorm-backward statistics from the epilogue (planes, mode 1)
  hipStream_t stream = nullptr;
  bool planes() const { return product == PRODUCT_PLANES2 || product == PRODUCT_PLANES3; }
};

// What the launchers need: the parameter block of the reduction (p) and of the tile kernel (pk: C = the scratch when split), the grid.
struct TilePlan { GemmParams p, pk; int BN, nsplit; bool full; dim3 grid; };

// The schedule's constants (each was an environment knob of the measurement builds up to commit 137e5be; results under profiles/)
constexpr int kNarrowTileMaxN = 64;            // N up to here: 128 x 64 tiles, else 128 x 128
constexpr int kSplitWorkgroups = 768;          // workgroups a split reduction aims for: 3 resident per CU
constexpr int kPlanesSplitWorkgroups = 512;    // ... of the plane kernel: two per CU
constexpr bool kPlanesSmallSplit = true;       // plane products without a bias split from 512 k on when at most 128 tiles would run
constexpr bool kXcdPinnedSplit = true;         // 8 or more K ranges are pinned to XCDs
constexpr bool kWholeTileKernels = true;       // whole tiles with 16-byte accesses run the unguarded instantiations

static inline int aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// Argument checks, vector legality, tile width, tile counts and the split-K plan of one launch -- the same for the three kernels up to
// kchunk (k per chunk: 32 fp32, 64 otherwise), split_target, small_split (the planes-only rule above) and xcd_split (the fp32 kernel keeps
// a 2-D grid).  Returns CRNN_OK or the code the entry point returns with nothing launched.
static inline int plan_tile_gemm(const TileGemm& g, int kchunk, int split_target, bool small_split, bool xcd_split, TilePlan& t) {
  const int mode = g.mode, M = g.M, N = g.N, K = g.K;
  const bool planes = g.planes();
  if (M <= 0 || N <= 0 || K <= 0) return CRNN_ERR_ARG;
  if (g.bnb && (g.bias || g.act || g.accumulate || g.permP || g.stats || g.cscale || g.ascale || g.dtC != CRNN_F32 || !g.bnb->d || !g.bnb->bnstate || !g.bnb->partials)) return CRNN_ERR_ARG;
  if (planes && (g.dtA != CRNN_F32 || g.dtB != CRNN_F32)) return CRNN_ERR_ARG;   // plane products: fp32 operands
  if (planes && g.ascale && (mode == 1 || (mode == 0 && K > TR_TAB) || g.bnb)) return CRNN_ERR_UNSUPPORTED;   // producer prologue of the plane kernel: modes 0 and 2
  if (g.permP && (M % g.permP) != 0) return CRNN_ERR_ARG;
  if (g.stats && (g.bias || g.act || g.accumulate || g.permP || g.scratch || g.cscale)) return CRNN_ERR_ARG;   // statistics of the plain product only
  if (g.cscale && (g.scratch || g.accumulate || !g.cshift)) return CRNN_ERR_ARG;                               // no split reduction with the folded BatchNorm
  if ((g.ascale != nullptr) != (g.ashift != nullptr)) return CRNN_ERR_ARG;
  GemmParams& p = t.p;
  p.stats = g.stats; p.cscale = g.cscale; p.cshift = g.cshift; p.ascale = g.ascale; p.ashift = g.ashift;
  p.bnD = g.bnb ? g.bnb->d : nullptr; p.ldd = g.bnb ? g.bnb->ldd : 0; p.bnstate = g.bnb ? g.bnb->bnstate : nullptr; p.bnpart = g.bnb ? g.bnb->partials : nullptr;
  p.A = (const float*)g.A; p.B = (const float*)g.B; p.C = (float*)g.C; p.M = M; p.N = N; p.K = K; p.lda = g.lda; p.ldb = g.ldb; p.ldc = g.ldc;
  p.bias = g.bias; p.act = g.act; p.accumulate = g.accumulate; p.permP = g.permP;
  p.dtA = g.dtA; p.dtB = g.dtB; p.dtC = g.dtC;
  const bool a_km = (mode == 2), b_km = (mode != 1);
  // vector accesses: 16 bytes per lane (4 fp32 or 8 bf16 elements) over the contiguous extent of each operand: A: K (m-major) or M (k-major);
  // B: N (k-major) or K (n-major)
  auto vw = [](int dt) { return dt == CRNN_BF16 ? 8 : 4; };
  p.vecA = aligned16(g.A) && (g.lda % vw(g.dtA) == 0) && ((a_km ? M : K) % vw(g.dtA) == 0);
  p.vecB = aligned16(g.B) && (g.ldb % vw(g.dtB) == 0) && ((b_km ? N : K) % vw(g.dtB) == 0);
  p.vecC = aligned16(g.C) && (g.ldc % vw(g.dtC) == 0) && (N % vw(g.dtC) == 0) && (!g.scratch || aligned16(g.scratch));
  if (g.ascale && !planes) {   // producer prologue of the bf16 kernel: bf16 operands, 16-byte loads of A, channel table in LDS
    if (g.dtA != CRNN_BF16 || g.dtB != CRNN_BF16 || !p.vecA) return CRNN_ERR_UNSUPPORTED;
    if (mode != 2 && K > TR_TAB) return CRNN_ERR_UNSUPPORTED;
  }
  const int BN = (N <= kNarrowTileMaxN) ? 64 : 128;
  const int tilesM = cdiv(M, 128), tilesN = cdiv(N, BN);
  p.tilesN = tilesN;
  const int tiles = tilesM * tilesN;
  int nsplit = 1;
  // (small_split, round 6, plane products without a bias -- gradients: at most 128 tiles leave more than half of the CUs idle for three to six products per k-step: split
  // those too.  Products with a bias are forward layers: their summation order stays what it was at every batch size, so that an inference result does not change with it.)
  if (g.scratch && ((tiles < 256 && K >= 2048) || (tiles <= 16 && K >= 512) || (small_split && !g.bias && tiles <= 128 && K >= 512))) {
    nsplit = cdiv(split_target, tiles);
    int maxs = K / (K >= 2048 ? 512 : 128); if (maxs < 1) maxs = 1;
    if (nsplit > maxs) nsplit = maxs;
    size_t per = (size_t)M * N * sizeof(float);
    size_t fit = g.scratch_bytes / per;
    if ((size_t)nsplit > fit) nsplit = (int)fit;
    if (nsplit < 1) nsplit = 1;
  }
  int klen = cdiv(K, nsplit);
  klen = ((klen + kchunk - 1) / kchunk) * kchunk;
  nsplit = cdiv(K, klen);
  p.xsplit = 0;
  if (xcd_split && nsplit >= 8) {   // K ranges pinned to XCDs: the split count becomes a multiple of 8 (empty tail ranges write zeros)
    const int ns8 = ((nsplit + 7) / 8) * 8;
    if ((size_t)ns8 * M * N * sizeof(float) <= g.scratch_bytes) {
      klen = cdiv(K, ns8); klen = ((klen + kchunk - 1) / kchunk) * kchunk;
      nsplit = ns8; p.xsplit = ns8;
    }
  }
  p.klen = klen;
  t.pk = p;
  if (nsplit > 1) t.pk.C = g.scratch;
  t.BN = BN; t.nsplit = nsplit;
  t.grid = dim3(p.xsplit ? tiles * nsplit : tiles, p.xsplit ? 1 : nsplit);
  // every tile whole, every k-chunk whole, 16-byte accesses legal: the unguarded instantiation
  t.full = (M % 128 == 0) && (N % BN == 0) && (K % kchunk == 0) && p.vecA && p.vecB && p.vecC && kWholeTileKernels;
  if (g.bnb) {
    // the BatchNorm-backward statistics live in the unguarded epilogue of an unsplit product: whole tiles, 16-byte accesses to d and the state
    if (!t.full || nsplit > 1 || (g.bnb->ldd & 3) || ((uintptr_t)g.bnb->d & 15) || ((uintptr_t)g.bnb->bnstate & 15)) return CRNN_ERR_UNSUPPORTED;
    if (!planes || mode != 1) return CRNN_ERR_UNSUPPORTED;
  }
  return CRNN_OK;
}

// second stage of a split reduction (gemm.hip): C = act(sum of the nsplit partial results in scratch + bias) (+ C)
void launch_splitk_reduce(const float* scratch, int nsplit, const GemmParams& p, hipStream_t stream);
// what every launcher ends with: the tile kernel's launch status, then the second stage of a split reduction
static inline int finish_tile_gemm(const TileGemm& g, const TilePlan& t) {
  CRNN_LAUNCH_CHECK();
  if (t.nsplit > 1) {
    launch_splitk_reduce(g.scratch, t.nsplit, t.p, g.stream);
    CRNN_LAUNCH_CHECK();
  }
  return CRNN_OK;
}

// the three kernels' launchers (gemm.hip, gemm_bf16.hip, gemm_planes.hip) and the choice between them
int gemm_tile_f32(const TileGemm& g);
int gemm_tile_bf16(const TileGemm& g);
int gemm_tile_planes(const TileGemm& g);
static inline int gemm_tile(const TileGemm& g) {
  return g.product == PRODUCT_F32 ? gemm_tile_f32(g) : g.product == PRODUCT_BF16 ? gemm_tile_bf16(g) : gemm_tile_planes(g);
}

}  // namespace crnn_tile
