// bf16-MFMA GEMM (the throughput modes, crnn_config.mfma_bf16 = 1 | 2): same three operand modes and epilogue as
// gemm.hip, products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Each operand / the result is stored either
// as fp32 (rounded to bf16 with v_cvt_pk_bf16_f32, RNE, while it is staged into LDS) or as bf16 (16-byte loads / stores,
// template flags A_BF / B_BF, run-time dtC); with bf16 tensors the conv-stack GEMMs are HBM-bound.  The fp32 kernel in
// gemm.hip is the parity mode.
//
// 128 x {128,64} x 64 block tile, 4 waves, 2x2 / 1x2 MFMA 32x32 accumulators per wave.
// LDS layouts (18 / 20 KiB per 128-row operand, conflict-free):
//   row-major-in-k operand:  bf16 [rows][64 + 8]    -> one ds_read_b128 = the 8 consecutive k a lane feeds the MFMA
//   k-major operand:         bf16 [64 k][rows + 32] -> two ds_read_b64_tr_b16 (gfx950 transpose read: a 16-lane group fetches a
//                            4 k x 16 row block as 16 x 8 bytes and hands lane i the 4 k of row i); the 64-byte row pad puts
//                            the 4 k-rows x 2 groups of a 32-lane half on disjoint banks.  (Round 1 interleaved k pairs into
//                            u32 words and read them with four ds_read_b32 per fragment: the weight-gradient GEMMs, both
//                            operands k-major, were bound by LDS read issue.)
// Lane l of the MFMA holds k = 8*(l>>5)..+7 of row l&31 for both A and B.
#include "gemm_tile.h"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// ---- global -> registers (already converted to bf16) ------------------------------------------------------
// row-major-in-k operand, ROWS x 64 k, staged as ROWS/8 words (bf16 pairs) per thread:
//   fp32 source: ROWS/16 items of (row, 4 k)  = one float4 -> 2 words;   bf16 source: ROWS/32 items of (row, 8 k) = one 16-byte load -> 4 words
__device__ __forceinline__ unsigned ldg_bf16_guard(const bf16_t* p, int i, int n) { return (i < n) ? (unsigned)p[i] : 0u; }
// FULL: the tile lies inside the operand and 16-byte loads are legal -- straight-line vector loads, no guards (the guarded form costs
// the fp32 paths ~2 us per k-chunk: every load sits behind its own branch and the loads of a chunk are waited one by one)
template <int ROWS, bool BF, bool FULL = false>
__device__ __forceinline__ void load_rm(const float* __restrict__ X, int ld, int row0, int nrows, int k0, int kend, int vec,
                                        int tid, unsigned (&r)[ROWS / 8]) {
  if constexpr (BF) {
#pragma unroll
    for (int it = 0; it < ROWS / 32; ++it) {
      int idx = tid + it * 256, row = idx >> 3, k8 = idx & 7;
      int gr = row0 + row, gk = k0 + 8 * k8;
      uint4 u = make_uint4(0u, 0u, 0u, 0u);
      if (FULL || (gr < nrows && gk < kend)) {
        const bf16_t* p = reinterpret_cast<const bf16_t*>(X) + (long)gr * ld + gk;
        if (FULL || vec) u = *reinterpret_cast<const uint4*>(p);
        else {
          int n = kend - gk;
          u = make_uint4(ldg_bf16_guard(p, 0, n) | (ldg_bf16_guard(p, 1, n) << 16), ldg_bf16_guard(p, 2, n) | (ldg_bf16_guard(p, 3, n) << 16),
                         ldg_bf16_guard(p, 4, n) | (ldg_bf16_guard(p, 5, n) << 16), ldg_bf16_guard(p, 6, n) | (ldg_bf16_guard(p, 7, n) << 16));
        }
      }
      r[4 * it] = u.x; r[4 * it + 1] = u.y; r[4 * it + 2] = u.z; r[4 * it + 3] = u.w;
    }
  } else {
#pragma unroll
    for (int it = 0; it < ROWS / 16; ++it) {
      int idx = tid + it * 256, row = idx >> 4, k4 = idx & 15;
      int gr = row0 + row, gk = k0 + 4 * k4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (FULL || (gr < nrows && gk < kend)) {
        const float* p = X + (long)gr * ld + gk;
        if (FULL || vec) v = *reinterpret_cast<const float4*>(p);
        else { v.x = p[0]; if (gk + 1 < kend) v.y = p[1]; if (gk + 2 < kend) v.z = p[2]; if (gk + 3 < kend) v.w = p[3]; }
      }
      r[2 * it] = pack_bf16(v.x, v.y); r[2 * it + 1] = pack_bf16(v.z, v.w);
    }
  }
}
template <int ROWS, bool BF>
__device__ __forceinline__ void store_rm(unsigned short* Xs, int tid, const unsigned (&r)[ROWS / 8]) {
  if constexpr (BF) {
#pragma unroll
    for (int it = 0; it < ROWS / 32; ++it) {
      int idx = tid + it * 256, row = idx >> 3, k8 = idx & 7;
      *reinterpret_cast<uint4*>(&Xs[row * HLD + 8 * k8]) = make_uint4(r[4 * it], r[4 * it + 1], r[4 * it + 2], r[4 * it + 3]);
    }
  } else {
#pragma unroll
    for (int it = 0; it < ROWS / 16; ++it) {
      int idx = tid + it * 256, row = idx >> 4, k4 = idx & 15;
      *reinterpret_cast<uint2*>(&Xs[row * HLD + 4 * k4]) = make_uint2(r[2 * it], r[2 * it + 1]);
    }
  }
}
// k-major operand, 64 k x ROWS, staged as ROWS/8 words per thread (word = bf16 k, k+1 of one row):
//   fp32 source: ROWS/32 items of (k-pair, 4 rows) = two float4 -> 4 words;  bf16 source: ROWS/64 items of (k-pair, 8 rows) = two 16-byte loads -> 8 words
__device__ __forceinline__ uint4 ldg_bf16x8(const bf16_t* p, int n, int vec) {   // n = elements available at p
  if (n <= 0) return make_uint4(0u, 0u, 0u, 0u);
  if (vec) return *reinterpret_cast<const uint4*>(p);
  return make_uint4(ldg_bf16_guard(p, 0, n) | (ldg_bf16_guard(p, 1, n) << 16), ldg_bf16_guard(p, 2, n) | (ldg_bf16_guard(p, 3, n) << 16),
                    ldg_bf16_guard(p, 4, n) | (ldg_bf16_guard(p, 5, n) << 16), ldg_bf16_guard(p, 6, n) | (ldg_bf16_guard(p, 7, n) << 16));
}
template <int ROWS, bool BF, bool FULL = false>
__device__ __forceinline__ void load_km(const float* __restrict__ X, int ld, int row0, int nrows, int k0, int kend, int vec,
                                        int tid, unsigned (&r)[ROWS / 8]) {
  if constexpr (BF) {
    constexpr int ITEMS = ROWS / 64;                         // per thread (ROWS = 64: one item, upper half of the block idles)
#pragma unroll
    for (int it = 0; it < (ITEMS ? ITEMS : 1); ++it) {
      int idx = tid + it * 256, kp = idx / (ROWS / 8), c8 = idx % (ROWS / 8);
      int gk = k0 + 2 * kp, gc = row0 + 8 * c8;
      const bf16_t* Xb = reinterpret_cast<const bf16_t*>(X);
      uint4 ua = make_uint4(0u, 0u, 0u, 0u), ub = ua;
      if (FULL) {
        if (ITEMS || kp < 32) {
          ua = *reinterpret_cast<const uint4*>(Xb + (long)gk * ld + gc);
          ub = *reinterpret_cast<const uint4*>(Xb + (long)(gk + 1) * ld + gc);
        }
      } else if (kp < 32) {
        if (gk < kend) ua = ldg_bf16x8(Xb + (long)gk * ld + gc, nrows - gc, vec);
        if (gk + 1 < kend) ub = ldg_bf16x8(Xb + (long)(gk + 1) * ld + gc, nrows - gc, vec);
      }
      r[8 * it + 0] = ua.x; r[8 * it + 1] = ua.y; r[8 * it + 2] = ua.z; r[8 * it + 3] = ua.w;
      r[8 * it + 4] = ub.x; r[8 * it + 5] = ub.y; r[8 * it + 6] = ub.z; r[8 * it + 7] = ub.w;
    }
  } else {
#pragma unroll
    for (int it = 0; it < ROWS / 32; ++it) {
      int idx = tid + it * 256, kp = idx / (ROWS / 4), c4 = idx % (ROWS / 4);
      int gk = k0 + 2 * kp, gc = row0 + 4 * c4;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (FULL) {
        a = *reinterpret_cast<const float4*>(X + (long)gk * ld + gc);
        b = *reinterpret_cast<const float4*>(X + (long)(gk + 1) * ld + gc);
      } else if (gc < nrows) {
        if (gk < kend) {
          const float* p = X + (long)gk * ld + gc;
          if (vec) a = *reinterpret_cast<const float4*>(p);
          else { a.x = p[0]; if (gc + 1 < nrows) a.y = p[1]; if (gc + 2 < nrows) a.z = p[2]; if (gc + 3 < nrows) a.w = p[3]; }
        }
        if (gk + 1 < kend) {
          const float* p = X + (long)(gk + 1) * ld + gc;
          if (vec) b = *reinterpret_cast<const float4*>(p);
          else { b.x = p[0]; if (gc + 1 < nrows) b.y = p[1]; if (gc + 2 < nrows) b.z = p[2]; if (gc + 3 < nrows) b.w = p[3]; }
        }
      }
      r[4 * it] = pack_bf16(a.x, a.y); r[4 * it + 1] = pack_bf16(a.z, a.w); r[4 * it + 2] = pack_bf16(b.x, b.y); r[4 * it + 3] = pack_bf16(b.z, b.w);
    }
  }
}
// k-major LDS image: bf16 [64 k][KLD(ROWS)]; a thread's item = rows k, k+1 of 8 (bf16 source) / 4 (fp32 source) tile rows
template <int ROWS, bool BF>
__device__ __forceinline__ void store_km(unsigned short* Xs, int tid, const unsigned (&r)[ROWS / 8]) {
  if constexpr (BF) {
    constexpr int ITEMS = ROWS / 64;
#pragma unroll
    for (int it = 0; it < (ITEMS ? ITEMS : 1); ++it) {
      int idx = tid + it * 256, kp = idx / (ROWS / 8), c8 = idx % (ROWS / 8);
      if (kp < 32) {
        *reinterpret_cast<uint4*>(&Xs[(2 * kp) * KLD(ROWS) + 8 * c8]) = make_uint4(r[8 * it], r[8 * it + 1], r[8 * it + 2], r[8 * it + 3]);
        *reinterpret_cast<uint4*>(&Xs[(2 * kp + 1) * KLD(ROWS) + 8 * c8]) = make_uint4(r[8 * it + 4], r[8 * it + 5], r[8 * it + 6], r[8 * it + 7]);
      }
    }
  } else {
#pragma unroll
    for (int it = 0; it < ROWS / 32; ++it) {
      int idx = tid + it * 256, kp = idx / (ROWS / 4), c4 = idx % (ROWS / 4);
      *reinterpret_cast<uint2*>(&Xs[(2 * kp) * KLD(ROWS) + 4 * c4]) = make_uint2(r[4 * it], r[4 * it + 1]);
      *reinterpret_cast<uint2*>(&Xs[(2 * kp + 1) * KLD(ROWS) + 4 * c4]) = make_uint2(r[4 * it + 2], r[4 * it + 3]);
    }
  }
}
// ---- producer prologue (GemmParams::ascale/ashift): ReLU6(x * s + t) on 8 bf16 values, result rounded to bf16 (RNE) ----
// Same arithmetic as bn_act_pool_drop_kernel on a bf16 tensor (fp32 fma, clamp, v_cvt_pk_bf16_f32), so the fused and the
// two-pass paths give bit-identical operands.  tab = [scale[n] | shift[n]] in LDS, i = first of the 8 channels.
__device__ __forceinline__ unsigned bnrelu6_pair(unsigned w, f32x2 s, f32x2 t) {
  f32x2 v = {__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
  v = __builtin_elementwise_fma(v, s, t);                                   // v_pk_fma_f32 (same rounding as two fmaf)
  v[0] = __builtin_amdgcn_fmed3f(v[0], 0.f, 6.f); v[1] = __builtin_amdgcn_fmed3f(v[1], 0.f, 6.f);   // = min(max(v, 0), 6)
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ uint4 bnrelu6_bf16x8(uint4 u, const float* tab, int i) {
  const float4 s0 = *reinterpret_cast<const float4*>(tab + i), s1 = *reinterpret_cast<const float4*>(tab + i + 4);
  const float4 t0 = *reinterpret_cast<const float4*>(tab + TR_TAB + i), t1 = *reinterpret_cast<const float4*>(tab + TR_TAB + i + 4);
  uint4 o;
  o.x = bnrelu6_pair(u.x, f32x2{s0.x, s0.y}, f32x2{t0.x, t0.y});
  o.y = bnrelu6_pair(u.y, f32x2{s0.z, s0.w}, f32x2{t0.z, t0.w});
  o.z = bnrelu6_pair(u.z, f32x2{s1.x, s1.y}, f32x2{t1.x, t1.y});
  o.w = bnrelu6_pair(u.w, f32x2{s1.z, s1.w}, f32x2{t1.z, t1.w});
  return o;
}
// row-major-in-k bf16 operand (vector loads only): transform the staged words in place just before they go to LDS.
// A thread's 8 k are the same for all of its items; rows past M and k past the end must stay exactly zero.
template <int ROWS>
__device__ __forceinline__ void transform_rm(unsigned (&r)[ROWS / 8], const float* tab, int row0, int nrows, int k0, int kend, int tid) {
  const int k8 = tid & 7, gk = k0 + 8 * k8;
#pragma unroll
  for (int it = 0; it < ROWS / 32; ++it) {
    const int row = (tid + it * 256) >> 3;
    if (row0 + row < nrows && gk < kend) {
      uint4 o = bnrelu6_bf16x8(make_uint4(r[4 * it], r[4 * it + 1], r[4 * it + 2], r[4 * it + 3]), tab, gk);
      r[4 * it] = o.x; r[4 * it + 1] = o.y; r[4 * it + 2] = o.z; r[4 * it + 3] = o.w;
    }
  }
}
// k-major bf16 operand with the prologue: the registers keep the two raw rows (k, k+1) of 8 channels; transform and the
// k-pair interleave both happen at store time (so nothing waits on the global load when it is issued).
template <int ROWS, bool FULL = false>
__device__ __forceinline__ void load_km_raw(const float* __restrict__ X, int ld, int row0, int nrows, int k0, int kend, int tid,
                                            unsigned (&r)[ROWS / 8]) {
  constexpr int ITEMS = ROWS / 64;
#pragma unroll
  for (int it = 0; it < (ITEMS ? ITEMS : 1); ++it) {
    int idx = tid + it * 256, kp = idx / (ROWS / 8), c8 = idx % (ROWS / 8);
    int gk = k0 + 2 * kp, gc = row0 + 8 * c8;
    const bf16_t* Xb = reinterpret_cast<const bf16_t*>(X);
    uint4 ua = make_uint4(0u, 0u, 0u, 0u), ub = ua;
    if (FULL) {
      if (ITEMS || kp < 32) {
        ua = *reinterpret_cast<const uint4*>(Xb + (long)gk * ld + gc);
        ub = *reinterpret_cast<const uint4*>(Xb + (long)(gk + 1) * ld + gc);
      }
    } else if (kp < 32 && gc < nrows) {
      if (gk < kend) ua = *reinterpret_cast<const uint4*>(Xb + (long)gk * ld + gc);
      if (gk + 1 < kend) ub = *reinterpret_cast<const uint4*>(Xb + (long)(gk + 1) * ld + gc);
    }
    r[8 * it + 0] = ua.x; r[8 * it + 1] = ua.y; r[8 * it + 2] = ua.z; r[8 * it + 3] = ua.w;
    r[8 * it + 4] = ub.x; r[8 * it + 5] = ub.y; r[8 * it + 6] = ub.z; r[8 * it + 7] = ub.w;
  }
}
template <int ROWS>
__device__ __forceinline__ void store_km_tr(unsigned short* Xs, int tid, const unsigned (&r)[ROWS / 8], const float* tab, int row0, int nrows,
                                            int k0, int kend) {
  constexpr int ITEMS = ROWS / 64;
#pragma unroll
  for (int it = 0; it < (ITEMS ? ITEMS : 1); ++it) {
    int idx = tid + it * 256, kp = idx / (ROWS / 8), c8 = idx % (ROWS / 8);
    if (kp < 32) {
      const int gk = k0 + 2 * kp;
      uint4 ua = make_uint4(r[8 * it], r[8 * it + 1], r[8 * it + 2], r[8 * it + 3]);
      uint4 ub = make_uint4(r[8 * it + 4], r[8 * it + 5], r[8 * it + 6], r[8 * it + 7]);
      if (row0 + 8 * c8 < nrows) {
        if (gk < kend) ua = bnrelu6_bf16x8(ua, tab, 8 * c8);
        if (gk + 1 < kend) ub = bnrelu6_bf16x8(ub, tab, 8 * c8);
      }
      *reinterpret_cast<uint4*>(&Xs[(2 * kp) * KLD(ROWS) + 8 * c8]) = ua;
      *reinterpret_cast<uint4*>(&Xs[(2 * kp + 1) * KLD(ROWS) + 8 * c8]) = ub;
    }
  }
}

template <int BN, bool A_KM, bool B_KM, bool A_BF, bool B_BF, bool A_TR = false, bool FULL = false>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmParams p) {
  static_assert(!A_TR || A_BF, "the producer prologue is implemented for bf16 A");
  constexpr int BM = 128;
  constexpr int WAVES_N = (BN == 128) ? 2 : 1;
  constexpr int WM = (BN == 128) ? 64 : 32;
  constexpr int TM = WM / 32, TN = 2;
  constexpr int A_BYTES = A_KM ? HBK * KLD(BM) * 2 : BM * HLD * 2, B_BYTES = B_KM ? HBK * KLD(BN) * 2 : BN * HLD * 2;
  constexpr int C_BYTES = 64 * (BN + 4) * 4;
  constexpr int SM_BYTES = (A_BYTES + B_BYTES) > C_BYTES ? (A_BYTES + B_BYTES) : C_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char smem_raw[SM_BYTES];
  __shared__ __attribute__((aligned(16))) float tr_tab[A_TR ? 2 * TR_TAB : 4];
  unsigned char* const As = smem_raw;
  unsigned char* const Bs = smem_raw + A_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * 64;
  const TileCoord tc = gemm_tile_coord(p);
  const int tm = tc.tm, tn = tc.tn, ksplit = tc.ksplit;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = ksplit * p.klen;
  const int kend = min(p.K, kbeg + p.klen);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  unsigned ra[BM / 8], rb[BN / 8];   // staged operand words (bf16 pairs)
  auto loadA = [&](int k0) {
    if constexpr (A_KM && A_TR) load_km_raw<BM, FULL>(p.A, p.lda, m0, p.M, k0, kend, tid, ra);
    else if constexpr (A_KM) load_km<BM, A_BF, FULL>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, tid, ra);
    else load_rm<BM, A_BF, FULL>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, tid, ra);
  };
  auto loadB = [&](int k0) {
    if constexpr (B_KM) load_km<BN, B_BF, FULL>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, tid, rb);
    else load_rm<BN, B_BF, FULL>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, tid, rb);
  };
  if (!FULL || kbeg < kend) { loadA(kbeg); loadB(kbeg); }   // (an empty tail range of a split reduction must not touch memory unguarded)
  if constexpr (A_TR) {   // channel table: the reduction range (modes 0/1, K <= TR_TAB) or this tile's 128 A rows (mode 2)
    const int base = A_KM ? m0 : 0, lim = A_KM ? p.M : p.K, n = A_KM ? BM : TR_TAB;
    for (int i = tid; i < n; i += 256) {
      const bool ok = base + i < lim;
      tr_tab[i] = ok ? p.ascale[base + i] : 0.f;
      tr_tab[TR_TAB + i] = ok ? p.ashift[base + i] : 0.f;
    }
    __syncthreads();
  }

  for (int k0 = kbeg; k0 < kend; k0 += HBK) {
    if constexpr (A_KM && A_TR) store_km_tr<BM>(reinterpret_cast<unsigned short*>(As), tid, ra, tr_tab, m0, p.M, k0, kend);
    else if constexpr (A_KM) store_km<BM, A_BF>(reinterpret_cast<unsigned short*>(As), tid, ra);
    else {
      if constexpr (A_TR) transform_rm<BM>(ra, tr_tab, m0, p.M, k0, kend, tid);
      store_rm<BM, A_BF>(reinterpret_cast<unsigned short*>(As), tid, ra);
    }
    if constexpr (B_KM) store_km<BN, B_BF>(reinterpret_cast<unsigned short*>(Bs), tid, rb); else store_rm<BN, B_BF>(reinterpret_cast<unsigned short*>(Bs), tid, rb);
    __syncthreads();
    if (k0 + HBK < kend) { loadA(k0 + HBK); loadB(k0 + HBK); }   // prefetch the next chunk; in flight during the MFMAs below
#pragma unroll
    for (int ks = 0; ks < HBK / 16; ++ks) {
      bf16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = read_frag_h<A_KM, BM>(As, wm0 + i * 32, ks, half, l31);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = read_frag_h<B_KM, BN>(Bs, wn0 + j * 32, ks, half, l31);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  gemm_tile_epilogue<BN, TM, TN, FULL>(p, acc, smem_raw, tid, m0, n0, tm, wm0, wn0, ksplit);
}

namespace crnn_tile {

// (BN, mode, storage of A and B, prologue, whole tiles) -> the instantiation.  The prologue takes bf16 operands (checked by the planner).
typedef void (*bf16_kernel_t)(GemmParams);
template <int BN, bool A_KM, bool B_KM, bool A_BF, bool B_BF, bool A_TR>
static bf16_kernel_t bf16_kernel_full(bool full) {
  return full ? gemm_bf16_kernel<BN, A_KM, B_KM, A_BF, B_BF, A_TR, true> : gemm_bf16_kernel<BN, A_KM, B_KM, A_BF, B_BF, A_TR, false>;
}
template <int BN, bool A_KM, bool B_KM>
static bf16_kernel_t bf16_kernel_storage(bool abf, bool bbf, bool prologue, bool full) {
  if (prologue) return bf16_kernel_full<BN, A_KM, B_KM, true, true, true>(full);
  if (abf) return bbf ? bf16_kernel_full<BN, A_KM, B_KM, true, true, false>(full) : bf16_kernel_full<BN, A_KM, B_KM, true, false, false>(full);
  return bbf ? bf16_kernel_full<BN, A_KM, B_KM, false, true, false>(full) : bf16_kernel_full<BN, A_KM, B_KM, false, false, false>(full);
}
template <int BN>
static bf16_kernel_t bf16_kernel(int mode, bool abf, bool bbf, bool prologue, bool full) {
  return mode == 0 ? bf16_kernel_storage<BN, false, true>(abf, bbf, prologue, full)
       : mode == 1 ? bf16_kernel_storage<BN, false, false>(abf, bbf, prologue, full) : bf16_kernel_storage<BN, true, true>(abf, bbf, prologue, full);
}

int gemm_tile_bf16(const TileGemm& g) {
  if (g.product != PRODUCT_BF16) return CRNN_ERR_ARG;
  TilePlan t;
  CRNN_TRY(plan_tile_gemm(g, HBK, kSplitWorkgroups, false, kXcdPinnedSplit, t));
  const bool abf = g.dtA == CRNN_BF16, bbf = g.dtB == CRNN_BF16, prologue = g.ascale != nullptr;
  const bf16_kernel_t kernel = t.BN == 128 ? bf16_kernel<128>(g.mode, abf, bbf, prologue, t.full) : bf16_kernel<64>(g.mode, abf, bbf, prologue, t.full);
  hipLaunchKernelGGL(kernel, t.grid, dim3(256), 0, g.stream, t.pk);
  return finish_tile_gemm(g, t);
}

}  // namespace crnn_tile
