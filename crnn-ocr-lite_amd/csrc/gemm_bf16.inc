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
// (textually included at the end of gemm.hip: shares GemmParams and the split-reduce kernel)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define HBK 64                 // fp32 k per chunk
#define HLD (HBK + 8)          // bf16 row stride of the row-major-in-k layout (144 B)
#ifndef CRNN_KLD_PAD
#define CRNN_KLD_PAD 32
#endif
#define KLD(ROWS) ((ROWS) + CRNN_KLD_PAD)   // bf16 row stride of the k-major layout

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
#define TR_TAB 512             // channels the LDS table holds (K <= 512 in modes 0/1; the 128 tile rows in mode 2)
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

// ---- fp32-accurate products from three bf16 planes (X3 instantiations: the parity mode's GEMMs) ------------------------------------
// x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (round-to-nearest-even each; the differences are exact
// in fp32): |x - (hi + mid + lo)| <= 2^-27 |x|.  A product keeps hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi (the dropped terms are
// <= 2^-26 of it) and every partial product of bf16 values is exact in the MFMA's fp32 accumulator: six v_mfma_f32_32x32x16_bf16
// (6 x 32 cycles per 32x32x16 block) replace the eight v_mfma_f32_32x32x2_f32 (8 x 64 cycles) of the fp32 kernel with fp32-level accuracy
// (not the bit pattern of an fmaf chain: crnn_gemm_f32 stays for that).  Non-finite inputs become NaN in all three planes' products.
#ifndef X3P_SPLIT
#define X3P_SPLIT 0   // experiment builds (scripts/build_x3_split_variants.sh, profiles/r04_x3_split_variants.txt): 1 = last plane by v_perm_b32, 2 = middle plane too
#endif
__device__ __forceinline__ void split3_pair(float v0, float v1, unsigned& w0, unsigned& w1, unsigned& w2) {
#if X3P_SPLIT == 0
  crnn_split3_pair(v0, v1, w0, w1, w2);          // common.h: the spelling every plane-forming kernel shares
#else
#pragma clang fp contract(off)
  w0 = pack_bf16(v0, v1);
  const float r0 = sub_unpacked(v0, __uint_as_float(w0 << 16)), r1 = sub_unpacked(v1, __uint_as_float(w0 & 0xffff0000u));
#if X3P_SPLIT >= 2   // experiment: middle plane by truncation (an integer operation; x = hi + mid + lo stays exact, the dropped product terms double)
  w1 = __builtin_amdgcn_perm(__float_as_uint(r1), __float_as_uint(r0), 0x07060302u);
#else
  w1 = pack_bf16(r0, r1);
#endif
  const float s0 = sub_unpacked(r0, __uint_as_float(w1 << 16)), s1 = sub_unpacked(r1, __uint_as_float(w1 & 0xffff0000u));
  // the last residual has at most 8 significant bits (a 24-bit significand minus two 8-bit planes): its upper half IS its bf16 value -- an integer
  // v_perm_b32 instead of a third v_cvt_pk_bf16_f32, the same bits.  Measured: K = 64 shape -13 %, K >= 256 shapes + 3..5 % (the schedule around the
  // MFMAs shifts): not the default
  w2 = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
#endif
}
// raw fp32 items of a row-major-in-k operand tile (the addressing of load_rm's fp32 branch): ROWS/16 float4 per thread
template <int ROWS, bool FULL>
__device__ __forceinline__ void load_rm_raw32(const float* __restrict__ X, int ld, int row0, int nrows, int k0, int kend, int vec, int tid,
                                              float4 (&raw)[ROWS / 16]) {
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
    raw[it] = v;
  }
}
template <int ROWS>
__device__ __forceinline__ void split_rm(const float4 (&raw)[ROWS / 16], unsigned (&r)[3][ROWS / 8], int part = 0, int parts = 1) {
#pragma unroll
  for (int it = part * (ROWS / 16) / parts; it < (part + 1) * (ROWS / 16) / parts; ++it) {
    split3_pair(raw[it].x, raw[it].y, r[0][2 * it], r[1][2 * it], r[2][2 * it]);
    split3_pair(raw[it].z, raw[it].w, r[0][2 * it + 1], r[1][2 * it + 1], r[2][2 * it + 1]);
  }
}
// pair `pi` (compile-time after unrolling) of a staged operand: raw items -> word pi of the three planes
template <int ROWS, bool KM>
__device__ __forceinline__ void split_pair_at(const float4 (&raw)[ROWS / 16], unsigned (&r)[3][ROWS / 8], int pi) {
  float v0, v1;
  if constexpr (!KM) { const float4 v = raw[pi >> 1]; v0 = (pi & 1) ? v.z : v.x; v1 = (pi & 1) ? v.w : v.y; }
  else { const float4 v = raw[2 * (pi >> 2) + ((pi >> 1) & 1)]; v0 = (pi & 1) ? v.z : v.x; v1 = (pi & 1) ? v.w : v.y; }
  split3_pair(v0, v1, r[0][pi], r[1][pi], r[2][pi]);
  // the words are consumed an iteration later: without an anchor the instruction selector emits these 11 instructions after the block's
  // MFMAs (pure arithmetic is not ordered against sched_barrier); the empty volatile asm pins them to this spot of the schedule
  asm volatile("" : "+v"(r[0][pi]), "+v"(r[1][pi]), "+v"(r[2][pi]));
}
// raw fp32 items of a k-major operand tile (load_km's fp32 branch): ROWS/32 items of two float4 (rows k, k+1 of 4 tile rows)
template <int ROWS, bool FULL>
__device__ __forceinline__ void load_km_raw32(const float* __restrict__ X, int ld, int row0, int nrows, int k0, int kend, int vec, int tid,
                                              float4 (&raw)[ROWS / 16]) {
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
    raw[2 * it] = a; raw[2 * it + 1] = b;
  }
}
template <int ROWS>
__device__ __forceinline__ void split_km(const float4 (&raw)[ROWS / 16], unsigned (&r)[3][ROWS / 8], int part = 0, int parts = 1) {
#pragma unroll
  for (int it = part * (ROWS / 32) / parts; it < (part + 1) * (ROWS / 32) / parts; ++it) {
    const float4 a = raw[2 * it], b = raw[2 * it + 1];
    split3_pair(a.x, a.y, r[0][4 * it], r[1][4 * it], r[2][4 * it]);
    split3_pair(a.z, a.w, r[0][4 * it + 1], r[1][4 * it + 1], r[2][4 * it + 1]);
    split3_pair(b.x, b.y, r[0][4 * it + 2], r[1][4 * it + 2], r[2][4 * it + 2]);
    split3_pair(b.z, b.w, r[0][4 * it + 3], r[1][4 * it + 3], r[2][4 * it + 3]);
  }
}

// fragment = the 8 bf16 (k = 16*ks + 8*half .. +7) of row r0 + l31
typedef short s16x4 __attribute__((ext_vector_type(4)));
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
#ifdef CRNN_GEMM_EXP
          if ((p.exp & 1) && v.lo.x != 12345.678f) continue;
#endif
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
#ifdef CRNN_GEMM_EXP
        if ((p.exp & 1) && v.x != 12345.678f) continue;
#endif
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
    const float binv[4] = {1.0f / sqrtf(va.x + 1e-3f), 1.0f / sqrtf(va.y + 1e-3f), 1.0f / sqrtf(va.z + 1e-3f), 1.0f / sqrtf(va.w + 1e-3f)};   // BN_EPS, the spelling of bn_bwd_kernel
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

template <int BN, bool A_KM, bool B_KM, bool A_BF, bool B_BF, bool A_TR = false, bool FULL = false, bool X3 = false>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmParams p) {
  static_assert(!A_TR || A_BF, "the producer prologue is implemented for bf16 A");
  static_assert(!X3 || (!A_BF && !B_BF && !A_TR), "three-plane products take fp32 operands");
  constexpr int NP = X3 ? 3 : 1;                     // bf16 planes per operand
  constexpr int BM = 128;
  constexpr int WAVES_N = (BN == 128) ? 2 : 1;
  constexpr int WM = (BN == 128) ? 64 : 32;
  constexpr int TM = WM / 32, TN = 2;
  constexpr int A_BYTES = A_KM ? HBK * KLD(BM) * 2 : BM * HLD * 2, B_BYTES = B_KM ? HBK * KLD(BN) * 2 : BN * HLD * 2;
  constexpr int C_BYTES = 64 * (BN + 4) * 4;
  constexpr int SM_BYTES = NP * (A_BYTES + B_BYTES) > C_BYTES ? NP * (A_BYTES + B_BYTES) : C_BYTES;
  // X3: 111 - 123 KiB (three planes per operand), past the 64 KiB of static LDS: dynamic, size from the launcher (gemm_x3_lds_bytes)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
  __shared__ __attribute__((aligned(16))) unsigned char smem_static[X3 ? 16 : SM_BYTES];
  unsigned char* const smem_raw = X3 ? smem_dyn : smem_static;
  __shared__ __attribute__((aligned(16))) float tr_tab[A_TR ? 2 * TR_TAB : 4];
  unsigned char* const As = smem_raw;                // plane pl of A at As + pl * A_BYTES
  unsigned char* const Bs = smem_raw + NP * A_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * 64;
  int lid, ksplit;
  if (p.xsplit > 0) {   // split reduction over a huge K (weight gradients): every K range lives on ONE XCD, where all output tiles
    // of that range run together and share the operand rows through its L2 (the rows are read from HBM once instead of
    // once per tile row / column)
    const int bid = blockIdx.x, ntile = gridDim.x / p.xsplit, rest = bid >> 3;
    lid = rest % ntile; ksplit = (rest / ntile) * 8 + (bid & 7);
  } else {
    int nwg = gridDim.x, bid = blockIdx.x;
    int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
    lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    ksplit = blockIdx.y;
  }
  const int tm = lid / p.tilesN, tn = lid % p.tilesN;
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

  unsigned ra3[X3 ? 3 : 1][BM / 8], rb3[X3 ? 3 : 1][BN / 8];   // staged operand words (bf16 pairs), one set per plane
  unsigned (&ra)[BM / 8] = ra3[0]; unsigned (&rb)[BN / 8] = rb3[0];
  float4 rawA[X3 ? BM / 16 : 1], rawB[X3 ? BN / 16 : 1];        // X3: the fp32 items of the chunk in flight
  auto loadA = [&](int k0) {
    if constexpr (X3) {
      if constexpr (A_KM) load_km_raw32<BM, FULL>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, tid, rawA);
      else load_rm_raw32<BM, FULL>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, tid, rawA);
    } else
    if constexpr (A_KM && A_TR) load_km_raw<BM, FULL>(p.A, p.lda, m0, p.M, k0, kend, tid, ra);
    else if constexpr (A_KM) load_km<BM, A_BF, FULL>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, tid, ra);
    else load_rm<BM, A_BF, FULL>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, tid, ra);
  };
  auto loadB = [&](int k0) {
    if constexpr (X3) {
      if constexpr (B_KM) load_km_raw32<BN, FULL>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, tid, rawB);
      else load_rm_raw32<BN, FULL>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, tid, rawB);
    } else if constexpr (B_KM) load_km<BN, B_BF, FULL>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, tid, rb);
    else load_rm<BN, B_BF, FULL>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, tid, rb);
  };
  auto split_planes = [&](int part = 0, int parts = 1) {   // X3: raw fp32 items -> three planes of bf16 words (one part of `parts`)
    if constexpr (X3) {
      if constexpr (A_KM) split_km<BM>(rawA, ra3, part, parts); else split_rm<BM>(rawA, ra3, part, parts);
      if constexpr (B_KM) split_km<BN>(rawB, rb3, part, parts); else split_rm<BN>(rawB, rb3, part, parts);
    }
  };
#ifdef CRNN_GEMM_EXP
  unsigned long long* trc = (p.trace && blockIdx.x == 300 && tid == 0) ? p.trace : nullptr;
  int trn = 0;
#define GEMM_TRC() do { if (trc && trn < 30) trc[trn++] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define GEMM_TRC() do {} while (0)
#endif
  GEMM_TRC();
  if (!FULL || kbeg < kend) { loadA(kbeg); loadB(kbeg); split_planes(); }   // (an empty tail range of a split reduction must not touch memory unguarded)
  if constexpr (X3) {   // chunk 1 in flight while chunk 0 is multiplied (a one-chunk range reads chunk 0 again)
    if (!FULL || kbeg < kend) { const int k1 = kbeg + HBK < kend ? kbeg + HBK : kbeg; loadA(k1); loadB(k1); }
  }
  GEMM_TRC();
  if constexpr (A_TR) {   // channel table: the reduction range (modes 0/1, K <= TR_TAB) or this tile's 128 A rows (mode 2)
    const int base = A_KM ? m0 : 0, lim = A_KM ? p.M : p.K, n = A_KM ? BM : TR_TAB;
    for (int i = tid; i < n; i += 256) {
      const bool ok = base + i < lim;
      tr_tab[i] = ok ? p.ascale[base + i] : 0.f;
      tr_tab[TR_TAB + i] = ok ? p.ashift[base + i] : 0.f;
    }
    __syncthreads();
  }

  // X3 main loop: one workgroup per CU (111 - 123 KiB of LDS), so nothing overlaps a wave's staging unless the wave does it itself.
  // Software pipeline over two ping-pong sets of raw registers: iteration k stores chunk k's planes to LDS, requests the raw items of
  // chunk k+2 into the free set, and while the 96 MFMAs of chunk k are issued splits the raw items of chunk k+1 (requested an iteration
  // ago, the other set) into planes in the matrix pipe's shadow -- one pair per three MFMAs, every MFMA pinned by a sched_barrier.
  // Loads and splits are unconditional (past the end the last chunk is read / split again and never stored) and the loop is unrolled
  // by two instead of copying registers: with a branch or a copy between a load and its use the wait-count insertion waits for the
  // loads issued in the SAME iteration (vmcnt(15) .. vmcnt(0) right behind them: nothing was ever prefetched).
  if constexpr (X3) {
    float4 rawA2[BM / 16], rawB2[BN / 16];
    const int klast = kend - HBK > kbeg ? kbeg + ((kend - 1 - kbeg) / HBK) * HBK : kbeg;   // start of the last chunk
    auto load_raw = [&](int k0, float4 (&dA)[BM / 16], float4 (&dB)[BN / 16]) {
      k0 = k0 < klast ? k0 : klast;
      if constexpr (A_KM) load_km_raw32<BM, FULL>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, tid, dA);
      else load_rm_raw32<BM, FULL>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, tid, dA);
      if constexpr (B_KM) load_km_raw32<BN, FULL>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, tid, dB);
      else load_rm_raw32<BN, FULL>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, tid, dB);
    };
    auto iteration = [&](int k0, float4 (&curA)[BM / 16], float4 (&curB)[BN / 16], float4 (&nxtA)[BM / 16], float4 (&nxtB)[BN / 16]) {
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        if constexpr (A_KM) store_km<BM, false>(reinterpret_cast<unsigned short*>(As + pl * A_BYTES), tid, ra3[pl]);
        else store_rm<BM, false>(reinterpret_cast<unsigned short*>(As + pl * A_BYTES), tid, ra3[pl]);
        if constexpr (B_KM) store_km<BN, false>(reinterpret_cast<unsigned short*>(Bs + pl * B_BYTES), tid, rb3[pl]);
        else store_rm<BN, false>(reinterpret_cast<unsigned short*>(Bs + pl * B_BYTES), tid, rb3[pl]);
      }
      GEMM_TRC();
      __syncthreads();
      GEMM_TRC();
      load_raw(k0 + 2 * HBK, nxtA, nxtB);
      __builtin_amdgcn_sched_barrier(0);
      {
        constexpr int NKS = HBK / 16, NM = 6 * TM * TN, NPAIR = BM / 8 + BN / 8, NMF = NM * NKS;
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};   // lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi: small terms first
        bf16x8 fa[2][3][TM], fb[2][3][TN];
        auto read_frags = [&](int ks, int buf) {
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[buf][pl][i] = read_frag_h<A_KM, BM>(As + pl * A_BYTES, wm0 + i * 32, ks, half, l31);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[buf][pl][j] = read_frag_h<B_KM, BN>(Bs + pl * B_BYTES, wn0 + j * 32, ks, half, l31);
          }
        };
        read_frags(0, 0);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
#pragma unroll
          for (int g = 0; g < NM; ++g) {
            if (g == 2 && ks + 1 < NKS) read_frags(ks + 1, (ks + 1) & 1);
            const int t = g / (TM * TN), i = (g / TN) % TM, j = g % TN;   // the product type is the outer loop: consecutive MFMAs, different accumulators
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks & 1][PA[t]][i], fb[ks & 1][PB[t]][j], acc[i][j], 0, 0, 0);
            const int gg = ks * NM + g, p0 = gg * NPAIR / NMF, p1 = (gg + 1) * NPAIR / NMF;
#if !defined(CRNN_X3_EXP) || !(CRNN_X3_EXP & 1)     // (trace builds: 1 = no plane split in the MFMA block)
            if (p1 > p0) {                                             // (p1 - p0 <= 1: NPAIR <= NMF)
              if (p0 < BM / 8) split_pair_at<BM, A_KM>(curA, ra3, p0);
              else split_pair_at<BN, B_KM>(curB, rb3, p0 - BM / 8);
            }
#endif
            __builtin_amdgcn_sched_barrier(0);
          }
          GEMM_TRC();
        }
      }
      GEMM_TRC();
      __syncthreads();
      GEMM_TRC();
    };
    // (the prologue above left chunk 0's planes in ra3 / rb3 and requested chunk 1 into rawA / rawB)
    for (int k0 = kbeg; k0 < kend; k0 += 2 * HBK) {
      iteration(k0, rawA, rawB, rawA2, rawB2);
      if (k0 + HBK < kend) iteration(k0 + HBK, rawA2, rawB2, rawA, rawB);
    }
  } else
  for (int k0 = kbeg; k0 < kend; k0 += HBK) {
    if constexpr (X3) {
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        if constexpr (A_KM) store_km<BM, false>(reinterpret_cast<unsigned short*>(As + pl * A_BYTES), tid, ra3[pl]);
        else store_rm<BM, false>(reinterpret_cast<unsigned short*>(As + pl * A_BYTES), tid, ra3[pl]);
        if constexpr (B_KM) store_km<BN, false>(reinterpret_cast<unsigned short*>(Bs + pl * B_BYTES), tid, rb3[pl]);
        else store_rm<BN, false>(reinterpret_cast<unsigned short*>(Bs + pl * B_BYTES), tid, rb3[pl]);
      }
    } else {
    if constexpr (A_KM && A_TR) store_km_tr<BM>(reinterpret_cast<unsigned short*>(As), tid, ra, tr_tab, m0, p.M, k0, kend);
    else if constexpr (A_KM) store_km<BM, A_BF>(reinterpret_cast<unsigned short*>(As), tid, ra);
    else {
      if constexpr (A_TR) transform_rm<BM>(ra, tr_tab, m0, p.M, k0, kend, tid);
      store_rm<BM, A_BF>(reinterpret_cast<unsigned short*>(As), tid, ra);
    }
    if constexpr (B_KM) store_km<BN, B_BF>(reinterpret_cast<unsigned short*>(Bs), tid, rb); else store_rm<BN, B_BF>(reinterpret_cast<unsigned short*>(Bs), tid, rb);
    }
    GEMM_TRC();
    __syncthreads();
    GEMM_TRC();
#ifdef CRNN_GEMM_EXP
    if (k0 + HBK < kend) { if (!(p.exp & 8)) loadA(k0 + HBK); if (!(p.exp & 4)) loadB(k0 + HBK); }
    if (!(p.exp & 2))
#else
    if (k0 + HBK < kend) { loadA(k0 + HBK); loadB(k0 + HBK); }
#endif
#pragma unroll
    for (int ks = 0; ks < HBK / 16; ++ks) {
      if constexpr (X3) {
        bf16x8 fa[3][TM], fb[3][TN];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
          for (int i = 0; i < TM; ++i) fa[pl][i] = read_frag_h<A_KM, BM>(As + pl * A_BYTES, wm0 + i * 32, ks, half, l31);
#pragma unroll
          for (int j = 0; j < TN; ++j) fb[pl][j] = read_frag_h<B_KM, BN>(Bs + pl * B_BYTES, wn0 + j * 32, ks, half, l31);
        }
        // small terms first; the product type is the outer loop so that consecutive MFMAs go to different accumulators
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};   // lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA[t]][i], fb[PB[t]][j], acc[i][j], 0, 0, 0);
      } else {
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
    }
    if constexpr (X3) { if (k0 + HBK < kend) split_planes(); }   // the next chunk's planes, formed while the matrix pipe drains
    GEMM_TRC();
    __syncthreads();
    GEMM_TRC();
  }

  GEMM_TRC();
  gemm_tile_epilogue<BN, TM, TN, FULL>(p, acc, smem_raw, tid, m0, n0, tm, wm0, wn0, ksplit);
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Three-plane products on PRODUCER WAVES (round 3): the X3 instantiation above needs 111-123 KiB of LDS, so one workgroup per CU has to
// stage (load fp32, split into planes, write LDS) and multiply in the same four waves -- its trace shows 1.9 us of MFMAs inside a 4.1 us
// chunk.  Here a workgroup has 8 waves: waves 0-3 only multiply (128 x BN tile, 2x2 / 1x2 accumulators each, as above), waves 4-7 only
// stage.  A stage is 16 k; two stages live in LDS (2 x 3 planes x (A + B) = 72 KiB at BN = 128) and the kernel is held to 128 VGPRs, so
// TWO workgroups share a CU: one's barrier waits, prologue (first loads) and epilogue run under the other's MFMAs.  While the MFMA waves
// read stage s from slot s & 1, the staging waves split the fp32 items they requested two stages earlier into the planes of stage s+1 and
// write them to slot (s+1) & 1 (released by the barrier that ended stage s-1), then request stage s+3.  One s_barrier per stage.
// Layouts: row-major-in-k planes bf16 [rows][16 + 8] (48-byte rows: the 8 lanes a ds_read_b128 serves per clock land in 8 different
// 16-byte slots), k-major planes bf16 [16 k][rows + 32] (the transposing reads of the 64-k kernel).  Same split, same six products in the
// same order per k-step, same epilogue as the X3 instantiation: results equal it to the last bit.
// Measured on 119808 x 512 x 512 (profiles/r03_gemm_x3_bench_variants.txt, r03_gemm_x3p_experiments.txt): fp32 MFMA 629 us; 32-k stages, one
// workgroup per CU, 4 staging waves 420 us (MFMA waves wait 0.4 of every 1.7 us for the planes); 8 staging waves 434; 16-k stages 402; two
// workgroups per CU 370 (41 % of the dense bf16 peak).  What is left (timing builds -DX3P_EXP): no split arithmetic -20 %, no fragment reads
// -7 %, no B operand at all -27 %, MFMAs + A loads only -28 %: the float VALU work of the split shares issue with the matrix pipe
// (scripts/probes/mfma_valu_probe.hip: integer VALU of another wave overlaps MFMAs, v_sub_f32 / v_cvt_pk_bf16_f32 only partly).
#ifndef X3P_EXP
#define X3P_EXP 0                // timing experiments (scripts/_trace builds): 16 no split, 32 no split and no stores, 64 no fragment reads, 128 no B, 256 no split of B
#endif
#ifndef PBK
#define PBK 16                   // k per stage
#endif
#define PLD (PBK + 8)
#ifndef X3P_STAGERS
#define X3P_STAGERS 256          // staging threads (4 waves: one per SIMD beside its MFMA wave)
#endif
#ifndef X3P_WGS
#define X3P_WGS 2                // workgroups per CU the register budget is held to (2 x 8 waves = 4 per SIMD, 128 VGPRs)
#endif
#define X3P_K4 (PBK / 4)         // float4 per row of a row-major-in-k stage
// items (float4) a staging thread holds per stage of a ROWS-row operand
#define X3P_ITEMS(ROWS) (((ROWS) * X3P_K4 + X3P_STAGERS - 1) / X3P_STAGERS)
#define X3P_KTOT(ROWS) ((PBK / 2) * ((ROWS) / 4))                           // k-major: items of two float4 (k, k+1 of 4 tile rows)
#define X3P_KITEMS(ROWS) ((X3P_KTOT(ROWS) + X3P_STAGERS - 1) / X3P_STAGERS)
#define X3P_RAW(ROWS) (X3P_ITEMS(ROWS) > 2 * X3P_KITEMS(ROWS) ? X3P_ITEMS(ROWS) : 2 * X3P_KITEMS(ROWS))
template <int ROWS>
__device__ __forceinline__ void x3p_load_rm(const float* __restrict__ X, int ld, int row0, int nrows, int k0, int kend, int vec, bool full, int st,
                                            float4 (&raw)[X3P_RAW(ROWS)]) {
#pragma unroll
  for (int it = 0; it < X3P_ITEMS(ROWS); ++it) {   // ROWS x PBK/4 float4 over the staging threads
    const int idx = st + it * X3P_STAGERS, row = idx / X3P_K4, k4 = idx % X3P_K4;
    const int gr = row0 + row, gk = k0 + 4 * k4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((ROWS * X3P_K4) % X3P_STAGERS != 0 && idx >= ROWS * X3P_K4) { raw[it] = v; continue; }
    if (full || (gr < nrows && gk < kend)) {
      const float* p = X + (long)gr * ld + gk;
      if (full || vec) v = *reinterpret_cast<const float4*>(p);
      else { v.x = p[0]; if (gk + 1 < kend) v.y = p[1]; if (gk + 2 < kend) v.z = p[2]; if (gk + 3 < kend) v.w = p[3]; }
    }
    raw[it] = v;
  }
}
template <int ROWS, int NPL = 3>
__device__ __forceinline__ void x3p_store_rm(unsigned char* Xs, int plane_bytes, int st, const float4 (&raw)[X3P_RAW(ROWS)]) {
#pragma unroll
  for (int it = 0; it < X3P_ITEMS(ROWS); ++it) {
    const int idx = st + it * X3P_STAGERS, row = idx / X3P_K4, k4 = idx % X3P_K4;
    if ((ROWS * X3P_K4) % X3P_STAGERS != 0 && idx >= ROWS * X3P_K4) continue;
    unsigned a0, a1, a2, b0, b1, b2;
    split3_pair(raw[it].x, raw[it].y, a0, a1, a2);
    split3_pair(raw[it].z, raw[it].w, b0, b1, b2);
    unsigned short* d = reinterpret_cast<unsigned short*>(Xs) + row * PLD + 4 * k4;
    *reinterpret_cast<uint2*>(d) = make_uint2(a0, b0);
    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(d) + plane_bytes) = make_uint2(a1, b1);
    if constexpr (NPL > 2) *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(d) + 2 * plane_bytes) = make_uint2(a2, b2);
  }
}
// k-major operand: PBK/2 k-pairs x ROWS/4 column groups, items of two float4 (rows k, k+1 of 4 tile rows)
template <int ROWS>
__device__ __forceinline__ void x3p_load_km(const float* __restrict__ X, int ld, int row0, int nrows, int k0, int kend, int vec, bool full, int st,
                                            float4 (&raw)[X3P_RAW(ROWS)]) {
#pragma unroll
  for (int it = 0; it < X3P_KITEMS(ROWS); ++it) {
    const int idx = st + it * X3P_STAGERS, kp = idx / (ROWS / 4), c4 = idx % (ROWS / 4);
    const int gk = k0 + 2 * kp, gc = row0 + 4 * c4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (X3P_KTOT(ROWS) % X3P_STAGERS != 0 && idx >= X3P_KTOT(ROWS)) { raw[2 * it] = a; raw[2 * it + 1] = b; continue; }
    if (full) {
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
    raw[2 * it] = a; raw[2 * it + 1] = b;
  }
}
template <int ROWS, int NPL = 3>
__device__ __forceinline__ void x3p_store_km(unsigned char* Xs, int plane_bytes, int st, const float4 (&raw)[X3P_RAW(ROWS)]) {
#pragma unroll
  for (int it = 0; it < X3P_KITEMS(ROWS); ++it) {
    const int idx = st + it * X3P_STAGERS, kp = idx / (ROWS / 4), c4 = idx % (ROWS / 4);
    if (X3P_KTOT(ROWS) % X3P_STAGERS != 0 && idx >= X3P_KTOT(ROWS)) continue;
    const float4 a = raw[2 * it], b = raw[2 * it + 1];
    unsigned w[4][3];
    split3_pair(a.x, a.y, w[0][0], w[0][1], w[0][2]); split3_pair(a.z, a.w, w[1][0], w[1][1], w[1][2]);
    split3_pair(b.x, b.y, w[2][0], w[2][1], w[2][2]); split3_pair(b.z, b.w, w[3][0], w[3][1], w[3][2]);
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
      unsigned short* d = reinterpret_cast<unsigned short*>(Xs + pl * plane_bytes);
      *reinterpret_cast<uint2*>(&d[(2 * kp) * KLD(ROWS) + 4 * c4]) = make_uint2(w[0][pl], w[1][pl]);
      *reinterpret_cast<uint2*>(&d[(2 * kp + 1) * KLD(ROWS) + 4 * c4]) = make_uint2(w[2][pl], w[3][pl]);
    }
  }
}
// fragment of a stage: the 8 bf16 (k = 16 ks + 8 half .. +7) of row r0 + l31
template <bool KM, int ROWS>
__device__ __forceinline__ bf16x8 x3p_frag(const unsigned char* Xs, int r0, int ks, int half, int l31) {
  if constexpr (KM) return read_frag_h<true, ROWS>(Xs, r0, ks, half, l31);      // [k][rows + pad]: the 64-k kernel's transposing read, rows 0..31 of k
  else return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(Xs) + (r0 + l31) * PLD + ks * 16 + 8 * half));
}

// ATR: the A operand the planes are formed from is ReLU6(A * ascale[ch] + ashift[ch]) (GemmParams::ascale / ashift; ch = the reduction index in mode 0, the A
// row in mode 2), applied by the staging waves to the raw fp32 items before the split -- the BatchNorm + ReLU6 between a depthwise and a pointwise
// convolution in the parity mode, the very arithmetic of bn_act_pool_drop_kernel, without the activated tensor in HBM.
// NPL = 2: two planes per operand and the three products hi*hi + hi*mid + mid*hi -- 16 significant bits per factor (relative error of a product
// <= 3 * 2^-18, fp32 accumulation): half the MFMA work and two thirds of the LDS traffic of the three-plane form.
template <int BN, bool A_KM, bool B_KM, bool FULL, bool BNB = false, bool ATR = false, int NPL = 3>
__global__ __launch_bounds__(256 + X3P_STAGERS) __attribute__((amdgpu_waves_per_eu(X3P_WGS * (256 + X3P_STAGERS) / 256)))
void gemm_x3p_kernel(GemmParams p) {
  static_assert(NPL == 2 || NPL == 3, "two or three planes");
  constexpr int BM = 128;
  constexpr int WAVES_N = (BN == 128) ? 2 : 1;
  constexpr int WM = (BN == 128) ? 64 : 32;
  constexpr int TM = WM / 32, TN = 2;
  constexpr int A_PL = A_KM ? PBK * KLD(BM) * 2 : BM * PLD * 2, B_PL = B_KM ? PBK * KLD(BN) * 2 : BN * PLD * 2;   // bytes of one plane
  constexpr int STAGE = NPL * (A_PL + B_PL);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];      // two stages; the epilogue's 33 KiB staging tile reuses them
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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
  const int tm = lid / p.tilesN, tn = lid % p.tilesN;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = ksplit * p.klen;
  const int kend = min(p.K, kbeg + p.klen);
  const int nst = kend > kbeg ? (kend - kbeg + PBK - 1) / PBK : 0;              // stages of this K range
#if defined(CRNN_GEMM_EXP) && defined(CRNN_X3P_STAMPS)   // (a stamp waits for the wave's LDS traffic too: timing experiments run without)
  unsigned long long* xtrc = (p.trace && blockIdx.x == 300 && lane == 0) ? p.trace + wave * 64 : nullptr;   // 64 stamps per wave
  int xtn = 0;
#define X3P_TRC() do { if (xtrc && xtn < 64) xtrc[xtn++] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define X3P_TRC() do {} while (0)
#endif
  X3P_TRC();
  float* const atab = reinterpret_cast<float*>(smem_dyn + 2 * STAGE);            // ATR, mode 0: [scale | shift] x TR_TAB reduction channels
  if constexpr (ATR && !A_KM) {
    for (int i = tid; i < TR_TAB; i += 256 + X3P_STAGERS) { const bool in = i < p.K; atab[i] = in ? p.ascale[i] : 0.f; atab[TR_TAB + i] = in ? p.ashift[i] : 0.f; }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                                 // every wave: the table is in LDS before the first plane is formed
  }

  if (wave >= 4) {
    // ------------------------------------------------------------------ staging waves
    const int st = tid - 256;
    using RawA = float4[X3P_RAW(BM)];
    using RawB = float4[X3P_RAW(BN)];
    RawA rawA[2]; RawB rawB[2];
    auto load = [&](int s, RawA& dA, RawB& dB) {
      s = s < nst ? s : (nst > 0 ? nst - 1 : 0);                                 // past the end: the last stage again (never stored)
      const int k0 = kbeg + s * PBK;
      const bool full = FULL && nst > 0;
      if constexpr (A_KM) x3p_load_km<BM>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, full, st, dA);
      else x3p_load_rm<BM>(p.A, p.lda, m0, p.M, k0, kend, p.vecA, full, st, dA);
#if X3P_EXP & 128
      { for (int i = 0; i < X3P_RAW(BN); ++i) dB[i] = make_float4(0.f, 0.f, 0.f, 0.f); return; }   // experiment: B neither loaded, split nor stored
#endif
      if constexpr (B_KM) x3p_load_km<BN>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, full, st, dB);
      else x3p_load_rm<BN>(p.B, p.ldb, n0, p.N, k0, kend, p.vecB, full, st, dB);
    };
    float kmsc[4] = {0.f, 0.f, 0.f, 0.f}, kmsh[4] = {0.f, 0.f, 0.f, 0.f};          // ATR, mode 2: scale / shift of this thread's four A rows (channels)
    if constexpr (ATR && A_KM) {
      const int gc = m0 + 4 * (st % (BM / 4));
#pragma unroll
      for (int e = 0; e < 4; ++e) if (FULL || gc + e < p.M) { kmsc[e] = p.ascale[gc + e]; kmsh[e] = p.ashift[gc + e]; }
    }
    auto store = [&](int s, const RawA& dA, const RawB& dB) {
      unsigned char* base = smem_dyn + (s & 1) * STAGE;
#if X3P_EXP & 32
      {                                                          // experiment: no split, no LDS stores (the loads stay: one value kept live)
        float acc0 = 0.f;
        for (int i = 0; i < X3P_RAW(BM); ++i) acc0 += dA[i].x + dA[i].y + dA[i].z + dA[i].w;
        for (int i = 0; i < X3P_RAW(BN); ++i) acc0 += dB[i].x + dB[i].y + dB[i].z + dB[i].w;
        if (acc0 == 12345.678f) base[st] = 1;
        return;
      }
#endif
#if X3P_EXP & 16
      {                                                          // experiment: LDS stores of unsplit bits (no float arithmetic)
        for (int i = 0; i < X3P_RAW(BM); ++i) {
          const uint4 u = __builtin_bit_cast(uint4, dA[i]);
          uint2* d = reinterpret_cast<uint2*>(base + ((st + i * X3P_STAGERS) * 8) % A_PL);
          d[0] = make_uint2(u.x, u.y); d[A_PL / 8] = make_uint2(u.z, u.w); d[2 * A_PL / 8] = make_uint2(u.x ^ u.z, u.y ^ u.w);
        }
        for (int i = 0; i < X3P_RAW(BN); ++i) {
          const uint4 u = __builtin_bit_cast(uint4, dB[i]);
          uint2* d = reinterpret_cast<uint2*>(base + 3 * A_PL + ((st + i * X3P_STAGERS) * 8) % B_PL);
          d[0] = make_uint2(u.x, u.y); d[B_PL / 8] = make_uint2(u.z, u.w); d[2 * B_PL / 8] = make_uint2(u.x ^ u.z, u.y ^ u.w);
        }
        return;
      }
#endif
      if constexpr (ATR) {
        float4 tA[X3P_RAW(BM)];
        const int k0 = kbeg + s * PBK;
        auto tr1 = [](float v, float sc, float sh) { return relu6f(fmaf(v, sc, sh)); };
        if constexpr (!A_KM) {
#pragma unroll
          for (int it = 0; it < X3P_ITEMS(BM); ++it) {
            const int k4 = (st + it * X3P_STAGERS) % X3P_K4, kabs = k0 + 4 * k4;
            const float4 sc = *reinterpret_cast<const float4*>(atab + kabs), sh = *reinterpret_cast<const float4*>(atab + TR_TAB + kabs);
            float4 v = dA[it];
            v.x = tr1(v.x, sc.x, sh.x); v.y = tr1(v.y, sc.y, sh.y); v.z = tr1(v.z, sc.z, sh.z); v.w = tr1(v.w, sc.w, sh.w);
            if constexpr (!FULL) {                                                // k past the range contributes nothing (the raw item holds 0 there)
              if (kabs >= kend) v.x = 0.f; if (kabs + 1 >= kend) v.y = 0.f; if (kabs + 2 >= kend) v.z = 0.f; if (kabs + 3 >= kend) v.w = 0.f;
            }
            tA[it] = v;
          }
          x3p_store_rm<BM, NPL>(base, A_PL, st, tA);
        } else {
#pragma unroll
          for (int it = 0; it < X3P_KITEMS(BM); ++it) {
            const int idx = st + it * X3P_STAGERS, kp = idx / (BM / 4), c4 = idx % (BM / 4);
            const int gk = k0 + 2 * kp, gc = m0 + 4 * c4;
            static_assert(!(ATR && A_KM) || X3P_KITEMS(BM) == 1, "one k-major item per staging thread: its four channels are fixed over the stages");
            const float (&sc)[4] = kmsc, (&sh)[4] = kmsh; (void)gc;
            float4 a = dA[2 * it], b = dA[2 * it + 1];
            a.x = tr1(a.x, sc[0], sh[0]); a.y = tr1(a.y, sc[1], sh[1]); a.z = tr1(a.z, sc[2], sh[2]); a.w = tr1(a.w, sc[3], sh[3]);
            b.x = tr1(b.x, sc[0], sh[0]); b.y = tr1(b.y, sc[1], sh[1]); b.z = tr1(b.z, sc[2], sh[2]); b.w = tr1(b.w, sc[3], sh[3]);
            if constexpr (!FULL) {
              if (gk >= kend) a = make_float4(0.f, 0.f, 0.f, 0.f);
              if (gk + 1 >= kend) b = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            tA[2 * it] = a; tA[2 * it + 1] = b;
          }
          x3p_store_km<BM, NPL>(base, A_PL, st, tA);
        }
      }
      else if constexpr (A_KM) x3p_store_km<BM, NPL>(base, A_PL, st, dA); else x3p_store_rm<BM, NPL>(base, A_PL, st, dA);
#if X3P_EXP & 128
      return;
#endif
#if X3P_EXP & 256
      {                                                          // experiment: B without split arithmetic (what pre-split weight planes would leave)
        for (int i = 0; i < X3P_RAW(BN); ++i) {
          const uint4 u = __builtin_bit_cast(uint4, dB[i]);
          uint2* d = reinterpret_cast<uint2*>(base + 3 * A_PL + ((st + i * X3P_STAGERS) * 8) % B_PL);
          d[0] = make_uint2(u.x, u.y); d[B_PL / 8] = make_uint2(u.z, u.w); d[2 * B_PL / 8] = make_uint2(u.x ^ u.z, u.y ^ u.w);
        }
        return;
      }
#endif
      if constexpr (B_KM) x3p_store_km<BN, NPL>(base + NPL * A_PL, B_PL, st, dB); else x3p_store_rm<BN, NPL>(base + NPL * A_PL, B_PL, st, dB);
    };
    if (nst > 0) {
      load(0, rawA[0], rawB[0]); load(1, rawA[1], rawB[1]);
      store(0, rawA[0], rawB[0]); load(2, rawA[0], rawB[0]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                                               // barrier 0: stage 0 is in LDS
      int s = 0;
      X3P_TRC();
      for (; s + 2 <= nst; s += 2) {                                              // straight-line pairs: the loads in flight stay countable
        store(s + 1, rawA[1], rawB[1]); load(s + 3, rawA[1], rawB[1]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        X3P_TRC();
        __builtin_amdgcn_s_barrier();                                             // end of stage s: stage s+1 is in LDS, slot s & 1 is free
        X3P_TRC();
        store(s + 2, rawA[0], rawB[0]); load(s + 4, rawA[0], rawB[0]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        X3P_TRC();
        __builtin_amdgcn_s_barrier();                                             // end of stage s+1
        X3P_TRC();
      }
      if (s < nst) {                                                              // odd count: the last stage's end
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    return;
  }
  // -------------------------------------------------------------------- MFMA waves
  const int half = lane >> 5, l31 = lane & 31;
  const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * 64;
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  if (nst > 0) {
    __builtin_amdgcn_s_barrier();                                                 // barrier 0
    constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};         // lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi: small terms first
    constexpr int T0 = NPL == 3 ? 0 : 3;                                          // two planes: the last three products
    for (int s = 0; s < nst; ++s) {
      const unsigned char* As = smem_dyn + (s & 1) * STAGE;
      const unsigned char* Bs = As + NPL * A_PL;
#pragma unroll
      for (int ks = 0; ks < PBK / 16; ++ks) {
        bf16x8 fa[3][TM], fb[3][TN];
#if X3P_EXP & 64
        if (s > 0) {                                              // experiment: no fragment reads after the first stage
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[pl][i] = __builtin_bit_cast(bf16x8, make_uint4(lane + pl, s, i, ks));
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[pl][j] = __builtin_bit_cast(bf16x8, make_uint4(lane - pl, s, j, ks));
          }
        } else
#endif
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
          for (int i = 0; i < TM; ++i) fa[pl][i] = x3p_frag<A_KM, BM>(As + pl * A_PL, wm0 + i * 32, ks, half, l31);
#pragma unroll
          for (int j = 0; j < TN; ++j) {
#if X3P_EXP & 128
            { fb[pl][j] = __builtin_bit_cast(bf16x8, make_uint4(lane - pl, s, j, ks)); continue; }
#endif
            fb[pl][j] = x3p_frag<B_KM, BN>(Bs + pl * B_PL, wn0 + j * 32, ks, half, l31);
          }
        }
#pragma unroll
        for (int t = T0; t < 6; ++t)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA[t]][i], fb[PB[t]][j], acc[i][j], 0, 0, 0);
      }
      X3P_TRC();
      __builtin_amdgcn_s_barrier();                                               // end of stage s
      X3P_TRC();
    }
  }
  gemm_tile_epilogue<BN, TM, TN, FULL, BNB>(p, acc, smem_dyn, tid, m0, n0, tm, wm0, wn0, ksplit);
}


// Same contract as crnn_gemm_f32 (include/crnn_mi355x.h); products in bf16, accumulation in fp32.  dtA/dtB/dtC give
// the storage of A, B and C (CRNN_F32 | CRNN_BF16); leading dimensions are in elements of the respective type.
static bool xcd_split_off() { return crnn_knob("CRNN_XSPLIT", 1) == 0; }
struct BnBwdEpilogue { const float* d; int ldd; const float* bnstate; float* partials; };   // GemmParams::bnD .. bnpart
static int gemm_bf16_impl(int mode, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb,
                          int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                          size_t scratch_bytes, int dtA, int dtB, int dtC, float* stats, hipStream_t stream,
                          const float* cscale = nullptr, const float* cshift = nullptr, const float* ascale = nullptr,
                          const float* ashift = nullptr, bool x3 = false, const BnBwdEpilogue* bnb = nullptr, int nplanes = 3) {
  if (M <= 0 || N <= 0 || K <= 0) return CRNN_ERR_ARG;
  if (nplanes != 3 && (nplanes != 2 || !x3)) return CRNN_ERR_ARG;
  if (bnb && (bias || act || accumulate || permP || stats || cscale || ascale || dtC != CRNN_F32 || !bnb->d || !bnb->bnstate || !bnb->partials)) return CRNN_ERR_ARG;
  if (x3 && (dtA != CRNN_F32 || dtB != CRNN_F32)) return CRNN_ERR_ARG;   // three-plane products: fp32 operands
  if (x3 && ascale && (mode == 1 || (mode == 0 && K > TR_TAB) || bnb)) return CRNN_ERR_UNSUPPORTED;   // producer prologue of the three-plane kernel: modes 0 and 2
  if (permP && (M % permP) != 0) return CRNN_ERR_ARG;
  if (stats && (bias || act || accumulate || permP || scratch || cscale)) return CRNN_ERR_ARG;   // statistics of the plain product only
  if (cscale && (scratch || accumulate || !cshift)) return CRNN_ERR_ARG;                          // no split reduction with the folded BatchNorm
  GemmParams p;
#ifdef CRNN_GEMM_EXP
  p.exp = crnn_knob("CRNN_GEMM_EXP", 0);
  { const char* e = getenv("CRNN_GEMM_TRACE"); p.trace = e ? (unsigned long long*)strtoull(e, nullptr, 0) : nullptr; }
#endif
  p.stats = stats; p.cscale = cscale; p.cshift = cshift; p.ascale = ascale; p.ashift = ashift;
  p.bnD = bnb ? bnb->d : nullptr; p.ldd = bnb ? bnb->ldd : 0; p.bnstate = bnb ? bnb->bnstate : nullptr; p.bnpart = bnb ? bnb->partials : nullptr;
  if ((ascale != nullptr) != (ashift != nullptr)) return CRNN_ERR_ARG;
  p.A = (const float*)A; p.B = (const float*)B; p.C = (float*)C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.bias = bias; p.act = act; p.accumulate = accumulate; p.permP = permP;
  p.dtA = dtA; p.dtB = dtB; p.dtC = dtC;
  const bool a_km = (mode == 2), b_km = (mode != 1);
  // vector accesses: 16 bytes per lane (4 fp32 or 8 bf16 elements)
  auto vw = [](int dt) { return dt == CRNN_BF16 ? 8 : 4; };
  p.vecA = aligned16(A) && (lda % vw(dtA) == 0) && ((a_km ? M : K) % vw(dtA) == 0);
  p.vecB = aligned16(B) && (ldb % vw(dtB) == 0) && ((b_km ? N : K) % vw(dtB) == 0);
  p.vecC = aligned16(C) && (ldc % vw(dtC) == 0) && (N % vw(dtC) == 0) && (!scratch || aligned16(scratch));
  if (ascale && !x3) {   // producer prologue: bf16 operands, 16-byte loads of A, channel table in LDS
    if (dtA != CRNN_BF16 || dtB != CRNN_BF16 || !p.vecA) return CRNN_ERR_UNSUPPORTED;
    if (mode != 2 && K > TR_TAB) return CRNN_ERR_UNSUPPORTED;
  }
  const int bn_env = crnn_knob("CRNN_GEMM_BN", 0);   // 64 forces the 128x64 tile
  const int BN = (N <= 64 || bn_env == 64) ? 64 : 128;
  const int tilesM = cdiv(M, 128), tilesN = cdiv(N, BN);
  p.tilesN = tilesN;
  int tiles = tilesM * tilesN;
  int nsplit = 1;
  const int split_target = x3 ? 512 : crnn_knob("CRNN_SPLIT_WGS", 768);   // workgroups a split reduction aims for: 3 resident per CU (X3: one, two rounds)
  // (round 6, plane products without a bias -- gradients: at most 128 tiles leave more than half of the CUs idle for three to six products per k-step: split those
  // too.  Products with a bias are forward layers: their summation order stays what it was at every batch size, so that an inference result does not change with it.)
  if (scratch && ((tiles < 256 && K >= 2048) || (tiles <= 16 && K >= 512) || (x3 && !bias && tiles <= 128 && K >= 512 && crnn_knob("CRNN_X3_SMALL_SPLIT", 1)))) {
    nsplit = cdiv(split_target, tiles);
    int maxs = K / (K >= 2048 ? 512 : 128); if (maxs < 1) maxs = 1;
    if (nsplit > maxs) nsplit = maxs;
    size_t per = (size_t)M * N * sizeof(float);
    size_t fit = scratch_bytes / per;
    if ((size_t)nsplit > fit) nsplit = (int)fit;
    if (nsplit < 1) nsplit = 1;
  }
  int klen = cdiv(K, nsplit);
  klen = ((klen + HBK - 1) / HBK) * HBK;
  nsplit = cdiv(K, klen);
  p.xsplit = 0;
  if (nsplit >= 8 && !xcd_split_off()) {   // K ranges pinned to XCDs: the split count becomes a multiple of 8 (empty tail ranges write zeros)
    const int ns8 = ((nsplit + 7) / 8) * 8;
    if ((size_t)ns8 * M * N * sizeof(float) <= scratch_bytes) {
      klen = cdiv(K, ns8); klen = ((klen + HBK - 1) / HBK) * HBK;
      nsplit = ns8; p.xsplit = ns8;
    }
  }
  p.klen = klen;
  GemmParams pk = p;
  if (nsplit > 1) pk.C = scratch;
  dim3 grid(p.xsplit ? tiles * nsplit : tiles, p.xsplit ? 1 : nsplit), block(256);
  // every tile whole, every k-chunk whole, 16-byte accesses legal: the unguarded instantiation
  const bool full = (M % 128 == 0) && (N % BN == 0) && (K % HBK == 0) && p.vecA && p.vecB && p.vecC && crnn_knob("CRNN_GEMM_FULL", 1);
  // the BatchNorm-backward statistics live in the unguarded epilogue of an unsplit product: whole tiles, 16-byte accesses to d and the state
  if (bnb && (!full || nsplit > 1 || (bnb->ldd & 3) || ((uintptr_t)bnb->d & 15) || ((uintptr_t)bnb->bnstate & 15))) return CRNN_ERR_UNSUPPORTED;
#define LAUNCH(BNV, AK, BKM, ABF, BBF) do { if (full) hipLaunchKernelGGL((gemm_bf16_kernel<BNV, AK, BKM, ABF, BBF, false, true>), grid, block, 0, stream, pk); \
                                            else hipLaunchKernelGGL((gemm_bf16_kernel<BNV, AK, BKM, ABF, BBF>), grid, block, 0, stream, pk); } while (0)
#define LAUNCH_BN(AK, BKM, ABF, BBF) do { if (BN == 128) LAUNCH(128, AK, BKM, ABF, BBF); else LAUNCH(64, AK, BKM, ABF, BBF); } while (0)
  const bool abf = (dtA == CRNN_BF16), bbf = (dtB == CRNN_BF16);
#define LAUNCH_DT(AK, BKM) do { if (abf && bbf) LAUNCH_BN(AK, BKM, true, true); else if (abf) LAUNCH_BN(AK, BKM, true, false); \
                              else if (bbf) LAUNCH_BN(AK, BKM, false, true); else LAUNCH_BN(AK, BKM, false, false); } while (0)
#define LAUNCH_TR(AK, BKM) do { if (BN == 128 && full) hipLaunchKernelGGL((gemm_bf16_kernel<128, AK, BKM, true, true, true, true>), grid, block, 0, stream, pk); \
                              else if (BN == 128) hipLaunchKernelGGL((gemm_bf16_kernel<128, AK, BKM, true, true, true>), grid, block, 0, stream, pk); \
                              else if (full) hipLaunchKernelGGL((gemm_bf16_kernel<64, AK, BKM, true, true, true, true>), grid, block, 0, stream, pk); \
                              else hipLaunchKernelGGL((gemm_bf16_kernel<64, AK, BKM, true, true, true>), grid, block, 0, stream, pk); } while (0)
  // three planes per operand: dynamic LDS (each instantiation raises its limit once per device), one workgroup per CU
#define LAUNCH_X3(BNV, AK, BKM, FL) do { constexpr int lds3 = 3 * ((AK ? HBK * KLD(128) * 2 : 128 * HLD * 2) + (BKM ? HBK * KLD(BNV) * 2 : BNV * HLD * 2)); \
    CRNN_LDS_ATTR((gemm_bf16_kernel<BNV, AK, BKM, false, false, false, FL, true>), lds3); \
    hipLaunchKernelGGL((gemm_bf16_kernel<BNV, AK, BKM, false, false, false, FL, true>), grid, block, lds3, stream, pk); } while (0)
#define LAUNCH_X3M(AK, BKM) do { if (BN == 128) { if (full) LAUNCH_X3(128, AK, BKM, true); else LAUNCH_X3(128, AK, BKM, false); } \
                                 else { if (full) LAUNCH_X3(64, AK, BKM, true); else LAUNCH_X3(64, AK, BKM, false); } } while (0)
  // producer-wave kernel (768 threads, two 32-k stages in LDS); -DCRNN_X3_INWAVE keeps the in-wave pipeline above for scripts/gemm_x3_trace.py
#define LAUNCH_X3P(BNV, AK, BKM, FL, NPLV) do { constexpr int ldsr = 2 * NPLV * ((AK ? PBK * KLD(128) * 2 : 128 * PLD * 2) + (BKM ? PBK * KLD(BNV) * 2 : BNV * PLD * 2)); \
    constexpr int ldsp = ldsr > 36 * 1024 ? ldsr : 36 * 1024;   /* (the epilogue's staging tile reuses the stages: <= 34.8 KiB) */ \
    CRNN_LDS_ATTR((gemm_x3p_kernel<BNV, AK, BKM, FL, false, false, NPLV>), ldsp); \
    hipLaunchKernelGGL((gemm_x3p_kernel<BNV, AK, BKM, FL, false, false, NPLV>), grid, dim3(256 + X3P_STAGERS), ldsp, stream, pk); } while (0)
#define LAUNCH_X3PN(BNV, AK, BKM, FL) do { if (nplanes == 2) LAUNCH_X3P(BNV, AK, BKM, FL, 2); else LAUNCH_X3P(BNV, AK, BKM, FL, 3); } while (0)
#define LAUNCH_X3PM(AK, BKM) do { if (BN == 128) { if (full) LAUNCH_X3PN(128, AK, BKM, true); else LAUNCH_X3PN(128, AK, BKM, false); } \
                                  else { if (full) LAUNCH_X3PN(64, AK, BKM, true); else LAUNCH_X3PN(64, AK, BKM, false); } } while (0)
  if (bnb) {      // (x3, mode 1, whole tiles: checked above)
    if (!x3 || mode != 1) return CRNN_ERR_UNSUPPORTED;
    constexpr int l128 = 2 * 3 * (128 * PLD * 2 + 128 * PLD * 2), l64 = 2 * 3 * (128 * PLD * 2 + 64 * PLD * 2);
#define LAUNCH_X3PB(NPLV) do { \
    if (BN == 128) { CRNN_LDS_ATTR((gemm_x3p_kernel<128, false, false, true, true, false, NPLV>), l128 / 3 * NPLV); \
                     hipLaunchKernelGGL((gemm_x3p_kernel<128, false, false, true, true, false, NPLV>), grid, dim3(256 + X3P_STAGERS), l128 / 3 * NPLV, stream, pk); } \
    else { CRNN_LDS_ATTR((gemm_x3p_kernel<64, false, false, true, true, false, NPLV>), l64 / 3 * NPLV); \
           hipLaunchKernelGGL((gemm_x3p_kernel<64, false, false, true, true, false, NPLV>), grid, dim3(256 + X3P_STAGERS), l64 / 3 * NPLV, stream, pk); } } while (0)
    static_assert(l64 / 3 * 2 >= 128 * (64 + 4) * 4 && l128 / 3 * 2 >= 64 * (128 + 4) * 4, "the epilogue's staging tile fits the two-plane stages");
    if (nplanes == 2) LAUNCH_X3PB(2); else LAUNCH_X3PB(3);
#undef LAUNCH_X3PB
  } else
  if (x3 && ascale) {   // modes 0 / 2 with the producer prologue (+ 4 KiB of LDS for mode 0's channel table)
#define LAUNCH_X3PT(BNV, AK, BKM, FL, NPLV) do { constexpr int ldsr = 2 * NPLV * ((AK ? PBK * KLD(128) * 2 : 128 * PLD * 2) + (BKM ? PBK * KLD(BNV) * 2 : BNV * PLD * 2)); \
    constexpr int ldst = (ldsr > 36 * 1024 ? ldsr : 36 * 1024) + (AK ? 0 : 2 * TR_TAB * 4);   /* (the epilogue's staging tile reuses the stages: <= 34.8 KiB) */ \
    static_assert(!(NPLV == 2 && !AK) || ldsr >= 36 * 1024, "mode 0: the channel table sits right behind the stages"); \
    CRNN_LDS_ATTR((gemm_x3p_kernel<BNV, AK, BKM, FL, false, true, NPLV>), ldst); \
    hipLaunchKernelGGL((gemm_x3p_kernel<BNV, AK, BKM, FL, false, true, NPLV>), grid, dim3(256 + X3P_STAGERS), ldst, stream, pk); } while (0)
#define LAUNCH_X3PTN(BNV, AK, BKM, FL) do { if (nplanes == 2) LAUNCH_X3PT(BNV, AK, BKM, FL, 2); else LAUNCH_X3PT(BNV, AK, BKM, FL, 3); } while (0)
#define LAUNCH_X3PTM(AK, BKM) do { if (BN == 128) { if (full) LAUNCH_X3PTN(128, AK, BKM, true); else LAUNCH_X3PTN(128, AK, BKM, false); } \
                                   else { if (full) LAUNCH_X3PTN(64, AK, BKM, true); else LAUNCH_X3PTN(64, AK, BKM, false); } } while (0)
    if (mode == 0) LAUNCH_X3PTM(false, true); else LAUNCH_X3PTM(true, true);
#undef LAUNCH_X3PTM
#undef LAUNCH_X3PTN
#undef LAUNCH_X3PT
  } else
#ifdef CRNN_X3_INWAVE
  if (x3 && nplanes != 3) return CRNN_ERR_UNSUPPORTED;
  else if (x3) { if (mode == 0) LAUNCH_X3M(false, true); else if (mode == 1) LAUNCH_X3M(false, false); else LAUNCH_X3M(true, true); }
#else
  if (x3) { if (mode == 0) LAUNCH_X3PM(false, true); else if (mode == 1) LAUNCH_X3PM(false, false); else LAUNCH_X3PM(true, true); }
#endif
#undef LAUNCH_X3PM
#undef LAUNCH_X3PN
#undef LAUNCH_X3P
  else if (ascale) { if (mode == 0) LAUNCH_TR(false, true); else if (mode == 1) LAUNCH_TR(false, false); else LAUNCH_TR(true, true); }
  else if (mode == 0) LAUNCH_DT(false, true); else if (mode == 1) LAUNCH_DT(false, false); else LAUNCH_DT(true, true);
#undef LAUNCH_X3M
#undef LAUNCH_X3
#undef LAUNCH_TR
#undef LAUNCH_DT
#undef LAUNCH_BN
#undef LAUNCH
  CRNN_LAUNCH_CHECK();
  if (nsplit > 1) {
    launch_splitk_reduce(scratch, nsplit, p, stream);
    CRNN_LAUNCH_CHECK();
  }
  return CRNN_OK;
}
extern "C" int crnn_gemm_bf16_ex(int mode, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb,
                                 int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                                 size_t scratch_bytes, int dtA, int dtB, int dtC, hipStream_t stream) {
  return gemm_bf16_impl(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, accumulate, permP, scratch, scratch_bytes, dtA, dtB, dtC, nullptr, stream);
}
// fp32 in, fp32 out, fp32-accurate products from three bf16 planes per operand (six bf16 MFMAs per k-step instead of the eight four-times
// slower fp32 ones): the contract of crnn_gemm_f32 with results equal to it to fp32 round-off (not bit for bit) -- the parity mode's
// conv-stack / dense / RNN-projection GEMMs of the parity mode (unless crnn_config.flags has CRNN_FLAG_F32_MFMA_GEMMS).
extern "C" int crnn_gemm_f32x3(int mode, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb,
                               int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                               size_t scratch_bytes, hipStream_t stream) {
  return gemm_bf16_impl(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, accumulate, permP, scratch, scratch_bytes, CRNN_F32, CRNN_F32, CRNN_F32,
                        nullptr, stream, nullptr, nullptr, nullptr, nullptr, true);
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
extern "C" int crnn_gemm_f32x3_bnstats(const float* dq, const float* W, float* da, long M, int N, int K, const float* d, const float* bnstate,
                                       float* stat_partials, hipStream_t stream) {
  CRNN_TRY(crnn_gemm_f32x3_bnstats_supported(M, N, K));
  const BnBwdEpilogue e{d, N, bnstate, stat_partials};
  return gemm_bf16_impl(1, dq, W, da, (int)M, N, K, K, K, N, nullptr, 0, 0, 0, nullptr, 0, CRNN_F32, CRNN_F32, CRNN_F32, nullptr, stream, nullptr, nullptr,
                        nullptr, nullptr, true, &e);
}
// crnn_gemm_f32x3 with two planes per operand (hi*hi + hi*mid + mid*hi: 16 significant bits per factor): same contract
extern "C" int crnn_gemm_f32x2(int mode, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb,
                               int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                               size_t scratch_bytes, hipStream_t stream) {
  return gemm_bf16_impl(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, accumulate, permP, scratch, scratch_bytes, CRNN_F32, CRNN_F32, CRNN_F32,
                        nullptr, stream, nullptr, nullptr, nullptr, nullptr, true, nullptr, 2);
}
// Two-plane form of crnn_gemm_f32x3_bnstats: operands split into two bf16 planes, products hi*hi + hi*mid + mid*hi (16 significant bits per factor,
// fp32 accumulation; relative error of a product <= 3 * 2^-18): half the MFMA work.  The parity mode's default for the BACKWARD GEMMs of the conv stack.
extern "C" int crnn_gemm_f32x2_bnstats(const float* dq, const float* W, float* da, long M, int N, int K, const float* d, const float* bnstate,
                                       float* stat_partials, hipStream_t stream) {
  CRNN_TRY(crnn_gemm_f32x3_bnstats_supported(M, N, K));
  const BnBwdEpilogue e{d, N, bnstate, stat_partials};
  return gemm_bf16_impl(1, dq, W, da, (int)M, N, K, K, K, N, nullptr, 0, 0, 0, nullptr, 0, CRNN_F32, CRNN_F32, CRNN_F32, nullptr, stream, nullptr, nullptr,
                        nullptr, nullptr, true, &e, 2);
}
// The three bf16 planes of n fp32 values (n % 4 == 0, x 16-byte and planes 8-byte aligned, plane_stride % 4 == 0 elements): plane pl of x[i] at
// planes[pl * plane_stride + i] -- the words the three-plane kernel's staging waves form (split3_pair).
__global__ __launch_bounds__(256) void split3_planes_kernel(const float4* __restrict__ x, uint2* __restrict__ planes, long n4, long ps4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = x[i];
  unsigned a0, a1, a2, b0, b1, b2;
  split3_pair(v.x, v.y, a0, a1, a2);
  split3_pair(v.z, v.w, b0, b1, b2);
  planes[i] = make_uint2(a0, b0); planes[ps4 + i] = make_uint2(a1, b1); planes[2 * ps4 + i] = make_uint2(a2, b2);
}
extern "C" int crnn_split3_planes(const float* x, void* planes, long n, long plane_stride, hipStream_t stream) {
  if (n <= 0 || (n & 3) || (plane_stride & 3) || plane_stride < n || ((uintptr_t)x & 15) || ((uintptr_t)planes & 7)) return CRNN_ERR_ARG;
  hipLaunchKernelGGL(split3_planes_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, stream, (const float4*)x, (uint2*)planes, n / 4, plane_stride / 4);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
extern "C" int crnn_gemm_bf16(int mode, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb,
                              int ldc, const float* bias, int act, int accumulate, int permP, float* scratch,
                              size_t scratch_bytes, hipStream_t stream) {
  return crnn_gemm_bf16_ex(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, accumulate, permP, scratch, scratch_bytes, CRNN_F32, CRNN_F32,
                           CRNN_F32, stream);
}
