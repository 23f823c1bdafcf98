// fp32-accurate products from two / three bf16 planes per fp32 operand (the parity mode's GEMMs), on producer waves.
//
// x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (round-to-nearest-even each; the differences are exact
// in fp32): |x - (hi + mid + lo)| <= 2^-27 |x|.  A product keeps hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi (the dropped terms are
// <= 2^-26 of it) and every partial product of bf16 values is exact in the MFMA's fp32 accumulator: six v_mfma_f32_32x32x16_bf16
// (6 x 32 cycles per 32x32x16 block) replace the eight v_mfma_f32_32x32x2_f32 (8 x 64 cycles) of the fp32 kernel with fp32-level accuracy
// (not the bit pattern of an fmaf chain: crnn_gemm_f32 stays for that).  Non-finite inputs become NaN in all three planes' products.
// The split is crnn_split3_pair (common.h), the spelling every plane-forming kernel shares.
//
// Round 2 formed the planes in the four waves that multiply (an instantiation of the bf16 kernel, removed after commit 137e5be): 111-123 KiB
// of LDS, so one workgroup per CU had to stage (load fp32, split into planes, write LDS) and multiply in the same waves -- its trace shows
// 1.9 us of MFMAs inside a 4.1 us chunk (profiles/r03_gemm_x3_trace.txt).  Here a workgroup has 8 waves: waves 0-3 only multiply (128 x BN
// tile, 2x2 / 1x2 accumulators each, as in the bf16 kernel), waves 4-7 only stage.  A stage is 16 k; two stages live in LDS (2 x 3 planes x
// (A + B) = 72 KiB at BN = 128) and the kernel is held to 128 VGPRs, so TWO workgroups share a CU: one's barrier waits, prologue (first
// loads) and epilogue run under the other's MFMAs.  While the MFMA waves read stage s from slot s & 1, the staging waves split the fp32
// items they requested two stages earlier into the planes of stage s+1 and write them to slot (s+1) & 1 (released by the barrier that
// ended stage s-1), then request stage s+3.  One s_barrier per stage.
// Layouts: row-major-in-k planes bf16 [rows][16 + 8] (48-byte rows: the 8 lanes a ds_read_b128 serves per clock land in 8 different
// 16-byte slots), k-major planes bf16 [16 k][rows + 32] (the transposing reads of the 64-k kernel).  Same split, same six products in the
// same order per k-step, same epilogue as the in-wave form: results equal it to the last bit.
// Measured on 119808 x 512 x 512 (profiles/r03_gemm_x3_bench_variants.txt, r03_gemm_x3p_experiments.txt): fp32 MFMA 629 us; 32-k stages, one
// workgroup per CU, 4 staging waves 420 us (MFMA waves wait 0.4 of every 1.7 us for the planes); 8 staging waves 434; 16-k stages 402; two
// workgroups per CU 370 (41 % of the dense bf16 peak).  What is left (timing builds of that commit): no split arithmetic -20 %, no fragment
// reads -7 %, no B operand at all -27 %, MFMAs + A loads only -28 %: the float VALU work of the split shares issue with the matrix pipe
// (scripts/probes/mfma_valu_probe.hip: integer VALU of another wave overlaps MFMAs, v_sub_f32 / v_cvt_pk_bf16_f32 only partly).  Forming the
// last (and the middle) plane by v_perm_b32 instead of a conversion: K = 64 shape -13 %, K >= 256 shapes + 3..5 % (the schedule around the
// MFMAs shifts; profiles/r04_x3_split_variants.txt): not adopted.
#include "gemm_tile.h"

constexpr int PBK = 16;                  // k per stage
constexpr int PLD = PBK + 8;
constexpr int X3P_STAGERS = 256;         // staging threads (4 waves: one per SIMD beside its MFMA wave)
constexpr int X3P_WGS = 2;               // workgroups per CU the register budget is held to (2 x 8 waves = 4 per SIMD, 128 VGPRs)
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
    crnn_split3_pair(raw[it].x, raw[it].y, a0, a1, a2);
    crnn_split3_pair(raw[it].z, raw[it].w, b0, b1, b2);
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
    crnn_split3_pair(a.x, a.y, w[0][0], w[0][1], w[0][2]); crnn_split3_pair(a.z, a.w, w[1][0], w[1][1], w[1][2]);
    crnn_split3_pair(b.x, b.y, w[2][0], w[2][1], w[2][2]); crnn_split3_pair(b.z, b.w, w[3][0], w[3][1], w[3][2]);
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

// Dynamic LDS of gemm_x3p_kernel<BN, A_KM, B_KM, ..., ATR, NPL>: two stages of NPL planes per operand -- at least the 36 KiB the epilogue's staging
// tile (<= 34.8 KiB, it reuses the stages) is given -- plus, for the mode-0 prologue, the [scale | shift] x TR_TAB channel table behind the stages.
constexpr int x3p_plane_bytes(int rows, bool km) { return km ? PBK * KLD(rows) * 2 : rows * PLD * 2; }
constexpr int x3p_stage_bytes(int BN, bool A_KM, bool B_KM, int NPL) { return NPL * (x3p_plane_bytes(128, A_KM) + x3p_plane_bytes(BN, B_KM)); }
constexpr int x3p_table_bytes(bool A_KM, bool ATR) { return ATR && !A_KM ? 2 * TR_TAB * 4 : 0; }
constexpr int x3p_lds_bytes(int BN, bool A_KM, bool B_KM, bool ATR, int NPL) {
  const int stages = 2 * x3p_stage_bytes(BN, A_KM, B_KM, NPL);
  return (stages > 36 * 1024 ? stages : 36 * 1024) + x3p_table_bytes(A_KM, ATR);
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
  constexpr int A_PL = x3p_plane_bytes(BM, A_KM), B_PL = x3p_plane_bytes(BN, B_KM);   // bytes of one plane
  constexpr int STAGE = NPL * (A_PL + B_PL);
  constexpr int LDS = x3p_lds_bytes(BN, A_KM, B_KM, ATR, NPL);                        // what the launcher provides
  static_assert(STAGE == x3p_stage_bytes(BN, A_KM, B_KM, NPL) && 2 * STAGE + x3p_table_bytes(A_KM, ATR) <= LDS, "two stages, and the channel table right behind them");
  static_assert(64 * (BN + 4) * 4 <= LDS && (!BNB || (256 / (BN / 4)) * 2 * BN * 4 <= LDS), "the epilogue's staging tile and the BatchNorm-backward partial rows reuse the stages");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];      // two stages; the epilogue's 33 KiB staging tile reuses them
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const TileCoord tc = gemm_tile_coord(p);
  const int tm = tc.tm, tn = tc.tn, ksplit = tc.ksplit;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = ksplit * p.klen;
  const int kend = min(p.K, kbeg + p.klen);
  const int nst = kend > kbeg ? (kend - kbeg + PBK - 1) / PBK : 0;              // stages of this K range
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
      if constexpr (B_KM) x3p_store_km<BN, NPL>(base + NPL * A_PL, B_PL, st, dB); else x3p_store_rm<BN, NPL>(base + NPL * A_PL, B_PL, st, dB);
    };
    if (nst > 0) {
      load(0, rawA[0], rawB[0]); load(1, rawA[1], rawB[1]);
      store(0, rawA[0], rawB[0]); load(2, rawA[0], rawB[0]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                                               // barrier 0: stage 0 is in LDS
      int s = 0;
      for (; s + 2 <= nst; s += 2) {                                              // straight-line pairs: the loads in flight stay countable
        store(s + 1, rawA[1], rawB[1]); load(s + 3, rawA[1], rawB[1]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                             // end of stage s: stage s+1 is in LDS, slot s & 1 is free
        store(s + 2, rawA[0], rawB[0]); load(s + 4, rawA[0], rawB[0]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                             // end of stage s+1
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
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
          for (int i = 0; i < TM; ++i) fa[pl][i] = x3p_frag<A_KM, BM>(As + pl * A_PL, wm0 + i * 32, ks, half, l31);
#pragma unroll
          for (int j = 0; j < TN; ++j) fb[pl][j] = x3p_frag<B_KM, BN>(Bs + pl * B_PL, wn0 + j * 32, ks, half, l31);
        }
#pragma unroll
        for (int t = T0; t < 6; ++t)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[PA[t]][i], fb[PB[t]][j], acc[i][j], 0, 0, 0);
      }
      __builtin_amdgcn_s_barrier();                                               // end of stage s
    }
  }
  gemm_tile_epilogue<BN, TM, TN, FULL, BNB>(p, acc, smem_dyn, tid, m0, n0, tm, wm0, wn0, ksplit);
}

namespace crnn_tile {

// one instantiation's launch: dynamic LDS (its limit is raised once per device), 8 waves
template <int BN, bool A_KM, bool B_KM, bool FULL, bool BNB, bool ATR, int NPL>
static int launch_x3p(const TileGemm& g, const TilePlan& t) {
  constexpr int lds = x3p_lds_bytes(BN, A_KM, B_KM, ATR, NPL);
  CRNN_LDS_ATTR((gemm_x3p_kernel<BN, A_KM, B_KM, FULL, BNB, ATR, NPL>), lds);
  hipLaunchKernelGGL((gemm_x3p_kernel<BN, A_KM, B_KM, FULL, BNB, ATR, NPL>), t.grid, dim3(256 + X3P_STAGERS), lds, g.stream, t.pk);
  return CRNN_OK;
}
// (planes, BN, whole tiles) -> the instantiation of one (mode, epilogue, prologue) form
template <bool A_KM, bool B_KM, bool BNB, bool ATR>
static int launch_x3p_form(const TileGemm& g, const TilePlan& t) {
  const bool wide = t.BN == 128;
  if constexpr (BNB) {   // whole tiles only (checked by the planner)
    if (g.product == PRODUCT_PLANES2) return wide ? launch_x3p<128, A_KM, B_KM, true, true, ATR, 2>(g, t) : launch_x3p<64, A_KM, B_KM, true, true, ATR, 2>(g, t);
    return wide ? launch_x3p<128, A_KM, B_KM, true, true, ATR, 3>(g, t) : launch_x3p<64, A_KM, B_KM, true, true, ATR, 3>(g, t);
  } else {
    if (g.product == PRODUCT_PLANES2) {
      if (wide) return t.full ? launch_x3p<128, A_KM, B_KM, true, false, ATR, 2>(g, t) : launch_x3p<128, A_KM, B_KM, false, false, ATR, 2>(g, t);
      return t.full ? launch_x3p<64, A_KM, B_KM, true, false, ATR, 2>(g, t) : launch_x3p<64, A_KM, B_KM, false, false, ATR, 2>(g, t);
    }
    if (wide) return t.full ? launch_x3p<128, A_KM, B_KM, true, false, ATR, 3>(g, t) : launch_x3p<128, A_KM, B_KM, false, false, ATR, 3>(g, t);
    return t.full ? launch_x3p<64, A_KM, B_KM, true, false, ATR, 3>(g, t) : launch_x3p<64, A_KM, B_KM, false, false, ATR, 3>(g, t);
  }
}

int gemm_tile_planes(const TileGemm& g) {
  if (!g.planes()) return CRNN_ERR_ARG;
  TilePlan t;
  CRNN_TRY(plan_tile_gemm(g, HBK, kPlanesSplitWorkgroups, kPlanesSmallSplit, kXcdPinnedSplit, t));
  // the forms the kernel is built in: the BatchNorm-backward epilogue in mode 1, the staging prologue in modes 0 and 2 (the planner refuses the rest)
  if (g.bnb) CRNN_TRY((launch_x3p_form<false, false, true, false>(g, t)));
  else if (g.ascale && g.mode == 0) CRNN_TRY((launch_x3p_form<false, true, false, true>(g, t)));
  else if (g.ascale) CRNN_TRY((launch_x3p_form<true, true, false, true>(g, t)));
  else if (g.mode == 0) CRNN_TRY((launch_x3p_form<false, true, false, false>(g, t)));
  else if (g.mode == 1) CRNN_TRY((launch_x3p_form<false, false, false, false>(g, t)));
  else CRNN_TRY((launch_x3p_form<true, true, false, false>(g, t)));
  return finish_tile_gemm(g, t);
}

}  // namespace crnn_tile

// The three bf16 planes of n fp32 values (n % 4 == 0, x 16-byte and planes 8-byte aligned, plane_stride % 4 == 0 elements): plane pl of x[i] at
// planes[pl * plane_stride + i] -- the words the plane kernel's staging waves form (crnn_split3_pair).
__global__ __launch_bounds__(256) void split3_planes_kernel(const float4* __restrict__ x, uint2* __restrict__ planes, long n4, long ps4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = x[i];
  unsigned a0, a1, a2, b0, b1, b2;
  crnn_split3_pair(v.x, v.y, a0, a1, a2);
  crnn_split3_pair(v.z, v.w, b0, b1, b2);
  planes[i] = make_uint2(a0, b0); planes[ps4 + i] = make_uint2(a1, b1); planes[2 * ps4 + i] = make_uint2(a2, b2);
}
extern "C" int crnn_split3_planes(const float* x, void* planes, long n, long plane_stride, hipStream_t stream) {
  if (n <= 0 || (n & 3) || (plane_stride & 3) || plane_stride < n || ((uintptr_t)x & 15) || ((uintptr_t)planes & 7)) return CRNN_ERR_ARG;
  hipLaunchKernelGGL(split3_planes_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, stream, (const float4*)x, (uint2*)planes, n / 4, plane_stride / 4);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
