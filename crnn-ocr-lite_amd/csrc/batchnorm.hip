// BatchNorm of the conv stack (axis = -1), NHWC, 16-byte vectors: apply (+ReLU6 +MaxPool +Dropout, + the pool windows' arg-max values) and the two-pass
// backward through Dropout / MaxPool / ReLU6 (statistics pass, apply pass; dx as a tensor or as bf16 planes).  The second stages that sit between the
// passes are reduce.hip's.  HBM-bandwidth bound but for the pooled backward kernels (VALU-bound, see there).
#include "common.h"
#include "conv_vec.h"

// Cache policy of the streaming passes (round 5).  The 256 MB last-level cache holds about two of the conv stack's 123 MB tensors; a pass that reads a
// tensor for the LAST time in the step (or for the last time before the other half of the step) loads it nontemporally so that it does not push out what the
// next kernel is about to read (its own output, the tensors still to be re-read).  Same values, same order: results bit-identical.  Measured on the bf16s step
// (profiles/r05_nt_loads_ab.txt): BatchNorm-backward apply pass -0.03 ms, depthwise-stage backward -0.07 ms, together with the forward passes -0.2 ms.
constexpr bool kNtBnBwd2 = true;   // BatchNorm backward, apply pass: q and g are read for the last time (profiles/r05_nt_loads_ab.txt)
constexpr bool kNtBnAct = true;    // BatchNorm-2 + ReLU6 + pool + dropout (forward): q is not read again before the backward pass (same file)

// ---------------------------------------------------------------------------------------------
// y = Dropout(MaxPool(ReLU6(x*scale+shift)))   (utils.py:45-56).  ph=pw=1: no pooling; rate=0: no dropout.
// x [B,H,W,C] -> y [B,H/ph,W/pw,C]
// ---------------------------------------------------------------------------------------------
// IDX: index type of the element counter -- unsigned (32-bit divisions: ~25 VALU instructions each) whenever the tensor has fewer than 2^31
// vectors, long otherwise (64-bit divisions cost ~100 each, and a vector needs two to five of them against ~60 instructions of payload).
// PHT x PWT: the pool window as compile-time constants (0 x 0: run-time ph x pw).
template <int VEC, typename TI, typename TO, typename IDX, int PHT, int PWT>
__global__ void bn_act_pool_drop_kernel(const TI* __restrict__ x, const float* __restrict__ bnstate,
                                        TO* __restrict__ y, int B, int H, int W, int C, int ph_, int pw_, float rate,
                                        uint64_t seed, uint32_t layer, TI* __restrict__ qmax = nullptr) {
  const int ph = PHT ? PHT : ph_, pw = PWT ? PWT : pw_;
  const int Ho = H / ph, Wo = W / pw, CL = C / VEC;
  const IDX total = (IDX)((long)B * Ho * Wo * CL);
  const float inv_keep = rate > 0.f ? 1.f / (1.f - rate) : 1.f;
  const float* sc = bnstate + 2 * C; const float* sh = bnstate + 3 * C;
  for (IDX i = (IDX)blockIdx.x * (IDX)blockDim.x + threadIdx.x; i < total; i += (IDX)gridDim.x * (IDX)blockDim.x) {
    const int cl = (int)(i % (IDX)CL); const IDX pix = i / (IDX)CL;
    VecF<VEC> m, s = vload<VEC>(sc + cl * VEC), t = vload<VEC>(sh + cl * VEC);
    if (ph * pw == 1) {
      VecF<VEC> v = vload_s<VEC, kNtBnAct>(&x[(long)pix * C + cl * VEC]);
#pragma unroll
      for (int e = 0; e < VEC; ++e) m.v[e] = relu6f(fmaf(v.v[e], s.v[e], t.v[e]));
    } else {
      const int wo = (int)(pix % (IDX)Wo); const IDX r = pix / (IDX)Wo; const int ho = (int)(r % (IDX)Ho); const long b = (long)(r / (IDX)Ho);
#pragma unroll
      for (int e = 0; e < VEC; ++e) m.v[e] = -INFINITY;
      const long base = ((b * H + (long)ho * ph) * W + (long)wo * pw) * C + cl * VEC;
      if (PHT && qmax) {   // training: also x at the window's FIRST maximum of the unclamped BatchNorm value (the backward's statistics pass reads it instead of the window)
        VecF<VEC> bt, bq;
#pragma unroll
        for (int e = 0; e < VEC; ++e) { bt.v[e] = -INFINITY; bq.v[e] = 0.f; }
#pragma unroll
        for (int ii = 0; ii < (PHT ? PHT : 1); ++ii)
#pragma unroll
          for (int j = 0; j < (PWT ? PWT : 1); ++j) {
            VecF<VEC> v = vload_s<VEC, kNtBnAct>(&x[base + ((long)ii * W + j) * C]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const float tt = fmaf(v.v[e], s.v[e], t.v[e]);
              bq.v[e] = tt > bt.v[e] ? v.v[e] : bq.v[e];        // strict '>': the first maximum in scan order (bn_bwd_pool_kernel's rule)
              bt.v[e] = fmaxf(bt.v[e], tt);
            }
          }
#pragma unroll
        for (int e = 0; e < VEC; ++e) m.v[e] = relu6f(bt.v[e]);  // ReLU6 is monotone: the maximum of the clamped values is the clamped maximum, exactly
        vstore<VEC>(&qmax[(long)pix * C + cl * VEC], bq);
      } else if (PHT) {
#pragma unroll
        for (int ii = 0; ii < (PHT ? PHT : 1); ++ii)
#pragma unroll
          for (int j = 0; j < (PWT ? PWT : 1); ++j) {
            VecF<VEC> v = vload_s<VEC, kNtBnAct>(&x[base + ((long)ii * W + j) * C]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) m.v[e] = fmaxf(m.v[e], relu6f(fmaf(v.v[e], s.v[e], t.v[e])));
          }
      } else {
        for (int ii = 0; ii < ph; ++ii)
          for (int j = 0; j < pw; ++j) {
            VecF<VEC> v = vload_s<VEC, kNtBnAct>(&x[base + ((long)ii * W + j) * C]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) m.v[e] = fmaxf(m.v[e], relu6f(fmaf(v.v[e], s.v[e], t.v[e])));
          }
      }
    }
    if (!y) continue;                                          // (qmax only: the next depthwise kernel forms the block output from it)
    const long obase = (long)pix * C + cl * VEC;
    float dm[VEC];
    drop_scale_vec<VEC>(seed, layer, (uint64_t)obase, rate, inv_keep, dm);
#pragma unroll
    for (int e = 0; e < VEC; ++e) m.v[e] *= dm[e];
    vstore<VEC>(&y[obase], m);
  }
}

template <int VEC, typename TI, typename TO>
static void bn_act_go(const TI* x, const float* bnstate, TO* y, int B, int H, int W, int C, int ph, int pw, float rate, uint64_t seed,
                      uint32_t layer, hipStream_t stream, TI* qmax = nullptr) {
  long total = (long)B * (H / ph) * (W / pw) * C;
  int blocks = cdiv(total / VEC, 256); if (blocks > 8192) blocks = 8192;
  const bool small = total / VEC + 8192L * 256 < (1L << 31);       // the grid-stride counter stays below 2^31 + one stride: fits unsigned
  const dim3 g(blocks), t(256);
#define BN_ACT_LAUNCH(IDX, PHT, PWT) hipLaunchKernelGGL((bn_act_pool_drop_kernel<VEC, TI, TO, IDX, PHT, PWT>), g, t, 0, stream, x, bnstate, y, B, H, W, C, ph, pw, rate, seed, layer, qmax)
  if (!small) BN_ACT_LAUNCH(long, 0, 0);
  else if (ph == 2 && pw == 2) BN_ACT_LAUNCH(unsigned, 2, 2);
  else if (ph == 1 && pw == 2) BN_ACT_LAUNCH(unsigned, 1, 2);
  else BN_ACT_LAUNCH(unsigned, 0, 0);
#undef BN_ACT_LAUNCH
}
template <typename TI, typename TO>
static int bn_act_launch(const TI* x, const float* bnstate, TO* y, int B, int H, int W, int C, int ph, int pw, float rate, uint64_t seed,
                         uint32_t layer, hipStream_t stream, TI* qmax = nullptr) {
  if (qmax && !((ph == 2 && pw == 2) || (ph == 1 && pw == 2))) return CRNN_ERR_UNSUPPORTED;   // (the compile-time windows)
  if (qmax && (long)B * (H / ph) * (W / pw) * C + 8192L * 256 * 8 >= (1L << 31)) return CRNN_ERR_UNSUPPORTED;
  const bool al = ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)bnstate | (uintptr_t)qmax) & 15) == 0);
  const int VM = (VecMax<TI>::value == 8 && VecMax<TO>::value == 8) ? 8 : 4;
  if (VM == 8 && al && C % 8 == 0) bn_act_go<(VecMax<TI>::value == 8 && VecMax<TO>::value == 8) ? 8 : 4>(x, bnstate, y, B, H, W, C, ph, pw, rate, seed, layer, stream, qmax);
  else if (al && C % 4 == 0) bn_act_go<4>(x, bnstate, y, B, H, W, C, ph, pw, rate, seed, layer, stream, qmax);
  else bn_act_go<1>(x, bnstate, y, B, H, W, C, ph, pw, rate, seed, layer, stream, qmax);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
// the storage types of both entry points, cast once: dt_in = storage of x and qmax (may be null), dt_out = storage of y
static int bn_act_any(const void* x, const float* bnstate, void* y, void* qmax, int B, int H, int W, int C, int ph, int pw, float rate, uint64_t seed,
                      uint32_t layer, int dt_in, int dt_out, hipStream_t stream) {
  if (dt_in == CRNN_BF16 && dt_out == CRNN_BF16) return bn_act_launch((const bf16_t*)x, bnstate, (bf16_t*)y, B, H, W, C, ph, pw, rate, seed, layer, stream, (bf16_t*)qmax);
  if (dt_in == CRNN_BF16) return bn_act_launch((const bf16_t*)x, bnstate, (float*)y, B, H, W, C, ph, pw, rate, seed, layer, stream, (bf16_t*)qmax);
  if (dt_out == CRNN_BF16) return bn_act_launch((const float*)x, bnstate, (bf16_t*)y, B, H, W, C, ph, pw, rate, seed, layer, stream, (float*)qmax);
  return bn_act_launch((const float*)x, bnstate, (float*)y, B, H, W, C, ph, pw, rate, seed, layer, stream, (float*)qmax);
}
// dt_in / dt_out: storage of x / y
extern "C" int crnn_bn_act_pool_drop_ex(const void* x, const float* bnstate, void* y, int B, int H, int W, int C, int ph,
                                        int pw, float rate, uint64_t seed, uint32_t layer, int dt_in, int dt_out, hipStream_t stream) {
  return bn_act_any(x, bnstate, y, nullptr, B, H, W, C, ph, pw, rate, seed, layer, dt_in, dt_out, stream);
}
// ... that also writes qmax [B][H/ph][W/pw][C] (storage dt_in): x at the first maximum of x * scale + shift over each pool window (2 x 2 or 1 x 2 only) --
// what crnn_bn_bwd_qmax_ex's statistics pass reads instead of the whole window.  y as above, bit for bit; y NULL: qmax only (the block output is then
// Dropout(ReLU6(qmax * scale + shift)) element by element -- what crnn_dwconv3x3_fwd_stream_pro_ex forms from it, bit for bit).
extern "C" int crnn_bn_act_pool_drop_qmax_ex(const void* x, const float* bnstate, void* y, void* qmax, int B, int H, int W, int C, int ph, int pw, float rate,
                                             uint64_t seed, uint32_t layer, int dt_in, int dt_out, hipStream_t stream) {
  if (!x || !bnstate || !qmax) return CRNN_ERR_ARG;          // y may be NULL: qmax only
  return bn_act_any(x, bnstate, y, qmax, B, H, W, C, ph, pw, rate, seed, layer, dt_in, dt_out, stream);
}

// ---------------------------------------------------------------------------------------------
// BatchNorm backward (train mode).  x = pre-BN tensor [B,H,W,C]; the upstream gradient arrives as
// g [B,H/ph,W/pw,C] w.r.t. Dropout(MaxPool(ReLU6(BN(x)))) and is routed on the fly:
//   gy = [first-argmax of the pool window] * g * dropmask * [0 < relu6(bn(x)) < 6]
// pass 1 (reduce): partials [chunk][2][C] = (sum gy, sum gy*xhat)
// pass 2 (apply):  dx = scale * (gy - c1 - xhat*c2),   c1 = sum(gy)/n, c2 = sum(gy*xhat)/n
// Threads: VEC channels per thread (16-byte accesses when C % 4 == 0), CW channel-threads x 256/CW
// row-threads; rows = pixels.  POOL=false (ph=pw=1) needs no per-element index arithmetic at all.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct BnBwdArgsT {
  const T* x; const T* g; const float* bnstate; const float* gamma;
  int B, H, W, C, ph, pw; float rate; uint64_t seed; uint32_t layer;
  // round 6 (fp32 tensors): pass 2 writes dx as bf16 PLANES instead (plane pl of element i at dxp[pl * dxps + i]; the words of crnn_split3_pair) -- what the
  // pointwise GEMMs that read dx (gemm_pres.hip, gemm_wgrad3.hip) stage, split once here instead of once per tile there.  Null: dx as T
  unsigned short* dxp = nullptr; long dxps = 0; int dxpl = 0;
  // round 6: x at each pool window's first maximum, written by the forward (crnn_bn_act_pool_drop_qmax_ex): the statistics pass of the pooled kernel reads it
  // (one value per window) instead of the window -- the same sums bit for bit from a quarter (half) of the bytes
  const T* qmax = nullptr;
};
// dx (fp32 values) of VEC consecutive elements as planes (VEC = 4: two words per plane)
template <int VEC, typename T>
__device__ __forceinline__ void bn_store_dx(const BnBwdArgsT<T>& a, T* dx, long idx, const VecF<VEC>& o) {
  if constexpr (VEC == 4 && sizeof(T) == 4) {
    if (a.dxp) {
      unsigned w0[3], w1[3];
      crnn_split3_pair(o.v[0], o.v[1], w0[0], w0[1], w0[2]);
      crnn_split3_pair(o.v[2 % VEC], o.v[3 % VEC], w1[0], w1[1], w1[2]);
      unsigned short* q = a.dxp + idx;
      *reinterpret_cast<uint2*>(q) = make_uint2(w0[0], w1[0]);
      *reinterpret_cast<uint2*>(q + a.dxps) = make_uint2(w0[1], w1[1]);
      if (a.dxpl == 3) *reinterpret_cast<uint2*>(q + 2 * a.dxps) = make_uint2(w0[2], w1[2]);
      return;
    }
  }
  vstore<VEC>(&dx[idx], o);
}

// gy for VEC consecutive channels starting at c0 of pixel row r
template <int VEC, bool POOL, typename T, bool NT = false>
__device__ __forceinline__ VecF<VEC> bn_gy_vec(const BnBwdArgsT<T>& a, long r, int c0, const VecF<VEC>& xv, const VecF<VEC>& sc,
                                               const VecF<VEC>& sh, float inv_keep) {
  VecF<VEC> out, y;
  // no pooling: only 0 < y < 6 is asked of y below, which the clamp does not change (it is skipped); the window scan needs the clamped value
#pragma unroll
  for (int e = 0; e < VEC; ++e) { const float t = fmaf(xv.v[e], sc.v[e], sh.v[e]); y.v[e] = POOL ? relu6f(t) : t; }
  long oidx;
  bool arg[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) arg[e] = true;
  if (!POOL) {
    oidx = r * a.C + c0;
  } else {
    const int Ho = a.H / a.ph, Wo = a.W / a.pw;
    int w = (int)(r % a.W); long rr = r / a.W; int h = (int)(rr % a.H); long b = rr / a.H;
    int ho = h / a.ph, wo = w / a.pw;
    if (ho >= Ho || wo >= Wo) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) out.v[e] = 0.f;
      return out;
    }
    int si = h - ho * a.ph, sj = w - wo * a.pw;
    for (int ii = 0; ii < a.ph; ++ii)
      for (int j = 0; j < a.pw; ++j) {
        if (ii == si && j == sj) continue;
        VecF<VEC> o = vload_s<VEC, NT>(&a.x[(((long)b * a.H + ho * a.ph + ii) * a.W + wo * a.pw + j) * a.C + c0]);
        bool earlier = (ii < si) || (ii == si && j < sj);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          float oy = relu6f(fmaf(o.v[e], sc.v[e], sh.v[e]));
          if (earlier ? (oy >= y.v[e]) : (oy > y.v[e])) arg[e] = false;   // not the first maximum
        }
      }
    oidx = (((long)b * Ho + ho) * Wo + wo) * a.C + c0;
  }
  VecF<VEC> gv = vload_s<VEC, NT>(&a.g[oidx]);
  float dm[VEC];
  drop_scale_vec<VEC>(a.seed, a.layer, (uint64_t)oidx, a.rate, inv_keep, dm);
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    bool live = arg[e] && (y.v[e] > 0.f) && (y.v[e] < 6.f);
    out.v[e] = live ? gv.v[e] * dm[e] : 0.f;
  }
  return out;
}

template <int PASS, int VEC, bool POOL, typename T>
__global__ __launch_bounds__(256) void bn_bwd_kernel(BnBwdArgsT<T> a, float* __restrict__ partials,
                                                     const float* __restrict__ coef, T* __restrict__ dx, int CW,
                                                     int rows_per_chunk) {
  __shared__ float red[2][256 * VEC];
  const int tid = threadIdx.x, cl = tid % CW, rt = tid / CW, RT = 256 / CW;
  const long M = (long)a.B * a.H * a.W;
  const long r0 = (long)blockIdx.x * rows_per_chunk;
  long r1 = r0 + rows_per_chunk; if (r1 > M) r1 = M;
  const int CL = a.C / VEC;
  const float inv_keep = a.rate > 0.f ? 1.f / (1.f - a.rate) : 1.f;
  for (int cb = 0; cb < CL; cb += CW) {
    const int c = cb + cl, c0 = c * VEC;
    VecF<VEC> s, q;
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s.v[e] = 0.f; q.v[e] = 0.f; }
    if (c < CL) {
      VecF<VEC> mu = vload<VEC>(a.bnstate + c0), var = vload<VEC>(a.bnstate + a.C + c0);
      VecF<VEC> sc = vload<VEC>(a.bnstate + 2 * a.C + c0), sh = vload<VEC>(a.bnstate + 3 * a.C + c0);
      VecF<VEC> inv, c1, c2;
#pragma unroll
      for (int e = 0; e < VEC; ++e) { inv.v[e] = 1.0f / sqrtf(var.v[e] + BN_EPS); c1.v[e] = 0.f; c2.v[e] = 0.f; }
      VecF<VEC> Pc, Qc;
#pragma unroll
      for (int e = 0; e < VEC; ++e) { Pc.v[e] = 0.f; Qc.v[e] = 0.f; }
      if (PASS == 2) {
        c1 = vload<VEC>(coef + c0); c2 = vload<VEC>(coef + a.C + c0);
#pragma unroll
        for (int e = 0; e < VEC; ++e) bn_bwd_pq(sc.v[e], c1.v[e], c2.v[e], mu.v[e], inv.v[e], Pc.v[e], Qc.v[e]);
      }
      long r = r0 + rt;
      constexpr bool NT = kNtBnBwd2 && PASS == 2;
      for (; r + RT < r1; r += 2L * RT) {   // two rows in flight (independent loads)
        VecF<VEC> xa = vload_s<VEC, NT>(&a.x[r * a.C + c0]);
        VecF<VEC> xb = vload_s<VEC, NT>(&a.x[(r + RT) * a.C + c0]);
        VecF<VEC> ga = bn_gy_vec<VEC, POOL, T, NT>(a, r, c0, xa, sc, sh, inv_keep);
        VecF<VEC> gb = bn_gy_vec<VEC, POOL, T, NT>(a, r + RT, c0, xb, sc, sh, inv_keep);
        VecF<VEC> oa, ob;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          float ha = (xa.v[e] - mu.v[e]) * inv.v[e], hb = (xb.v[e] - mu.v[e]) * inv.v[e];
          if (PASS == 1) {
            s.v[e] += ga.v[e]; q.v[e] = fmaf(ga.v[e], ha, q.v[e]);
            s.v[e] += gb.v[e]; q.v[e] = fmaf(gb.v[e], hb, q.v[e]);
          } else {
            oa.v[e] = bn_bwd_dx_pq(xa.v[e], ga.v[e], sc.v[e], Pc.v[e], Qc.v[e]);
            ob.v[e] = bn_bwd_dx_pq(xb.v[e], gb.v[e], sc.v[e], Pc.v[e], Qc.v[e]);
          }
        }
        if (PASS == 2) { bn_store_dx<VEC, T>(a, dx, r * a.C + c0, oa); bn_store_dx<VEC, T>(a, dx, (r + RT) * a.C + c0, ob); }
      }
      for (; r < r1; r += RT) {
        VecF<VEC> xv = vload_s<VEC, NT>(&a.x[r * a.C + c0]);
        VecF<VEC> gy = bn_gy_vec<VEC, POOL, T, NT>(a, r, c0, xv, sc, sh, inv_keep);
        VecF<VEC> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          float xh = (xv.v[e] - mu.v[e]) * inv.v[e];
          if (PASS == 1) { s.v[e] += gy.v[e]; q.v[e] = fmaf(gy.v[e], xh, q.v[e]); }
          else o.v[e] = bn_bwd_dx_pq(xv.v[e], gy.v[e], sc.v[e], Pc.v[e], Qc.v[e]);
        }
        if (PASS == 2) bn_store_dx<VEC, T>(a, dx, r * a.C + c0, o);
      }
    }
    if (PASS == 1) {
      __syncthreads();
#pragma unroll
      for (int e = 0; e < VEC; ++e) { red[0][tid * VEC + e] = s.v[e]; red[1][tid * VEC + e] = q.v[e]; }
      __syncthreads();
      if (rt == 0 && c < CL) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          float s2 = 0.f, q2 = 0.f;
          for (int r = 0; r < RT; ++r) { s2 += red[0][(r * CW + cl) * VEC + e]; q2 += red[1][(r * CW + cl) * VEC + e]; }
          partials[((long)blockIdx.x * 2 + 0) * a.C + c0 + e] = s2;
          partials[((long)blockIdx.x * 2 + 1) * a.C + c0 + e] = q2;
        }
      }
    }
  }
}

// Pooled variant (H % ph == 0, W % pw == 0): one thread owns a whole pool window x VEC channels, so every
// pre-BN value is read exactly once per pass and the arg-max is found once per window.
// PHT x PWT: the window as compile-time constants (0 x 0: run-time a.ph x a.pw) -- the window loops unroll without guards and the index
// arithmetic has no run-time divisions: a thread decomposes its first window index once and then steps (b, ho, wo) by RT windows.
template <int PASS, int VEC, typename T, int PHT = 0, int PWT = 0>
__global__ __launch_bounds__(256) void bn_bwd_pool_kernel(BnBwdArgsT<T> a, float* __restrict__ partials,
                                                          const float* __restrict__ coef, T* __restrict__ dx, int CW,
                                                          int rows_per_chunk) {
  __shared__ float red[2][256 * VEC];
  const int tid = threadIdx.x, cl = tid % CW, rt = tid / CW, RT = 256 / CW;
  const int ph = PHT ? PHT : a.ph, pw = PWT ? PWT : a.pw;
  const int Ho = a.H / ph, Wo = a.W / pw;
  const long Mo = (long)a.B * Ho * Wo;
  const long r0 = (long)blockIdx.x * rows_per_chunk;
  long r1 = r0 + rows_per_chunk; if (r1 > Mo) r1 = Mo;
  const int CL = a.C / VEC;
  const float inv_keep = a.rate > 0.f ? 1.f / (1.f - a.rate) : 1.f;
  const int nwin = ph * pw;       // <= 4
  // first window of this thread: (b, ho, wo), stepped by RT windows per iteration
  struct Pos { int b, ho, wo; };
  auto pos_of = [&](long r) { Pos p; p.wo = (int)(r % Wo); const long rr = r / Wo; p.ho = (int)(rr % Ho); p.b = (int)(rr / Ho); return p; };
  auto advance = [&](Pos& p, int n) {
    p.wo += n;
    while (p.wo >= Wo) { p.wo -= Wo; if (++p.ho == Ho) { p.ho = 0; ++p.b; } }
  };
  for (int cb = 0; cb < CL; cb += CW) {
    const int c = cb + cl, c0i = c * VEC;
    VecF<VEC> s, q;
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s.v[e] = 0.f; q.v[e] = 0.f; }
    if (c < CL) {
      VecF<VEC> mu = vload<VEC>(a.bnstate + c0i), var = vload<VEC>(a.bnstate + a.C + c0i);
      VecF<VEC> sc = vload<VEC>(a.bnstate + 2 * a.C + c0i), sh = vload<VEC>(a.bnstate + 3 * a.C + c0i);
      VecF<VEC> inv, c1, c2;
#pragma unroll
      for (int e = 0; e < VEC; ++e) { inv.v[e] = 1.0f / sqrtf(var.v[e] + BN_EPS); c1.v[e] = 0.f; c2.v[e] = 0.f; }
      if (PASS == 2) { c1 = vload<VEC>(coef + c0i); c2 = vload<VEC>(coef + a.C + c0i); }
      // one pool window per step; pass 1 (reduce only) keeps two windows' loads in flight
      auto load_window = [&](long r, const Pos& p, VecF<VEC>& gv, VecF<VEC> (&xw)[4], long& xbase) {
        constexpr bool NT = kNtBnBwd2 && PASS == 2;
        gv = vload_s<VEC, NT>(&a.g[r * a.C + c0i]);
        xbase = (((long)p.b * a.H + p.ho * ph) * a.W + p.wo * pw) * a.C + c0i;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < nwin) { int ii = k / pw, j = k - ii * pw; xw[k] = vload_s<VEC, NT>(&a.x[xbase + ((long)ii * a.W + j) * a.C]); }
      };
      // These two kernels are VALU-bound (SQ counters: ~3 resident waves/SIMD each 27-34 % VALU-active), so the window is
      // processed with as few operations as the arithmetic allows: only the arg-max position carries gradient, hence
      //   pass 1: sum gy = gsel, sum gy*xhat = gsel * xhat(x at the arg-max)            (x tracked alongside the maximum)
      //   pass 2: dx_k = scale*(gy_k - c1 - xhat_k*c2) = fma(cx, x_k, c0) + [k == arg] * scale*gsel
      //           with the per-channel constants cx = -scale*c2*inv, c0 = -scale*c1 - cx*mu.
      VecF<VEC> cx, c0;
#pragma unroll
      for (int e = 0; e < VEC; ++e) { cx.v[e] = -sc.v[e] * c2.v[e] * inv.v[e]; c0.v[e] = -sc.v[e] * c1.v[e] - cx.v[e] * mu.v[e]; }
      auto do_window = [&](long r, const VecF<VEC>& gv, const VecF<VEC> (&xw)[4], long xbase) {
        const long oidx = r * a.C + c0i;
        // The scan runs on the UNCLAMPED BatchNorm value t: a window carries gradient only if its maximum lies in (0, 6), and then the
        // first maximum of ReLU6(t) is the first maximum of t (values below 0 clamp to 0 < max, none reaches 6); for every other
        // window gsel = 0 and neither xs nor arg is used.  Same bits, two VALU operations per element fewer.
        float best[VEC], xs[VEC]; int arg[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) { best[e] = -INFINITY; xs[e] = 0.f; arg[e] = 0; }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < nwin) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              float y = fmaf(xw[k].v[e], sc.v[e], sh.v[e]);
              const bool up = y > best[e];                      // strict '>' keeps the FIRST maximum (scan order)
              best[e] = up ? y : best[e];
              if (PASS == 1) xs[e] = up ? xw[k].v[e] : xs[e]; else arg[e] = up ? k : arg[e];
            }
          }
        }
        float gsel[VEC], dm[VEC];
        drop_scale_vec<VEC>(a.seed, a.layer, (uint64_t)oidx, a.rate, inv_keep, dm);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          bool live = (best[e] > 0.f) && (best[e] < 6.f);
          gsel[e] = live ? gv.v[e] * dm[e] : 0.f;
        }
        if (PASS == 1) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            s.v[e] += gsel[e];
            q.v[e] = fmaf(gsel[e], (xs[e] - mu.v[e]) * inv.v[e], q.v[e]);
          }
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) gsel[e] *= sc.v[e];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (k < nwin) {
              VecF<VEC> o;
#pragma unroll
              for (int e = 0; e < VEC; ++e) o.v[e] = fmaf(cx.v[e], xw[k].v[e], c0.v[e]) + ((arg[e] == k) ? gsel[e] : 0.f);
              int ii = k / pw, j = k - ii * pw;
              bn_store_dx<VEC, T>(a, dx, xbase + ((long)ii * a.W + j) * a.C, o);
            }
          }
        }
      };
      long r = r0 + rt;
      Pos pa = pos_of(r < r1 ? r : r0);
      if (PASS == 1 && a.qmax) {   // the window's maximum is x * scale + shift of the saved x; four windows in flight
        auto one = [&](long rr, const VecF<VEC>& gv, const VecF<VEC>& xs) {
          float dm[VEC];
          drop_scale_vec<VEC>(a.seed, a.layer, (uint64_t)(rr * a.C + c0i), a.rate, inv_keep, dm);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float best = fmaf(xs.v[e], sc.v[e], sh.v[e]);
            const bool live = (best > 0.f) && (best < 6.f);
            const float gsel = live ? gv.v[e] * dm[e] : 0.f;
            s.v[e] += gsel;
            q.v[e] = fmaf(gsel, (xs.v[e] - mu.v[e]) * inv.v[e], q.v[e]);
          }
        };
        for (; r + 3L * RT < r1; r += 4L * RT) {
          VecF<VEC> gv[4], xs[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) { gv[u] = vload<VEC>(&a.g[(r + u * RT) * a.C + c0i]); xs[u] = vload<VEC>(&a.qmax[(r + u * RT) * a.C + c0i]); }
#pragma unroll
          for (int u = 0; u < 4; ++u) one(r + u * RT, gv[u], xs[u]);
        }
        for (; r < r1; r += RT) {
          const VecF<VEC> gv = vload<VEC>(&a.g[r * a.C + c0i]), xs = vload<VEC>(&a.qmax[r * a.C + c0i]);
          one(r, gv, xs);
        }
      } else
      if (PASS == 1) {
        for (; r + RT < r1; r += 2L * RT) {
          VecF<VEC> ga, gb, xa[4], xb[4]; long ba, bb;
          Pos pb = pa; advance(pb, RT);
          load_window(r, pa, ga, xa, ba);
          load_window(r + RT, pb, gb, xb, bb);
          do_window(r, ga, xa, ba);
          do_window(r + RT, gb, xb, bb);
          pa = pb; advance(pa, RT);
        }
      }
      for (; r < r1; r += RT) {
        VecF<VEC> gv, xw[4]; long xbase;
        load_window(r, pa, gv, xw, xbase);
        do_window(r, gv, xw, xbase);
        advance(pa, RT);
      }
    }
    if (PASS == 1) {
      __syncthreads();
#pragma unroll
      for (int e = 0; e < VEC; ++e) { red[0][tid * VEC + e] = s.v[e]; red[1][tid * VEC + e] = q.v[e]; }
      __syncthreads();
      if (rt == 0 && c < CL) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          float s2 = 0.f, q2 = 0.f;
          for (int r = 0; r < RT; ++r) { s2 += red[0][(r * CW + cl) * VEC + e]; q2 += red[1][(r * CW + cl) * VEC + e]; }
          partials[((long)blockIdx.x * 2 + 0) * a.C + c0i + e] = s2;
          partials[((long)blockIdx.x * 2 + 1) * a.C + c0i + e] = q2;
        }
      }
    }
  }
}

// Chunking of the two BatchNorm-backward passes: rows per chunk = the largest power of two <= 512 that still yields kBnbMinChunks
// chunks.  256 (468 partial rows for the 52-row maps at batch 256, 1872 for the 104-row maps) measured best over 256 / 512 / 768 / 1024 /
// 2048 (scripts/bnp1_bench.py): the statistics pass itself barely cares, the finalize that reads the partial rows halves; chunks of 1024
// rows (936 workgroups) cost the 104-row maps 6 % in the step.
constexpr int kBnbMinChunks = 256;
// (a statistics pass with four rows in flight per thread sat behind a macro that was tested before it was defined: the library never contained it)
static inline int bn_bwd_rows_per_chunk(long rows) { long r = 512; while (r > 16 && rows / r < kBnbMinChunks) r >>= 1; return (int)r; }
// upper bound on the number of partial rows for a [M][C] BN backward (pooled variants iterate over M/2 or M/4 windows)
extern "C" int crnn_bn_bwd_chunks(long M) {
  int best = 0;
  for (int div = 1; div <= 4; div *= 2) { int c = cdiv(M / div, bn_bwd_rows_per_chunk(M / div)); if (c > best) best = c; }
  return best;
}

// Which kernel a map's pool window selects, decided once for both passes: whole windows of at most four pixels take bn_bwd_pool_kernel (the CRNN's two pool
// shapes as compile-time windows, any other at run time); no pooling, and a pooled map that is no whole number of windows (RAGGED), take bn_bwd_kernel.
enum BnWindow { BN_WIN_NONE, BN_WIN_RAGGED, BN_WIN_2X2, BN_WIN_1X2, BN_WIN_RUNTIME };
static BnWindow bn_window(int H, int W, int ph, int pw) {
  if (ph * pw <= 1) return BN_WIN_NONE;
  if (H % ph || W % pw || ph * pw > 4) return BN_WIN_RAGGED;
  return (ph == 2 && pw == 2) ? BN_WIN_2X2 : (ph == 1 && pw == 2) ? BN_WIN_1X2 : BN_WIN_RUNTIME;
}
// one pass (1: parts <- statistics, coef and dx null; 2: dx <- coef, parts null): the same launch whichever kernel the window selects
template <int PASS, int VEC, typename T>
static void bn_bwd_pass(BnWindow win, const BnBwdArgsT<T>& a, float* parts, const float* coef, T* dx, int chunks, int CW, int rpc, hipStream_t stream) {
#define BN_BWD_LAUNCH(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(chunks), dim3(256), 0, stream, a, parts, coef, dx, CW, rpc)
  switch (win) {
    case BN_WIN_2X2: BN_BWD_LAUNCH(bn_bwd_pool_kernel<PASS, VEC, T, 2, 2>); break;
    case BN_WIN_1X2: BN_BWD_LAUNCH(bn_bwd_pool_kernel<PASS, VEC, T, 1, 2>); break;
    case BN_WIN_RUNTIME: BN_BWD_LAUNCH(bn_bwd_pool_kernel<PASS, VEC, T>); break;
    case BN_WIN_RAGGED: BN_BWD_LAUNCH(bn_bwd_kernel<PASS, VEC, true, T>); break;
    case BN_WIN_NONE: BN_BWD_LAUNCH(bn_bwd_kernel<PASS, VEC, false, T>); break;
  }
#undef BN_BWD_LAUNCH
}
template <int VEC, typename T>
static int bn_bwd_launch(const BnBwdArgsT<T>& a, T* dx, float* dgamma, float* dbeta, float* parts, float* coef, bool apply_only, hipStream_t stream) {
  const long M = (long)a.B * a.H * a.W;
  const int CL = a.C / VEC;
  const int CW = pow2_ge(CL < 256 ? CL : 256);
  const BnWindow win = bn_window(a.H, a.W, a.ph, a.pw);
  const long rows = (win == BN_WIN_NONE || win == BN_WIN_RAGGED) ? M : M / (a.ph * a.pw);   // the pooled kernel's rows are windows
  const int rpc = bn_bwd_rows_per_chunk(rows), chunks = cdiv(rows, rpc);
  if (!apply_only) {   // (apply_only: coef comes from elsewhere -- the statistics were taken by the kernel that produced g)
    bn_bwd_pass<1, VEC, T>(win, a, parts, nullptr, nullptr, chunks, CW, rpc, stream);
    CRNN_LAUNCH_CHECK();
    CRNN_TRY(crnn_bn_bwd_finalize(parts, chunks, a.C, M, dgamma, dbeta, coef, stream));
  }
  if (dx == nullptr && a.dxp == nullptr) return CRNN_OK;   // statistics only: dgamma, dbeta and coef = [mean(gy) | mean(gy * xhat)]; the caller applies pass 2 itself
  bn_bwd_pass<2, VEC, T>(win, a, nullptr, coef, dx, chunks, CW, rpc, stream);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// What every backward entry point below asks for, in one place: tensors of storage T (cast here, once), the optional pieces -- gamma / dgamma / dbeta /
// scratch_partials (null with apply_only: coef is an input then), dx as a tensor or (fp32 only) as `planes` bf16 planes, qmax -- and the vector width.
template <typename T>
static int bn_bwd_typed(const void* x, const void* g, const float* bnstate, const float* gamma, void* dx, void* dx_planes, long plane_stride, int planes,
                        const void* qmax, float* dgamma, float* dbeta, float* scratch_partials, float* coef, int B, int H, int W, int C, int ph, int pw, float rate,
                        uint64_t seed, uint32_t layer, bool apply_only, hipStream_t stream) {
  BnBwdArgsT<T> a{(const T*)x, (const T*)g, bnstate, gamma, B, H, W, C, ph, pw, rate, seed, layer};
  if (qmax) {   // (the pooled kernel's compile-time windows only)
    if (!((ph == 2 && pw == 2) || (ph == 1 && pw == 2)) || H % ph || W % pw || ((uintptr_t)qmax & 15)) return CRNN_ERR_ARG;
    a.qmax = (const T*)qmax;
  }
  if (dx_planes) {   // fp32 tensors, four channels per thread, the planes 8-byte aligned
    if (sizeof(T) != 4 || dx || (planes != 2 && planes != 3) || (C & 3) || ((uintptr_t)dx_planes & 7) || (plane_stride & 3) || plane_stride < (long)B * H * W * C ||
        (((uintptr_t)x | (uintptr_t)g | (uintptr_t)bnstate | (uintptr_t)coef) & 15)) return CRNN_ERR_ARG;
    a.dxp = reinterpret_cast<unsigned short*>(dx_planes); a.dxps = plane_stride; a.dxpl = planes;
  }
  const bool al = ((((uintptr_t)x | (uintptr_t)g | (uintptr_t)dx | (uintptr_t)bnstate | (uintptr_t)coef) & 15) == 0);   // (dx may be null: statistics only)
  if (VecMax<T>::value == 8 && al && C % 8 == 0) return bn_bwd_launch<VecMax<T>::value, T>(a, (T*)dx, dgamma, dbeta, scratch_partials, coef, apply_only, stream);
  if (C % 4 == 0 && al) return bn_bwd_launch<4, T>(a, (T*)dx, dgamma, dbeta, scratch_partials, coef, apply_only, stream);
  return bn_bwd_launch<1, T>(a, (T*)dx, dgamma, dbeta, scratch_partials, coef, apply_only, stream);
}
static int bn_bwd_any(int dtype, const void* x, const void* g, const float* bnstate, const float* gamma, void* dx, void* dx_planes, long plane_stride, int planes,
                      const void* qmax, float* dgamma, float* dbeta, float* scratch_partials, float* coef, int B, int H, int W, int C, int ph, int pw, float rate,
                      uint64_t seed, uint32_t layer, bool apply_only, hipStream_t stream) {
  if (dtype == CRNN_BF16)
    return bn_bwd_typed<bf16_t>(x, g, bnstate, gamma, dx, dx_planes, plane_stride, planes, qmax, dgamma, dbeta, scratch_partials, coef, B, H, W, C, ph, pw, rate, seed,
                                layer, apply_only, stream);
  return bn_bwd_typed<float>(x, g, bnstate, gamma, dx, dx_planes, plane_stride, planes, qmax, dgamma, dbeta, scratch_partials, coef, B, H, W, C, ph, pw, rate, seed, layer,
                             apply_only, stream);
}

// Full BN backward through Dropout/MaxPool/ReLU6: writes dx [B,H,W,C], dgamma[C], dbeta[C].
// scratch_partials: [crnn_bn_bwd_chunks(B*H*W)][2][C]; coef: [2*C].  dtype = storage of x, g and dx.
extern "C" int crnn_bn_bwd_ex(const void* x, const void* g, const float* bnstate, const float* gamma, void* dx,
                              float* dgamma, float* dbeta, float* scratch_partials, float* coef, int B, int H, int W, int C,
                              int ph, int pw, float rate, uint64_t seed, uint32_t layer, int dtype, hipStream_t stream) {
  return bn_bwd_any(dtype, x, g, bnstate, gamma, dx, nullptr, 0, 0, nullptr, dgamma, dbeta, scratch_partials, coef, B, H, W, C, ph, pw, rate, seed, layer, false, stream);
}
// Pass 2 of crnn_bn_bwd_ex alone: dx = scale * (gy - coef[0..C) - xhat * coef[C..2C)) with coef = [mean(gy) | mean(gy * xhat)] from crnn_bn_bwd_finalize
// (the statistics taken by the kernel that produced g: crnn_gemm_wres_bf16_bnstats, crnn_gemm_f32x3_bnstats).  Same arguments otherwise.
extern "C" int crnn_bn_bwd_apply_ex(const void* x, const void* g, const float* bnstate, const float* coef, void* dx, int B, int H, int W, int C,
                                    int ph, int pw, float rate, uint64_t seed, uint32_t layer, int dtype, hipStream_t stream) {
  if (!x || !g || !bnstate || !coef || !dx) return CRNN_ERR_ARG;
  return bn_bwd_any(dtype, x, g, bnstate, nullptr, dx, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, const_cast<float*>(coef), B, H, W, C, ph, pw, rate, seed, layer,
                    true, stream);
}
// crnn_bn_bwd_ex / crnn_bn_bwd_apply_ex for fp32 tensors with dx written as bf16 planes (planes = 2 | 3; plane pl of dx[i] at dx_planes[pl * plane_stride + i], the
// words of crnn_split3_planes of the fp32 dx the entry points above write) -- the operand format of crnn_gemm_pres_bnstats and crnn_pwconv_bnrelu6_wgrad_planes_stream_gp.
extern "C" int crnn_bn_bwd_planes_ex(const float* x, const float* g, const float* bnstate, const float* gamma, void* dx_planes, long plane_stride, int planes,
                                     float* dgamma, float* dbeta, float* scratch_partials, float* coef, int B, int H, int W, int C, int ph, int pw, float rate,
                                     uint64_t seed, uint32_t layer, hipStream_t stream) {
  if (!x || !g || !bnstate || !dx_planes || !coef) return CRNN_ERR_ARG;
  return bn_bwd_any(CRNN_F32, x, g, bnstate, gamma, nullptr, dx_planes, plane_stride, planes, nullptr, dgamma, dbeta, scratch_partials, coef, B, H, W, C, ph, pw, rate, seed,
                    layer, false, stream);
}
extern "C" int crnn_bn_bwd_apply_planes_ex(const float* x, const float* g, const float* bnstate, const float* coef, void* dx_planes, long plane_stride, int planes,
                                           int B, int H, int W, int C, int ph, int pw, float rate, uint64_t seed, uint32_t layer, hipStream_t stream) {
  if (!x || !g || !bnstate || !coef || !dx_planes) return CRNN_ERR_ARG;
  return bn_bwd_any(CRNN_F32, x, g, bnstate, nullptr, nullptr, dx_planes, plane_stride, planes, nullptr, nullptr, nullptr, nullptr, const_cast<float*>(coef), B, H, W, C,
                    ph, pw, rate, seed, layer, true, stream);
}
// The general form: crnn_bn_bwd_ex with qmax (may be NULL; storage `dtype` like x: the forward's crnn_bn_act_pool_drop_qmax_ex output -- the statistics pass of a
// pooled BatchNorm then reads one value per window, same sums bit for bit) and dx either as a tensor of `dtype` or (fp32 only, dx NULL) as `planes` bf16 planes.
extern "C" int crnn_bn_bwd_qmax_ex(const void* x, const void* qmax, const void* g, const float* bnstate, const float* gamma, void* dx, void* dx_planes, long plane_stride,
                                   int planes, float* dgamma, float* dbeta, float* scratch_partials, float* coef, int B, int H, int W, int C, int ph, int pw, float rate,
                                   uint64_t seed, uint32_t layer, int dtype, hipStream_t stream) {
  if (!x || !g || !bnstate || !coef || (dx && dx_planes)) return CRNN_ERR_ARG;
  if (dtype == CRNN_BF16 && dx_planes) return CRNN_ERR_ARG;
  return bn_bwd_any(dtype, x, g, bnstate, gamma, dx, dx_planes, plane_stride, planes, qmax, dgamma, dbeta, scratch_partials, coef, B, H, W, C, ph, pw, rate, seed, layer,
                    false, stream);
}
