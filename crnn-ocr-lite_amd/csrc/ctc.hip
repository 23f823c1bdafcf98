// Softmax, CTC loss + gradient, greedy and beam CTC decoding -- one 64-lane wavefront per sample.
//   K.ctc_batch_cost(labels, y_pred[:, 2:, :], input_length, label_length)   (utils.py:98-103)
//   K.ctc_decode(greedy=True|False, beam_width, top_paths=1)                 (utils.py:347-357)
// The extended label sequence (S = 2L+1 <= 64) lives one state per lane; the alpha/beta recursions use
// wavefront shuffles for the s-1 / s-2 neighbours, log-space fp32 throughout.
// The arithmetic shared with lexicon.hip and align.hip -- the constants, lse2 / lse3, the row softmax and log-softmax, the alpha recursion -- is in ctc_core.h.
#include "common.h"
#include "ctc_core.h"


// ---- row softmax over C (<= 128) classes: one wave per row ------------------------------------------
// CPL = classes per lane: 1 for C <= 64 (lane l = class l), 2 for 65..128 (lane l = classes l and l + 64: the second value rides through the same
// wave_max / wave_sum).  The entry points pick the instantiation from C, so the narrow alphabets run the one-class-per-lane code unchanged.
template <int CPL>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ z, float* __restrict__ p, long rows, int C) {
  long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float v = lane < C ? z[row * C + lane] : NEG_INF;
  float v1 = NEG_INF;
  if constexpr (CPL == 2) v1 = lane + 64 < C ? z[row * C + lane + 64] : NEG_INF;
  const ctc_lane_pair pr = softmax_row<CPL>(v, v1, lane, C);
  if (lane < C) p[row * C + lane] = pr.lo;
  if constexpr (CPL == 2) if (lane + 64 < C) p[row * C + lane + 64] = pr.hi;
}
extern "C" int crnn_softmax_rows(const float* z, float* p, long rows, int C, hipStream_t stream) {
  if (C > 128) return CRNN_ERR_UNSUPPORTED;
  if (C <= 64) hipLaunchKernelGGL(softmax_rows_kernel<1>, dim3(cdiv(rows, 4)), dim3(256), 0, stream, z, p, rows, C);
  else hipLaunchKernelGGL(softmax_rows_kernel<2>, dim3(cdiv(rows, 4)), dim3(256), 0, stream, z, p, rows, C);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// dense2's epilogue in one pass (round 5): z [rows][ldz] are the raw products of the streaming GEMM over a padded weight matrix (columns >= C are never read);
// logits = z + bias go out in permuted row order (out row = (m % P) * (rows / P) + m / P: time-major rows back to batch-major, as the tile GEMM's epilogue
// does) together with their softmax p1 (workspace) and p2 (the caller's y_pred, may be NULL) -- the softmax and copy launches of the unfused path.
template <int CPL>
__global__ __launch_bounds__(256) void softmax_rows_perm_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ bias, float* __restrict__ logits,
                                                                float* __restrict__ p1, float* __restrict__ p2, long rows, int C, int P) {
  const long m = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= rows) return;
  const long orow = P ? (m % P) * (rows / P) + m / P : m;
  const float v = lane < C ? z[m * ldz + lane] + (bias ? bias[lane] : 0.f) : NEG_INF;
  float v1 = NEG_INF;
  if constexpr (CPL == 2) v1 = lane + 64 < C ? z[m * ldz + lane + 64] + (bias ? bias[lane + 64] : 0.f) : NEG_INF;
  const ctc_lane_pair pr = softmax_row<CPL>(v, v1, lane, C);
  if (lane < C) {
    logits[orow * C + lane] = v;
    p1[orow * C + lane] = pr.lo;
    if (p2) p2[orow * C + lane] = pr.lo;
  }
  if constexpr (CPL == 2) if (lane + 64 < C) {
    logits[orow * C + lane + 64] = v1;
    p1[orow * C + lane + 64] = pr.hi;
    if (p2) p2[orow * C + lane + 64] = pr.hi;
  }
}
extern "C" int crnn_softmax_rows_perm(const float* z, int ldz, const float* bias, float* logits, float* p1, float* p2, long rows, int C, int permP,
                                      hipStream_t stream) {
  if (!z || !logits || !p1 || rows <= 0 || C < 1 || ldz < C || permP < 0 || (permP && rows % permP)) return CRNN_ERR_ARG;
  if (C > 128) return CRNN_ERR_UNSUPPORTED;
  if (C <= 64) hipLaunchKernelGGL(softmax_rows_perm_kernel<1>, dim3(cdiv(rows, 4)), dim3(256), 0, stream, z, ldz, bias, logits, p1, p2, rows, C, permP);
  else hipLaunchKernelGGL(softmax_rows_perm_kernel<2>, dim3(cdiv(rows, 4)), dim3(256), 0, stream, z, ldz, bias, logits, p1, p2, rows, C, permP);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// ---- CTC loss + gradient w.r.t. the dense2 logits -------------------------------------------------------
// y [B][T][C] softmax (batch-major), labels [B][Lmax] int32, lengths int32.
// loss[b] = -log p(label | y[:, skip:skip+Tb]);  dlogits [T][B][C] TIME-major, = grad_scale * d loss_b / d logits
// (through log(y+eps), TF's internal re-softmax, and the model's softmax); rows outside [skip, skip+Tb) are 0.
// One workgroup of CTC_WAVES wavefronts per sample; the extended label (S = 2L+1 <= 64 states) lives one state per lane:
//   phase 1  all waves : posteriors -> LDS (coalesced), log-softmax of log(y+eps) (a time step per wave, a class per lane)
//   phase 2  wave 0    : alpha recursion (t ascending)   ||   wave 1 : beta recursion (t descending)  -> LDS
//   phase 3  all waves : time steps dealt round-robin to the waves: w_s = exp(alpha+beta-lsm-ll) per state lane, then
//                        class lane k adds the w_s of its states (bit mask, ascending s; the blank class by a wave reduction) and chains to the logits
// Round 5 (phase-ablation builds that are gone; profiles/r05_ctc_bench.txt): 61 -> 28 us per launch at batch 256 -- the gradient phase was 30 us of it (the blank lane walking
// its 24-state mask through LDS with the wave waiting, two workgroup barriers per time step), the log-softmax phase ran on 50 lanes of 256.
// LDS: lsm [Tb][C], alpha [Tb][64], beta [Tb][64], ys [Tb][C], ab [4][64].
// CPL = classes per lane: with 65..128 classes (CPL = 2) the class lane l of phases 1 and 3 owns classes l and l + 64 -- two log-softmax values, two
// occupancy masks, two gradient elements, one wave reduction over both --; the state lanes and the recursions do not depend on the class count.
constexpr int CTC_WAVES = 16;   // round 5: 4 -> 16 (phases 1 and 3 deal the time steps over the waves: 41 -> 28 us at batch 256; 8 waves: 31.5; profiles/r05_ctc_bench.txt)
template <int CPL>
__global__ __launch_bounds__(64 * CTC_WAVES) void ctc_loss_grad_kernel(const float* __restrict__ y, const int* __restrict__ labels,
                                                                       const int* __restrict__ input_len, const int* __restrict__ label_len,
                                                                       float* __restrict__ loss, float* __restrict__ dlogits, int B, int T,
                                                                       int C, int Lmax, int skip, float grad_scale) {
  extern __shared__ float sm[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blank = C - 1;
  const int Tmax = T - skip;
  const int Tb = ctc_window(input_len[b], Tmax);
  const int L = label_len[b];
  const int S = 2 * L + 1;
  float* lsm = sm;                     // [Tmax][C]
  float* alpha = lsm + Tmax * C;       // [Tmax][64]
  float* beta = alpha + Tmax * 64;     // [Tmax][64]
  float* ys = beta + Tmax * 64;        // [Tmax][C]
  float* ab = ys + Tmax * C;           // [CTC_WAVES][64]
  float& ll_sh = ab[64 * CTC_WAVES];   // log-likelihood, handed from the alpha wave to everyone
  const float* yg = y + ((long)b * T + skip) * C;
  for (int i = tid; i < Tb * C; i += 64 * CTC_WAVES) ys[i] = yg[i];
  // zero gradient rows outside the valid window
  for (int t = wave; t < T; t += CTC_WAVES) {
    bool inside = (t >= skip && t < skip + Tb);
    if (!inside && lane < C) dlogits[((long)t * B + b) * C + lane] = 0.f;
    if constexpr (CPL == 2) if (!inside && lane + 64 < C) dlogits[((long)t * B + b) * C + lane + 64] = 0.f;
  }
  if (Tb == 0 || S > 64) {             // degenerate sample (uniform across the workgroup)
    if (tid == 0) loss[b] = (Tb == 0 && L == 0) ? 0.f : INFINITY;
    for (int t = skip + wave; t < skip + Tb; t += CTC_WAVES) {
      if (lane < C) dlogits[((long)t * B + b) * C + lane] = 0.f;
      if constexpr (CPL == 2) if (lane + 64 < C) dlogits[((long)t * B + b) * C + lane + 64] = 0.f;
    }
    return;
  }
  __syncthreads();
  // phase 1: log-softmax of z = log(y + eps): a time step per wave, a class per lane (round 5: was one time step per THREAD -- 50 busy lanes of 256, each
  // evaluating 3 C logarithms and C exponentials in sequence: a fifth of the kernel)
  for (int t = wave; t < Tb; t += CTC_WAVES) log_softmax_of_log_row<CPL>(ys + t * C, lsm + t * C, lane, C);
  __syncthreads();
  // extended label of this lane (every wave holds its own copy)
  const int s = lane;
  int ext = blank;
  if (s < S && (s & 1)) ext = labels[(long)b * Lmax + (s >> 1)];
  // phase 2: the two recursions on two waves
  if (wave == 0) {
    const bool can_skip = ctc_can_skip(ext, s, S, blank);
    float a = ctc_alpha_init(lsm, ext, s, S);
    alpha[s] = a;
    for (int t = 1; t < Tb; ++t) {
      const float em = lsm[t * C + ext];                        // (independent of the chain: issued ahead of it)
      a = ctc_alpha_step(a, em, s, S, can_skip);
      alpha[t * 64 + s] = a;
    }
    const float ll0 = ctc_alpha_total(a, 0, S);
    if (lane == 0) ll_sh = ll0;
  } else if (wave == 1) {
    // beta includes the emission at t, like alpha
    int extn2 = __shfl_down(ext, 2, 64);
    const bool can_skip_b = (s + 2 < S) && (ext != blank) && (ext != extn2);
    float bt = NEG_INF;
    for (int t = Tb - 1; t >= 0; --t) {
      if (t == Tb - 1) {
        bt = (s == S - 1 || (s == S - 2 && S > 1)) ? lsm[t * C + ext] : NEG_INF;
      } else {
        const float em = lsm[t * C + ext];
        const float b1 = __shfl_down(bt, 1, 64), b2 = __shfl_down(bt, 2, 64);
        const float v = lse3(bt, s + 1 < S ? b1 : NEG_INF, can_skip_b ? b2 : NEG_INF);
        bt = (s < S && v != NEG_INF) ? v + em : NEG_INF;
      }
      beta[t * 64 + s] = bt;
    }
  }
  __syncthreads();
  const float ll = ll_sh;
  if (tid == 0) loss[b] = -ll;
  if (ll == NEG_INF) {  // no valid path: TF reports inf loss, zero gradient
    for (int t = skip + wave; t < skip + Tb; t += CTC_WAVES) {
      if (lane < C) dlogits[((long)t * B + b) * C + lane] = 0.f;
      if constexpr (CPL == 2) if (lane + 64 < C) dlogits[((long)t * B + b) * C + lane + 64] = 0.f;
    }
    return;
  }
  // which extended-label states carry class `lane` (bit s set <=> ext_s == lane).  The BLANK class sits on every even state (L + 1 of them): its lane takes
  // the sum from a wave reduction of the state lanes' own registers instead of walking its mask (round 5: 24 dependent LDS reads per time step on one lane
  // -- with the whole wave waiting for it -- were 30 of the kernel's 55 us; phase timings in scripts/ctc_bench.py)
  unsigned long long occ_mask = 0ull, occ_mask1 = 0ull;   // (occ_mask1: class lane + 64, CPL == 2 only)
  for (int s2 = 0; s2 < S; ++s2) {
    int e2 = __shfl(ext, s2, 64);
    if (e2 == lane && lane != blank) occ_mask |= 1ull << s2;
    if constexpr (CPL == 2) if (e2 == lane + 64 && lane + 64 != blank) occ_mask1 |= 1ull << s2;
  }
  // phase 3: gradient, time steps round-robin over the waves.  A wave works on its own ab row only: the hand-over from the state lanes to the class lanes is
  // inside the wave (LDS operations of one wave complete in order), no workgroup barrier.
  float* abw = ab + wave * 64;
  for (int t = wave; t < Tb; t += CTC_WAVES) {
    const float v = (s < S) ? alpha[t * 64 + s] + beta[t * 64 + s] : NEG_INF;   // both contain lsm[t][ext] once
    const float w = (v != NEG_INF) ? expf(v - lsm[t * C + ext] - ll) : 0.f;
    const float wblank = wave_sum((s < S && ext == blank) ? w : 0.f);
    abw[s] = w;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    float gyk = 0.f, pk = 0.f;
    if (lane < C) {
      const float l = lsm[t * C + lane];
      float occ = (lane == blank) ? wblank : 0.f;
      for (unsigned long long m = occ_mask; m; m &= m - 1) occ += abw[__ffsll((long long)m) - 1];
      const float gz = expf(l) - occ;
      pk = ys[t * C + lane];
      gyk = gz / (pk + CTC_EPS);          // d loss / d y_pred[t][k]
    }
    if constexpr (CPL == 1) {
      const float dot = wave_sum(gyk * pk);
      if (lane < C) dlogits[((long)(t + skip) * B + b) * C + lane] = grad_scale * pk * (gyk - dot);
    } else {
      const int k1 = lane + 64;
      float gyk1 = 0.f, pk1 = 0.f;
      if (k1 < C) {
        const float l = lsm[t * C + k1];
        float occ = (k1 == blank) ? wblank : 0.f;
        for (unsigned long long m = occ_mask1; m; m &= m - 1) occ += abw[__ffsll((long long)m) - 1];
        const float gz = expf(l) - occ;
        pk1 = ys[t * C + k1];
        gyk1 = gz / (pk1 + CTC_EPS);
      }
      const float dot = wave_sum(gyk * pk + gyk1 * pk1);
      if (lane < C) dlogits[((long)(t + skip) * B + b) * C + lane] = grad_scale * pk * (gyk - dot);
      if (k1 < C) dlogits[((long)(t + skip) * B + b) * C + k1] = grad_scale * pk1 * (gyk1 - dot);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();       // (the class lanes are done with this row before the state lanes overwrite it)
  }
}

extern "C" int crnn_ctc_loss_grad(const float* y, const int* labels, const int* input_len, const int* label_len, float* loss,
                                  float* dlogits, int B, int T, int C, int Lmax, int skip, float grad_scale, hipStream_t stream) {
  if (C > 128 || C < 2 || T <= skip) return CRNN_ERR_UNSUPPORTED;
  if (Lmax < 0 || 2 * Lmax + 1 > 64) return CRNN_ERR_UNSUPPORTED;   // the extended label (2L+1 states) lives on the 64 lanes of one wavefront
  if (B <= 0) return CRNN_ERR_ARG;
  size_t lds = (2 * (size_t)(T - skip) * C + 2 * (size_t)(T - skip) * 64 + 64 * CTC_WAVES + 4) * sizeof(float);
  if (lds > 160 * 1024) return CRNN_ERR_UNSUPPORTED;
  auto kernel = C <= 64 ? ctc_loss_grad_kernel<1> : ctc_loss_grad_kernel<2>;   // one class per lane, or two (lane l: classes l and l + 64)
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, dim3(B), dim3(64 * CTC_WAVES), lds, stream, y, labels, input_len, label_len, loss, dlogits, B, T, C, Lmax, skip, grad_scale);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// ---- greedy decode (tf.nn.ctc_greedy_decoder, merge_repeated=True) --------------------------------------
// y [B][T][C]; out [B][T] int32 padded with -1; out_len [B].  argmax = first maximum.
__global__ __launch_bounds__(64) void ctc_greedy_kernel(const float* __restrict__ y, const int* __restrict__ input_len,
                                                        int* __restrict__ out, int* __restrict__ out_len, int T, int C) {
  extern __shared__ int am[];
  const int b = blockIdx.x, lane = threadIdx.x;
  int Tb = input_len ? input_len[b] : T; if (Tb > T) Tb = T;
  const float* yb = y + (long)b * T * C;
  for (int t = lane; t < Tb; t += 64) {
    float m = yb[t * C]; int k0 = 0;
    for (int k = 1; k < C; ++k) { float v = yb[t * C + k]; if (v > m) { m = v; k0 = k; } }
    am[t] = k0;
  }
  for (int t = lane; t < T; t += 64) out[(long)b * T + t] = -1;
  __syncthreads();
  if (lane == 0) {
    int n = 0, prev = -1;
    for (int t = 0; t < Tb; ++t) {
      int k = am[t];
      if (k != C - 1 && k != prev) out[(long)b * T + n++] = k;
      prev = k;
    }
    out_len[b] = n;
  }
}
extern "C" int crnn_ctc_greedy_decode(const float* y, const int* input_len, int* out, int* out_len, int B, int T, int C,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(64), (size_t)T * sizeof(int), stream, y, input_len, out, out_len, T, C);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
