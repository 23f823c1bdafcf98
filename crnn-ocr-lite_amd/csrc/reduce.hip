// Reductions of the conv stack: the generic column reduction over a row-major matrix, and every RED_CH x RED_PL second stage that turns a list of
// partial rows into per-channel results -- plain sums, the BatchNorm statistics finalize (forward and backward, with their folded forms for long
// lists) -- plus the inference-mode BatchNorm state.  Deterministic: fixed chunking, fixed order, second stages accumulate in double.
#include "common.h"
#include "conv_vec.h"

// ---------------------------------------------------------------------------------------------
// Column reductions over a row-major [M][C] matrix -> partials [nchunk][NV][C]
// NV=1: sum; NV=2: sum and sum of squares.  Deterministic (fixed chunking, fixed order).
// ---------------------------------------------------------------------------------------------
template <int VEC, int NV, typename T>
__global__ __launch_bounds__(256) void colreduce_kernel(const T* __restrict__ x, float* __restrict__ partials, long M,
                                                        int C, int ld, int CW, int rows_per_chunk) {
  // CW = power of two >= min(C/VEC, 256); thread -> (cl = tid % CW, rt = tid / CW)
  __shared__ float red[2][256 * VEC];
  const int tid = threadIdx.x, cl = tid % CW, rt = tid / CW, RT = 256 / CW;
  const long r0 = (long)blockIdx.x * rows_per_chunk;
  long r1 = r0 + rows_per_chunk; if (r1 > M) r1 = M;
  const int CL = C / VEC;
  for (int cb = 0; cb < CL; cb += CW) {
    int c = cb + cl;
    float s[VEC], q[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s[e] = 0.f; q[e] = 0.f; }
    if (c < CL) {
      long r = r0 + rt;
      if (VEC > 1) {  // 4 rows in flight per thread (independent 16-byte loads)
        for (; r + 3L * RT < r1; r += 4L * RT) {
          VecF<VEC> v0 = vload<VEC>(&x[r * ld + VEC * c]);
          VecF<VEC> v1 = vload<VEC>(&x[(r + RT) * ld + VEC * c]);
          VecF<VEC> v2 = vload<VEC>(&x[(r + 2L * RT) * ld + VEC * c]);
          VecF<VEC> v3 = vload<VEC>(&x[(r + 3L * RT) * ld + VEC * c]);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            s[e] += (v0.v[e] + v1.v[e]) + (v2.v[e] + v3.v[e]);
            if (NV == 2) q[e] += (v0.v[e] * v0.v[e] + v1.v[e] * v1.v[e]) + (v2.v[e] * v2.v[e] + v3.v[e] * v3.v[e]);
          }
        }
      }
      for (; r < r1; r += RT) {
        VecF<VEC> v = vload<VEC>(&x[r * ld + VEC * c]);
#pragma unroll
        for (int e = 0; e < VEC; ++e) { s[e] += v.v[e]; if (NV == 2) q[e] = fmaf(v.v[e], v.v[e], q[e]); }
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < VEC; ++e) { red[0][tid * VEC + e] = s[e]; if (NV == 2) red[1][tid * VEC + e] = q[e]; }
    __syncthreads();
    if (rt == 0 && c < CL) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float a = 0.f, b2 = 0.f;
        for (int r = 0; r < RT; ++r) { a += red[0][(r * CW + cl) * VEC + e]; if (NV == 2) b2 += red[1][(r * CW + cl) * VEC + e]; }
        partials[((long)blockIdx.x * NV + 0) * C + c * VEC + e] = a;
        if (NV == 2) partials[((long)blockIdx.x * NV + 1) * C + c * VEC + e] = b2;
      }
    }
  }
}

extern "C" int crnn_colreduce_chunks(long M) { return cdiv(M, colreduce_rpc(M)); }

// partials [crnn_colreduce_chunks(M)][nv][C]; dtype = storage of x
template <int VEC, typename T>
static void colreduce_go(const T* x, float* partials, long M, int C, int ld, int nv, int chunks, int rpc, hipStream_t stream) {
  const int CL = C / VEC, CW = pow2_ge(CL < 256 ? CL : 256);
  if (nv == 1) hipLaunchKernelGGL((colreduce_kernel<VEC, 1, T>), dim3(chunks), dim3(256), 0, stream, x, partials, M, C, ld, CW, rpc);
  else hipLaunchKernelGGL((colreduce_kernel<VEC, 2, T>), dim3(chunks), dim3(256), 0, stream, x, partials, M, C, ld, CW, rpc);
}
template <typename T>
static int colreduce_launch(const T* x, float* partials, long M, int C, int ld, int nv, hipStream_t stream) {
  int rpc = colreduce_rpc(M);
  int chunks = cdiv(M, rpc);
  const int VM = VecMax<T>::value;
  const bool al = ((((uintptr_t)x) & 15) == 0);
  if (VM == 8 && al && (C % 8 == 0) && (ld % 8 == 0)) colreduce_go<VecMax<T>::value, T>(x, partials, M, C, ld, nv, chunks, rpc, stream);
  else if (al && (C % 4 == 0) && (ld % 4 == 0)) colreduce_go<4, T>(x, partials, M, C, ld, nv, chunks, rpc, stream);
  else colreduce_go<1, T>(x, partials, M, C, ld, nv, chunks, rpc, stream);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
extern "C" int crnn_colreduce_ex(const void* x, float* partials, long M, int C, int ld, int nv, int dtype, hipStream_t stream) {
  if (nv != 1 && nv != 2) return CRNN_ERR_ARG;
  if (dtype == CRNN_BF16) return colreduce_launch<bf16_t>((const bf16_t*)x, partials, M, C, ld, nv, stream);
  return colreduce_launch<float>((const float*)x, partials, M, C, ld, nv, stream);
}

// one sum per lane of a RED_CH x RED_PL block (conv_vec.h): every RED_PL-th partial in double, four independent loads in flight
__device__ __forceinline__ double part_lane_sum(const float* __restrict__ base, long stride, int nparts, int lane) {
  double a = 0.0;
  int p = lane;
  for (; p + 3 * RED_PL < nparts; p += 4 * RED_PL) {
    float v0 = base[(long)p * stride], v1 = base[(long)(p + RED_PL) * stride];
    float v2 = base[(long)(p + 2 * RED_PL) * stride], v3 = base[(long)(p + 3 * RED_PL) * stride];
    a += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
  }
  for (; p < nparts; p += RED_PL) a += (double)base[(long)p * stride];
  return a;
}

// out[i] = scale * sum_p partials[p][i], i < n  (double accumulation)
__global__ __launch_bounds__(RED_CH * RED_PL) void partials_sum_kernel(const float* __restrict__ partials, int nparts, int n, float* __restrict__ out, float scale) {
  // gridDim.y > 1: blockIdx.y reduces its own contiguous chunk of the partial rows into out[blockIdx.y][n]
  __shared__ double red[RED_PL][RED_CH];
  const int chunk = (nparts + gridDim.y - 1) / gridDim.y;
  const int p0 = blockIdx.y * chunk;
  const int np = min(chunk, nparts - p0);
  int i = blockIdx.x * RED_CH + threadIdx.x;
  red[threadIdx.y][threadIdx.x] = (i < n && np > 0) ? part_lane_sum(partials + (long)p0 * n + i, n, np, threadIdx.y) : 0.0;
  __syncthreads();
  if (threadIdx.y == 0 && i < n) {
    double s = 0.0;
    for (int r = 0; r < RED_PL; ++r) s += red[r][threadIdx.x];
    out[(long)blockIdx.y * n + i] = (float)(s * scale);
  }
}

extern "C" int crnn_partials_sum(const float* partials, int nparts, int n, float* out, float scale, hipStream_t stream) {
  hipLaunchKernelGGL(partials_sum_kernel, dim3(cdiv(n, RED_CH)), dim3(RED_CH, RED_PL), 0, stream, partials, nparts, n, out, scale);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// ---------------------------------------------------------------------------------------------
// BatchNorm (axis=-1, eps=1e-3): statistics finalize.  bnstate = [mean | var | scale | shift] (4*C)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RED_CH * RED_PL) void bn_finalize_kernel(const float* __restrict__ partials, int nparts, int C, double inv_n,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      float* __restrict__ bnstate) {
  __shared__ double red[2][RED_PL][RED_CH];
  int c = blockIdx.x * RED_CH + threadIdx.x;
  double s = 0.0, q = 0.0;
  if (c < C) part_lane_sum2(partials + c, partials + C + c, 2L * C, nparts, threadIdx.y, s, q);
  red[0][threadIdx.y][threadIdx.x] = s; red[1][threadIdx.y][threadIdx.x] = q;
  lanes_sum2(red, s, q);
  if (threadIdx.y == 0 && c < C) {
    double mean = s * inv_n;
    double var = q * inv_n - mean * mean;
    if (var < 0.0) var = 0.0;
    float inv = (float)(1.0 / sqrt(var + (double)BN_EPS));
    float sc = gamma[c] * inv;
    bnstate[c] = (float)mean; bnstate[C + c] = (float)var;
    bnstate[2 * C + c] = sc; bnstate[3 * C + c] = beta[c] - (float)mean * sc;
  }
}

// inference mode: scale/shift from the moving statistics
__global__ void bn_infer_state_kernel(const float* __restrict__ mmean, const float* __restrict__ mvar,
                                      const float* __restrict__ gamma, const float* __restrict__ beta, int C,
                                      float* __restrict__ bnstate) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    float sc = gamma[c] / sqrtf(mvar[c] + BN_EPS);
    bnstate[c] = mmean[c]; bnstate[C + c] = mvar[c];
    bnstate[2 * C + c] = sc; bnstate[3 * C + c] = beta[c] - mmean[c] * sc;
  }
}

extern "C" int crnn_bn_finalize(const float* partials, int nparts, int C, long n, const float* gamma, const float* beta,
                                float* bnstate, hipStream_t stream) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, RED_CH)), dim3(RED_CH, RED_PL), 0, stream, partials, nparts, C, 1.0 / (double)n, gamma, beta, bnstate);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
// Same, for long partial lists (one row per GEMM tile): a first launch folds the rows into CRNN_BN_FOLD_ROWS chunk
// sums (scratch: CRNN_BN_FOLD_ROWS * 2 * C floats) with hundreds of workgroups, the finalize then reads those.
#define CRNN_BN_FOLD_ROWS 32
extern "C" int crnn_bn_finalize_folded(const float* partials, int nparts, int C, long n, const float* gamma, const float* beta,
                                       float* bnstate, float* scratch, hipStream_t stream) {
  if (nparts <= 1024 || scratch == nullptr) return crnn_bn_finalize(partials, nparts, C, n, gamma, beta, bnstate, stream);
  hipLaunchKernelGGL(partials_sum_kernel, dim3(cdiv(2 * C, RED_CH), CRNN_BN_FOLD_ROWS), dim3(RED_CH, RED_PL), 0, stream, partials, nparts, 2 * C, scratch, 1.f);
  CRNN_LAUNCH_CHECK();
  return crnn_bn_finalize(scratch, CRNN_BN_FOLD_ROWS, C, n, gamma, beta, bnstate, stream);
}

extern "C" int crnn_bn_infer_state(const float* mmean, const float* mvar, const float* gamma, const float* beta, int C,
                                   float* bnstate, hipStream_t stream) {
  hipLaunchKernelGGL(bn_infer_state_kernel, dim3(cdiv(C, 256)), dim3(256), 0, stream, mmean, mvar, gamma, beta, C, bnstate);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
// The same for up to CRNN_BN_INFER_BATCH_MAX BatchNorm layers in one launch (the predict path knows all of them before its first conv: 14
// launches of ~5 us each otherwise): arrays of n device pointers / channel counts on the host; grid.y = layer.
struct BnInferBatch { const float* mmean[CRNN_BN_INFER_BATCH_MAX]; const float* mvar[CRNN_BN_INFER_BATCH_MAX]; const float* gamma[CRNN_BN_INFER_BATCH_MAX];
                      const float* beta[CRNN_BN_INFER_BATCH_MAX]; float* bnstate[CRNN_BN_INFER_BATCH_MAX]; int C[CRNN_BN_INFER_BATCH_MAX]; };
__global__ void bn_infer_state_batch_kernel(BnInferBatch b) {
  const int j = blockIdx.y, C = b.C[j], c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    const float mm = b.mmean[j][c], mv = b.mvar[j][c];
    const float sc = b.gamma[j][c] / sqrtf(mv + BN_EPS);
    float* st = b.bnstate[j];
    st[c] = mm; st[C + c] = mv; st[2 * C + c] = sc; st[3 * C + c] = b.beta[j][c] - mm * sc;
  }
}
extern "C" int crnn_bn_infer_state_batch(int n, const float* const* mmean, const float* const* mvar, const float* const* gamma, const float* const* beta,
                                         const int* C, float* const* bnstate, hipStream_t stream) {
  if (n < 0 || n > CRNN_BN_INFER_BATCH_MAX || (n && (!mmean || !mvar || !gamma || !beta || !C || !bnstate))) return CRNN_ERR_ARG;
  if (n == 0) return CRNN_OK;
  BnInferBatch b; int cmax = 0;
  for (int j = 0; j < n; ++j) {
    if (!mmean[j] || !mvar[j] || !gamma[j] || !beta[j] || !bnstate[j] || C[j] <= 0) return CRNN_ERR_ARG;
    b.mmean[j] = mmean[j]; b.mvar[j] = mvar[j]; b.gamma[j] = gamma[j]; b.beta[j] = beta[j]; b.bnstate[j] = bnstate[j]; b.C[j] = C[j];
    if (C[j] > cmax) cmax = C[j];
  }
  hipLaunchKernelGGL(bn_infer_state_batch_kernel, dim3(cdiv(cmax, 256), n), dim3(256), 0, stream, b);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// dgamma = sum gy*xhat, dbeta = sum gy; coef = [c1 | c2]
__global__ __launch_bounds__(RED_CH * RED_PL) void bn_bwd_finalize_kernel(const float* __restrict__ partials, int nparts, int C, double inv_n,
                                                                          float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef) {
  __shared__ double red[2][RED_PL][RED_CH];
  int c = blockIdx.x * RED_CH + threadIdx.x;
  double s = 0.0, q = 0.0;
  if (c < C) part_lane_sum2(partials + c, partials + C + c, 2L * C, nparts, threadIdx.y, s, q);
  red[0][threadIdx.y][threadIdx.x] = s; red[1][threadIdx.y][threadIdx.x] = q;
  lanes_sum2(red, s, q);
  if (threadIdx.y == 0 && c < C) {
    dbeta[c] = (float)s; dgamma[c] = (float)q;
    coef[c] = (float)(s * inv_n); coef[C + c] = (float)(q * inv_n);
  }
}

// Second stage of a BatchNorm backward: partials [nparts][2][C] = partial sums of gy and gy * xhat over `count` elements per channel -> dgamma, dbeta
// and coef = [mean(gy) | mean(gy * xhat)] (what pass 2 of crnn_bn_bwd_ex, crnn_dwconv3x3_bwd_stream / crnn_dwconv3x3_bwd_fused apply).  The
// statistics pass is crnn_bn_bwd_ex's own (batchnorm.hip) or ran elsewhere (crnn_gemm_wres_bf16_bnstats).
extern "C" int crnn_bn_bwd_finalize(const float* partials, int nparts, int C, long count, float* dgamma, float* dbeta, float* coef, hipStream_t stream) {
  if (!partials || nparts < 1 || C < 1 || count < 1 || !dgamma || !dbeta || !coef) return CRNN_ERR_ARG;
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, RED_CH)), dim3(RED_CH, RED_PL), 0, stream, partials, nparts, C, 1.0 / (double)count, dgamma, dbeta, coef);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
// Same, for long partial lists (one row per GEMM tile row: crnn_gemm_f32x3_bnstats): rows folded into CRNN_BN_FOLD_ROWS chunk sums first
// (scratch: CRNN_BN_FOLD_ROWS * 2 * C floats), as crnn_bn_finalize_folded does for the forward statistics.
extern "C" int crnn_bn_bwd_finalize_folded(const float* partials, int nparts, int C, long count, float* dgamma, float* dbeta, float* coef, float* scratch,
                                           hipStream_t stream) {
  if (nparts <= 1024 || scratch == nullptr) return crnn_bn_bwd_finalize(partials, nparts, C, count, dgamma, dbeta, coef, stream);
  hipLaunchKernelGGL(partials_sum_kernel, dim3(cdiv(2 * C, RED_CH), CRNN_BN_FOLD_ROWS), dim3(RED_CH, RED_PL), 0, stream, partials, nparts, 2 * C, scratch, 1.f);
  CRNN_LAUNCH_CHECK();
  return crnn_bn_bwd_finalize(scratch, CRNN_BN_FOLD_ROWS, C, count, dgamma, dbeta, coef, stream);
}
