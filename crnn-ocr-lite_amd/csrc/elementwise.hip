// Small elementwise kernels of the step: add, the dropout family (apply, apply + keep bytes, the multiplier as a tensor, keep bytes of several sites in one
// launch), the backward of ReLU / Dropout-of-ReLU, and BatchNorm + ReLU6 alone.
#include "common.h"

__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) o[i] = a[i] + b[i];
}
extern "C" int crnn_add(const float* a, const float* b, float* o, long n, hipStream_t stream) {
  int blocks = cdiv(n, 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(add_kernel, dim3(blocks), dim3(256), 0, stream, a, b, o, n);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// y[r*ldy + c] = x[r*ldx + c] * dropmask(idx = r*C + c)   (rows x C view, strided)
__global__ void dropout_kernel(const float* __restrict__ x, float* __restrict__ y, long rows, int C, int ldx, int ldy,
                               float rate, uint64_t seed, uint32_t layer) {
  long n = rows * C;
  float inv_keep = rate > 0.f ? 1.f / (1.f - rate) : 1.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    long r = i / C; int c = (int)(i % C);
    y[r * ldy + c] = x[r * ldx + c] * drop_scale(seed, layer, (uint64_t)i, rate, inv_keep);
  }
}
// four consecutive elements per thread: one 16-byte load / store and ONE hash (drop_scale_vec: a hash covers an aligned group of four
// element indices) instead of four of each; 32-bit index arithmetic.  C, ldx, ldy multiples of 4, 16-byte aligned, < 2^31 vectors.
__global__ void dropout_vec4_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned nvec, int C4, int ldx, int ldy,
                                    float rate, uint64_t seed, uint32_t layer) {
  const float inv_keep = rate > 0.f ? 1.f / (1.f - rate) : 1.f;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += gridDim.x * blockDim.x) {
    const unsigned r = i / (unsigned)C4, c4 = i - r * (unsigned)C4;
    const float4 v = *reinterpret_cast<const float4*>(x + (long)r * ldx + 4 * c4);
    float dm[4];
    drop_scale_vec<4>(seed, layer, (uint64_t)i * 4, rate, inv_keep, dm);
    *reinterpret_cast<float4*>(y + (long)r * ldy + 4 * c4) = make_float4(v.x * dm[0], v.y * dm[1], v.z * dm[2], v.w * dm[3]);
  }
}
extern "C" int crnn_dropout(const float* x, float* y, long rows, int C, int ldx, int ldy, float rate, uint64_t seed,
                            uint32_t layer, hipStream_t stream) {
  long n = rows * C;
  if (C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && n / 4 + 4096L * 256 < (1L << 31) && n > 0) {
    int blocks = cdiv(n / 4, 256); if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(dropout_vec4_kernel, dim3(blocks), dim3(256), 0, stream, x, y, (unsigned)(n / 4), C / 4, ldx, ldy, rate, seed, layer);
    CRNN_LAUNCH_CHECK();
    return CRNN_OK;
  }
  int blocks = cdiv(n, 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dropout_kernel, dim3(blocks), dim3(256), 0, stream, x, y, rows, C, ldx, ldy, rate, seed, layer);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// eight consecutive elements per thread: two 16-byte loads / stores, ONE hash, and the group's keep byte (bit e: element 8 g + e is kept -- the table
// crnn_dropout_keep_bytes writes) next to the dropped activations: dense2's one-pass backward (dense.hip) reads the decisions instead of hashing again
__global__ void dropout_vec8_keep_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned char* __restrict__ keep, unsigned ngroups, int C8,
                                         int ldx, int ldy, float rate, uint64_t seed, uint32_t layer) {
  const float inv_keep = rate > 0.f ? 1.f / (1.f - rate) : 1.f;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < ngroups; i += gridDim.x * blockDim.x) {
    const unsigned r = i / (unsigned)C8, c8 = i - r * (unsigned)C8;
    const float4 v0 = *reinterpret_cast<const float4*>(x + (long)r * ldx + 8 * c8), v1 = *reinterpret_cast<const float4*>(x + (long)r * ldx + 8 * c8 + 4);
    float dm[8];
    drop_scale_vec<8>(seed, layer, (uint64_t)i * 8, rate, inv_keep, dm);
    *reinterpret_cast<float4*>(y + (long)r * ldy + 8 * c8) = make_float4(v0.x * dm[0], v0.y * dm[1], v0.z * dm[2], v0.w * dm[3]);
    *reinterpret_cast<float4*>(y + (long)r * ldy + 8 * c8 + 4) = make_float4(v1.x * dm[4], v1.y * dm[5], v1.z * dm[6], v1.w * dm[7]);
    unsigned m = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) m |= (dm[e] != 0.f ? 1u : 0u) << e;
    keep[i] = (unsigned char)m;
  }
}
// whole groups of 8 columns, rows that start on 16 bytes, a 32-bit group counter
extern "C" int crnn_dropout_keep_supported(long rows, int C, int ldx, int ldy) {
  const long n = rows * C;
  return (C % 8 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && n > 0 && n / 8 + 4096L * 256 < (1L << 31)) ? CRNN_OK : CRNN_ERR_UNSUPPORTED;
}
extern "C" int crnn_dropout_keep(const float* x, float* y, void* keep, long rows, int C, int ldx, int ldy, float rate, uint64_t seed, uint32_t layer,
                                 hipStream_t stream) {
  const long n = rows * C;
  if (!x || !y || !keep || rate >= 1.f) return CRNN_ERR_ARG;
  CRNN_TRY(crnn_dropout_keep_supported(rows, C, ldx, ldy));
  if ((((uintptr_t)x | (uintptr_t)y) & 15)) return CRNN_ERR_UNSUPPORTED;
  int blocks = cdiv(n / 8, 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dropout_vec8_keep_kernel, dim3(blocks), dim3(256), 0, stream, x, y, static_cast<unsigned char*>(keep), (unsigned)(n / 8), C / 8, ldx, ldy, rate, seed, layer);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// materialise the multiplier (0 or 1/(1-rate)) that dropout site `layer` applies -- test hook
__global__ void dropout_mask_kernel(float* __restrict__ m, long n, float rate, uint64_t seed, uint32_t layer) {
  float inv_keep = rate > 0.f ? 1.f / (1.f - rate) : 1.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    m[i] = drop_scale(seed, layer, (uint64_t)i, rate, inv_keep);
}
extern "C" int crnn_dropout_mask(float* m, long n, float rate, uint64_t seed, uint32_t layer, hipStream_t stream) {
  int blocks = cdiv(n, 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(blocks), dim3(256), 0, stream, m, n, rate, seed, layer);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// Keep bits of a dropout site, one BYTE per group of 8 consecutive elements (bit e: element 8 g + e is kept) -- what drop_scale /
// drop_scale_vec decide, in the form the prologue row-stream depthwise kernels read (dwconv_stream.hip, dwconv_bwd_stream.hip): the mask
// depends on (seed, site, index) only, so it is evaluated once per step here -- four groups per thread, their dropout words side by side --
// instead of once per consumer pass inside kernels whose transform waves have no spare issue slots (36 of ~100 operations per group).
struct KeepBatch { unsigned* out[CRNN_KEEP_BATCH_MAX]; long nwords[CRNN_KEEP_BATCH_MAX]; long ngroups[CRNN_KEEP_BATCH_MAX]; uint32_t layer[CRNN_KEEP_BATCH_MAX]; };
__global__ __launch_bounds__(256) void dropout_keep_bytes_kernel(KeepBatch b, uint32_t thr, uint64_t seed) {
  const int site = blockIdx.y;
  const crnn_rng_key key = crnn_rng_make_key(seed, b.layer[site]);
  unsigned* __restrict__ out = b.out[site];
  const long nwords = b.nwords[site], ngroups = b.ngroups[site];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nwords; i += (long)gridDim.x * blockDim.x) {
    uint32_t w[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) crnn_rng8(key, (uint64_t)(4 * i + j), w[j]);
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned m = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        m |= ((w[j][q] & 0xffffu) >= thr ? 1u : 0u) << (2 * q);
        m |= ((w[j][q] >> 16) >= thr ? 1u : 0u) << (2 * q + 1);
      }
      if (4 * i + j >= ngroups) m = 0;
      v |= m << (8 * j);
    }
    out[i] = v;
  }
}
// out: 4-byte aligned, (ngroups + 3) / 4 * 4 bytes are written (the tail bytes of the last word are zero); rate <= 0: every element kept (0xFF)
extern "C" int crnn_dropout_keep_bytes_batch(int n, void* const* out, const long* ngroups, const uint32_t* layer, float rate, uint64_t seed, hipStream_t stream) {
  if (n < 0 || n > CRNN_KEEP_BATCH_MAX || rate >= 1.f || (n && (!out || !ngroups || !layer))) return CRNN_ERR_ARG;
  KeepBatch b; long maxw = 0; int m = 0;
  for (int i = 0; i < n; ++i) {
    if (!out[i] || ngroups[i] < 0 || ((uintptr_t)out[i] & 3)) return CRNN_ERR_ARG;
    if (ngroups[i] == 0) continue;
    const long nw = (ngroups[i] + 3) / 4;
    if (rate <= 0.f) {
      hipError_t e = hipMemsetAsync(out[i], 0xFF, (size_t)nw * 4, stream);
      if (e != hipSuccess) return (int)e;
      continue;
    }
    b.out[m] = (unsigned*)out[i]; b.nwords[m] = nw; b.ngroups[m] = ngroups[i]; b.layer[m] = layer[i]; ++m;
    if (nw > maxw) maxw = nw;
  }
  if (m == 0) return CRNN_OK;
  long blocks = (maxw + 255) / 256; if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(dropout_keep_bytes_kernel, dim3((unsigned)blocks, m), dim3(256), 0, stream, b, crnn_drop_threshold(rate), seed);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
extern "C" int crnn_dropout_keep_bytes(void* out, long ngroups, float rate, uint64_t seed, uint32_t layer, hipStream_t stream) {
  return crnn_dropout_keep_bytes_batch(1, &out, &ngroups, &layer, rate, seed, stream);
}

// g_out[perm(r)][c] = g[r][c] * [y[r][c] > 0]      (backward of ReLU, and of Dropout∘ReLU when y is the
// dropped activation: the 1/(1-p) factor is passed as `scale`).  permP as in the GEMM epilogue.
__global__ void relu_bwd_kernel(const float* __restrict__ y, const float* __restrict__ g, float* __restrict__ go, bf16_t* __restrict__ go16,
                                long rows, int C, float scale, int permP) {
  long n = rows * C;
  long Q = permP ? rows / permP : 0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    long r = i / C; int c = (int)(i % C);
    long orow = permP ? (r % permP) * Q + r / permP : r;
    const float v = (y[i] > 0.f) ? g[i] * scale : 0.f;
    go[orow * C + c] = v;
    if (go16) st1(go16 + orow * C + c, v);      // the same values rounded to bf16 (round to nearest even): the data-gradient GEMM's operand
  }
}
extern "C" int crnn_relu_bwd_ex(const float* y, const float* g, float* go, void* go_bf16, long rows, int C, float scale, int permP,
                                hipStream_t stream) {
  long n = rows * C;
  int blocks = cdiv(n, 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(blocks), dim3(256), 0, stream, y, g, go, static_cast<bf16_t*>(go_bf16), rows, C, scale, permP);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

// a = ReLU6(x*scale+shift) (the pointwise conv's input; kept for its weight gradient): batchnorm.hip's kernel without pool or dropout
extern "C" int crnn_bn_act(const float* x, const float* bnstate, float* y, long M, int C, hipStream_t stream) {
  return crnn_bn_act_pool_drop_ex(x, bnstate, y, 1, 1, (int)M, C, 1, 1, 0.f, 0, 0, CRNN_F32, CRNN_F32, stream);
}
