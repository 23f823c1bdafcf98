// Helpers shared by the conv stack's units (dwconv_tile.hip, reduce.hip, batchnorm.hip, elementwise.hip, block1.hip): channel vectors of a pixel in either
// storage type, the lane sums of the RED_CH x RED_PL second-stage reductions, and the chunking rules more than one unit sizes its launches by.
// NHWC tensors stored as fp32 or bf16 (CRNN_F32 / CRNN_BF16, chosen per call), arithmetic and statistics always fp32.  Include after common.h.
#pragma once
#include "common.h"
#include "stream_ops.h"

// VEC consecutive channels of one pixel, widened to fp32 (VEC = 1, 4 or 8; 8 = one 16-byte access of bf16 storage)
template <int VEC>
struct VecF { float v[VEC]; };

template <int VEC, typename T>
__device__ __forceinline__ VecF<VEC> vload(const T* p) {
  VecF<VEC> r;
  if (VEC == 8) {
    float8 q = ld8(p);
    r.v[0] = q.lo.x; r.v[1 % VEC] = q.lo.y; r.v[2 % VEC] = q.lo.z; r.v[3 % VEC] = q.lo.w;
    r.v[4 % VEC] = q.hi.x; r.v[5 % VEC] = q.hi.y; r.v[6 % VEC] = q.hi.z; r.v[7 % VEC] = q.hi.w;
  } else if (VEC == 4) {
    float4 q = ld4(p); r.v[0] = q.x; r.v[1 % VEC] = q.y; r.v[2 % VEC] = q.z; r.v[3 % VEC] = q.w;
  } else {
    r.v[0] = ld1(p);
  }
  return r;
}
template <int VEC, typename T>
__device__ __forceinline__ void vstore(T* p, const VecF<VEC>& r) {
  if (VEC == 8) {
    float8 q;
    q.lo = make_float4(r.v[0], r.v[1 % VEC], r.v[2 % VEC], r.v[3 % VEC]);
    q.hi = make_float4(r.v[4 % VEC], r.v[5 % VEC], r.v[6 % VEC], r.v[7 % VEC]);
    st8(p, q);
  } else if (VEC == 4) {
    st4(p, make_float4(r.v[0], r.v[1 % VEC], r.v[2 % VEC], r.v[3 % VEC]));
  } else {
    st1(p, r.v[0]);
  }
}
// the nontemporal forms (a tensor read for the last time: batchnorm.hip says which passes and what it measured)
template <int VEC, typename T>
__device__ __forceinline__ VecF<VEC> vload_nt(const T* p) {
  VecF<VEC> r;
  if constexpr (VEC == 8 && sizeof(T) == 2) {
    const u32x4 u = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
#pragma unroll
    for (int q = 0; q < 4; ++q) { r.v[2 * q] = __uint_as_float(u[q] << 16); r.v[2 * q + 1] = __uint_as_float(u[q] & 0xffff0000u); }
    return r;
  } else if constexpr (VEC % 4 == 0 && sizeof(T) == 4) {
#pragma unroll
    for (int h = 0; h < VEC / 4; ++h) {
      const u32x4 u = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + h);
#pragma unroll
      for (int q = 0; q < 4; ++q) r.v[4 * h + q] = __uint_as_float(u[q]);
    }
    return r;
  } else {
    return vload<VEC>(p);
  }
}
template <int VEC, bool NT, typename T>
__device__ __forceinline__ VecF<VEC> vload_s(const T* p) {
  if constexpr (NT) return vload_nt<VEC>(p); else return vload<VEC>(p);
}
// widest vector the storage type moves in one 16-byte access
template <typename T> struct VecMax { static const int value = 4; };
template <> struct VecMax<bf16_t> { static const int value = 8; };

// raw channel vector of the storage type (what sits in HBM and in the LDS tile): 4 fp32 (16 B) or 4 bf16 (8 B; 8 bf16 per lane was built once and not adopted, its figures were not kept)
template <typename T> struct RawV;
template <> struct RawV<float> { typedef float4 type; static const int N = 4; };
template <> struct RawV<bf16_t> { typedef uint2 type; static const int N = 4; };
template <typename V, typename T> __device__ __forceinline__ V ldraw(const T* p) { return *reinterpret_cast<const V*>(p); }

static inline int pow2_ge(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// rows per chunk: aim for >= ~512 chunks (fills 256 CUs), between 16 and 1024 rows each
static inline int colreduce_rpc(long M) { long r = 1024; while (r > 16 && M / r < 512) r >>= 1; return (int)r; }

// Second-stage reductions run as (RED_CH outputs) x (RED_PL part-lanes) blocks: each lane adds every RED_PL-th
// partial in double, four independent loads in flight; lanes are then combined in a fixed order (deterministic).
#define RED_CH 16
#define RED_PL 64

// two interleaved sums (sum / sum-of-products rows of one partials array): eight independent loads in flight
__device__ __forceinline__ void part_lane_sum2(const float* __restrict__ b0, const float* __restrict__ b1, long stride, int nparts, int lane,
                                               double& s0, double& s1) {
  double a = 0.0, b = 0.0;
  int p = lane;
  // sixteen independent loads in flight: a lane's share of ~1900 partial rows is ~30 rows, i.e. four round trips to a remote L2 / HBM instead of eight
  for (; p + 7 * RED_PL < nparts; p += 8 * RED_PL) {
    float v[8], w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const long o = (long)(p + u * RED_PL) * stride; v[u] = b0[o]; w[u] = b1[o]; }
    a += (((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3])) + (((double)v[4] + (double)v[5]) + ((double)v[6] + (double)v[7]));
    b += (((double)w[0] + (double)w[1]) + ((double)w[2] + (double)w[3])) + (((double)w[4] + (double)w[5]) + ((double)w[6] + (double)w[7]));
  }
  for (; p + 3 * RED_PL < nparts; p += 4 * RED_PL) {
    const long o0 = (long)p * stride, o1 = (long)(p + RED_PL) * stride, o2 = (long)(p + 2 * RED_PL) * stride, o3 = (long)(p + 3 * RED_PL) * stride;
    float v0 = b0[o0], v1 = b0[o1], v2 = b0[o2], v3 = b0[o3];
    float w0 = b1[o0], w1 = b1[o1], w2 = b1[o2], w3 = b1[o3];
    a += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
    b += ((double)w0 + (double)w1) + ((double)w2 + (double)w3);
  }
  for (; p < nparts; p += RED_PL) { a += (double)b0[(long)p * stride]; b += (double)b1[(long)p * stride]; }
  s0 = a; s1 = b;
}
// lanes -> one value per output, fixed two-level order (8 groups of 8 lanes): red[2][RED_PL][RED_CH], result valid for y == 0
__device__ __forceinline__ void lanes_sum2(double (&red)[2][RED_PL][RED_CH], double& s, double& q) {
  static_assert(RED_PL == 64, "two-level lane reduction is written for 64 part-lanes");
  __syncthreads();
  const int x = threadIdx.x, y = threadIdx.y;
  if (y < 8) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) { a += red[0][y * 8 + r][x]; b += red[1][y * 8 + r][x]; }
    red[0][y * 8][x] = a; red[1][y * 8][x] = b;      // (only this thread reads rows y*8 .. y*8+7)
  }
  __syncthreads();
  s = 0.0; q = 0.0;
  if (y == 0) {
#pragma unroll
    for (int r = 0; r < 8; ++r) { s += red[0][r * 8][x]; q += red[1][r * 8][x]; }
  }
}
