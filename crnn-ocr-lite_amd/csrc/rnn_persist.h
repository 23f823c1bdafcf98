// Skeleton shared by the persistent recurrences (rnn_persist.hip: LSTM, gru_persist.hip: GRU): everything a kernel does besides
// its cell, and the host side of a launch.  The exchange ring itself (sentinel hand-off, status words, cluster maps) is rnn_exchange.h.
//
// Decomposition.  h_t[b, :] depends on h_{t-1}[b, :] only -- batch rows never mix -- so the recurrence of a 16-row batch tile of one
// direction is an independent chain.  A chain is run by a CLUSTER of u/(16 kUW) workgroups.  A workgroup has 4 kUW waves = kUW "unit
// groups" of 16 hidden units; wave w works for unit group w >> 2 on K quarter (LSTM forward: gate) w & 3:
//   * its slice of the recurrent weights is loaded ONCE into registers as MFMA B fragments (load_frags) and stays there for all T steps;
//   * the state / gradient carry of its (row, unit) pairs never leaves registers;
//   * per step the only inter-workgroup traffic is the all-gather of the cluster's values of that step: every wave publishes the 4 rows
//     it produced (publish_rows), every workgroup polls the complete tile into LDS as the MFMA A operand of the next product (gather_rows /
//     gather_gated), and re-poisons its slice of the slot two exchanges ahead (poison_rows).
// One schedule: kUW = 2 (512 threads).  Measured at u = 256, B = 256, bf16 forward: 148 / 126 / 182 us with 1 / 2 / 4 unit groups (16-wave
// barriers cost more than the smaller cluster saves), 32-row tiles 203-288 us (profiles/r02_lstm_bench.json, r03_lstm_bench.json).
//
// Numerics: bit-identical to the per-step kernels of rnn.hip -- every K quarter accumulates in ascending k (quarter_chain), the quarters
// combine as ((q0+q1)+(q2+q3)) + x (sum_quarters), the cells are rnn_cell.h's; in the bf16 modes the exchanged values are the round-to-nearest-even
// bf16 values the step kernels formed while packing (to_e).
#pragma once
#include "rnn_exchange.h"

namespace {

constexpr int kUW = 2, kThreads = 256 * kUW;    // unit groups per workgroup, threads per workgroup

template <bool WBF> __device__ __forceinline__ typename XE<WBF>::type to_e(float v);
template <> __device__ __forceinline__ bf16_t to_e<true>(float v) { return (bf16_t)(pack2_bf16(v, 0.f) & 0xffffu); }
template <> __device__ __forceinline__ float to_e<false>(float v) { return v; }

// one K-quarter chain of a 16x16 tile: acc += A[r][k0 + ...] * Bfrag over NKC k-chunks, ascending (the step kernels' order)
template <bool WBF, int NKC, typename E>
__device__ __forceinline__ f32x4 quarter_chain(const E* As, int lda, int k0, const u32x4 (&b)[NKC], int r, int q) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kc = 0; kc < NKC; ++kc) {
    if constexpr (WBF) {
      const u32x4 av = *reinterpret_cast<const u32x4*>(&As[r * lda + k0 + 32 * kc + 8 * q]);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av), __builtin_bit_cast(bf16x8_t, b[kc]), acc, 0, 0, 0);
    } else {
      const float4 av = *reinterpret_cast<const float4*>(&As[r * lda + k0 + 16 * kc + 4 * q]);
      const float4 bv = __builtin_bit_cast(float4, b[kc]);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
    }
  }
  return acc;
}
// NKC fragments of the weight row at element offset row_elems_off (k contiguous) starting at column k0: lane (r, q) holds k = k0 + chunk + (8|4) q ...
template <bool WBF, int NKC>
__device__ __forceinline__ void load_frags(const void* w, long row_elems_off, int k0, int q, u32x4 (&b)[NKC]) {
#pragma unroll
  for (int kc = 0; kc < NKC; ++kc) {
    if constexpr (WBF) b[kc] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(w) + row_elems_off + k0 + 32 * kc + 8 * q);
    else b[kc] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(w) + row_elems_off + k0 + 16 * kc + 4 * q);
  }
}

// the tile of exchange number e (ring slot e % kRing) of chain (dir, bt)
template <typename E>
__device__ __forceinline__ E* slot_tile(E* xdata, int dir, int e, int nbt, int bt, long tile_elems) {
  return xdata + (((long)dir * kRing + (e & (kRing - 1))) * nbt + bt) * tile_elems;
}
// A wave publishes the rows it produced (4 of the 16-row tile: rows 4 kq .. 4 kq + 3), RE elements each, 16 bytes per lane: the element
// offset of this lane's chunk within the unit group's [16][RE] slice (staging area and exchange tile alike), -1 for a lane without one
template <int RE, typename E>
__device__ __forceinline__ int row_chunk(int kq, int lane) {
  constexpr int ES = sizeof(E), CPR = RE * ES / 16;                 // 16-byte chunks per row
  return lane < 4 * CPR ? (4 * kq + lane / CPR) * RE + (lane % CPR) * (16 / ES) : -1;
}
// from the LDS staging area to the wave's rows of an exchange tile (write-through, or plain inside a verified one-XCD cluster)
template <int RE, typename E>
__device__ __forceinline__ void publish_rows(const E* stage, E* slice, int eoff, bool local) {
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(slice, 16 * RE * sizeof(E));
  if (eoff >= 0) xstore(*reinterpret_cast<const u32x4*>(&stage[eoff]), rs, eoff * sizeof(E), local);
}
template <int RE, typename E>
__device__ __forceinline__ void poison_rows(E* slice, int eoff, bool local) {
  if (eoff >= 0) xstore((u32x4){kSentinel, kSentinel, kSentinel, kSentinel}, make_rsrc(slice, 16 * RE * sizeof(E)), eoff * sizeof(E), local);
}
// all-gather of a tile of U values per row, layout [unit group][row][16]  ->  A[row][group*16 + jj]
template <int U, typename E>
__device__ __forceinline__ void gather_rows(const E* tile, E* As, int lda, int tid, unsigned* status, bool& dead) {
  constexpr int ES = sizeof(E);
  gather_tile<16 * U * ES / 16, kThreads>(tile, tid, status, dead, [&](int idx, const u32x4& v) {
    const int e0 = idx * (16 / ES), sg2 = e0 / (16 * 16), rem = e0 % (16 * 16);
    *reinterpret_cast<u32x4*>(&As[(rem >> 4) * lda + sg2 * 16 + (rem & 15)]) = v;
  });
}
// ... of NG gates of U values per row, layout [unit group][row][gate][16]  ->  A[row][gate*U + group*16 + jj]
template <int NG, int U, typename E>
__device__ __forceinline__ void gather_gated(const E* tile, E* As, int lda, int tid, unsigned* status, bool& dead) {
  static_assert(NG == 2 || NG == 4, "the gate index is a bit field of the element offset");
  constexpr int ES = sizeof(E), LG = NG == 4 ? 2 : 1;
  gather_tile<16 * NG * U * ES / 16, kThreads>(tile, tid, status, dead, [&](int idx, const u32x4& v) {
    const int e0 = idx * (16 / ES), sg2 = e0 / (16 * 16 * NG), rem = e0 % (16 * 16 * NG);
    const int rw = rem >> (4 + LG), g = (rem >> 4) & (NG - 1), jj = rem & 15;
    *reinterpret_cast<u32x4*>(&As[rw * lda + g * U + sg2 * 16 + jj]) = v;
  });
}

// a wave's 16x16 MFMA result into an LDS plane [256] (C/D layout: row = 4q+e, col = r), and the fixed-order sum of four of them
__device__ __forceinline__ void put_frag(float* plane, const f32x4& acc, int r, int q) {
#pragma unroll
  for (int e = 0; e < 4; ++e) plane[(q * 4 + e) * 16 + r] = acc[e];
}
// (p = one element of quarter 0's plane, the quarters' planes `stride` floats apart)
__device__ __forceinline__ float sum_quarters(const float* p, int stride) { return (p[0] + p[stride]) + (p[2 * stride] + p[3 * stride]); }

// Bias gradient of the layer (Keras' recurrent bias: db = column sums of dz over time and batch) from bs[g], every thread's (row, unit)
// share of gate g summed over the steps: the 16 rows of the tile are 4 lanes apart in 4 waves -- shuffles, then the waves through LDS in
// a fixed order; one partial row [NG*U] per 16-row batch tile.  `red` = the unit group's four quarter planes, free after the last step.
template <int NG, int U>
__device__ __forceinline__ void bias_partials(const float (&bs)[NG], float (&red)[4][256], float* dbp, int kq, int lane, int b0, int b_end, int j0) {
  __syncthreads();
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    float v = bs[g];
    v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
    if (lane < 16) red[kq][g * 16 + lane] = v;
  }
  __syncthreads();
  if (kq == 0 && lane < NG * 16 && b0 < b_end) {
    const int g = lane >> 4, cc = lane & 15;
    dbp[(long)(b0 >> 4) * (NG * U) + g * U + j0 + cc] = sum_quarters(&red[0][g * 16 + cc], 256);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
// The (dt_u, u) pairs that have persistent kernels (fp32: u in {64,128,256}; bf16: u in {128,256,512}): index into a PERSIST_KERNELS
// table, -1 when there is none (callers use the per-step kernels then)
inline int width_index(int u, int dt_u) {
  if (dt_u == CRNN_BF16) return u == 128 ? 3 : u == 256 ? 4 : u == 512 ? 5 : -1;
  return u == 64 ? 0 : u == 128 ? 1 : u == 256 ? 2 : -1;
}
#define PERSIST_KERNELS(K) {K<false, 64>, K<false, 128>, K<false, 256>, K<true, 128>, K<true, 256>, K<true, 512>}

// One launch per chunk of co-resident chains: grid = clusters x members.  kernels: a PERSIST_KERNELS table; lds(u, es): the kernels' static
// LDS (residency); per_row: exchanged values per batch row and slot.  xreq & 1: XCD-local map (needs #clusters % 8 == 0, else the linear
// one); xreq & 2 (CRNN_RNN_DEBUG_DROP_MEMBER, tests only): the last workgroup is not launched -- its cluster waits, gives up and says so.
template <typename Dir>
int launch_persist(void (*const (&kernels)[6])(Dir, Dir, int, int, int, int, unsigned char*, int), size_t (*lds)(int, int), int per_row, const Dir& a,
                   const Dir& b, int T, int B, int u, int dt_u, void* xbuf, size_t xbuf_bytes, int xreq, hipStream_t stream) {
  const int wi = width_index(u, dt_u), es = (dt_u == CRNN_BF16) ? 2 : 4, nsw = u / (16 * kUW);
  if (wi < 0) return CRNN_ERR_UNSUPPORTED;
  const auto kernel = kernels[wi];
  const Chunking ck = chunking(B, nsw, kThreads, es, lds(u, es), per_row, (const void*)kernel);
  for (int lo = 0; lo < B; lo += ck.rows_per_launch) {
    const int cnt = (B - lo < ck.rows_per_launch) ? B - lo : ck.rows_per_launch;
    CRNN_TRY(prep_xbuf(xbuf, xbuf_bytes, ck.xdata_bytes, stream));     // every slot is written once per launch: poison first
    const int ncl = 2 * cdiv(cnt, 16);
    hipLaunchKernelGGL(kernel, dim3(ncl * nsw - ((xreq & 2) ? 1 : 0)), dim3(kThreads), 0, stream, a, b, T, B, lo, cnt, (unsigned char*)xbuf,
                       ((xreq & 1) && ncl % 8 == 0) ? 1 : 0);
  }
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

}  // namespace
