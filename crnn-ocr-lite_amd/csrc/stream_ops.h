// Device helpers shared by the streaming kernels (weights-resident / plane / weight-gradient GEMMs, depthwise row streams, dense2's backward, the
// persistent recurrences): the 16-byte vector types, LDS-DMA in its two forms, counted vector-memory waits, MFMA fragment reads from LDS and the
// element forms of a 16-byte chunk.  One copy of each; include after common.h.
#pragma once
#include "common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // native vector: a uint4 struct copy becomes a memcpy through scratch
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(uintptr_t)((__attribute__((address_space(3))) const unsigned char*)p); }

// LDS-DMA the compiler does not see: 16 bytes per lane from each lane's own global address to lds_dst (wave-uniform, from lds_addr) + 16 lane.  Inline asm,
// so the compiler neither drains it (it would wait vmcnt(0) before every LDS read that follows a DMA it knows of) nor counts it: pair it with wait_vm<N>.
__device__ __forceinline__ void dma16_m0(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// LDS-DMA through the builtin: 16 bytes per lane to l (wave-uniform) + 16 lane.  POLICY = the cache-policy bits: 0 plain, 2 nontemporal.
template <int POLICY>
__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, POLICY);
}
template <int N> __device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// MFMA operand fragment (8 bf16) as one 16-byte LDS read
__device__ __forceinline__ bf16x8_t frag16(const unsigned char* p) { return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4*>(p)); }
// fragment = the 8 bf16 (k = 16 ks + 8 half .. +7) of tile row r0 + l31, from a k-major stage of row stride LD bf16 (as gemm_tile.h read_frag_h<true>):
// two ds_read_b64_tr_b16
template <int LD>
__device__ __forceinline__ bf16x8_t frag_tr(const unsigned char* Xs, int r0, int ks, int half, int l31) {
  const int li = l31 & 15;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(Xs) + (ks * 16 + 8 * half + (li >> 2)) * LD + r0 + (l31 & 16) + (li & 3) * 4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)X);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(X + 4 * LD));
  const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
  return __builtin_bit_cast(bf16x8_t, make_uint4(a.x, a.y, b.x, b.y));
}
// the same from a swizzled, unpadded stage (row = pixel, 128 channels = 256 B; 16-byte chunk c of row r at position c ^ ((r & 3) << 2))
__device__ __forceinline__ bf16x8_t frag_tr_sw(const unsigned char* Xs, int r0, int ks, int half, int l31) {
  const int li = l31 & 15;
  const int row = ks * 16 + 8 * half + (li >> 2), col = r0 + (l31 & 16) + (li & 3) * 4;
  const unsigned short* X = reinterpret_cast<const unsigned short*>(Xs) + row * 128 + ((((col >> 3) ^ ((row & 3) << 2)) << 3) | (col & 7));
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)X);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(X + 4 * 128));
  const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
  return __builtin_bit_cast(bf16x8_t, make_uint4(a.x, a.y, b.x, b.y));
}

__device__ __forceinline__ void widen8(const u32x4& u, float (&f)[8]) {
  f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
  f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
  f[4] = __uint_as_float(u.z << 16); f[5] = __uint_as_float(u.z & 0xffff0000u);
  f[6] = __uint_as_float(u.w << 16); f[7] = __uint_as_float(u.w & 0xffff0000u);
}
// element forms of a 16-byte chunk: 8 bf16 (EPC = 8) or 4 fp32 (EPC = 4; the parity mode's depthwise streams)
template <int EPC> __device__ __forceinline__ void widenE(const u32x4& u, float (&f)[EPC]);
template <> __device__ __forceinline__ void widenE<8>(const u32x4& u, float (&f)[8]) { widen8(u, f); }
template <> __device__ __forceinline__ void widenE<4>(const u32x4& u, float (&f)[4]) {
  f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y); f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
}
template <int EPC> __device__ __forceinline__ u32x4 packE(const float (&f)[EPC]);
template <> __device__ __forceinline__ u32x4 packE<8>(const float (&f)[8]) {
  u32x4 o; o.x = pack2_bf16(f[0], f[1]); o.y = pack2_bf16(f[2], f[3]); o.z = pack2_bf16(f[4], f[5]); o.w = pack2_bf16(f[6], f[7]); return o;
}
template <> __device__ __forceinline__ u32x4 packE<4>(const float (&f)[4]) {
  u32x4 o; o.x = __float_as_uint(f[0]); o.y = __float_as_uint(f[1]); o.z = __float_as_uint(f[2]); o.w = __float_as_uint(f[3]); return o;
}
