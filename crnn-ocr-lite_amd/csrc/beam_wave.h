// Wave-level helpers of the beam-search decoders (beam.hip, beam_lm.hip): one 64-lane wavefront per sample, lane = beam entry.
#pragma once
#include "common.h"
#include "ctc_core.h"      // NEG_INF

#define BEAM_MAX 64          // one beam entry per lane

__device__ __forceinline__ float blse(float a, float b) {
  if (a == NEG_INF) return b;
  if (b == NEG_INF) return a;
  float m = fmaxf(a, b), n = fminf(a, b);
  return m + log1pf(expf(n - m));
}

// Value of lane l (wave-uniform l) as a scalar: v_readlane_b32 instead of the LDS round trip of ds_bpermute_b32 -- the decoder is one wave per
// sample, a chain of several hundred dependent cross-lane reads per time step, so their latency IS its run time.
__device__ __forceinline__ int rl(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float rl(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// (min value, its lane) over lanes < cnt; ties -> lowest lane.  Result is wave-uniform.  The first four butterfly steps stay inside a row of
// 16 lanes (DPP: quad permutes, half-row mirror, row mirror -- any pairing works for an idempotent reduction); beams of at most 16 entries
// (the reference decodes with 5 or 10) never leave the row.
template <int CTRL>
__device__ __forceinline__ float max_dpp(float v) {
  return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false)));
}
// maximum over the 64 lanes, wave-uniform: four in-row DPP steps, then the four row maxima as scalars
__device__ __forceinline__ float wave_max64(float v) {
  v = max_dpp<0xB1>(v); v = max_dpp<0x4E>(v); v = max_dpp<0x141>(v); v = max_dpp<0x140>(v);
  return fmaxf(fmaxf(rl(v, 0), rl(v, 16)), fmaxf(rl(v, 32), rl(v, 48)));
}
template <int CTRL>
__device__ __forceinline__ void argmin_dpp(float& mv, int& ml) {
  const float ov = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(mv), __float_as_int(mv), CTRL, 0xf, 0xf, false));
  const int ol = __builtin_amdgcn_update_dpp(ml, ml, CTRL, 0xf, 0xf, false);
  if (ov < mv || (ov == mv && ol < ml)) { mv = ov; ml = ol; }
}
__device__ __forceinline__ void wave_argmin(float v, int lane, int cnt, float& mv, int& ml) {
  mv = (lane < cnt) ? v : INFINITY; ml = lane;
  argmin_dpp<0xB1>(mv, ml);      // quad_perm [1,0,3,2]
  argmin_dpp<0x4E>(mv, ml);      // quad_perm [2,3,0,1]
  argmin_dpp<0x141>(mv, ml);     // row_half_mirror
  argmin_dpp<0x140>(mv, ml);     // row_mirror
  if (cnt > 16) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      float ov = __shfl_xor(mv, o, 64); int ol = __shfl_xor(ml, o, 64);
      if (ov < mv || (ov == mv && ol < ml)) { mv = ov; ml = ol; }
    }
  }
  mv = rl(mv, 0); ml = rl(ml, 0);
}
