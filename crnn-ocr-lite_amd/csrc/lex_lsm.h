// The pre-pass shared by lexicon.hip (scores of a word list) and align.hip (best path of one transcription): one definition, so that both leave
// the same bits in the workspace.
//   lsm [B][Tmax][C] = log_softmax(log(y[b, skip + t] + eps)), Tmax = T - skip -- phase 1 of ctc_loss_grad_kernel word for word (a time step per
//   wave, CPL = 1 or 2 classes per lane).
#pragma once
#include "common.h"

#define LEX_EPS 1e-7f
#define NEG_INF (-INFINITY)

// ---- pre-pass: lsm [B][Tmax][C] = log_softmax(log(y[b, skip + t] + eps)), one wave per row ----------------------------------------------
template <int CPL>
__global__ __launch_bounds__(256) void lex_lsm_kernel(const float* __restrict__ y, float* __restrict__ lsm, long rows, int T, int Tmax, int C, int skip) {
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long b = row / Tmax;
  const int t = (int)(row - b * Tmax);
  const float* ys = y + ((long)b * T + skip + t) * C;
  float* out = lsm + row * C;
  const float z = lane < C ? logf(ys[lane] + LEX_EPS) : NEG_INF;
  if constexpr (CPL == 1) {
    const float m = wave_max(z);
    const float e = lane < C ? expf(z - m) : 0.f;
    const float lz = m + logf(wave_sum(e));
    if (lane < C) out[lane] = z - lz;
  } else {
    const bool up = lane + 64 < C;
    const float z1 = up ? logf(ys[lane + 64] + LEX_EPS) : NEG_INF;
    const float m = wave_max(fmaxf(z, z1));
    const float e = (lane < C ? expf(z - m) : 0.f) + (up ? expf(z1 - m) : 0.f);
    const float lz = m + logf(wave_sum(e));
    if (lane < C) out[lane] = z - lz;
    if (up) out[lane + 64] = z1 - lz;
  }
}

// B >= 1, 2 <= C <= 128, T > skip >= 0 (the callers have checked)
static inline int lex_lsm_launch(const float* y, float* lsm, int B, int T, int C, int skip, hipStream_t stream) {
  const int Tmax = T - skip;
  const long rows = (long)B * Tmax;
  if (C <= 64) hipLaunchKernelGGL(lex_lsm_kernel<1>, dim3(cdiv(rows, 4)), dim3(256), 0, stream, y, lsm, rows, T, Tmax, C, skip);
  else hipLaunchKernelGGL(lex_lsm_kernel<2>, dim3(cdiv(rows, 4)), dim3(256), 0, stream, y, lsm, rows, T, Tmax, C, skip);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
