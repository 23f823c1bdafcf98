// The CTC arithmetic of ctc.hip (loss and gradient), lexicon.hip (scores of a word list) and align.hip (best path of one transcription): one
// definition of each piece, because the public contract holds them together -- a lexicon score is the negated loss bit for bit, and the
// alignment leaves the lexicon's bits in the workspace.  Everything is __forceinline__ (what that does to the kernels' code: profiles/ctc_core_isa.txt).
// beam.hip takes the two constants and the window only; its arithmetic is TF's beam search, not this.
//   rows        one wave per row, lane l = class l, and class l + 64 as well when CPL (classes per lane) is 2, under `if constexpr (CPL == 2)`
//   recursion   the extended label (S = 2L + 1 <= 64 states) lives one state per lane, the s - 1 / s - 2 neighbours come by wave shuffles, fp32 in log space
#pragma once
#include "common.h"

#define CTC_EPS 1e-7f
#define NEG_INF (-INFINITY)

__device__ __forceinline__ float lse2(float a, float b) {
  if (a == NEG_INF) return b;
  if (b == NEG_INF) return a;
  float m = fmaxf(a, b);
  return m + logf(expf(a - m) + expf(b - m));
}
// log(e^a + e^b + e^c) in one go, branch-free (absent terms are -inf: e^-inf = 0): three exponentials and one logarithm on the recursions' dependent chain
// where two nested lse2 took four and two
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  const float mm = (m == NEG_INF) ? 0.f : m;                  // (all three absent: the sum below is 0 and its logarithm -inf)
  return mm + logf(expf(a - mm) + expf(b - mm) + expf(c - mm));
}

struct ctc_lane_pair { float lo, hi; };      // the values of classes lane and lane + 64 (hi: CPL == 2 only)
// softmax of one row: v / v1 = the lane's logits, NEG_INF where the class does not exist -> its probabilities
template <int CPL>
__device__ __forceinline__ ctc_lane_pair softmax_row(float v, float v1, int lane, int C) {
  float m = v;
  if constexpr (CPL == 2) m = fmaxf(v, v1);
  m = wave_max(m);
  const float e = lane < C ? expf(v - m) : 0.f;
  float e1 = 0.f, es = e;
  if constexpr (CPL == 2) { e1 = lane + 64 < C ? expf(v1 - m) : 0.f; es = e + e1; }
  const float s = wave_sum(es);
  ctc_lane_pair p = {e / s, 0.f};
  if constexpr (CPL == 2) p.hi = e1 / s;
  return p;
}

// out[0..C) = log_softmax(log(y[0..C) + eps)): Keras' ctc_batch_cost hands TF log(y + eps), and TF takes its own log-softmax of that
template <int CPL>
__device__ __forceinline__ void log_softmax_of_log_row(const float* y, float* out, int lane, int C) {
  const float z = lane < C ? logf(y[lane] + CTC_EPS) : NEG_INF;
  const bool up = CPL == 2 && lane + 64 < C;
  float z1 = NEG_INF, m = z;
  if constexpr (CPL == 2) { z1 = up ? logf(y[lane + 64] + CTC_EPS) : NEG_INF; m = fmaxf(z, z1); }
  m = wave_max(m);
  float e = lane < C ? expf(z - m) : 0.f;
  if constexpr (CPL == 2) e = e + (up ? expf(z1 - m) : 0.f);
  const float lz = m + logf(wave_sum(e));
  if (lane < C) out[lane] = z - lz;
  if constexpr (CPL == 2) if (up) out[lane + 64] = z1 - lz;
}

// frames of a sample's window: its input length, or all Tmax where no lengths are given, clamped to [0, Tmax]
__device__ __forceinline__ int ctc_window(int len, int Tmax) { if (len > Tmax) len = Tmax; if (len < 0) len = 0; return len; }
__device__ __forceinline__ int ctc_window(const int* input_len, int b, int Tmax) { return ctc_window(input_len ? input_len[b] : Tmax, Tmax); }

// State s of the extended label of an UNTRUSTED row (S = 2L + 1 states, L already checked): even states are the blank, odd s is label (s - 1) / 2.
// A label outside [0, C - 2] is replaced by the blank BEFORE the value is used as an index, and clears `ok` for every lane of its segment
// (segmask: the lanes that walk the same word; all 64 where a wave walks one).
__device__ __forceinline__ int ctc_ext_checked(const int* row, int S, int s, int C, unsigned long long segmask, bool& ok) {
  int ext = C - 1;
  bool bad = false;
  if (s < S && (s & 1)) {
    const int v = row[s >> 1];
    if (v < 0 || v > C - 2) bad = true; else ext = v;
  }
  ok = ok && !(__ballot(bad) & segmask);
  return ext;
}

// may state s be entered from s - 2: not a blank, and not the same character as the one before (a repeat needs the blank between)
__device__ __forceinline__ bool ctc_can_skip(int ext, int s, int S, int blank) {
  const int ext2 = __shfl_up(ext, 2, 64);
  return (s >= 2) && (s < S) && (ext != blank) && (ext != ext2);
}

// the alpha recursion: alpha_t(s) = log p(the first t + 1 frames end in state s), the emission at t included.  lsm0 = the first frame's row
__device__ __forceinline__ float ctc_alpha_init(const float* lsm0, int ext, int s, int S) {
  float a = NEG_INF;
  if (s == 0) a = lsm0[ext];
  else if (s == 1 && S > 1) a = lsm0[ext];
  return a;
}
// em = lsm[t][ext]: independent of the chain, so the caller loads it ahead of this
__device__ __forceinline__ float ctc_alpha_step(float a, float em, int s, int S, bool can_skip) {
  const float a1 = __shfl_up(a, 1, 64), a2 = __shfl_up(a, 2, 64);
  const float v = lse3(a, s >= 1 ? a1 : NEG_INF, can_skip ? a2 : NEG_INF);
  return (s < S && v != NEG_INF) ? v + em : NEG_INF;
}
// log p(label) = lse2 of the last two states; base = the lane of the word's state 0
__device__ __forceinline__ float ctc_alpha_total(float a, int base, int S) {
  const float aL = __shfl(a, base + S - 1, 64);
  const float aL2 = __shfl(a, base + (S > 1 ? S - 2 : 0), 64);
  return lse2(aL, S > 1 ? aL2 : NEG_INF);
}

// pre-pass of the lexicon scores and the alignment, once per sample: lsm [B][Tmax][C] = log_softmax(log(y[b, skip + t] + eps)), Tmax = T - skip,
// one wave per row as in phase 1 of ctc_loss_grad_kernel
template <int CPL>
__global__ __launch_bounds__(256) void lex_lsm_kernel(const float* __restrict__ y, float* __restrict__ lsm, long rows, int T, int Tmax, int C, int skip) {
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long b = row / Tmax;
  const int t = (int)(row - b * Tmax);
  log_softmax_of_log_row<CPL>(y + ((long)b * T + skip + t) * C, lsm + row * C, lane, C);
}

// B >= 1, 2 <= C <= 128, T > skip >= 0 (the callers have checked).  A template only so that a file that never calls it (ctc.hip, beam.hip) instantiates,
// and so emits, no pre-pass kernel.
template <typename = void>
static inline int lex_lsm_launch(const float* y, float* lsm, int B, int T, int C, int skip, hipStream_t stream) {
  const int Tmax = T - skip;
  const long rows = (long)B * Tmax;
  if (C <= 64) hipLaunchKernelGGL(lex_lsm_kernel<1>, dim3(cdiv(rows, 4)), dim3(256), 0, stream, y, lsm, rows, T, Tmax, C, skip);
  else hipLaunchKernelGGL(lex_lsm_kernel<2>, dim3(cdiv(rows, 4)), dim3(256), 0, stream, y, lsm, rows, T, Tmax, C, skip);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
// bytes of lsm: what crnn_ctc_lexicon_workspace_bytes and crnn_ctc_align_workspace_bytes answer
static inline size_t lex_lsm_bytes(int B, int T, int C, int skip) {
  if (B < 0 || C < 1 || skip < 0 || T <= skip) return 0;
  return (size_t)B * (size_t)(T - skip) * (size_t)C * sizeof(float);
}
