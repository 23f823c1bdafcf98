// Character alignment: the best CTC path (Viterbi) of one given transcription per sample through the sample's posterior map, with its backtrace --
// where each character sits on the time axis and how sure the network is of each one.
//   score[b]        = max over the CTC paths pi of labels[b] of sum_t lsm[t][pi_t],  lsm = log_softmax(log(y[b, skip : skip + Tb] + 1e-7))
//   states[b][t]    = state of the best path at frame t (extended label: even = blank, odd s = character (s - 1) / 2), -1 for t >= Tb
//   start / end [l] = first frame of character l and one past its last;  char_logp[l] = sum of lsm[t][label_l] over that span
// Two kernels: lex_lsm_kernel (ctc_core.h, the pre-pass of lexicon.hip: the same bits in the same workspace) and ctc_align_kernel.
//   ctc_align_kernel   one wavefront = one sample, ALIGN_WAVES samples per workgroup.  The extended label (S = 2L + 1 <= 63 states) lives one state
//                      per lane as in ctc.hip / lexicon.hip.  Per frame: the s - 1 / s - 2 neighbours by two DPP wave shifts (a vector move each, no
//                      LDS round trip), two compares, an add.  lsm[t][ext] does not depend on the chain: the 16 values of the NEXT block of frames
//                      are loaded (from the workspace; a 512 x 128 map does not fit LDS) before the chain walks the current block.  Backpointers
//                      (0 = stay, 1 = from s - 1, 2 = from s - 2) are packed 2 bits per frame into a register and stored to LDS once per 16 frames:
//                      [ceil(Tmax / 16)][64] dwords, 8 KB per wave at 512 frames.  The backtrace is a wave-uniform loop over those words and leaves
//                      the path in LDS; then lane t writes states[t] and marks where a character's run begins and ends, and lane l adds up
//                      character l's span.  No global scratch beyond lsm.
// Tie rule (part of the contract, include/crnn_mi355x.h): equal values go to the HIGHER state index -- stay beats s - 1 beats s - 2 (strict > in that
// order), and at the end S - 1 beats S - 2 unless v[S - 2] > v[S - 1].  max and add are exactly rounded, so the recursion is reproducible bit for
// bit on the host (tests/align_ref.py) and score equals the fp32 sum of the path's lsm values added in increasing t.
// Nothing is indexed through an untrusted value: a label_len outside [0, min(Lmax, 31)] walks as the empty word and a label outside [0, C - 2] as
// the blank; the sample's results are then replaced by "no alignment" (score -inf, states -1, no spans).  A map that is not a softmax map (a NaN, an infinity, a
// negative entry) makes the path's value NaN: no alignment either, and the span pass reads only spans the path marked.
#include "common.h"
#include "ctc_core.h"

#define ALIGN_WAVES 4
#define ALIGN_MAX_LABEL_LEN 31
#define ALIGN_MAX_FRAMES 512
#define ALIGN_BLOCK 16                 // frames per backpointer word (2 bits each) and per block of prefetched lsm values

// A wave's LDS region is its own: a wave-level fence orders its writes before its later reads (the LDS executes one wave's operations in order),
// so the samples of a workgroup never wait for each other.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// lane i <- lane i - 1 of the wavefront (DPP wave_shr:1); lane 0 keeps `fill`
__device__ __forceinline__ float wave_shr1(float v, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// LDS of one wave, in dwords: backpointer words, the path, and the characters' first / one-past-last frames
__host__ __device__ static inline int align_wave_dwords(int Tmax) { return (Tmax + ALIGN_BLOCK - 1) / ALIGN_BLOCK * 64 + Tmax + 64; }

__global__ __launch_bounds__(64 * ALIGN_WAVES) void ctc_align_kernel(const float* __restrict__ lsm_g, const int* __restrict__ input_len,
                                                                     const int* __restrict__ labels, const int* __restrict__ label_len,
                                                                     float* __restrict__ score, int* __restrict__ states, int* __restrict__ start,
                                                                     int* __restrict__ end, float* __restrict__ char_logp, int B, int Tmax, int C,
                                                                     int Lmax) {
  extern __shared__ int align_lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nblk = (Tmax + ALIGN_BLOCK - 1) / ALIGN_BLOCK;
  int* bp = align_lds + wave * align_wave_dwords(Tmax);   // [nblk][64]
  int* path = bp + nblk * 64;                             // [Tmax]
  int* cs = path + Tmax;                                  // [32] first frame of character l
  int* ce = cs + 32;                                      // [32] one past its last
  const int b = blockIdx.x * ALIGN_WAVES + wave;
  if (b >= B) return;                                     // (wave-uniform; no workgroup barrier below)
  cs[lane] = -1;                                          // cs and ce: no span until the path marks one
  const int blank = C - 1;
  const int Tb = __builtin_amdgcn_readfirstlane(ctc_window(input_len, b, Tmax));
  int len = label_len[b];
  bool ok = len >= 0 && len <= Lmax && len <= ALIGN_MAX_LABEL_LEN;
  const int L = __builtin_amdgcn_readfirstlane(ok ? len : 0);      // an untrusted length walks as the empty word; its results are replaced below
  const int S = 2 * L + 1, s = lane;
  const int ext = ctc_ext_checked(labels + (long)b * Lmax, S, s, C, ~0ull, ok);
  const int mylab = __shfl(ext, (2 * lane + 1) & 63, 64);          // lane l: the label of character l (validated above)
  const bool can_skip = ctc_can_skip(ext, s, S, blank);
  const float* lsm_b = lsm_g + (long)b * Tmax * C;
  const float* col = lsm_b + ext;                                  // lsm[t][ext] = col[t * C]

  float res = NEG_INF;
  int fin = 0;
  if (Tb == 0) {
    res = L == 0 ? 0.f : NEG_INF;
  } else {
    float em[ALIGN_BLOCK], emn[ALIGN_BLOCK];
#pragma unroll
    for (int k = 0; k < ALIGN_BLOCK; ++k) em[k] = col[(long)min(k, Tb - 1) * C];
    float v = (s == 0 || (s == 1 && S > 1)) ? em[0] : NEG_INF;
    const int nb = (Tb + ALIGN_BLOCK - 1) / ALIGN_BLOCK;
    for (int c = 0; c < nb; ++c) {
      const int t0 = c * ALIGN_BLOCK;
      if (c + 1 < nb) {
#pragma unroll
        for (int k = 0; k < ALIGN_BLOCK; ++k) emn[k] = col[(long)min(t0 + ALIGN_BLOCK + k, Tb - 1) * C];      // (ahead of the chain: independent of it)
      }
      unsigned word = 0;
#pragma unroll
      for (int k = 0; k < ALIGN_BLOCK; ++k) {
        const int t = t0 + k;
        if (t >= 1 && t < Tb) {                                    // wave-uniform
          const float v1 = wave_shr1(v, NEG_INF);
          const float v2r = wave_shr1(v1, NEG_INF);
          const float v2 = can_skip ? v2r : NEG_INF;
          float best = v;
          unsigned code = 0;
          if (v1 > best) { best = v1; code = 1; }
          if (v2 > best) { best = v2; code = 2; }
          v = s < S ? best + em[k] : NEG_INF;
          word |= code << (2 * k);
        }
      }
      bp[c * 64 + lane] = (int)word;
      if (c + 1 < nb) {
#pragma unroll
        for (int k = 0; k < ALIGN_BLOCK; ++k) em[k] = emn[k];
      }
    }
    const float vL = __shfl(v, S - 1, 64);
    const float vL2 = __shfl(v, S > 1 ? S - 2 : 0, 64);
    fin = S - 1;
    res = vL;
    if (S > 1 && vL2 > vL) { fin = S - 2; res = vL2; }
  }
  if (!ok) res = NEG_INF;
  // A map with a NaN, an infinity or a negative entry gives a NaN lsm row and a NaN value in every state: no comparison of the chain held, the
  // backpointers say nothing -- no alignment.  (res > NEG_INF is false for NaN.)
  const bool aligned = res > NEG_INF && res < INFINITY;            // wave-uniform
  if (!aligned) res = NEG_INF;
  wave_lds_fence();                                                // the backpointer words are in LDS
  if (aligned && Tb > 0) {
    int sp = __builtin_amdgcn_readfirstlane(fin);
    for (int t = Tb - 1; t >= 1; --t) {
      path[t] = sp;
      const unsigned w = (unsigned)bp[(t >> 4) * 64 + sp];
      sp -= (int)((w >> (2 * (t & 15))) & 3u);
    }
    path[0] = sp;
  }
  wave_lds_fence();                                                // the path is in LDS
  for (int t = lane; t < Tmax; t += 64) {
    int st = -1;
    if (aligned && t < Tb) {
      st = path[t];
      if (st & 1) {
        if (t == 0 || path[t - 1] != st) cs[st >> 1] = t;
        if (t == Tb - 1 || path[t + 1] != st) ce[st >> 1] = t + 1;
      }
    }
    if (states) states[(long)b * Tmax + t] = st;
  }
  wave_lds_fence();                                                // every character's span is in LDS
  for (int l = lane; l < Lmax; l += 64) {
    int a = -1, e = -1;
    float lp = NEG_INF;
    if (aligned && l < L) {
      a = cs[l]; e = ce[l];
      if (a >= 0 && e > a && e <= Tb) {                            // (every character of an aligned path has a span; nothing is read outside the window)
        const float* cl = lsm_b + mylab;
        lp = cl[(long)a * C];
        for (int t = a + 1; t < e; ++t) lp += cl[(long)t * C];
      } else {
        a = -1; e = -1;
      }
    }
    const long o = (long)b * Lmax + l;
    if (start) start[o] = a;
    if (end) end[o] = e;
    if (char_logp) char_logp[o] = lp;
  }
  if (lane == 0) score[b] = res;
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------------
extern "C" size_t crnn_ctc_align_workspace_bytes(int B, int T, int C, int skip) {
  return lex_lsm_bytes(B, T, C, skip);
}

extern "C" int crnn_ctc_align(const float* y, const int* input_len, const int* labels, const int* label_len, float* score, int* states, int* start,
                              int* end, float* char_logp, void* ws, size_t ws_bytes, int B, int T, int C, int skip, int Lmax, hipStream_t stream) {
  if (!y || !labels || !label_len || !score || !ws) return CRNN_ERR_ARG;
  if (B < 0 || T < 0 || C < 2 || skip < 0 || T <= skip || Lmax < 1) return CRNN_ERR_ARG;
  const int Tmax = T - skip;
  if (C > 128 || Tmax > ALIGN_MAX_FRAMES) return CRNN_ERR_UNSUPPORTED;
  if (ws_bytes < lex_lsm_bytes(B, T, C, skip)) return CRNN_ERR_ARG;
  if (B == 0) return CRNN_OK;
  float* lsm = (float*)ws;
  CRNN_TRY(lex_lsm_launch(y, lsm, B, T, C, skip, stream));
  const size_t lds = (size_t)ALIGN_WAVES * align_wave_dwords(Tmax) * sizeof(int);      // 42 KB at 512 frames
  hipLaunchKernelGGL(ctc_align_kernel, dim3(cdiv(B, ALIGN_WAVES)), dim3(64 * ALIGN_WAVES), lds, stream, (const float*)lsm, input_len, labels, label_len,
                     score, states, start, end, char_logp, B, Tmax, C, Lmax);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
