// Lexicon decoding: the CTC log-probability of every word of a table under every sample's posterior map, and the best k words per sample.
//   scores[b][j] = log p(word_j | y[b, skip : skip + Tb]) = -K.ctc_batch_cost(word_j, y[b, skip:], Tb, |word_j|)     (utils.py:98-103 per pair)
// B x N independent alpha recursions over the same B maps: a throughput kernel, not a loop over ctc_loss_grad_kernel (16 waves, a beta recursion
// and a gradient phase per pair).  Three kernels:
//   lex_lsm_kernel     (ctc_core.h) pre-pass, once per sample: lsm = log_softmax(log(y + 1e-7)) of the window's rows into the workspace, so that the
//                      per-image-candidates mode (a few dozen words per image) does not pay a log-softmax per workgroup.
//   lex_score_kernel   one workgroup = one sample x a tile of 4 x wpw words (wpw = 16; ceil(M / 4), at least 4, for rows of fewer than 64 words).  The sample's lsm [Tb][C] is copied into LDS (7.6 KB at T = 50, C = 38:
//                      the 32 waves of a CU are resident); each wave walks wpw words of the tile.  The extended label
//                      (S = 2L + 1 <= 63 states) lives one state per lane as in ctc.hip; per frame one LDS gather lsm[t][ext] (independent of the chain,
//                      issued ahead of it), the s - 1 / s - 2 neighbours by wave shuffles, lse3 and an add.  The chain per frame -- a cross-lane
//                      move, three exponentials, a logarithm -- is latency-bound in one wave; throughput comes from the resident waves and from
//                      short words sharing a wave: 2 words side by side in 32-lane segments when both have S <= 32 (L <= 15), 4 in 16-lane segments
//                      when all have S <= 16 (L <= 7; LEX_PACK >= 2).  No value crosses a segment: lane s == 0 of a segment never takes its s - 1
//                      neighbour and no lane with s < 2 takes s - 2 -- the masks the recursion has anyway -- so a full-width shuffle is enough and a
//                      word's score is the same bits whichever way it was packed and whoever its neighbours were.
//                      A table entry that cannot be trusted (word_len outside [0, Lmax], a label outside [0, C - 2], a candidate index outside
//                      [0, N)) scores -inf and indexes nothing: the label is replaced by the blank before it is used as an LDS index.
//   lex_topk_kernel    one workgroup per sample: every thread keeps the 8 best of its strided share (strict >, ascending position: the earlier
//                      position wins a tie), then k rounds of a workgroup arg-max over the threads' heads (value descending, position ascending).
//                      One launch, a fixed order: two calls agree bit for bit.
// Arithmetic: the operations of ctc_loss_grad_kernel in its order (logf(y + eps), max-shifted log-softmax, lse3 in fp32, lse2 of the last two
// states) -- the loss kernel's own code: both take the rows, the trusted label and the alpha recursion from ctc_core.h.
// Measured (scripts/lexicon_bench.py -> profiles/lexicon_bench.txt; batch 1024, T = 52, C = 38, lexicons of lengths 2..23 sorted by length, MI355X):
//   * The recursion step is 66 vector instructions (3 v_exp, 1 v_log; expf / logf with their range reduction are most of it), 2 ds_bpermute, 1 ds_read: with 8
//     waves per SIMD the kernel is bound by vector issue, not by the chain's latency -- 210 cycles per (wave x frame) and SIMD at the nominal clock against about
//     145 of pure issue.  So words per wave-step is what pays: LEX_PACK = 0 (one word per wave) 2.29e8 pairs/s, 1 (two where both have L <= 15) 3.94e8,
//     2 (also four where all have L <= 7) 4.70e8 -- kept; the plain form's two runs differ by 0.3 %.
//   * tile = blockIdx.x % tiles: with 16 tiles per sample (N = 1000) the longest words of every sample -- the last tile of a sorted table -- ran on one XCD and
//     the packing bought nothing (4.76 ms against 4.63 unpacked); rotated by the sample index: 2.60 ms.
//   * K = 50 candidates per sample: 16 words per wave leave the fourth wave 2 words (253 us); 4 words per wave and thirteen workgroups per sample 264 us; the
//     row dealt evenly (13, 13, 13, 11) 208 us -- kept.
//   * Not built: a linear-domain recursion with a wave-wide scale -- it flushes unlikely words to -inf where the oracle has -200; two independent words
//     interleaved in one wave's instruction stream -- the issue slots it would fill are full.
#include "common.h"
#include "ctc_core.h"
#include <limits.h>

#ifndef LEX_PACK
#define LEX_PACK 2
#endif
#define LEX_WAVES 4
#define LEX_WORDS_PER_WAVE 16         // words a wave walks: one copy of the map into LDS serves 64 words; rows shorter than that (candidate lists) are dealt
#define LEX_WORDS_PER_WAVE_MIN 4      // evenly to the four waves, ceil(M / 4) each and at least 4 -- a workgroup's waves sit on the CU's four SIMDs
#define LEX_LDS_BYTES (64 * 1024)     // the lsm map of one sample: (T - skip) * C * 4 bytes must fit (include/crnn_mi355x.h states it)
#define LEX_MAX_LABEL_LEN 31
#define LEX_TOPK_MAX 8
#define LEX_TOPK_THREADS 256

// ---- scores ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * LEX_WAVES) void lex_score_kernel(const float* __restrict__ lsm_g, const int* __restrict__ input_len,
                                                                   const int* __restrict__ words, const int* __restrict__ word_len,
                                                                   const int* __restrict__ cand, float* __restrict__ scores, int Tmax, int C, int N,
                                                                   int Lmax, int M, int tiles, int wpw) {
  extern __shared__ float lsm[];       // [Tb][C]
  // blockIdx.x % 8 picks the XCD: with a tile count that is a multiple of 8 (N = 1000: 16 tiles) the plain tile = blockIdx.x % tiles would hand the longest
  // words of every sample -- the table is sorted by length -- to the same XCD; rotating by the sample spreads them (measured: 4.7 -> see profiles/lexicon_bench.txt)
  const int b = blockIdx.x / tiles;
  int tile = blockIdx.x - b * tiles + b % tiles; if (tile >= tiles) tile -= tiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Tb = ctc_window(input_len, b, Tmax);
  const float* src = lsm_g + (long)b * Tmax * C;
  for (int i = tid; i < Tb * C; i += 64 * LEX_WAVES) lsm[i] = src[i];
  __syncthreads();
  const int j0 = (tile * LEX_WAVES + wave) * wpw;
  const int j1 = min(j0 + wpw, M);
  for (int j = j0; j < j1;) {
    // the next (up to) four slots of this wave: table index, length, whether the entry can be trusted -- wave-uniform
    int nq[4], Lq[4];
    bool okq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int n = -1, L = -1;
      if (j + q < j1) {
        n = cand ? cand[(long)b * M + j + q] : j + q;
        if (n >= 0 && n < N) L = word_len[n];
      }
      okq[q] = L >= 0 && L <= Lmax;
      nq[q] = okq[q] ? n : 0;
      Lq[q] = okq[q] ? L : 0;                      // an untrusted slot walks as the empty word; its result is replaced below
    }
    int lg = 6;                                    // log2 of the segment width: 64 = one word, 32 = two, 16 = four
    if (LEX_PACK >= 1 && j + 1 < j1 && Lq[0] <= 15 && Lq[1] <= 15) lg = 5;
    if (LEX_PACK >= 2 && j + 3 < j1 && Lq[0] <= 7 && Lq[1] <= 7 && Lq[2] <= 7 && Lq[3] <= 7) lg = 4;
    const int seg = lane >> lg, s = lane & ((1 << lg) - 1);
    const int n = seg == 0 ? nq[0] : seg == 1 ? nq[1] : seg == 2 ? nq[2] : nq[3];
    const int L = seg == 0 ? Lq[0] : seg == 1 ? Lq[1] : seg == 2 ? Lq[2] : Lq[3];
    bool ok = seg == 0 ? okq[0] : seg == 1 ? okq[1] : seg == 2 ? okq[2] : okq[3];
    const int S = 2 * L + 1;
    const unsigned long long segmask = lg == 6 ? ~0ull : ((1ull << (1 << lg)) - 1) << (seg << lg);
    const int ext = ctc_ext_checked(words + (long)n * Lmax, S, s, C, segmask, ok);
    float res;
    if (Tb == 0) {
      res = L == 0 ? 0.f : NEG_INF;
    } else {
      const bool can_skip = ctc_can_skip(ext, s, S, C - 1);
      float a = ctc_alpha_init(lsm, ext, s, S);
      for (int t = 1; t < Tb; ++t) {
        const float em = lsm[t * C + ext];                        // (independent of the chain: issued ahead of it)
        a = ctc_alpha_step(a, em, s, S, can_skip);
      }
      res = ctc_alpha_total(a, lane - s, S);
    }
    if (!ok) res = NEG_INF;
    if (s == 0 && j + seg < j1) scores[(long)b * M + j + seg] = res;
    j += 64 >> lg;
  }
}

// ---- top k -----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lex_better(float v2, int p2, float v, int p) { return v2 > v || (v2 == v && p2 < p); }

__global__ __launch_bounds__(LEX_TOPK_THREADS) void lex_topk_kernel(const float* __restrict__ scores, const int* __restrict__ cand,
                                                                    int* __restrict__ idx, float* __restrict__ val, int M, int k) {
  __shared__ float wv[LEX_TOPK_THREADS / 64];
  __shared__ int wp[LEX_TOPK_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* sc = scores + (long)b * M;
  float v0 = NEG_INF, v1 = NEG_INF, v2 = NEG_INF, v3 = NEG_INF, v4 = NEG_INF, v5 = NEG_INF, v6 = NEG_INF, v7 = NEG_INF;
  int p0 = INT_MAX, p1 = INT_MAX, p2 = INT_MAX, p3 = INT_MAX, p4 = INT_MAX, p5 = INT_MAX, p6 = INT_MAX, p7 = INT_MAX;
  for (int p = tid; p < M; p += LEX_TOPK_THREADS) {
    const float v = sc[p];
    if (!(v > v7)) continue;                           // (strict: of equal values the earlier position stays; NaN and -inf never enter)
#define LEX_INS(hi, phi, lo, plo)      \
    if (v > hi) { lo = hi; plo = phi; } \
    else { lo = v; plo = p; continue; }
    LEX_INS(v6, p6, v7, p7)
    LEX_INS(v5, p5, v6, p6)
    LEX_INS(v4, p4, v5, p5)
    LEX_INS(v3, p3, v4, p4)
    LEX_INS(v2, p2, v3, p3)
    LEX_INS(v1, p1, v2, p2)
    LEX_INS(v0, p0, v1, p1)
#undef LEX_INS
    v0 = v; p0 = p;
  }
  for (int r = 0; r < k; ++r) {
    float bv = v0; int bp = p0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64); const int op = __shfl_xor(bp, o, 64);
      if (lex_better(ov, op, bv, bp)) { bv = ov; bp = op; }
    }
    if (lane == 0) { wv[wave] = bv; wp[wave] = bp; }
    __syncthreads();
    bv = wv[0]; bp = wp[0];
#pragma unroll
    for (int w = 1; w < LEX_TOPK_THREADS / 64; ++w)
      if (lex_better(wv[w], wp[w], bv, bp)) { bv = wv[w]; bp = wp[w]; }
    __syncthreads();
    const bool found = bv > NEG_INF;
    if (tid == 0) {
      idx[(long)b * k + r] = found ? (cand ? cand[(long)b * M + bp] : bp) : -1;
      val[(long)b * k + r] = found ? bv : NEG_INF;
    }
    if (found && bp == p0) {                             // the winner's owner moves its list up
      v0 = v1; p0 = p1; v1 = v2; p1 = p2; v2 = v3; p2 = p3; v3 = v4; p3 = p4; v4 = v5; p4 = p5; v5 = v6; p5 = p6; v6 = v7; p6 = p7;
      v7 = NEG_INF; p7 = INT_MAX;
    }
  }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------------
extern "C" size_t crnn_ctc_lexicon_workspace_bytes(int B, int T, int C, int skip) {
  return lex_lsm_bytes(B, T, C, skip);
}

extern "C" int crnn_ctc_lexicon_score(const float* y, const int* input_len, const int* words, const int* word_len, const int* cand, float* scores,
                                      void* ws, size_t ws_bytes, int B, int T, int C, int skip, int N, int Lmax, int K, hipStream_t stream) {
  if (!y || !words || !word_len || !scores || !ws) return CRNN_ERR_ARG;
  if (B < 0 || N < 0 || Lmax < 0 || C < 2 || skip < 0 || T <= skip || (cand && K < 0)) return CRNN_ERR_ARG;
  if (C > 128 || Lmax > LEX_MAX_LABEL_LEN) return CRNN_ERR_UNSUPPORTED;
  const int Tmax = T - skip;
  const size_t lds = (size_t)Tmax * C * sizeof(float);
  if (lds > LEX_LDS_BYTES) return CRNN_ERR_UNSUPPORTED;
  if (ws_bytes < lex_lsm_bytes(B, T, C, skip)) return CRNN_ERR_ARG;
  const int M = cand ? K : N;
  if (B == 0 || N == 0 || M == 0) return CRNN_OK;
  const int wpw = max(LEX_WORDS_PER_WAVE_MIN, min(LEX_WORDS_PER_WAVE, cdiv(M, LEX_WAVES)));
  const int tiles = cdiv(M, LEX_WAVES * wpw);
  if ((long)B * tiles > 0x7fffffffL) return CRNN_ERR_UNSUPPORTED;
  float* lsm = (float*)ws;
  CRNN_TRY(lex_lsm_launch(y, lsm, B, T, C, skip, stream));
  hipLaunchKernelGGL(lex_score_kernel, dim3(B * tiles), dim3(64 * LEX_WAVES), lds, stream, (const float*)lsm, input_len, words, word_len, cand, scores,
                     Tmax, C, N, Lmax, M, tiles, wpw);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

extern "C" int crnn_ctc_lexicon_topk(const float* scores, const int* cand, int* idx, float* val, int B, int M, int k, hipStream_t stream) {
  if (!scores || !idx || !val || B < 0 || M < 0) return CRNN_ERR_ARG;
  if (k < 1 || k > LEX_TOPK_MAX) return CRNN_ERR_ARG;
  if (B == 0) return CRNN_OK;
  hipLaunchKernelGGL(lex_topk_kernel, dim3(B), dim3(LEX_TOPK_THREADS), 0, stream, scores, cand, idx, val, M, k);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
