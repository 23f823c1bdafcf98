// Lexicon shortlists: for every sample the K words of a table nearest in edit distance to its decoded label rows -- the candidate lists that
// crnn_ctc_lexicon_score's `cand` mode then scores exactly -- made where the beam kernel leaves its paths and the table already lives.
//   d(b, j) = min over p < P of Levenshtein(query[b][p], word_j), unit costs; query[b][p] = the elements of queries[b][p][:] inside [0, C - 2], in
//   their order (the blank C - 1, the -1 padding and anything else dropped wherever it stands), cut to its first 64 symbols: words are at most
//   31 long, so a longer query is more than 33 edits from every word and the order among the words means nothing there.
// Two kernels, one workspace (hist [B][256] int32, then d [B][roundup(N, 4)] uint8):
//   near_dist_kernel    grid (tiles of NEAR_TILE words, B), one lane per word -- score.hip's one wavefront per pair is the wrong shape for B x 88 000
//                       pairs.  The workgroup first builds the sample's match masks Peq[p][c] in LDS (bit r of Peq[p][c] = "symbol r of query p is
//                       c"; the filter is score.hip's ballot + prefix popcount, the bits set with LDS integer OR), then every lane walks its word
//                       through Myers' recurrence (J. ACM 46(3), 1999, Hyyro's form; pattern = query, text = word; global distance:
//                       Ph = (Ph << 1) | 1 as in score.hip) with the state in its own registers and Eq one LDS read per character.  The machine
//                       word is 32 bits when every query of the sample has m <= 32 (the normal case) and 64 otherwise: one branch per workgroup,
//                       so wave-uniform.  Low and high halves of the masks are separate LDS planes, so the 32-bit walk reads consecutive banks
//                       for consecutive classes.  d goes out as one byte per word; the workgroup counts its d values in an LDS histogram and adds
//                       the non-empty bins to hist[b] -- integer atomics only: the sums do not depend on arrival order.
//                       A table entry that cannot be trusted (word_len outside [0, Lmax], a label outside [0, C - 2]) gets d = 255; its labels are
//                       replaced by 0 before they index the masks, and rows are read inside [0, Lmax) only.
//   near_select_kernel  one workgroup per sample: the threshold d* from the histogram (count below d* < K <= count up to d*), then one sweep of the
//                       d bytes in index order that compacts, by a packed (below, equal) prefix count, every index with d < d* and the first
//                       K - below of those with d == d*; the -1 tail.  The sweep ends as soon as the row is full.
// No float atomics, no fences, no waiting on another workgroup; every order is fixed by indices: two calls agree bit for bit.
#include "common.h"

#define NEAR_THREADS 256
#ifndef NEAR_WORDS_PER_THREAD
#define NEAR_WORDS_PER_THREAD 4                            // (scripts/build_nearest_variants.sh builds 1, 2 and 8 for scripts/lexicon_shortlist_bench.py)
#endif
#define NEAR_TILE (NEAR_THREADS * NEAR_WORDS_PER_THREAD)   // words per workgroup: one build of the masks serves 1024 words
#define NEAR_MAX_P 8
#define NEAR_MAX_C 128
#define NEAR_MAX_QCOLS 1024
#define NEAR_MAX_K 1024
#define NEAR_MAX_LABEL_LEN 31
#define NEAR_MAX_QUERY 64
#define NEAR_UNTRUSTED 255

static inline size_t near_row_bytes(int N) { return ((size_t)N + 3) & ~(size_t)3; }
static inline size_t near_hist_bytes(int B) { return (size_t)B * 256 * sizeof(int); }

__device__ __forceinline__ unsigned long long near_eq(const unsigned* lo, const unsigned* hi, int c, unsigned long long) {
  return (unsigned long long)lo[c] | ((unsigned long long)hi[c] << 32);
}
__device__ __forceinline__ unsigned near_eq(const unsigned* lo, const unsigned*, int c, unsigned) { return lo[c]; }

// four labels of a row from position i (a multiple of 4, i < Lmax): one 16-byte load where rows are 16-byte aligned, else dwords inside the row
__device__ __forceinline__ int4 near_load4(const int* row, int i, int Lmax, bool vec) {
  if (vec) return *reinterpret_cast<const int4*>(row + i);
  int4 q;
  q.x = row[i];
  q.y = i + 1 < Lmax ? row[i + 1] : 0;
  q.z = i + 2 < Lmax ? row[i + 2] : 0;
  q.w = i + 3 < Lmax ? row[i + 3] : 0;
  return q;
}

// Levenshtein(query, word) for a query of 1 <= m <= bits(W) symbols whose match masks are lo / hi[c]; every label is made a safe index first
template <typename W>
__device__ __forceinline__ int near_walk(const unsigned* lo, const unsigned* hi, int m, const int* row, int L, int Lmax, bool vec, int C) {
  const int bits = 8 * (int)sizeof(W);
  W Pv = m == bits ? ~(W)0 : ((W)1 << m) - 1, Mv = 0;
  const W top = (W)1 << (m - 1);
  int score = m;
  for (int i = 0; i < L; i += 4) {
    const int4 q = near_load4(row, i, Lmax, vec);
    const int c4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i + k < L) {
        const int c = (unsigned)c4[k] <= (unsigned)(C - 2) ? c4[k] : 0;
        const W Eq = near_eq(lo, hi, c, (W)0);
        const W Xv = Eq | Mv;
        const W Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        W Ph = Mv | ~(Xh | Pv);
        W Mh = Pv & Xh;
        score += (Ph & top) ? 1 : ((Mh & top) ? -1 : 0);
        Ph = (Ph << 1) | 1;
        Mh <<= 1;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
      }
    }
  }
  return score;
}

__global__ __launch_bounds__(NEAR_THREADS) void near_dist_kernel(const int* __restrict__ queries, int P, int qcols, const int* __restrict__ words,
                                                                 const int* __restrict__ word_len, unsigned char* __restrict__ d8,
                                                                 int* __restrict__ hist, int C, int N, int Lmax, long row_bytes, int vec) {
  __shared__ unsigned peq_lo[NEAR_MAX_P * NEAR_MAX_C], peq_hi[NEAR_MAX_P * NEAR_MAX_C];
  __shared__ int bins[256];
  __shared__ int qm[NEAR_MAX_P];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < P * C; i += NEAR_THREADS) { peq_lo[i] = 0; peq_hi[i] = 0; }
  bins[tid] = 0;
  __syncthreads();
  // the match masks: wave w filters queries w, w + 4; the kept symbols of each 64-column chunk get consecutive bit positions
  for (int p = wave; p < P; p += NEAR_THREADS / 64) {
    const int* q = queries + ((long)b * P + p) * qcols;
    int m = 0;
    for (int c0 = 0; c0 < qcols && m < NEAR_MAX_QUERY; c0 += 64) {
      const int col = c0 + lane;
      int v = -1;
      if (col < qcols) v = q[col];
      const bool keep = (unsigned)v <= (unsigned)(C - 2);
      const unsigned long long mask = __ballot(keep);
      const int r = m + __popcll(mask & ((1ull << lane) - 1));
      if (keep && r < NEAR_MAX_QUERY) {
        if (r < 32) atomicOr(&peq_lo[p * C + v], 1u << r);
        else atomicOr(&peq_hi[p * C + v], 1u << (r - 32));
      }
      m += __popcll(mask);
    }
    if (lane == 0) qm[p] = min(m, NEAR_MAX_QUERY);
  }
  __syncthreads();
  int mmax = 0;
  for (int p = 0; p < P; ++p) mmax = max(mmax, qm[p]);
  const bool wide = mmax > 32;                                // the same for the whole workgroup
  const long j0 = (long)blockIdx.x * NEAR_TILE;
  for (int w = 0; w < NEAR_WORDS_PER_THREAD; ++w) {
    const long j = j0 + w * NEAR_THREADS + tid;
    if (j >= N) break;
    const int* row = words + j * Lmax;
    int L = word_len[j];
    bool ok = L >= 0 && L <= Lmax;
    if (!ok) L = 0;
    for (int i = 0; i < L; i += 4) {
      const int4 q = near_load4(row, i, Lmax, vec);
      ok = ok && (unsigned)q.x <= (unsigned)(C - 2) && (i + 1 >= L || (unsigned)q.y <= (unsigned)(C - 2)) &&
           (i + 2 >= L || (unsigned)q.z <= (unsigned)(C - 2)) && (i + 3 >= L || (unsigned)q.w <= (unsigned)(C - 2));
    }
    int d = NEAR_UNTRUSTED;
    for (int p = 0; p < P; ++p) {
      const int m = qm[p];
      int dp = L;                                             // the empty query
      if (m > 0)
        dp = wide ? near_walk<unsigned long long>(peq_lo + p * C, peq_hi + p * C, m, row, L, Lmax, vec, C)
                  : near_walk<unsigned>(peq_lo + p * C, peq_hi + p * C, m, row, L, Lmax, vec, C);
      d = min(d, dp);
    }
    if (!ok) d = NEAR_UNTRUSTED;
    d8[(long)b * row_bytes + j] = (unsigned char)d;
    atomicAdd(&bins[d], 1);
  }
  __syncthreads();
  if (bins[tid]) atomicAdd(&hist[(long)b * 256 + tid], bins[tid]);
}

__global__ __launch_bounds__(NEAR_THREADS) void near_select_kernel(const unsigned char* __restrict__ d8, const int* __restrict__ hist,
                                                                   int* __restrict__ idx, int* __restrict__ dist, int N, long row_bytes, int K) {
  __shared__ int bins[256];
  __shared__ int s_dstar, s_below, s_need;
  __shared__ unsigned wt[2][NEAR_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bins[tid] = hist[(long)b * 256 + tid];
  __syncthreads();
  if (tid == 0) {
    int cum = 0, dstar = NEAR_UNTRUSTED;
    for (int d = 0; d < NEAR_UNTRUSTED; ++d) {
      if (cum + bins[d] >= K) { dstar = d; break; }
      cum += bins[d];
    }
    s_dstar = dstar; s_below = cum; s_need = dstar < NEAR_UNTRUSTED ? K - cum : 0;
  }
  __syncthreads();
  // dstar == 255: fewer than K trusted entries -- all of them are "below", none "equal"
  const int dstar = s_dstar, below = s_below, need = s_need;
  const unsigned* row = reinterpret_cast<const unsigned*>(d8 + (long)b * row_bytes);
  int* oi = idx + (long)b * K;
  int* od = dist + (long)b * K;
  int run_lt = 0, run_eq = 0;
  for (long base = 0, it = 0; base < N; base += 4 * NEAR_THREADS, ++it) {
    const long j = base + 4 * tid;
    unsigned w = 0xffffffffu;
    if (j < N) w = row[j >> 2];
    bool lt[4], eq[4];
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = (w >> (8 * k)) & 255;
      const bool in = j + k < N;
      lt[k] = in && d < dstar;
      eq[k] = in && d == dstar && dstar < NEAR_UNTRUSTED;
      v += (lt[k] ? 1u : 0u) + (eq[k] ? 0x10000u : 0u);
    }
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wt[it & 1][wave] = incl;
    __syncthreads();
    unsigned pre = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < NEAR_THREADS / 64; ++q) {
      const unsigned t = wt[it & 1][q];
      if (q < wave) pre += t;
      tot += t;
    }
    const unsigned excl = pre + incl - v;
    int lt_before = run_lt + (int)(excl & 0xffffu), eq_before = run_eq + (int)(excl >> 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int pos = -1;
      if (lt[k]) { pos = lt_before + min(eq_before, need); ++lt_before; }
      else if (eq[k]) { if (eq_before < need) pos = lt_before + eq_before; ++eq_before; }
      if (pos >= 0 && pos < K) { oi[pos] = (int)(j + k); od[pos] = (w >> (8 * k)) & 255; }
    }
    run_lt += (int)(tot & 0xffffu); run_eq += (int)(tot >> 16);
    if (run_lt == below && run_eq >= need) break;              // the row is full (the totals are the same in every thread)
  }
  const int filled = dstar < NEAR_UNTRUSTED ? K : below;
  for (int i = filled + tid; i < K; i += NEAR_THREADS) { oi[i] = -1; od[i] = -1; }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------------
extern "C" size_t crnn_lexicon_nearest_workspace_bytes(int B, int N) {
  if (B < 0 || N < 0) return 0;
  return near_hist_bytes(B) + (size_t)B * near_row_bytes(N);
}

extern "C" int crnn_lexicon_nearest(const int* queries, int P, int qcols, const int* words, const int* word_len, int* idx, int* dist, void* ws,
                                    size_t ws_bytes, int B, int C, int N, int Lmax, int K, hipStream_t stream) {
  if (!queries || !words || !word_len || !idx || !dist || !ws || B < 0 || N < 0) return CRNN_ERR_ARG;
  if (C < 2 || C > NEAR_MAX_C || Lmax < 1 || Lmax > NEAR_MAX_LABEL_LEN || P < 1 || P > NEAR_MAX_P || qcols < 1 || qcols > NEAR_MAX_QCOLS || K < 1 ||
      K > NEAR_MAX_K)
    return CRNN_ERR_UNSUPPORTED;
  if (B > 65535) return CRNN_ERR_UNSUPPORTED;                 // the sample is the grid's y
  if (ws_bytes < crnn_lexicon_nearest_workspace_bytes(B, N) || ((uintptr_t)ws & 3)) return CRNN_ERR_ARG;
  if (B == 0) return CRNN_OK;
  if (N == 0) {                                               // nothing to choose from: every slot is unused (-1 = all bits set)
    hipError_t e = hipMemsetAsync(idx, 0xff, (size_t)B * K * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(dist, 0xff, (size_t)B * K * sizeof(int), stream);
    return (int)e;
  }
  int* hist = (int*)ws;
  unsigned char* d8 = (unsigned char*)ws + near_hist_bytes(B);
  const long row_bytes = (long)near_row_bytes(N);
  hipError_t e = hipMemsetAsync(hist, 0, near_hist_bytes(B), stream);
  if (e != hipSuccess) return (int)e;
  const int vec = (Lmax & 3) == 0 && ((uintptr_t)words & 15) == 0;
  hipLaunchKernelGGL(near_dist_kernel, dim3(cdiv(N, NEAR_TILE), B), dim3(NEAR_THREADS), 0, stream, queries, P, qcols, words, word_len, d8, hist, C, N,
                     Lmax, row_bytes, vec);
  CRNN_LAUNCH_CHECK();
  hipLaunchKernelGGL(near_select_kernel, dim3(B), dim3(NEAR_THREADS), 0, stream, (const unsigned char*)d8, (const int*)hist, idx, dist, N, row_bytes, K);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
