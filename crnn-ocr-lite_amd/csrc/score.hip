// Batched edit distance of decoded label rows against the truth rows: what predict.py --validate reports, computed where the decode kernels
// leave their output.  One wavefront scores one pair; one launch per batch; no workspace, no LDS allocation.
//
// Myers' bit-vector algorithm (J. ACM 46(3), 1999) in Hyyro's formulation, with the wavefront as the machine word: the filtered truth row b
// (|b| = m <= 64) sits one symbol per lane, and for a prediction symbol c the match vector Eq is __ballot(lane < m && b[lane] == c) -- one
// v_cmp.  The vertical delta vectors Pv / Mv, Eq and the score are wave-uniform 64-bit values: the recurrence runs on the scalar unit, one
// step per kept prediction symbol, about 15 word operations each.  Both rows are filtered (every skip0 / skip1 removed, wherever it stands)
// with a ballot and a prefix popcount: the truth is compacted into the low lanes by one ds_permute (a push across lanes, no LDS memory); the
// prediction is not moved at all -- the kept lanes of each 64-column chunk are visited in order through the ballot mask and read with
// v_readlane.  Labels are only compared; nothing is indexed by a label value.
#include "common.h"

#define SCORE_WAVES 4              // pairs per workgroup
#define SCORE_MAX_TRUTH_COLS 64    // one Myers word
#define SCORE_MAX_PRED_COLS 1024

typedef unsigned long long score_word;

__global__ __launch_bounds__(64 * SCORE_WAVES) void edit_distance_kernel(const int* __restrict__ pred, int pred_cols, const int* __restrict__ truth,
                                                                         int truth_cols, int skip0, int skip1, int* __restrict__ dist,
                                                                         int* __restrict__ pred_len, int* __restrict__ truth_len, int n) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * SCORE_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= n) return;                                        // whole wavefronts leave: everything below is wave-uniform control flow

  // truth row -> b[0..m) in lanes 0..m-1; the dropped lanes' values go to the lanes above, so the push is a permutation
  int tv = skip0;
  if (lane < truth_cols) tv = truth[(long)row * truth_cols + lane];
  const bool tkeep = tv != skip0 && tv != skip1;
  const score_word tmask = __ballot(tkeep);
  const int m = __popcll(tmask);
  const int rank = __popcll(tmask & ((1ull << lane) - 1));
  const int b = __builtin_amdgcn_ds_permute((tkeep ? rank : m + lane - rank) << 2, tv);
  const bool live = lane < m;

  score_word Pv = m == 64 ? ~0ull : (1ull << m) - 1, Mv = 0;
  const score_word top = m ? 1ull << (m - 1) : 0;
  int score = m, alen = 0;
  for (int base = 0; base < pred_cols; base += 64) {
    const int col = base + lane;
    int pv = skip0;
    if (col < pred_cols) pv = pred[(long)row * pred_cols + col];
    score_word todo = __ballot(pv != skip0 && pv != skip1);    // the kept symbols of this chunk, visited from the lowest lane up
    alen += __popcll(todo);
    if (m == 0) continue;
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int c = __builtin_amdgcn_readlane(pv, src);
      const score_word Eq = __ballot(live && b == c);
      const score_word Xv = Eq | Mv;
      const score_word Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
      score_word Ph = Mv | ~(Xh | Pv);
      score_word Mh = Pv & Xh;
      score += (Ph & top) ? 1 : ((Mh & top) ? -1 : 0);
      Ph = (Ph << 1) | 1;
      Mh <<= 1;
      Pv = Mh | ~(Xv | Ph);
      Mv = Ph & Xv;
    }
  }
  if (lane == 0) {
    dist[row] = m ? score : alen;
    pred_len[row] = alen;
    truth_len[row] = m;
  }
}

extern "C" int crnn_edit_distance(const int* pred, int pred_cols, const int* truth, int truth_cols, int skip0, int skip1, int* dist, int* pred_len,
                                  int* truth_len, int n, hipStream_t stream) {
  if (!pred || !truth || !dist || !pred_len || !truth_len || n < 0 || pred_cols < 1 || truth_cols < 1) return CRNN_ERR_ARG;
  if (truth_cols > SCORE_MAX_TRUTH_COLS || pred_cols > SCORE_MAX_PRED_COLS) return CRNN_ERR_UNSUPPORTED;
  if (n == 0) return CRNN_OK;
  hipLaunchKernelGGL(edit_distance_kernel, dim3(cdiv(n, SCORE_WAVES)), dim3(64 * SCORE_WAVES), 0, stream, pred, pred_cols, truth, truth_cols, skip0,
                     skip1, dist, pred_len, truth_len, n);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
