// Edit scripts and character confusions of decoded label rows against the truth rows: which symbols the recogniser swaps, drops and invents, and
// where in the word.  The contract (the tie rule, the maps, the matrix) is at crnn_edit_ops in include/crnn_mi355x.h; the host definition is
// metrics.edit_ops.  One wavefront aligns one pair at a time; a workgroup of EDITOPS_WAVES wavefronts walks EDITOPS_PAIRS consecutive pairs.
//
// Forward: the recurrence of score.hip (Myers' bit vectors in Hyyro's formulation, the 64-bit ballot as the word: filtered truth b one symbol
// per lane, Eq = __ballot(lane < m && b[lane] == c), Pv / Mv / score wave-uniform on the scalar unit).  Before each kept prediction symbol j the
// lane (j mod 64) captures (Pv, Mv), the vertical deltas of column j; one 16-byte LDS store per lane and 64-column chunk keeps them, and one
// 4-byte store compacts the chunk's kept symbols next to them.  That is the whole matrix: D[i][j] = j + popc(Pv_j & low(i)) - popc(Mv_j & low(i)).
//
// Backtrace: from (m, n), diagonal > deletion > insertion, at most m + n wave-uniform steps.  The columns are taken 64 at a time from the top:
// lane l of a chunk holds column (base + l)'s deltas and symbol in registers, a step fetches them with v_readlane (no LDS latency inside the
// walk), and the lane a step lands on notes its partner -- truth_map in lane i - 1, the chunk's pred_map in lane j - 1 - base.  So the maps leave
// as whole rows from all lanes, and the four counts and the confusion cells are taken from the finished maps by every lane at once, not once per
// step.  Positions are filtered positions: the ds_permute that compacts the truth needs no inverse.
//
// Confusions: a private (C + 1)^2 matrix per workgroup in LDS (integer ds_add), flushed once with one global atomic per non-zero cell -- the
// form of detect.hip and deskew.hip.  Matches dominate, so the EDITOPS_PAIRS pairs of a workgroup mostly hit the same few diagonal cells.  Integer
// atomics only: the matrix is the same bits whatever the order.
//
// The recurrence and the row filter are spelled here as in score.hip and not shared through a header: moving them into forceinline helpers
// changed the register allocation and the schedule of edit_distance_kernel (profiles/editops_isa.txt), so score.hip stays as it is.
#include "common.h"

#define EDITOPS_WAVES 4                 // wavefronts per workgroup
#define EDITOPS_PAIRS_PER_WAVE 4        // pairs a wavefront aligns one after the other before the workgroup flushes its matrix
#define EDITOPS_PAIRS (EDITOPS_WAVES * EDITOPS_PAIRS_PER_WAVE)
#define EDITOPS_MAX_TRUTH_COLS 64       // one Myers word
#define EDITOPS_MAX_PRED_COLS 1024
#define EDITOPS_MAX_CLASSES 128

typedef unsigned long long eo_word;

// LDS, in dwords: the workgroup's matrix (only with conf), then per wavefront [pc4] (Pv, Mv) pairs and [pc4] symbols, pc4 = pred_cols rounded up to 4
__host__ __device__ static inline int editops_conf_dwords(int C, bool with_conf) { return with_conf ? ((C + 1) * (C + 1) + 3) & ~3 : 0; }
__host__ __device__ static inline int editops_wave_dwords(int pred_cols) { return 5 * ((pred_cols + 3) & ~3); }

// A wave's LDS region is its own: a wave-level fence orders its writes before its later reads (the LDS executes one wave's operations in order).
__device__ __forceinline__ void editops_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ eo_word editops_readlane64(eo_word v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, l), hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((eo_word)hi << 32) | lo;
}

__global__ __launch_bounds__(64 * EDITOPS_WAVES) void edit_ops_kernel(const int* __restrict__ pred, int pred_cols, const int* __restrict__ truth,
                                                                      int truth_cols, int skip0, int skip1, int C, int* __restrict__ ops,
                                                                      int* __restrict__ dist, int* __restrict__ pred_len, int* __restrict__ truth_len,
                                                                      int* __restrict__ truth_map, int* __restrict__ pred_map, int* __restrict__ conf,
                                                                      int n) {
  extern __shared__ __attribute__((aligned(16))) int eo_lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cells = conf ? (C + 1) * (C + 1) : 0;
  int* lconf = eo_lds;                                                            // [C + 1][C + 1], this workgroup's counts
  const int pc4 = (pred_cols + 3) & ~3;
  int* mine = eo_lds + editops_conf_dwords(C, conf != nullptr) + wave * editops_wave_dwords(pred_cols);
  ulonglong2* hist = reinterpret_cast<ulonglong2*>(mine);                         // [pc4] (Pv, Mv) of column j, j = 0 .. |a| - 1
  int* sym = mine + 4 * pc4;                                                      // [pc4] the filtered prediction a
  for (int k = threadIdx.x; k < cells; k += 64 * EDITOPS_WAVES) lconf[k] = 0;
  __syncthreads();

  for (int it = 0; it < EDITOPS_PAIRS_PER_WAVE; ++it) {
    const int row = blockIdx.x * EDITOPS_PAIRS + it * EDITOPS_WAVES + wave;
    if (row >= n) break;                                         // wave-uniform; every wave still reaches the barrier below

    // truth row -> b[0..m) in lanes 0..m-1; the dropped lanes' values go to the lanes above, so the push is a permutation
    int tv = skip0;
    if (lane < truth_cols) tv = truth[(long)row * truth_cols + lane];
    const bool tkeep = tv != skip0 && tv != skip1;
    const eo_word tmask = __ballot(tkeep);
    const int m = __popcll(tmask);
    const int rank = __popcll(tmask & ((1ull << lane) - 1));
    const int b = __builtin_amdgcn_ds_permute((tkeep ? rank : m + lane - rank) << 2, tv);
    const bool live = lane < m;
    bool bad = __ballot(tkeep && (unsigned)tv >= (unsigned)C) != 0;      // a kept label would index outside the matrix

    eo_word Pv = m == 64 ? ~0ull : (1ull << m) - 1, Mv = 0;
    const eo_word top = m ? 1ull << (m - 1) : 0;
    int score = m, alen = 0;
    for (int base = 0; base < pred_cols; base += 64) {
      const int col = base + lane;
      int pv = skip0;
      if (col < pred_cols) pv = pred[(long)row * pred_cols + col];
      const bool pkeep = pv != skip0 && pv != skip1;
      eo_word todo = __ballot(pkeep);                            // the kept symbols of this chunk, visited from the lowest lane up
      bad |= __ballot(pkeep && (unsigned)pv >= (unsigned)C) != 0;
      const int cnt = __popcll(todo);
      if (pkeep) sym[alen + __popcll(todo & ((1ull << lane) - 1))] = pv;     // a[alen ..): alen + cnt <= pred_cols
      eo_word hP = 0, hM = 0;
      int k = 0;
      while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int c = __builtin_amdgcn_readlane(pv, src);
        if (lane == k) { hP = Pv; hM = Mv; }                     // column alen + k, before this symbol
        ++k;
        const eo_word Eq = __ballot(live && b == c);
        const eo_word Xv = Eq | Mv;
        const eo_word Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        eo_word Ph = Mv | ~(Xh | Pv);
        eo_word Mh = Pv & Xh;
        score += (Ph & top) ? 1 : ((Mh & top) ? -1 : 0);
        Ph = (Ph << 1) | 1;
        Mh <<= 1;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
      }
      if (lane < cnt) hist[alen + lane] = make_ulonglong2(hP, hM);
      alen += cnt;
    }
    editops_wave_fence();
    const int na = alen;
    if (lane == 0) {
      dist[row] = m ? score : na;
      pred_len[row] = na;
      truth_len[row] = m;
    }

    if (bad) {                                                   // wave-uniform: nothing below may index by this pair's labels
      if (lane < 4) ops[(long)row * 4 + lane] = -1;
      if (truth_map && lane < truth_cols) truth_map[(long)row * truth_cols + lane] = -2;
      if (pred_map)
        for (int col = lane; col < pred_cols; col += 64) pred_map[(long)row * pred_cols + col] = -2;
      continue;
    }

    // backtrace from (i, j) = (m, na); (PvJ, MvJ) are column j's deltas, Dij = D[i][j]
    int i = m, j = na, Dij = m ? score : na;
    eo_word PvJ = Pv, MvJ = Mv;
    int tmapv = live ? -1 : -2;                                  // a truth symbol no diagonal step claims is a deletion
    for (int cbase = (pred_cols - 1) & ~63; cbase >= 0; cbase -= 64) {
      const int e = cbase + lane;
      const bool in = e < na;
      int pmv = in ? -1 : -2;                                    // a prediction symbol no diagonal step claims is an insertion
      int aS = 0;
      if (cbase < na) {
        ulonglong2 h = make_ulonglong2(0, 0);
        if (in) { h = hist[e]; aS = sym[e]; }
        while (j > cbase) {
          const int l = j - 1 - cbase;                           // the lane of column j - 1 and of symbol a[j - 1]
          const eo_word PvP = editops_readlane64(h.x, l), MvP = editops_readlane64(h.y, l);
          if (i > 0) {
            const eo_word low = (1ull << (i - 1)) - 1;           // rows 1 .. i - 1
            const int Ddiag = j - 1 + __popcll(PvP & low) - __popcll(MvP & low);
            const int cost = __builtin_amdgcn_readlane(b, i - 1) != __builtin_amdgcn_readlane(aS, l);
            if (Dij == Ddiag + cost) {                           // 1. diagonal: match or substitution
              if (lane == i - 1) tmapv = j - 1;
              if (lane == l) pmv = i - 1;
              Dij = Ddiag; --i; --j; PvJ = PvP; MvJ = MvP;
              continue;
            }
            const int Dup = j + __popcll(PvJ & low) - __popcll(MvJ & low);
            if (Dij == Dup + 1) {                                // 2. deletion of b[i - 1]
              Dij = Dup; --i;
              continue;
            }
          }
          --Dij; --j; PvJ = PvP; MvJ = MvP;                      // 3. insertion of a[j - 1]
        }
      }
      if (pred_map && e < pred_cols) pred_map[(long)row * pred_cols + e] = pmv;
      if (conf && pmv == -1) atomicAdd(&lconf[C * (C + 1) + aS], 1);
    }
    // j == 0: the i truth symbols left are deletions, which is what their lanes still say

    const bool paired = live && tmapv >= 0;
    const int pa = paired ? sym[tmapv] : C;                      // the prediction symbol of this lane's truth symbol, "nothing" for a deletion
    const int deletions = __popcll(__ballot(live && !paired));
    const int matches = __popcll(__ballot(paired && pa == b));
    const int subs = m - deletions - matches;
    if (lane < 4) ops[(long)row * 4 + lane] = lane == 0 ? matches : lane == 1 ? subs : lane == 2 ? deletions : na - matches - subs;
    if (truth_map && lane < truth_cols) truth_map[(long)row * truth_cols + lane] = tmapv;
    if (conf && live) atomicAdd(&lconf[b * (C + 1) + pa], 1);
    editops_wave_fence();                                        // the next pair overwrites hist and sym
  }

  __syncthreads();
  for (int k = threadIdx.x; k < cells; k += 64 * EDITOPS_WAVES) {
    const int v = lconf[k];
    if (v) atomicAdd(&conf[k], v);
  }
}

extern "C" int crnn_edit_ops(const int* pred, int pred_cols, const int* truth, int truth_cols, int skip0, int skip1, int num_classes, int* ops,
                             int* dist, int* pred_len, int* truth_len, int* truth_map, int* pred_map, int* conf, int n, hipStream_t stream) {
  if (!pred || !truth || !ops || !dist || !pred_len || !truth_len || n < 0 || pred_cols < 1 || truth_cols < 1 || num_classes < 1) return CRNN_ERR_ARG;
  if (truth_cols > EDITOPS_MAX_TRUTH_COLS || pred_cols > EDITOPS_MAX_PRED_COLS || num_classes > EDITOPS_MAX_CLASSES) return CRNN_ERR_UNSUPPORTED;
  if (n == 0) return CRNN_OK;
  const int lds = 4 * (editops_conf_dwords(num_classes, conf != nullptr) + EDITOPS_WAVES * editops_wave_dwords(pred_cols));
  if (lds > 65536)   // raised once per device, to the most any call can ask for (145 KiB of the CU's 160)
    CRNN_LDS_ATTR(edit_ops_kernel, 4 * (editops_conf_dwords(EDITOPS_MAX_CLASSES, true) + EDITOPS_WAVES * editops_wave_dwords(EDITOPS_MAX_PRED_COLS)));
  hipLaunchKernelGGL(edit_ops_kernel, dim3(cdiv(n, EDITOPS_PAIRS)), dim3(64 * EDITOPS_WAVES), lds, stream, pred, pred_cols, truth, truth_cols, skip0,
                     skip1, num_classes, ops, dist, pred_len, truth_len, truth_map, pred_map, conf, n);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
