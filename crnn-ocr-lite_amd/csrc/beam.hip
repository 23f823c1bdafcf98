// CTC beam-search decoding, plain or with a character language model (shallow fusion), one best path or the N best: one kernel, one 64-lane
// wavefront per sample; beam state lives in registers (lane i = beam entry i = TopN slot i), classes map to lanes for the expansion, the
// prefix-node table sits in LDS.
//
// Restates tf.nn.ctc_beam_search_decoder (TF r1.8 ctc_beam_search.h; reached by the reference through
// K.ctc_decode(greedy=False, beam_width, top_paths=1), utils.py:353) EXACTLY, including the order-dependent side
// effects of its sequential "grow new leaves" loop:
//   * entries are visited in descending previous-score order, their children in label order;
//   * a child is offered only if it is not currently in the beam; an accepted child evicts the current bottom;
//   * an entry that has been evicted earlier in the same step and is then re-offered by its parent fails the
//     candidate test and gets its old probabilities reset -- so it no longer expands when its own turn comes.
// A prefix trie is replaced by node identity = (parent node, label) in an LDS table, so a prefix that drops out
// and re-enters later is the same node again (its descendants regain their parent term).  The per-entry loop over
// the 37 children only iterates over "events" (labels that can enter the beam, or that name an existing entry),
// found with one wave ballot; every decision inside it is wave-uniform.
// Alphabets of 65..128 classes run the CPL = 2 instantiation (classes per lane): lane l holds the posteriors and the children of labels l and l + 64, gives
// one ballot per half, and the events of the lower half are consumed before those of the upper half -- label order, as above.  The blank (C - 1) then
// always sits in the upper half.  The beam itself stays one entry per lane.
//
// LM = true fills TF's BeamScorer hooks in with a dense n-gram table lm[rows][C] (column C - 1, the blank's slot, = the end-of-word weight):
//   * every prefix node carries ctx, its last order - 1 labels as a base-C number (symbol C - 1 = "before the word"), and
//     w = lm[parent.ctx][label], both fixed for the life of the node; the root's ctx is rows - 1;
//   * a re-scored entry adds its parent term as lse(newp.label, previous + w), a new child starts at inp[label] + (previous + w);
//   * after the last frame every leaf's total gets lm[ctx][C - 1] added and the top_paths best leaves are walked to the root.
// What the table costs: the expansion of entry i needs row lm[ctx_i] with lane = class.  Every beam slot therefore owns a row cache in
// LDS (beam_width * C floats); a row is fetched when its entry is CREATED -- the loads of all of a step's new entries are issued back to
// back, one global round trip per frame however many entries expand -- and an entry keeps its cache slot while it moves between lanes
// (ctx, w and the slot index travel through the end-of-step permutation with the rest of the entry).  The expansion then reads LDS only.
// A prefix that drops out and re-enters gets the same ctx and w again: both depend on (parent, label) alone.
// LM = false (no table) compiles every weight, the row cache and its LDS out: the plain decoder, crnn_ctc_beam_decode, is that instantiation
// with top_paths = 1, which ends in a wave-uniform branch of its own (entry 0 is the best path; lane 0 walks it).
//
// Since the plain decoder lost its own kernel, crnn_ctc_beam_decode checks its arguments as crnn_ctc_beam_decode_lm does: null y / out / out_len /
// scores or a negative B / T give CRNN_ERR_ARG, B = 0 gives CRNN_OK without a launch.  Every call that was valid before gives the same bits.
#include "common.h"
#include "ctc_core.h"      // CTC_EPS, NEG_INF, ctc_window

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

// Path of `node`: walk to the root, merge_repeated on the path's own sequence; labels are emitted leaf -> root straight into o, then flipped.  -> length
__device__ __forceinline__ int beam_emit_path(const int* nodes, int node, int* o, int merge_repeated) {
  int len = 0, prev = -1;
  while (node != 0) {
    int pk = nodes[node];
    int lab = (pk & 255) - 1;
    if (!merge_repeated || lab != prev) o[len++] = lab;
    prev = lab;
    node = (pk >> 8) - 1;
  }
  for (int i = 0; i < len / 2; ++i) { int a = o[i]; o[i] = o[len - 1 - i]; o[len - 1 - i] = a; }
  return len;
}

#define LM_FILL 4            // rows fetched per batch of loads when new entries are created

template <int CPL, bool LM>
__global__ __launch_bounds__(64) void ctc_beam_kernel(const float* __restrict__ y, const int* __restrict__ input_len,
                                                      const float* __restrict__ lm, int rows, int* __restrict__ out,
                                                      int* __restrict__ out_len, float* __restrict__ scores, int T, int C, int bw,
                                                      int top_paths, int merge_repeated, int nmax) {
  extern __shared__ int smem_i[];
  int* nodes = smem_i;                                   // [nmax] ((parent+1)<<8)|(label+1); node 0 = root
  int* s_ref = nodes + nmax;                             // [BEAM_MAX] sorted leaves: branch index or -1
  int* s_par = s_ref + BEAM_MAX;                         // parent branch index of a new child
  int* s_lab = s_par + BEAM_MAX;
  float* s_val = reinterpret_cast<float*>(s_lab + BEAM_MAX);
  int* s_used = reinterpret_cast<int*>(s_val + BEAM_MAX);   // [BEAM_MAX] row-cache slot taken by a surviving entry (LM only, as the cache: no LDS is charged for either without a table)
  float* cache = reinterpret_cast<float*>(s_used + BEAM_MAX);   // [bw][C] row lm[ctx] of the entry that owns the slot (LM only)
  const int b = blockIdx.x, lane = threadIdx.x, blank = C - 1;
  const int Tb = ctc_window(input_len, b, T);

  // beam entry `lane` (valid for lane < n)
  int b_node = 0, b_par = -1, b_lab = -1, b_act = 0;
  float b_ob = NEG_INF, b_ol = NEG_INF, b_ot = NEG_INF, b_nb = 0.f, b_nl = NEG_INF, b_nt = 0.f;
  int b_ctx = rows - 1, b_slot = 0; float b_w = 0.f;        // the root owns cache slot 0
  // TopN slot `lane` (valid for lane < nle)
  float l_v = NEG_INF; int l_ref = -1, l_par = -1, l_lab = -1;
  int n = 1, nnodes = 1;
  if (lane == 0) nodes[0] = 0;
  if constexpr (LM) {
    if (lane < C) cache[lane] = lm[(long)(rows - 1) * C + lane];
    if constexpr (CPL == 2) if (lane + 64 < C) cache[lane + 64] = lm[(long)(rows - 1) * C + lane + 64];
  }
  __syncthreads();
  // register copy of the node table, 64 nodes per register (node 64 k + lane in nd[k]): the search for a re-entering prefix compares against
  // registers instead of walking LDS -- up to ten searches per time step, each up to nnodes / 64 dependent LDS round trips before.  Tables
  // beyond kNodeRegs * 64 nodes (T * beam_width > 1023) keep the LDS walk.
  constexpr int kNodeRegs = 16;
  const bool regtab = nmax <= kNodeRegs * 64;
  int nd[kNodeRegs];
#pragma unroll
  for (int k = 0; k < kNodeRegs; ++k) nd[k] = -1;

  float ynext = (Tb > 0 && lane < C) ? y[(long)b * T * C + lane] : 0.f;        // the next step's posteriors are requested a step ahead
  float ynext1 = 0.f;                                                           // (class lane + 64, CPL == 2)
  if constexpr (CPL == 2) ynext1 = (Tb > 0 && lane + 64 < C) ? y[(long)b * T * C + lane + 64] : 0.f;
  for (int t = 0; t < Tb; ++t) {
    const float ycur = ynext;
    if (t + 1 < Tb && lane < C) ynext = y[((long)b * T + t + 1) * C + lane];
    float lg = (lane < C) ? logf(ycur + CTC_EPS) : NEG_INF;
    float inp, inp1 = NEG_INF, inp_blank;                   // lane = class (inp1: class lane + 64)
    if constexpr (CPL == 1) {
      inp = lg - wave_max64(lg);
      inp_blank = rl(inp, blank);
    } else {
      const float ycur1 = ynext1;
      if (t + 1 < Tb && lane + 64 < C) ynext1 = y[((long)b * T + t + 1) * C + lane + 64];
      const float lg1 = (lane + 64 < C) ? logf(ycur1 + CTC_EPS) : NEG_INF;
      const float mx = wave_max64(fmaxf(lg, lg1));
      inp = lg - mx; inp1 = lg1 - mx;
      inp_blank = rl(inp1, blank - 64);
    }
    // ---- oldp <- newp; re-score the entries (parent term only while the parent is in the beam)
    b_ob = b_nb; b_ol = b_nl; b_ot = b_nt;
    {
      float prev = NEG_INF; bool found = false;
      for (int j = 0; j < n; ++j) {
        int nj = rl(b_node, j), lj = rl(b_lab, j);
        float obj = rl(b_ob, j), otj = rl(b_ot, j);
        if (lane < n && b_node != 0 && nj == b_par) { found = true; prev = (b_lab == lj) ? obj : otj; }
      }
      if constexpr (LM) prev = prev + b_w;                 // -inf stays -inf: the table is finite
      float in_lab = __shfl(inp, b_lab & 63, 64);
      if constexpr (CPL == 2) {
        const float in_lab1 = __shfl(inp1, b_lab & 63, 64);
        if (b_lab >> 6) in_lab = in_lab1;                  // (the root's label -1 never reads in_lab)
      }
      if (lane < n) {
        float nl = NEG_INF;
        if (b_node != 0) {
          nl = found ? blse(b_ol, prev) : b_ol;
          nl = (nl == NEG_INF) ? NEG_INF : nl + in_lab;
        }
        b_nb = b_ot + inp_blank; b_nl = nl; b_nt = blse(b_nb, nl);
      }
    }
    // ---- TopN <- all entries
    int nle = n;
    l_v = b_nt; l_ref = lane; l_par = -1; l_lab = -1; b_act = (lane < n) ? 1 : 0;
    float bval; int bslot;
    wave_argmin(l_v, lane, nle, bval, bslot);
    // ---- grow new leaves, entry by entry
    for (int bi = 0; bi < n; ++bi) {
      const float bot = rl(b_ot, bi), bob = rl(b_ob, bi);
      const int blab = rl(b_lab, bi), bnode = rl(b_node, bi);
      if (!(bot > NEG_INF && (nle < bw || bot > bval))) continue;
      float prev = (lane == blab) ? bob : bot;
      float prev1 = (lane + 64 == blab) ? bob : bot;
      if constexpr (LM) {                                   // lane = child label: its weight is the entry's cached row at that label
        const int rbase = rl(b_slot, bi) * C;
        prev = prev + ((lane < blank) ? cache[rbase + lane] : 0.f);
        if constexpr (CPL == 2) prev1 = prev1 + ((lane + 64 < blank) ? cache[rbase + lane + 64] : 0.f);
      }
      const float v = (lane < blank && prev > NEG_INF) ? inp + prev : NEG_INF;
      float v1 = NEG_INF;                                                          // child label lane + 64 (CPL == 2)
      if constexpr (CPL == 2) v1 = (lane + 64 < blank && prev1 > NEG_INF) ? inp1 + prev1 : NEG_INF;
      int cb = -1, cb1 = -1;
      for (int j = 0; j < n; ++j) {
        int pj = rl(b_par, j), lj = rl(b_lab, j);
        if (pj == bnode && lj == lane) cb = j;                                  // this child is beam entry j
        if constexpr (CPL == 2) if (pj == bnode && lj == lane + 64) cb1 = j;
      }
      const bool ev = (lane < blank) && (cb >= 0 || (v > NEG_INF && (nle < bw || v > bval)));
      unsigned long long hmask[CPL];
      hmask[0] = __ballot(ev);
      if constexpr (CPL == 2) hmask[1] = __ballot((lane + 64 < blank) && (cb1 >= 0 || (v1 > NEG_INF && (nle < bw || v1 > bval))));
#pragma unroll
      for (int h = 0; h < CPL; ++h) {                                           // label order: the lower half's events, then the upper half's
        unsigned long long mask = hmask[h];
        const float vh = h ? v1 : v;
        const int cbh = h ? cb1 : cb;
        while (mask) {
          const int c = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          const float vc = rl(vh, c);
          const int ccb = rl(cbh, c);
          if (ccb >= 0 && rl(b_act, ccb)) continue;                       // child already in the beam
          if (vc > NEG_INF && (nle < bw || vc > bval)) {
            int slot;
            if (nle == bw) {                                                      // evict the bottom
              slot = bslot;
              int k = rl(l_ref, bslot);
              if (k >= 0 && lane == k) b_act = 0;
            } else {
              slot = nle++;
            }
            if (lane == slot) { l_v = vc; l_ref = -1; l_par = bi; l_lab = c + 64 * h; }
            wave_argmin(l_v, lane, nle, bval, bslot);
          } else if (ccb >= 0 && lane == ccb) {                                   // re-offered, rejected: reset oldp
            b_ob = b_ol = b_ot = NEG_INF;
          }
        }
      }
    }
    // ---- new beam = TopN sorted by descending score (ties: lower slot first)
    int rank = 0;
    for (int j = 0; j < nle; ++j) {
      float vj = rl(l_v, j);
      if (vj > l_v || (vj == l_v && j < lane)) ++rank;
    }
    __syncthreads();
    if (lane < nle) { s_ref[rank] = l_ref; s_par[rank] = l_par; s_lab[rank] = l_lab; s_val[rank] = l_v; }
    if constexpr (LM) s_used[lane] = 0;
    __syncthreads();
    int r_ref = -1, r_par = 0, r_lab = 0; float r_val = NEG_INF;
    if (lane < nle) { r_ref = s_ref[lane]; r_par = s_par[lane]; r_lab = s_lab[lane]; r_val = s_val[lane]; }
    // surviving entries: copy from their old lane; new children: parent node from the parent's lane
    const int src = (r_ref >= 0) ? r_ref : (r_par & 63);
    int g_node = __shfl(b_node, src, 64), g_par = __shfl(b_par, src, 64), g_lab = __shfl(b_lab, src, 64);
    float g_nb = __shfl(b_nb, src, 64), g_nl = __shfl(b_nl, src, 64), g_nt = __shfl(b_nt, src, 64);
    int new_node = g_node, new_par = g_par, new_lab = g_lab;
    float new_nb = g_nb, new_nl = g_nl, new_nt = g_nt;
    const bool is_new = (lane < nle) && (r_ref < 0);
    if (is_new) { new_par = g_node; new_lab = r_lab; new_nb = NEG_INF; new_nl = r_val; new_nt = r_val; new_node = -1; }
    int new_ctx = 0, new_slot = 0; float new_w = 0.f;
    if constexpr (LM) {
      new_ctx = __shfl(b_ctx, src, 64); new_slot = __shfl(b_slot, src, 64); new_w = __shfl(b_w, src, 64);
      if (is_new) {                                         // the parent's row is still cached: its slot is reassigned only below
        new_w = cache[new_slot * C + r_lab];
        new_ctx = (int)(((unsigned)new_ctx * (unsigned)C + (unsigned)r_lab) % (unsigned)rows);
        new_slot = -1;
      } else if (lane < nle) {
        s_used[new_slot] = 1;
      }
    }
    // resolve node ids of the new children one at a time (re-entering prefix -> reuse its node)
    unsigned long long nm = __ballot(is_new);
    while (nm) {
      const int r = __ffsll((long long)nm) - 1;
      nm &= nm - 1;
      const int packed = ((rl(new_par, r) + 1) << 8) | (rl(new_lab, r) + 1);
      int found = -1;
      if (regtab) {
#pragma unroll
        for (int k = 0; k < kNodeRegs; ++k) {
          if (found < 0 && k * 64 < nnodes) {                                   // (packed > 0 = nodes[0], and unused slots hold -1: no index test needed)
            const unsigned long long m = __ballot(nd[k] == packed);
            if (m) found = k * 64 + __ffsll((long long)m) - 1;
          }
        }
      } else {
        for (int base = 1; base < nnodes; base += 64) {
          int idx = base + lane;
          bool hit = (idx < nnodes) && (nodes[idx] == packed);
          unsigned long long m = __ballot(hit);
          if (m) { found = base + __ffsll((long long)m) - 1; break; }
        }
      }
      if (found < 0) {
        found = nnodes;
        if (nnodes < nmax) {
          if (lane == 0) nodes[nnodes] = packed;
          if (regtab) {
#pragma unroll
            for (int k = 0; k < kNodeRegs; ++k) if (k == (nnodes >> 6) && lane == (nnodes & 63)) nd[k] = packed;
          }
          ++nnodes;
        }
        __syncthreads();
      }
      if (lane == r) new_node = found;
    }
    if constexpr (LM) {
      // ---- the new entries take the cache slots no survivor holds (survivors + new = nle <= bw: there are enough) and fetch their rows,
      //      LM_FILL rows per batch of loads; absent entries of a batch read row 0 and store nothing, so the loads stay unconditional
      __syncthreads();
      unsigned long long freem = __ballot(lane < bw && s_used[lane] == 0);
      unsigned long long fm = __ballot(is_new);
      while (fm) {
        int sl[LM_FILL]; float rv[LM_FILL][CPL];
#pragma unroll
        for (int u = 0; u < LM_FILL; ++u) {
          const bool has = fm != 0;
          const int r = has ? __ffsll((long long)fm) - 1 : 0;
          const int s = has ? __ffsll((long long)freem) - 1 : -1;
          if (has) { fm &= fm - 1; freem &= freem - 1; }
          if (has && lane == r) new_slot = s;
          sl[u] = s;
          const long base = has ? (long)rl(new_ctx, r) * C : 0;
          rv[u][0] = (lane < C) ? lm[base + lane] : 0.f;
          if constexpr (CPL == 2) rv[u][1] = (lane + 64 < C) ? lm[base + lane + 64] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < LM_FILL; ++u) {
          if (sl[u] >= 0) {
            if (lane < C) cache[sl[u] * C + lane] = rv[u][0];
            if constexpr (CPL == 2) if (lane + 64 < C) cache[sl[u] * C + lane + 64] = rv[u][1];
          }
        }
      }
      __syncthreads();
      b_ctx = new_ctx; b_slot = new_slot; b_w = new_w;
    }
    b_node = new_node; b_par = new_par; b_lab = new_lab; b_nb = new_nb; b_nl = new_nl; b_nt = new_nt;
    n = nle;
  }
  if (!LM && top_paths == 1) {
    // ---- the plain decoder (wave-uniform branch): without end-of-word weights the best path is entry 0.  Lane 0 walks it from scalar registers;
    //      behind the per-lane ranking and walk below this launch measured 2.7 % slower
    for (int i = lane; i < T; i += 64) out[(long)b * T + i] = -1;
    const int best_node = rl(b_node, 0);
    const float best_score = rl(b_nt, 0);
    __syncthreads();
    if (lane == 0) {
      out_len[b] = beam_emit_path(nodes, best_node, out + (long)b * T, merge_repeated);
      scores[b] = best_score;
    }
    return;
  }
  // ---- final scores: total + end-of-word weight; the top_paths best by that sum (ties: the better rank before the addition = lower lane)
  float fin = b_nt;
  if constexpr (LM) if (lane < n) fin = b_nt + cache[b_slot * C + blank];
  int frank = 0;
  for (int j = 0; j < n; ++j) {
    const float fj = rl(fin, j);
    if (fj > fin || (fj == fin && j < lane)) ++frank;
  }
  int* outb = out + (long)b * top_paths * T;
  for (int i = lane; i < top_paths * T; i += 64) outb[i] = -1;
  if (lane >= n && lane < top_paths) { out_len[(long)b * top_paths + lane] = 0; scores[(long)b * top_paths + lane] = NEG_INF; }
  __syncthreads();
  if (lane < n && frank < top_paths) {
    const int len = beam_emit_path(nodes, b_node, outb + (long)frank * T, merge_repeated);
    scores[(long)b * top_paths + frank] = fin;
    out_len[(long)b * top_paths + frank] = len;
  }
}

extern "C" size_t crnn_ctc_lm_rows(int C, int order) {
  if (C < 2 || C > 128 || order < 1) return 0;
  size_t rows = 1;
  for (int i = 1; i < order; ++i) {
    rows *= (size_t)C;
    if (rows * (size_t)C * 4 > CRNN_LM_TABLE_MAX_BYTES) return 0;
  }
  return rows;
}

// Validates and launches one of the four instantiations; both entry points come here.
static int beam_launch(const float* y, const int* input_len, const float* lm, int order, int* out, int* out_len, float* scores, int B, int T,
                       int C, int beam_width, int top_paths, int merge_repeated, hipStream_t stream) {
  if (!y || !out || !out_len || !scores || B < 0 || T < 0) return CRNN_ERR_ARG;
  if (C > 128 || C < 2 || beam_width < 1 || beam_width > BEAM_MAX || top_paths < 1 || top_paths > beam_width || order < 1)
    return CRNN_ERR_UNSUPPORTED;
  const size_t rows = crnn_ctc_lm_rows(C, order);
  if (rows == 0) return CRNN_ERR_UNSUPPORTED;
  const int nmax = 1 + T * beam_width;
  const size_t lds = (size_t)nmax * 4 + BEAM_MAX * 16 + 64 + (lm ? BEAM_MAX * 4 + (size_t)beam_width * C * 4 : 0);   // s_used and the row cache: with a table only
  if (lds > 64 * 1024) return CRNN_ERR_UNSUPPORTED;
  if (B == 0) return CRNN_OK;
  auto kernel = lm ? (C <= 64 ? ctc_beam_kernel<1, true> : ctc_beam_kernel<2, true>)      // one class per lane, or two (lane l: classes l and l + 64)
                   : (C <= 64 ? ctc_beam_kernel<1, false> : ctc_beam_kernel<2, false>);
  hipLaunchKernelGGL(kernel, dim3(B), dim3(64), lds, stream, y, input_len, lm, (int)rows, out, out_len, scores, T, C, beam_width, top_paths,
                     merge_repeated, nmax);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}

extern "C" int crnn_ctc_beam_decode(const float* y, const int* input_len, int* out, int* out_len, float* scores, int B, int T,
                                    int C, int beam_width, int merge_repeated, hipStream_t stream) {
  return beam_launch(y, input_len, nullptr, 1, out, out_len, scores, B, T, C, beam_width, 1, merge_repeated, stream);   // out [B][1][T] = [B][T]
}

extern "C" int crnn_ctc_beam_decode_lm(const float* y, const int* input_len, const float* lm, int order, int* out, int* out_len,
                                       float* scores, int B, int T, int C, int beam_width, int top_paths, int merge_repeated,
                                       hipStream_t stream) {
  return beam_launch(y, input_len, lm, order, out, out_len, scores, B, T, C, beam_width, top_paths, merge_repeated, stream);
}
