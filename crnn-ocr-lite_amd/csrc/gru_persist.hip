// Persistent Bidirectional-GRU recurrence (Keras 2.2.2 GRUCell, reset_after=False, gate order z,r,h; utils.py:80-82 -- the cell
// the reference's train.py really builds, train.py:119): ONE launch per layer and pass instead of 2 T dependent launches (rnn.hip).
//
// The decomposition of rnn_persist.h, as in the persistent LSTM (rnn_persist.hip): the chain of one 16-row batch tile of one direction
// is run by a CLUSTER of workgroups; wave (ug, kq) = unit group ug, K quarter kq keeps its slices of the recurrent weights in registers
// for all T steps, and the hidden state / gradient carry of its (row, unit) pairs never leaves registers.
//
// The GRU needs TWO all-gathers per step where the LSTM needs one: the candidate's recurrent product takes r * h_prev of ALL units
//   forward   gather h_{t-1}            -> z, r of the own units -> publish r*h_prev  ->  gather r*h_prev -> hh, h_t -> publish h_t
//   backward  gather [dz|dr]_{t_next}   -> dh_t, dz_t, dhh_t     -> publish dhh_t     ->  gather dhh_t    -> dr_t, carry -> publish [dz|dr]_t
// Both go through ONE ring of kRing = 4 slots indexed by the linear exchange number e (forward: e = 2s for r*h, 2s+1 for h_s;
// backward: e = 2sb for dhh, 2sb+1 for [dz|dr]); a workgroup publishes e only after it gathered e-1, which is all the slot-reuse
// argument of rnn_exchange.h needs: after publishing e it re-poisons ITS slice of slot (e+2) % 4 (last used by e-2, which every
// member has finished reading) and drains its stores before publishing e+1.  Even and odd slots keep their tile shape.
// Sentinel: valid r*h, h (|.| < 1) and finite gradients never have an all-ones bf16 pair / fp32 pattern.
//
// Numerics: bit-identical to gru_*_kernel of rnn.hip in both modes (shared cell arithmetic rnn_cell.h, contraction off).
#include "common.h"
#include "rnn_cell.h"
#include "rnn_persist.h"

namespace {

struct GruFwdDir {
  const float* xw;   // [T][B][3u]  x*W + b
  const void* ut;    // U^T [3u][u], fp32 or bf16
  float* h; int ldh; // h(t,b,j) = h[(t*B+b)*ldh + j]
  float* gates;      // [T][B][3u] z, r, hh
  float* rh;         // [T][B][u]  r * h_prev
};
struct GruBwdDir {
  const void* uw;    // U [u][3u], fp32 or bf16
  const float* h; int ldh;
  const float* gates;
  const float* dout; int ldo;
  float* dz;         // [T][B][3u]
  float* dbp;        // may be null: [ceil(B / 16)][3u] bias-gradient partials, the column sums of dz over t of every 16-row batch tile
};

// static LDS of the kernels (the residency cap of a launch depends on it; each kernel asserts it against its arrays)
constexpr size_t gru_lds_fwd(int U, int ES) { return (size_t)16 * (U + 16 / ES) * ES + (size_t)kUW * 4 * 2 * 256 * 4 + (size_t)kUW * 16 * 16 * ES; }
constexpr size_t gru_lds_bwd(int U, int ES) { return (size_t)16 * (2 * U + 16 / ES) * ES + (size_t)kUW * 4 * 256 * 4 + (size_t)kUW * 16 * 32 * ES; }

// ---------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------
template <bool WBF, int U>
__global__ __launch_bounds__(kThreads) void gru_fwd_persist_kernel(GruFwdDir d0, GruFwdDir d1, int T, int B, int b_lo, int b_cnt, unsigned char* xbuf, int xmap) {
  typedef typename XE<WBF>::type E;
  constexpr int ES = sizeof(E), BT = 16, NSW = U / (16 * kUW);
  constexpr int LDA = U + 16 / ES;                       // +16 bytes per row
  constexpr int KQ = WBF ? U / 128 : U / 64;             // k-chunks per K quarter (one bf16 MFMA = 32 k; four fp32 MFMAs = 16 k)
  __shared__ __attribute__((aligned(16))) E As[BT * LDA];
  __shared__ __attribute__((aligned(16))) float red[kUW][4][2][256];
  __shared__ __attribute__((aligned(16))) E pub[kUW][BT * 16];
  static_assert(sizeof(As) + sizeof(red) + sizeof(pub) == gru_lds_fwd(U, ES), "gru_lds_fwd must state this kernel's static LDS");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int kq = wave & 3, ug = wave >> 2;
  const int bid = cluster_block_id(blockIdx.x, NSW, xmap);
  const int sl = bid % NSW, cl = bid / NSW, dir = cl & 1, bt = cl >> 1;
  const int nbt = (b_cnt + BT - 1) / BT;
  const GruFwdDir d = dir ? d1 : d0;
  const int sg = sl * kUW + ug;                           // this wave's unit group within the layer
  const int b0 = b_lo + bt * BT, b_end = b_lo + b_cnt, j0 = sg * 16;
  unsigned* status = reinterpret_cast<unsigned*>(xbuf);
  E* xdata = reinterpret_cast<E*>(xbuf + kStatusBytes);
  const long tile_elems = (long)BT * U;
  bool dead = false;
  const bool local = xmap && cluster_shares_xcd(xbuf, cl, sl, NSW, tid, status, dead);   // plain (L2-resident) exchange stores
  auto slot = [&](int e) { return slot_tile(xdata, dir, e, nbt, bt, tile_elems); };

  // this wave's K quarter of the z, r and candidate columns j0 .. j0+15 of U (rows of U^T), resident for all T steps
  u32x4 bz[KQ], br[KQ], bh[KQ];
  load_frags<WBF, KQ>(d.ut, ((long)0 * U + j0 + r) * U, kq * (U / 4), q, bz);
  load_frags<WBF, KQ>(d.ut, ((long)1 * U + j0 + r) * U, kq * (U / 4), q, br);
  load_frags<WBF, KQ>(d.ut, ((long)2 * U + j0 + r) * U, kq * (U / 4), q, bh);

  const int tl = tid & 255, row = tl >> 4, col = tl & 15, j = j0 + col;
  const int b = b0 + row;
  const bool live = b < b_end;
  const int pch = row_chunk<16, E>(kq, lane);
  float hprev = 0.f;
  auto gather_to_As = [&](int e) { gather_rows<U>(slot(e), As, LDA, tid, status, dead); };

#pragma unroll 1
  for (int s = 0; s < T; ++s) {
    const int t = dir ? T - 1 - s : s;
    const float* xw = d.xw + ((long)t * B + (live ? b : b_lo)) * 3 * U;
    const float xz = xw[j], xr = xw[U + j], xh = xw[2 * U + j];     // requested before the wait
    float sz = 0.f, sr = 0.f, sh = 0.f;
    if (s > 0) {
      gather_to_As(2 * s - 1);                                       // h_{s-1} of the whole cluster
      __syncthreads();
      const f32x4 az = quarter_chain<WBF, KQ>(As, LDA, kq * (U / 4), bz, r, q);
      const f32x4 ar = quarter_chain<WBF, KQ>(As, LDA, kq * (U / 4), br, r, q);
      put_frag(red[ug][kq][0], az, r, q);
      put_frag(red[ug][kq][1], ar, r, q);
      __syncthreads();
      sz = sum_quarters(&red[ug][0][0][tl], 2 * 256);
      sr = sum_quarters(&red[ug][0][1][tl], 2 * 256);
    }
    GruZR o = gru_cell_zr(sz + xz, sr + xr, hprev);
    if (!live) o.rh = 0.f;
    if (s > 0) {
      // publish r * h_prev of this unit group (exchange 2s): the candidate product of every member waits for it
      pub[ug][row * 16 + col] = to_e<WBF>(o.rh);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the re-poisoning after the previous exchange has landed
      publish_rows<16>(pub[ug], slot(2 * s) + (long)sg * BT * 16, pch, local);
    }
    if (live) {                                                      // what the backward pass reads: off the critical path
      float* gt = d.gates + ((long)t * B + b) * 3 * U;
      gt[j] = o.zg; gt[U + j] = o.rg;
      d.rh[((long)t * B + b) * U + j] = o.rh;
    }
    if (s > 0) {
      poison_rows<16>(slot(2 * s + 2) + (long)sg * BT * 16, pch, local);
      gather_to_As(2 * s);                                           // r * h_prev of the whole cluster
      __syncthreads();
      const f32x4 ah = quarter_chain<WBF, KQ>(As, LDA, kq * (U / 4), bh, r, q);
      put_frag(red[ug][kq][0], ah, r, q);
      __syncthreads();
      sh = sum_quarters(&red[ug][0][0][tl], 2 * 256);
    }
    GruH g = gru_cell_h(sh + xh, o.zg, hprev);
    if (!live) g.hn = 0.f;
    hprev = g.hn;
    if (s + 1 < T) {
      pub[ug][row * 16 + col] = to_e<WBF>(g.hn);                     // exchange 2s+1
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      publish_rows<16>(pub[ug], slot(2 * s + 1) + (long)sg * BT * 16, pch, local);
    }
    if (live) {
      d.gates[((long)t * B + b) * 3 * U + 2 * U + j] = g.hh;
      d.h[((long)t * B + b) * d.ldh + j] = g.hn;
    }
    if (s + 1 < T) poison_rows<16>(slot(2 * s + 3) + (long)sg * BT * 16, pch, local);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward (BPTT): dh_t = dout_t + [dz|dr]_{t_next} U[:, 0:2u]^T + carry ;  d(r h)_t = dhh_t U[:, 2u:3u]^T
// ---------------------------------------------------------------------------------------------------------------
template <bool WBF, int U>
__global__ __launch_bounds__(kThreads) void gru_bwd_persist_kernel(GruBwdDir d0, GruBwdDir d1, int T, int B, int b_lo, int b_cnt, unsigned char* xbuf, int xmap) {
  typedef typename XE<WBF>::type E;
  constexpr int ES = sizeof(E), BT = 16, NSW = U / (16 * kUW), K2 = 2 * U, G = 3 * U;
  constexpr int LDA = K2 + 16 / ES;
  constexpr int KQB = WBF ? U / 64 : U / 32;             // k-chunks per quarter of K = 2u
  constexpr int KQA = WBF ? U / 128 : U / 64;            // k-chunks per quarter of K = u
  __shared__ __attribute__((aligned(16))) E As[BT * LDA];
  __shared__ __attribute__((aligned(16))) float red[kUW][4][256];
  __shared__ __attribute__((aligned(16))) E pub[kUW][BT * 32];
  static_assert(sizeof(As) + sizeof(red) + sizeof(pub) == gru_lds_bwd(U, ES), "gru_lds_bwd must state this kernel's static LDS");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int kq = wave & 3, ug = wave >> 2;
  const int bid = cluster_block_id(blockIdx.x, NSW, xmap);
  const int sl = bid % NSW, cl = bid / NSW, dir = cl & 1, bt = cl >> 1;
  const int nbt = (b_cnt + BT - 1) / BT;
  const GruBwdDir d = dir ? d1 : d0;
  const int sg = sl * kUW + ug;
  const int b0 = b_lo + bt * BT, b_end = b_lo + b_cnt, j0 = sg * 16;
  unsigned* status = reinterpret_cast<unsigned*>(xbuf);
  E* xdata = reinterpret_cast<E*>(xbuf + kStatusBytes);
  const long tile_elems = (long)BT * K2;                 // slot stride (the dhh tiles use half of it)
  bool dead = false;
  const bool local = xmap && cluster_shares_xcd(xbuf, cl, sl, NSW, tid, status, dead);   // plain (L2-resident) exchange stores
  auto slot = [&](int e) { return slot_tile(xdata, dir, e, nbt, bt, tile_elems); };

  // U[j0 + r][.]: this wave's quarter of the z|r columns (K = 2u) and of the candidate columns (K = u)
  u32x4 bb[KQB], ba[KQA];
  load_frags<WBF, KQB>(d.uw, (long)(j0 + r) * G, kq * (U / 2), q, bb);
  load_frags<WBF, KQA>(d.uw, (long)(j0 + r) * G + 2 * U, kq * (U / 4), q, ba);

  const int tl = tid & 255, row = tl >> 4, col = tl & 15, j = j0 + col;
  const int b = b0 + row;
  const bool live = b < b_end;
  const long bbx = live ? b : b_lo;
  const int pch = row_chunk<16, E>(kq, lane), pch2 = row_chunk<32, E>(kq, lane);   // of a dhh row, of a [dz|dr] row
  float dhp = 0.f, bsz = 0.f, bsr = 0.f, bsh = 0.f;       // bs*: this thread's (row, unit) share of the bias gradient (z | r | candidate), summed over the steps

#pragma unroll 1
  for (int sb = 0; sb < T; ++sb) {
    const int sp = T - 1 - sb;                       // processing index of this time in the forward pass
    const int t = dir ? T - 1 - sp : sp;
    const int tprev = dir ? t + 1 : t - 1;
    const float* gt = d.gates + ((long)t * B + bbx) * G;              // epilogue operands, requested before the wait
    const float zg = gt[j], rg = gt[U + j], hh = gt[2 * U + j];
    const float hprev = (sp > 0) ? d.h[((long)tprev * B + bbx) * d.ldh + j] : 0.f;
    float dh = d.dout[((long)t * B + bbx) * d.ldo + j];
    if (sb > 0) {
      gather_gated<2, U>(slot(2 * sb - 1), As, LDA, tid, status, dead);   // [dz|dr] of the step before, whole cluster
      __syncthreads();
      put_frag(red[ug][kq], quarter_chain<WBF, KQB>(As, LDA, kq * (U / 2), bb, r, q), r, q);
      __syncthreads();
      dh += sum_quarters(&red[ug][0][tl], 256) + dhp;
    }
    GruBwdB ob = gru_cell_bwd_b(dh, zg, hh, hprev);
    if (!live) { ob.dzz = 0.f; ob.dhh = 0.f; }
    bsz += ob.dzz; bsh += ob.dhh;
    // publish dhh_t of this unit group (exchange 2sb)
    pub[ug][row * 16 + col] = to_e<WBF>(ob.dhh);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    publish_rows<16>(pub[ug], slot(2 * sb) + (long)sg * BT * 16, pch, local);
    if (live) {
      float* dz = d.dz + ((long)t * B + b) * G;
      dz[j] = ob.dzz; dz[2 * U + j] = ob.dhh;
    }
    poison_rows<16>(slot(2 * sb + 2) + (long)sg * BT * 16, pch, local);
    gather_rows<U>(slot(2 * sb), As, LDA, tid, status, dead);           // dhh_t of the whole cluster
    __syncthreads();
    put_frag(red[ug][kq], quarter_chain<WBF, KQA>(As, LDA, kq * (U / 4), ba, r, q), r, q);
    __syncthreads();
    const float drh = sum_quarters(&red[ug][0][tl], 256);
    GruBwdA oa = gru_cell_bwd_a(drh, dh, zg, rg, hprev);
    if (!live) { oa.dzr = 0.f; oa.dhp = 0.f; }
    bsr += oa.dzr;
    dhp = oa.dhp;
    if (sb + 1 < T) {
      pub[ug][(row * 2 + 0) * 16 + col] = to_e<WBF>(ob.dzz);         // exchange 2sb+1: [dz | dr]_t
      pub[ug][(row * 2 + 1) * 16 + col] = to_e<WBF>(oa.dzr);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      publish_rows<32>(pub[ug], slot(2 * sb + 1) + (long)sg * BT * 32, pch2, local);
    }
    if (live) d.dz[((long)t * B + b) * G + U + j] = oa.dzr;
    if (sb + 1 < T) poison_rows<32>(slot(2 * sb + 3) + (long)sg * BT * 32, pch2, local);
  }
  if (d.dbp) bias_partials<3, U>({bsz, bsr, bsh}, red[ug], d.dbp, kq, lane, b0, b_end, j0);
}

constexpr void (*kGruFwd[])(GruFwdDir, GruFwdDir, int, int, int, int, unsigned char*, int) = PERSIST_KERNELS(gru_fwd_persist_kernel);
constexpr void (*kGruBwd[])(GruBwdDir, GruBwdDir, int, int, int, int, unsigned char*, int) = PERSIST_KERNELS(gru_bwd_persist_kernel);

}  // namespace

// 0 when (u, dt_u) has a persistent GRU kernel (fp32: u in {64,128,256}; bf16: u in {128,256,512}), else -3 (use crnn_gru_*_ex)
extern "C" int crnn_gru_persist_supported(int u, int dt_u) { return width_index(u, dt_u) >= 0 ? CRNN_OK : CRNN_ERR_UNSUPPORTED; }

// Forward recurrence of one Bidirectional(GRU) layer in ONE launch.  Arguments as crnn_gru_fwd_ex; xbuf as for crnn_lstm_fwd_persist
// (crnn_lstm_persist_xbuf_bytes(T, B, u, dt_u) bytes, same status words).  flags: 0 or CRNN_RNN_XCD_LOCAL.
extern "C" int crnn_gru_fwd_persist(const float* xw0, const float* xw1, const void* ut0, const void* ut1, float* h0, float* h1, int ldh,
                                    float* g0, float* g1, float* rh0, float* rh1, int T, int B, int u, int dt_u, void* xbuf,
                                    size_t xbuf_bytes, int flags, hipStream_t stream) {
  CRNN_TRY(crnn_gru_persist_supported(u, dt_u));
  if (T < 1 || B < 1 || (((uintptr_t)ut0 | (uintptr_t)ut1) & 15)) return CRNN_ERR_ARG;
  GruFwdDir a{xw0, ut0, h0, ldh, g0, rh0}, b{xw1, ut1, h1, ldh, g1, rh1};
  return launch_persist(kGruFwd, gru_lds_fwd, u, a, b, T, B, u, dt_u, xbuf, xbuf_bytes, (flags & CRNN_RNN_XCD_LOCAL) ? 1 : 0, stream);
}

// BPTT of one Bidirectional(GRU) layer in ONE launch: fills dz[d] [T][B][3u] from dout[d].  Arguments as crnn_gru_bwd_ex without
// the dh / dhp scratch (both stay in registers).
// crnn_gru_bwd_persist_db: the same launch also leaves the bias-gradient partials db_partials0 / 1 [crnn_rnn_db_rows(B)][3u] (column sums of dz over time per 16-row tile)
extern "C" int crnn_gru_bwd_persist_db(const void* u0, const void* u1, const float* h0, const float* h1, int ldh, const float* g0, const float* g1,
                                       const float* dout0, const float* dout1, int ldo, float* dz0, float* dz1, float* db_partials0, float* db_partials1,
                                       int T, int B, int u, int dt_u, void* xbuf, size_t xbuf_bytes, int flags, hipStream_t stream);
extern "C" int crnn_gru_bwd_persist(const void* u0, const void* u1, const float* h0, const float* h1, int ldh, const float* g0, const float* g1,
                                    const float* dout0, const float* dout1, int ldo, float* dz0, float* dz1, int T, int B, int u, int dt_u,
                                    void* xbuf, size_t xbuf_bytes, int flags, hipStream_t stream) {
  return crnn_gru_bwd_persist_db(u0, u1, h0, h1, ldh, g0, g1, dout0, dout1, ldo, dz0, dz1, nullptr, nullptr, T, B, u, dt_u, xbuf, xbuf_bytes, flags, stream);
}
extern "C" int crnn_gru_bwd_persist_db(const void* u0, const void* u1, const float* h0, const float* h1, int ldh, const float* g0, const float* g1,
                                       const float* dout0, const float* dout1, int ldo, float* dz0, float* dz1, float* db_partials0, float* db_partials1,
                                       int T, int B, int u, int dt_u, void* xbuf, size_t xbuf_bytes, int flags, hipStream_t stream) {
  CRNN_TRY(crnn_gru_persist_supported(u, dt_u));
  if (T < 1 || B < 1 || (((uintptr_t)u0 | (uintptr_t)u1) & 15) || (!db_partials0) != (!db_partials1)) return CRNN_ERR_ARG;
  GruBwdDir a{u0, h0, ldh, g0, dout0, ldo, dz0, db_partials0}, b{u1, h1, ldh, g1, dout1, ldo, dz1, db_partials1};
  return launch_persist(kGruBwd, gru_lds_bwd, 2 * u, a, b, T, B, u, dt_u, xbuf, xbuf_bytes, (flags & CRNN_RNN_XCD_LOCAL) ? 1 : 0, stream);
}
