// Persistent Bidirectional-LSTM recurrence (Keras 2.2.2 LSTMCell, utils.py:77-82): ONE launch per layer instead of
// one launch per timestep (rnn.hip), forward and BPTT.
//
// The design -- a cluster of workgroups per 16-row batch tile, weights and carries in registers, one all-gather per step -- is
// rnn_persist.h's; the hand-off protocol is rnn_exchange.h's.  The LSTM's part: workgroup member `sl` owns the 4x16 gate columns
// {g*u + j0 + 0..15} of its unit groups (u = 256: a 256 x 64 slice of U per group, 32 VGPRs bf16 / 64 VGPRs fp32 per wave); the
// cell state c (forward) / the cell-gradient carry dc (backward) never leaves registers; exchange s carries h_t (forward: 16 x u)
// or the gate gradients dz_t (backward: 16 x 4u) of step s.
//
// Numerics: bit-identical to the per-step kernels of rnn.hip in both modes (shared cell arithmetic rnn_cell.h).
#include "common.h"
#include "rnn_cell.h"
#include "rnn_persist.h"

namespace {

struct FwdDir {
  const float* xw;   // [T][B][4u]  x*W + b
  const void* ut;    // U^T [4u][u], fp32 or bf16
  float* h; int ldh; // h(t,b,j) = h[(t*B+b)*ldh + j]
  float* c;          // [T][B][u]
  float* gates;      // [T][B][4u] activated i,f,g,o
};
struct BwdDir {
  const void* uw;    // U [u][4u], fp32 or bf16
  const float* c;    // [T][B][u]
  const float* gates;
  const float* dout; int ldo;
  float* dz;         // [T][B][4u]
  float* dbp;        // may be null: [ceil(B / 16)][4u] bias-gradient partials, the column sums of dz over t of every 16-row batch tile
};

// static LDS of the kernels (the residency cap of a launch depends on it; each kernel asserts it against its arrays)
constexpr size_t lstm_lds_fwd(int U, int ES) { return (size_t)16 * (U + 16 / ES) * ES + (size_t)kUW * 4 * 256 * 4 + (size_t)kUW * 16 * 16 * ES; }
constexpr size_t lstm_lds_bwd(int U, int ES) { return (size_t)16 * (4 * U + 16 / ES) * ES + (size_t)kUW * 4 * 256 * 4 + (size_t)kUW * 16 * 64 * ES; }

// ---------------------------------------------------------------------------------------------------------------
// forward: wave (ug, gate) owns gate `gate` of unit group ug over the whole K, as four quarter accumulators
// ---------------------------------------------------------------------------------------------------------------
template <bool WBF, int U>
__global__ __launch_bounds__(kThreads) void lstm_fwd_persist_kernel(FwdDir d0, FwdDir d1, int T, int B, int b_lo, int b_cnt, unsigned char* xbuf, int xmap) {
  typedef typename XE<WBF>::type E;
  constexpr int ES = sizeof(E), BT = 16, NSW = U / (16 * kUW);
  constexpr int LDA = U + 16 / ES;                       // +16 bytes per row
  constexpr int KQ = WBF ? U / 128 : U / 64;             // k-chunks per K quarter (one bf16 MFMA = 32 k; four fp32 MFMAs = 16 k)
  __shared__ __attribute__((aligned(16))) E As[BT * LDA];
  __shared__ __attribute__((aligned(16))) float red[kUW][4][256];
  __shared__ __attribute__((aligned(16))) E hout[kUW][BT * 16];
  static_assert(sizeof(As) + sizeof(red) + sizeof(hout) == lstm_lds_fwd(U, ES), "lstm_lds_fwd must state this kernel's static LDS");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int gate = wave & 3, ug = wave >> 2;
  const int bid = cluster_block_id(blockIdx.x, NSW, xmap);
  const int sl = bid % NSW, cl = bid / NSW, dir = cl & 1, bt = cl >> 1;
  const int nbt = (b_cnt + BT - 1) / BT;
  const FwdDir d = dir ? d1 : d0;
  const int sg = sl * kUW + ug;                          // this wave's unit group within the layer
  const int b0 = b_lo + bt * BT, b_end = b_lo + b_cnt, j0 = sg * 16;
  unsigned* status = reinterpret_cast<unsigned*>(xbuf);
  E* xdata = reinterpret_cast<E*>(xbuf + kStatusBytes);
  const long tile_elems = (long)BT * U;
  bool dead = false;
  const bool local = xmap && cluster_shares_xcd(xbuf, cl, sl, NSW, tid, status, dead);   // plain (L2-resident) exchange stores
  auto slot = [&](int e) { return slot_tile(xdata, dir, e, nbt, bt, tile_elems); };

  // this wave's gate columns j0 .. j0+15 of U (rows of U^T) as B fragments, resident for all T steps
  u32x4 breg[4][KQ];
#pragma unroll
  for (int a = 0; a < 4; ++a) load_frags<WBF, KQ>(d.ut, ((long)gate * U + j0 + r) * U, a * (U / 4), q, breg[a]);

  const int tl = tid & 255, row = tl >> 4, col = tl & 15, j = j0 + col;
  const int b = b0 + row;
  const int pch = row_chunk<16, E>(gate, lane);
  float cprev = 0.f;

#pragma unroll 1
  for (int s = 0; s < T; ++s) {
    const int t = dir ? T - 1 - s : s;
    float xwv[4];                                        // x W + b, requested before the wait
    {
      const float* xw = d.xw + ((long)t * B + (b < b_end ? b : b_lo)) * 4 * U;
#pragma unroll
      for (int g = 0; g < 4; ++g) xwv[g] = xw[g * U + j];
    }
    if (s > 0) {
      gather_rows<U>(slot(s - 1), As, LDA, tid, status, dead);   // h_{s-1} of the whole cluster
      __syncthreads();
      f32x4 acc[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) acc[a] = quarter_chain<WBF, KQ>(As, LDA, a * (U / 4), breg[a], r, q);
      put_frag(red[ug][gate], (acc[0] + acc[1]) + (acc[2] + acc[3]), r, q);
      __syncthreads();
    }
    float z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) z[g] = (s > 0 ? red[ug][g][tl] : 0.f) + xwv[g];
    LstmFwdOut o = lstm_cell_fwd(z, cprev);
    if (b >= b_end) o.hn = 0.f;
    cprev = o.cn;
    hout[ug][row * 16 + col] = to_e<WBF>(o.hn);
    if (s + 1 < T) {
      // publish this unit group's h_t slice first (the other workgroups of the cluster wait for it)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the re-poisoning of step s-1 has landed before step s goes out
      publish_rows<16>(hout[ug], slot(s) + (long)sg * BT * 16, pch, local);
    }
    if (b < b_end) {   // what the next layer / the backward pass read: off the critical path
      float* gt = d.gates + ((long)t * B + b) * 4 * U;
      gt[j] = o.ig; gt[U + j] = o.fg; gt[2 * U + j] = o.gg; gt[3 * U + j] = o.og;
      d.c[((long)t * B + b) * U + j] = o.cn;
      d.h[((long)t * B + b) * d.ldh + j] = o.hn;
    }
    if (s + 1 < T) poison_rows<16>(slot(s + 2) + (long)sg * BT * 16, pch, local);   // last: nobody waits for it
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward (BPTT): dh_{t}[b, j'] = sum_k dz_{t_next}[b, k] U[j', k] + dout_t[b, j'], then the gate gradients dz_t;
// wave (ug, kq) owns K quarter kq (= gate kq of dz) of unit group ug
// ---------------------------------------------------------------------------------------------------------------
template <bool WBF, int U>
__global__ __launch_bounds__(kThreads) void lstm_bwd_persist_kernel(BwdDir d0, BwdDir d1, int T, int B, int b_lo, int b_cnt, unsigned char* xbuf, int xmap) {
  typedef typename XE<WBF>::type E;
  constexpr int ES = sizeof(E), BT = 16, NSW = U / (16 * kUW), K = 4 * U;
  constexpr int LDA = K + 16 / ES;
  constexpr int KQ = WBF ? U / 32 : U / 16;              // k-chunks per quarter of K = 4u
  __shared__ __attribute__((aligned(16))) E As[BT * LDA];
  __shared__ __attribute__((aligned(16))) float red[kUW][4][256];
  __shared__ __attribute__((aligned(16))) E zout[kUW][BT * 64];
  static_assert(sizeof(As) + sizeof(red) + sizeof(zout) == lstm_lds_bwd(U, ES), "lstm_lds_bwd must state this kernel's static LDS");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int kq = wave & 3, ug = wave >> 2;
  const int bid = cluster_block_id(blockIdx.x, NSW, xmap);
  const int sl = bid % NSW, cl = bid / NSW, dir = cl & 1, bt = cl >> 1;
  const int nbt = (b_cnt + BT - 1) / BT;
  const BwdDir d = dir ? d1 : d0;
  const int sg = sl * kUW + ug;
  const int b0 = b_lo + bt * BT, b_end = b_lo + b_cnt, j0 = sg * 16;
  unsigned* status = reinterpret_cast<unsigned*>(xbuf);
  E* xdata = reinterpret_cast<E*>(xbuf + kStatusBytes);
  const long tile_elems = (long)BT * K;
  bool dead = false;
  const bool local = xmap && cluster_shares_xcd(xbuf, cl, sl, NSW, tid, status, dead);   // plain (L2-resident) exchange stores
  auto slot = [&](int e) { return slot_tile(xdata, dir, e, nbt, bt, tile_elems); };

  u32x4 breg[KQ];   // U[j0 + r][kq*u + k]: this wave's K quarter of the 16 output units
  load_frags<WBF, KQ>(d.uw, (long)(j0 + r) * K, kq * U, q, breg);

  const int tl = tid & 255, row = tl >> 4, col = tl & 15, j = j0 + col;
  const int b = b0 + row;
  const long bb = (b < b_end) ? b : b_lo;
  const int pch = row_chunk<64, E>(kq, lane);
  float dcin = 0.f, bs[4] = {0.f, 0.f, 0.f, 0.f};     // bs: this thread's (row, unit) share of the bias gradient, summed over the steps

#pragma unroll 1
  for (int sb = 0; sb < T; ++sb) {
    const int sp = T - 1 - sb;                       // processing index of this time in the forward pass
    const int t = dir ? T - 1 - sp : sp;
    const int tprev = dir ? t + 1 : t - 1;
    float gv[4];                                     // epilogue operands, requested before the wait
    const float* gt = d.gates + ((long)t * B + bb) * K;
#pragma unroll
    for (int g = 0; g < 4; ++g) gv[g] = gt[g * U + j];
    const float ctv = d.c[((long)t * B + bb) * U + j];
    const float cpv = (sp > 0) ? d.c[((long)tprev * B + bb) * U + j] : 0.f;
    const float dov = d.dout[((long)t * B + bb) * d.ldo + j];
    float part = 0.f;
    if (sb > 0) {
      gather_gated<4, U>(slot(sb - 1), As, LDA, tid, status, dead);   // dz of the step before, whole cluster
      __syncthreads();
      put_frag(red[ug][kq], quarter_chain<WBF, KQ>(As, LDA, kq * U, breg, r, q), r, q);
      __syncthreads();
      part = sum_quarters(&red[ug][0][tl], 256);
    }
    LstmBwdOut o = lstm_cell_bwd(part + dov, gv[0], gv[1], gv[2], gv[3], ctv, cpv, dcin);
    if (b >= b_end) { o.dz[0] = o.dz[1] = o.dz[2] = o.dz[3] = 0.f; o.dc = 0.f; }
    dcin = o.dc;
#pragma unroll
    for (int g = 0; g < 4; ++g) bs[g] += o.dz[g];
#pragma unroll
    for (int g = 0; g < 4; ++g) zout[ug][(row * 4 + g) * 16 + col] = to_e<WBF>(o.dz[g]);
    if (sb + 1 < T) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      publish_rows<64>(zout[ug], slot(sb) + (long)sg * BT * 64, pch, local);
    }
    if (b < b_end) {
      float* dz = d.dz + ((long)t * B + b) * K;
      dz[j] = o.dz[0]; dz[U + j] = o.dz[1]; dz[2 * U + j] = o.dz[2]; dz[3 * U + j] = o.dz[3];
    }
    if (sb + 1 < T) poison_rows<64>(slot(sb + 2) + (long)sg * BT * 64, pch, local);
  }
  if (d.dbp) bias_partials<4, U>(bs, red[ug], d.dbp, kq, lane, b0, b_end, j0);   // (`red` is free: the last step's sums were consumed)
}

constexpr void (*kLstmFwd[])(FwdDir, FwdDir, int, int, int, int, unsigned char*, int) = PERSIST_KERNELS(lstm_fwd_persist_kernel);
constexpr void (*kLstmBwd[])(BwdDir, BwdDir, int, int, int, int, unsigned char*, int) = PERSIST_KERNELS(lstm_bwd_persist_kernel);

// The schedule arguments of the C interface: one schedule exists -- 16-row tiles (mt = 1), two unit groups per workgroup (uw = 2); 0 = that
// one.  Returns the launcher's xreq bits (CRNN_RNN_XCD_LOCAL -> 1, CRNN_RNN_DEBUG_DROP_MEMBER -> 2), or a negative error for anything else.
int schedule_request(int mt_req, int uw_req) {
  const int uw = uw_req & 0xff;
  if ((mt_req != 0 && mt_req != 1) || (uw != 0 && uw != kUW)) return CRNN_ERR_UNSUPPORTED;
  return ((uw_req & CRNN_RNN_XCD_LOCAL) ? 1 : 0) | ((uw_req & CRNN_RNN_DEBUG_DROP_MEMBER) ? 2 : 0);
}

}  // namespace

// Bytes of the exchange buffer `xbuf` the persistent recurrences need for (T, B, u): a ring of kRing step slots per
// direction, sized for the LSTM backward (4u values per row and step); the other kernels use a part of it.
extern "C" size_t crnn_lstm_persist_xbuf_bytes(int T, int B, int u, int dt_u) {
  const size_t es = (dt_u == CRNN_BF16) ? 2 : 4;
  const size_t rows = (size_t)cdiv(B, 32) * 32;
  (void)T;
  return kStatusBytes + 2 * (size_t)kRing * rows * 4 * (size_t)u * es;
}

// 0 when (u, dt_u) has a persistent kernel; CRNN_ERR_UNSUPPORTED otherwise (callers fall back to the per-step kernels)
extern "C" int crnn_lstm_persist_supported(int u, int dt_u) { return width_index(u, dt_u) >= 0 ? CRNN_OK : CRNN_ERR_UNSUPPORTED; }

// Zero the sticky give-up counter at the head of an exchange buffer (once after allocation; see crnn_lstm_fwd_persist).
extern "C" int crnn_rnn_status_reset(void* xbuf, hipStream_t stream) {
  if (!xbuf || ((uintptr_t)xbuf & 15)) return CRNN_ERR_ARG;
  hipError_t e = hipMemsetAsync(xbuf, 0, 4, stream);
  return e == hipSuccess ? CRNN_OK : (int)e;
}

// Forward recurrence of one Bidirectional(LSTM) layer in ONE launch.  Arguments as crnn_lstm_fwd_ex; `xbuf` is
// caller-owned scratch of crnn_lstm_persist_xbuf_bytes() bytes (16-byte aligned, its first 4 bytes zeroed ONCE by the caller after
// allocation).  Status words: the unsigned at byte 0 is a sticky counter of give-ups since the caller zeroed it (no launch resets it);
// the unsigned at byte 16 is the per-launch status, 0xFFFFFFFF after a clean launch, anything else means a bounded wait gave up
// (results invalid).  crnn_rnn_status_reset(xbuf) zeroes the counter for callers that do not allocate with a zero fill (the earlier
// contract filled xbuf[0] with 0xFFFFFFFF per launch: such a buffer must be reset once before it is used with this version).
// mt_req / uw_req: the one schedule -- 0 or 1 / 0 or 2; anything else CRNN_ERR_UNSUPPORTED before any launch.  uw_req | CRNN_RNN_XCD_LOCAL
// (0x100) asks for the XCD-local workgroup -> cluster map (same results).
extern "C" int crnn_lstm_fwd_persist(const float* xw0, const float* xw1, const void* ut0, const void* ut1, float* h0, float* h1,
                                     int ldh, float* c0, float* c1, float* g0, float* g1, int T, int B, int u, int dt_u,
                                     void* xbuf, size_t xbuf_bytes, int mt_req, int uw_req, hipStream_t stream) {
  CRNN_TRY(crnn_lstm_persist_supported(u, dt_u));
  if (T < 1 || B < 1 || (((uintptr_t)ut0 | (uintptr_t)ut1) & 15)) return CRNN_ERR_ARG;
  FwdDir a{xw0, ut0, h0, ldh, c0, g0}, b{xw1, ut1, h1, ldh, c1, g1};
  const int xreq = schedule_request(mt_req, uw_req);
  if (xreq < 0) return xreq;
  return launch_persist(kLstmFwd, lstm_lds_fwd, u, a, b, T, B, u, dt_u, xbuf, xbuf_bytes, xreq, stream);
}

// BPTT of one Bidirectional(LSTM) layer in ONE launch: fills dz[d] [T][B][4u] from dout[d].  Arguments as
// crnn_lstm_bwd_ex without the dc scratch (the cell-gradient carry stays in registers).
// crnn_lstm_bwd_persist_db: the same launch also leaves the layer's bias-gradient partials, db_partials0 / 1 [crnn_rnn_db_rows(B)][4u] = column sums of dz0 / dz1 over
// time for every 16-row batch tile (finish with crnn_partials_sum over the rows) -- the stand-alone column reduction reads dz (54 MB per direction) once more.
extern "C" int crnn_rnn_db_rows(int B) { return cdiv(B, 16); }
extern "C" int crnn_lstm_bwd_persist_db(const void* u0, const void* u1, const float* c0, const float* c1, const float* g0,
                                        const float* g1, const float* dout0, const float* dout1, int ldo, float* dz0, float* dz1, float* db_partials0,
                                        float* db_partials1, int T, int B, int u, int dt_u, void* xbuf, size_t xbuf_bytes, int mt_req, int uw_req,
                                        hipStream_t stream);
extern "C" int crnn_lstm_bwd_persist(const void* u0, const void* u1, const float* c0, const float* c1, const float* g0,
                                     const float* g1, const float* dout0, const float* dout1, int ldo, float* dz0, float* dz1,
                                     int T, int B, int u, int dt_u, void* xbuf, size_t xbuf_bytes, int mt_req, int uw_req, hipStream_t stream) {
  return crnn_lstm_bwd_persist_db(u0, u1, c0, c1, g0, g1, dout0, dout1, ldo, dz0, dz1, nullptr, nullptr, T, B, u, dt_u, xbuf, xbuf_bytes, mt_req, uw_req, stream);
}
extern "C" int crnn_lstm_bwd_persist_db(const void* u0, const void* u1, const float* c0, const float* c1, const float* g0,
                                        const float* g1, const float* dout0, const float* dout1, int ldo, float* dz0, float* dz1, float* db_partials0,
                                        float* db_partials1, int T, int B, int u, int dt_u, void* xbuf, size_t xbuf_bytes, int mt_req, int uw_req,
                                        hipStream_t stream) {
  CRNN_TRY(crnn_lstm_persist_supported(u, dt_u));
  if (T < 1 || B < 1 || (((uintptr_t)u0 | (uintptr_t)u1) & 15) || (!db_partials0) != (!db_partials1)) return CRNN_ERR_ARG;
  BwdDir a{u0, c0, g0, dout0, ldo, dz0, db_partials0}, b{u1, c1, g1, dout1, ldo, dz1, db_partials1};
  const int xreq = schedule_request(mt_req, uw_req & ~CRNN_RNN_DEBUG_DROP_MEMBER);   // the drop-member grid is the forward's
  if (xreq < 0) return xreq;
  return launch_persist(kLstmBwd, lstm_lds_bwd, 4 * u, a, b, T, B, u, dt_u, xbuf, xbuf_bytes, xreq, stream);
}
