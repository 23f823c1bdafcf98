// Host-side driver of the CRNN-OCR hot path: parameter layout (Keras weight order), workspace plan,
// and the forward / backward kernel chains on one HIP stream.  Mirrors the graph of utils.py:58-96
// (CRNN.get_model) + utils.py:247-258 (STN) + utils.py:98-103 (CTC Lambda); no allocation, no sync.
#include "common.h"
#include "crnn_mi355x.h"
#include <string.h>
#include <stdio.h>
#include <string>
#include <vector>

namespace {

struct BlockSpec { int cout, ph, pw; };
const BlockSpec kBlocks[7] = {{64, 1, 1}, {128, 1, 1}, {256, 2, 2}, {256, 1, 1}, {512, 1, 2}, {512, 1, 1}, {512, 1, 1}};
const float kDropBlock = 0.1f, kDropDense1 = 0.4f, kDropRnn = 0.2f;  // utils.py:56,75,83
const uint32_t kLayerDense1 = 8, kLayerRnn = 9;

struct Tensor { std::string name; long off; long size; int ndim; int dims[4]; int dtype = CRNN_F32; };

struct Dims {
  int B, H0, W0, Hp, Wp, T, feat, C, L, tds, u, G, stn_flat;
  int Hs1, Ws1, Ho1, Wo1, Hs2, Ws2, Ho2, Wo2;  // STN locnet maps
  int bh[8], bw[8], bc[8];                      // input map of block i (1-based), bc[0] = 1
};

Dims make_dims(const crnn_config* c) {
  Dims d;
  d.B = c->batch; d.H0 = c->imgh; d.W0 = c->imgw; d.Hp = d.H0 + 4; d.Wp = d.W0 + 4;
  d.C = c->num_classes; d.L = c->max_len; d.tds = c->tds; d.u = c->units; d.G = (c->gru ? 3 : 4) * c->units;
  d.Hs1 = d.H0 / 2; d.Ws1 = d.W0 / 2; d.Ho1 = d.Hs1 - 4; d.Wo1 = d.Ws1 - 4;
  d.Hs2 = d.Ho1 / 2; d.Ws2 = d.Wo1 / 2; d.Ho2 = d.Hs2 - 4; d.Wo2 = d.Ws2 - 4;
  d.stn_flat = d.Ho2 * d.Wo2 * 20;
  int h = d.Hp, w = d.Wp, ch = 1;
  for (int i = 1; i <= 7; ++i) {
    d.bh[i] = h; d.bw[i] = w; d.bc[i - 1] = ch;
    h /= kBlocks[i - 1].ph; w /= kBlocks[i - 1].pw; ch = kBlocks[i - 1].cout;
  }
  d.bc[7] = ch;
  d.T = h; d.feat = w * ch;
  return d;
}

long pad4(long n) { return (n + 3) & ~3L; }

struct Layout {
  std::vector<Tensor> params;
  long total = 0;
  void add(const std::string& n, std::initializer_list<int> dims) {
    Tensor t; t.name = n; t.off = total; t.ndim = (int)dims.size(); t.size = 1;
    int i = 0; for (int v : dims) { t.dims[i++] = v; t.size *= v; }
    for (; i < 4; ++i) t.dims[i] = 1;
    params.push_back(t); total += pad4(t.size);
  }
  long off(const std::string& n) const { for (auto& t : params) if (t.name == n) return t.off; return -1; }
};

Layout make_layout(const crnn_config* c) {
  Dims d = make_dims(c);
  Layout L;
  L.add("stn_c1_k", {5, 5, 1, 20}); L.add("stn_c1_b", {20});
  L.add("stn_c2_k", {5, 5, 20, 20}); L.add("stn_c2_b", {20});
  L.add("stn_d1_w", {d.stn_flat, 50}); L.add("stn_d1_b", {50});
  L.add("stn_d2_w", {50, 6}); L.add("stn_d2_b", {6});
  for (int i = 1; i <= 7; ++i) {
    std::string p = "b" + std::to_string(i);
    int ci = d.bc[i - 1], co = d.bc[i];
    L.add(p + "_dw", {3, 3, ci}); L.add(p + "_bn1_g", {ci}); L.add(p + "_bn1_b", {ci});
    L.add(p + "_pw", {ci, co}); L.add(p + "_bn2_g", {co}); L.add(p + "_bn2_b", {co});
  }
  L.add("dense1_w", {d.feat, d.tds}); L.add("dense1_b", {d.tds});
  for (int l = 1; l <= 2; ++l)
    for (const char* dir : {"f", "b"}) {
      std::string p = "rnn" + std::to_string(l) + dir;
      L.add(p + "_w", {l == 1 ? d.tds : d.u, d.G}); L.add(p + "_u", {d.u, d.G}); L.add(p + "_b", {d.G});
    }
  L.add("dense2_w", {2 * d.u, d.C}); L.add("dense2_b", {d.C});
  return L;
}

// ---------------------------------------------------------------------------------------------------
struct Plan {
  std::vector<Tensor> t;
  long total = 0;
  // `count` elements of `dtype`; offsets/total are in floats (a bf16 tensor occupies count/2 floats)
  long add(const std::string& n, long count, int dtype = CRNN_F32) {
    Tensor x; x.name = n; x.off = total; x.size = count; x.ndim = 1; x.dims[0] = x.dims[1] = x.dims[2] = x.dims[3] = 1; x.dtype = dtype;
    long floats = (dtype == CRNN_BF16) ? (count + 1) / 2 : count;
    t.push_back(x); total += (floats + 63) & ~63L;  // 256-byte aligned
    return x.off;
  }
  int dt(const std::string& n) const { for (auto& x : t) if (x.name == n) return x.dtype; return CRNN_F32; }
  long off(const std::string& n) const { for (auto& x : t) if (x.name == n) return x.off; return -1; }
  bool has(const std::string& n) const { return off(n) >= 0; }
  long cnt(const std::string& n) const { for (auto& x : t) if (x.name == n) return x.size; return -1; }
};

long lmax(long a, long b) { return a > b ? a : b; }
const size_t kGemmScratchBytes = 64UL * 1024 * 1024;

// ---------------------------------------------------------------------------------------------------
// The schedule: which kernel runs for every conv block and for the layers above them.  decide() takes every decision ONCE per call -- host arithmetic on the
// configuration, the dimensions and the 16-byte alignment of the caller's three base pointers -- and make_plan (the tensors whose presence is a schedule
// decision), the forward and the backward only read the record: what both passes depend on is one field.  To change which kernel a block runs, change decide().
// Alignment: workspace tensors sit at 256-byte offsets (Plan::add), parameter and gradient tensors at 16-byte offsets (Layout::add), so a tensor meets the
// kernels' 16-byte rule exactly when its base pointer does; a bf16 shadow of a parameter tensor ("pbf" + its layout offset, 2 bytes per element) when the
// workspace base does and the offset is a multiple of 8.  make_plan and crnn_block_output_fused ask for aligned bases (AL_ALL), as torch allocations are.
// A kernel the record names has had its query asked and its alignment-checked operands looked at here, and its refusal at run time is the step's error.  The one
// exception: the depthwise row stream on bf16 maps (dws below) is chosen from the shapes alone -- the bf16-storage step has no other kernel for every stage on a
// misaligned workspace, and keeps returning -3 there and for misaligned parameters (the stream checks the depthwise weights).
enum { AL_WS = CRNN_ALIGNED_WORKSPACE, AL_PARAMS = CRNN_ALIGNED_PARAMS, AL_GRADS = CRNN_ALIGNED_GRADS, AL_ALL = CRNN_ALIGNED_ALL };
enum DwInfer { DWI_STREAM, DWI_FOLDED, DWI_PLAIN };          // inference depthwise: row stream | halo tile with BatchNorm-1 + ReLU6 folded in | plain kernel + apply pass
enum PwInfer { PWI_ONE, PWI_WRES, PWI_TILE };                // inference pointwise: block 1's outer product | weights resident (bf16 W^T) | tile kernel
enum DwFwd { DWF_PRO, DWF_STREAM, DWF_TILE_STATS, DWF_C1, DWF_TILE_COLREDUCE };   // training depthwise (+ BatchNorm-1 statistics)
enum Bn1 { BN1_PASS, BN1_GEMM_BF16, BN1_GEMM_PLANES, BN1_PW1 };   // who applies BatchNorm-1 + ReLU6: a pass of its own (writes `a`) | the pointwise GEMMs' staging (bf16 | planes) | block 1's outer product
enum PwFwd { PWF_PW1_BN, PWF_PW1, PWF_WRES3, PWF_PLANES_TILE, PWF_WRES, PWF_BNRELU6_TILE, PWF_TILE };   // training pointwise (+ BatchNorm-2 statistics)
enum BlockOut { OUT_NEXT_BLOCK, OUT_QMAX, OUT_PLAIN };       // x_i: formed inside block i+1's depthwise kernels (both passes) | written with q at the arg-max | written
enum Bn2Bwd { BN2_APPLY, BN2_QMAX, BN2_PLAIN };              // BatchNorm-2 backward: pass 2 alone (statistics from block i+1) | arg-max statistics | two-pass; each as planes where dq_planes
enum Wgrad { WG_PW1_BN, WG_PW1, WG_STREAM_BF16, WG_TILE_BF16, WG_PLANES_STREAM, WG_PLANES_TILE, WG_GEMM };
enum Dgrad { DG_PW1, DG_PRES, DG_WRES_BF16, DG_NT_BF16, DG_WRES3, DG_PLANES_TILE, DG_GEMM };   // (DG_WRES_BF16: with BatchNorm-1's backward statistics where dgrad_rows)
enum DwBwd { DWB_PRO, DWB_STREAM, DWB_TILE_FUSED, DWB_C1, DWB_THREE_KERNELS };   // depthwise stage backward; up to DWB_TILE_FUSED: one kernel
// the layers above the blocks.  C = A^T B over the rows (weight gradients): the pixel stream rounding fp32 operands on the way in | on bf16 operands | on two planes | tile GEMM
enum Tn { TN_STREAM, TN_STREAM_BF16, TN_PLANES_STREAM, TN_TILE };
enum Xw { XW_BOTH, XW_STRIPES, XW_TILE };                   // a recurrent layer's input projections: both directions in one persistent launch | one stripe-stream launch each | tile GEMMs
enum RnnDx { DX_STREAM_BF16, DX_PLANES_STREAM, DX_TILE };    // a recurrent layer's input gradient, both directions: one stripe-stream launch (bf16 shadows | two planes) | two tile GEMMs

struct BlockSched {
  int dtd, dtq, dtx;            // storage of d / a, of q, of the block output x
  long pwT_off;                 // element offset of the block's bf16 W^T copy inside "pwT" (bf16 modes, blocks 2..7), -1: none
  bool has_qm, has_dm;          // workspace tensors "qm<i>" (q at each pool window's arg-max) and "dm<i>" (keep bytes of the block output)
  // inference forward
  int inf_dw, inf_pw, pool_rows; bool inf_fold;   // pool_rows > 1: BatchNorm-2 + ReLU6 + MaxPool in the GEMM epilogue; inf_fold: BatchNorm-2 + ReLU6 there
  // training forward
  int dw, dw_rows, bn1, pw, pw_rows, out;         // *_rows: rows of statistic partials the kernel's epilogue leaves
  int bn2_rows;                                   // > 0: block i+1's depthwise backward also takes BatchNorm-2's backward statistics (rows in "bn2parts")
  // backward
  bool dq_planes;                                 // BatchNorm-2's input gradient is written as its two bf16 planes
  int bn2_bwd, wgrad, dgrad, dgrad_rows, dwb;     // dgrad_rows > 0: the data gradient also leaves BatchNorm-1's backward statistics
  bool dw_fused() const { return dwb <= DWB_TILE_FUSED; }   // (then the weight gradient may go to the side stream)
};
struct Sched {
  BlockSched b[8];              // 1-based
  long bn2parts;                // floats of "bn2parts", 0: absent
  long pwT_count, d2T_off, d1T_off;   // "pwT": its size; dense2's padded W^T and dense1's W^T behind the blocks' copies
  bool loc_fused;               // localisation net as one workgroup per sample, forward and backward
  // dense1_stream / dense2_stream: the W^T copies exist ("pwT"); *_fwd_stream: the stripe streams run on them.  dense1_gbm16: the bf16 copy of dense1's output gradient exists
  bool dense1_stream, dense1_fwd_stream, dense2_stream, dense2_fwd_stream, dense1_gbm16, dense1_dgrad_wres, dense2_bwd_fused, dense2_bwd_small;
  bool drop_keep_fused;         // Dropout(.2) under dense2: the dropped activations and the keep bytes in one pass (crnn_dropout_keep)
  bool xw_stream, rnn_persist, rnn_bwd_persist[2];   // xw_stream: the bf16 W^T copies of the projections exist ("wt<layer><dir>"); ([layer - 1])
  int xw[2], rnn_dw[2], rnn_du[2][2], rnn_dx[2], dense1_wgrad;           // Tn: dW of both directions, dU [layer - 1][forward | backward direction], dense1's dW; RnnDx
  int dtu, rnn_uw;
  int products, products_fwd, planes_fwd, planes_bwd;   // crnn_pwconv_fwd's product selectors; bf16 planes per operand of the parity mode's GEMMs
};

// Depthwise row streams: bf16 maps whose rows fill the 9 KiB step row, fp32 maps since round 4 (same outputs as the halo-tile kernels).  BatchNorm-1 + ReLU6
// in the pointwise GEMMs' staging: bf16 tensors (gemm_wres.hip / the tile GEMM) and the parity mode's plane kernels; the activated tensor `a` is then never
// written, so the weight gradient re-forms it the same way (bn1).  Block outputs formed inside the next block's depthwise kernels (OUT_NEXT_BLOCK): opt-in for
// bf16 tensors (CRNN_FLAG_BN2_DW_FUSION: VALU work the bf16 kernels have no issue slots for, measured neutral to slower), the default for
// fp32 tensors; a pooled block's output comes from q at each window's arg-max ("qm<i>"), which also serves the statistics pass of BatchNorm-2's backward
// (OUT_QMAX / BN2_QMAX, bit-identical sums).  Parity mode: three bf16 planes per operand forward (fp32-level accuracy), two backward (relative error of a
// product <= 3 * 2^-18); the weights-resident plane kernels (gemm_wres3.hip) for reductions of at most 256 channels -- at 512 the tile kernel is faster
// (profiles/r06_wres3_bench.txt) --, and dq written as planes for the two backward GEMMs (gemm_pres.hip, gemm_wgrad3.hip).
Sched decide(const crnn_config* c, const Dims& d, const Layout& L, int al = AL_ALL) {
  Sched S{};
  const int fl = c->flags, mode = c->mfma_bf16, B = d.B, u = d.u, G = d.G;
  const long TB = (long)d.T * B;
  const bool al_w = al & AL_WS, al_wp = al_w && (al & AL_PARAMS), al_wg = al_w && (al & AL_GRADS);
  auto shadow = [&](const std::string& n) { return al_w && L.off(n) % 8 == 0; };   // the bf16 shadow of parameter tensor n is 16-byte aligned
  auto at = [](long elems) { return elems % 4 == 0; };                              // an fp32 operand offset by `elems` keeps its tensor's alignment
  const bool tile_gemms = fl & CRNN_FLAG_GEMM_TILE_KERNELS, dw_tile = fl & CRNN_FLAG_DW_TILE_KERNEL, bn_stats = !(fl & CRNN_FLAG_NO_BN_STATS_FUSION);
  const bool dw_bn = !(fl & CRNN_FLAG_NO_DW_BN_FUSION), dw_bwd = !(fl & CRNN_FLAG_NO_DW_BWD_FUSION);
  const bool bn2_dw = !(fl & CRNN_FLAG_NO_BN2_DW_FUSION) && ((fl & CRNN_FLAG_BN2_DW_FUSION) || mode != 2);
  const bool bn2_stats = bn2_dw && ((fl & CRNN_FLAG_BN2_STATS_FUSION) || mode != 2);
  S.products = mode ? 1 : ((fl & CRNN_FLAG_F32_MFMA_GEMMS) ? 0 : 2);   // 1 = bf16 products, 2 = fp32-accurate plane products, 0 = fp32 MFMA
  S.planes_fwd = (fl & CRNN_FLAG_TWO_PLANE_FORWARD) ? 2 : 3;
  S.planes_bwd = (fl & CRNN_FLAG_THREE_PLANE_BACKWARD) ? 3 : 2;
  S.products_fwd = (S.products == 2 && S.planes_fwd == 2) ? 3 : S.products;   // (3 = two planes)
  // the backward's stand-alone GEMMs: the bf16 | two-plane stream kernels where their queries take the call and their operands are aligned
  const bool stream_bf16 = mode && !tile_gemms, stream_planes = S.products == 2 && S.planes_bwd == 2 && !tile_gemms;
  S.loc_fused = c->stn && !(fl & CRNN_FLAG_LOC_NET_KERNELS) && crnn_loc_net_fused_supported(d.H0, d.W0) == CRNN_OK && al_wp;
  // dense layers: the stripe streams / weights-resident kernels in the bf16 modes (whole 64-row stripes); dense2's one-pass fp32 backward in every mode
  S.dense2_stream = mode && !tile_gemms && d.C <= 128 && TB <= 0x7fffffffL && crnn_gemm_nt_f32_stream_bias_supported((int)TB, 128, 2 * u, 2 * u, 2 * u, 128) == CRNN_OK;
  S.dense1_stream = mode == 2 && !tile_gemms && crnn_dense_fwd_stream_supported_ld(TB, d.tds, d.feat, d.feat, d.feat, d.T) == CRNN_OK;
  S.dense1_gbm16 = mode == 2 && !tile_gemms && crnn_gemm_wres_supported(d.feat, d.tds) == CRNN_OK && TB * d.feat < (1L << 31);
  // dense1's backward: both GEMMs read the bf16 copy of its output gradient -- dW on the pixel stream (36 feature tiles x 7 row ranges), the data gradient on the
  // weights-resident GEMM (36 slices of 128 features keep their 128 x 128 weights in registers, the operand streams) against the bf16 shadow of W1
  S.dense1_wgrad = (S.dense1_gbm16 && al_wg && crnn_gemm_tn_bf16_stream_supported_ld(d.feat, d.tds, TB, d.feat, d.tds, d.tds, kGemmScratchBytes) == CRNN_OK) ? TN_STREAM_BF16
                   : (stream_planes && al_wg && crnn_gemm_tn_planes_stream_supported(d.feat, d.tds, TB, d.feat, d.tds, d.tds, kGemmScratchBytes) == CRNN_OK) ? TN_PLANES_STREAM : TN_TILE;
  S.dense1_dgrad_wres = S.dense1_gbm16 && shadow("dense1_w") && crnn_gemm_wres_bf16_supported(TB, d.feat, d.tds) == CRNN_OK;
  S.dense2_bwd_fused = !tile_gemms && crnn_dense_bwd_small_supported(TB, 2 * u, d.C) == CRNN_OK;
  S.dense2_bwd_small = S.dense2_bwd_fused && al_wp;
  S.drop_keep_fused = c->dropout && S.dense2_bwd_fused && al_w && crnn_dropout_keep_supported(TB, 2 * u, 2 * u, 2 * u) == CRNN_OK;
  // recurrences: bf16 U^T in the bf16 modes (u % 128 == 0); persistent one-launch-per-layer kernels with XCD-local clusters (profiles/r03_lstm_cache_policy.txt)
  S.dtu = (mode && u % 128 == 0) ? CRNN_BF16 : CRNN_F32;
  S.rnn_persist = !(fl & CRNN_FLAG_RNN_STEP_KERNELS) && (c->gru ? crnn_gru_persist_supported(u, S.dtu) : crnn_lstm_persist_supported(u, S.dtu)) == CRNN_OK;
  S.rnn_uw = (fl & CRNN_FLAG_RNN_LINEAR_CLUSTERS) ? 0 : CRNN_RNN_XCD_LOCAL;
  S.xw_stream = S.dtu == CRNN_BF16 && !tile_gemms && TB % 64 == 0 && G % 128 == 0 && d.tds % 64 == 0 && u % 64 == 0;
  for (int l = 0; l < 2; ++l) {
    const std::string n = "rnn" + std::to_string(l + 1);
    const int din = l ? u : d.tds, ldh = l ? 2 * u : u, Nh = c->gru ? 2 * u : G;   // (GRU: only the z, r columns see h_prev)
    // both directions' projections in one launch of persistent workgroups, else one stripe-stream launch each (bit-identical); both read the bias from the parameters
    S.xw[l] = !(S.xw_stream && al_wp) ? XW_TILE : crnn_rnn_input_proj_supported_ld((int)TB, G, din, din, din, G) == CRNN_OK ? XW_BOTH
              : crnn_gemm_nt_f32_stream_bias_supported((int)TB, G, din, din, din, G) == CRNN_OK ? XW_STRIPES : XW_TILE;
    // the persistent backward recurrence reads U from the bf16 shadow in the bf16 modes (u % 128 == 0), else from the fp32 parameter
    S.rnn_bwd_persist[l] = S.rnn_persist && (S.dtu == CRNN_BF16 ? shadow(n + "f_u") && shadow(n + "b_u") : (al & AL_PARAMS) != 0);
    // weight gradients C [M][N] = A^T B over K rows, A with row stride lda, dz and the gradient with G; `operands`: A and B as the driver offsets them are aligned
    auto tn = [&](int M, int N, long K, int lda, bool operands) {
      if (stream_bf16 && operands && al_wg && crnn_gemm_tn_stream_supported(M, N, K, lda, G, G, kGemmScratchBytes) == CRNN_OK) return TN_STREAM;
      if (stream_planes && operands && al_wg && crnn_gemm_tn_planes_stream_supported(M, N, K, lda, G, G, kGemmScratchBytes) == CRNN_OK) return TN_PLANES_STREAM;
      return TN_TILE;
    };
    S.rnn_dw[l] = tn(din, G, TB, din, true);                                        // dW = x^T dz over T*B rows
    S.rnn_du[l][0] = tn(u, Nh, TB - B, ldh, at((long)B * G));                       // dU = h_prev^T dz over (T-1)*B rows -- forward direction: dz from row B on
    S.rnn_du[l][1] = tn(u, Nh, TB - B, ldh, at((long)B * ldh + (l ? u : 0)));       // ... backward direction: h from row B on (layer 2: the second half of "h2")
    S.rnn_dx[l] = (stream_bf16 && shadow(n + "f_w") && shadow(n + "b_w") && crnn_gemm_nt_f32_stream_supported((int)TB, din, G, G, G, din) == CRNN_OK) ? DX_STREAM_BF16
                  : (stream_planes && al_wp && crnn_gemm_nt_f32x2_stream_supported((int)TB, din, G, G, G, din) == CRNN_OK) ? DX_PLANES_STREAM : DX_TILE;
  }
  for (int i = 1; i <= 6; ++i)   // BatchNorm-2 backward statistics taken by the next block's depthwise backward: they outlive that block's other partials
    S.bn2parts = lmax(S.bn2parts, (long)crnn_dwconv_bwd_stream_rows_ex(B, d.bh[i + 1], d.bw[i + 1], d.bc[i], mode == 2 ? CRNN_BF16 : CRNN_F32) * 2L * d.bc[i]);
  if (mode != 2 && !bn2_stats) S.bn2parts = 0;
  long pwT = 0;
  for (int i = 1; i <= 7; ++i) {
    BlockSched& b = S.b[i];
    const int H = d.bh[i], W = d.bw[i], ci = d.bc[i - 1], co = d.bc[i], ph = kBlocks[i - 1].ph, pw = kBlocks[i - 1].pw;
    const long M = (long)B * H * W, Mo = (long)B * (H / ph) * (W / pw);
    const bool pooled = ph * pw != 1;
    // storage mode 2 (bf16 tensors): every conv-stack tensor with >= 4 channels is kept as bf16
    const int dtd = b.dtd = (mode == 2 && ci % 4 == 0) ? CRNN_BF16 : CRNN_F32;
    const int dtq = b.dtq = b.dtx = (mode == 2) ? CRNN_BF16 : CRNN_F32;
    b.pwT_off = -1;
    if (mode && i >= 2 && ci % 8 == 0 && co % 8 == 0) { b.pwT_off = pwT; pwT += (long)ci * co; }
    if (i >= 2) S.pwT_count += (long)ci * co;
    b.has_qm = !(fl & CRNN_FLAG_NO_POOL_ARGMAX_Q) && pooled;
    b.has_dm = i < 7 && (!pooled || b.has_qm) && co % 8 == 0 && (mode == 2 || bn2_dw);
    const bool dws = dtd == CRNN_BF16 && !dw_tile && crnn_dwconv_fwd_stream_supported_ex(B, H, W, ci, CRNN_BF16) == CRNN_OK;
    const bool dws_f32 = dtd == CRNN_F32 && i > 1 && !dw_tile && crnn_dwconv_fwd_stream_supported_ex(B, H, W, ci, CRNN_F32) == CRNN_OK && al_wp;
    const int slab = (dtd == CRNN_BF16) ? 64 : 32;
    const bool one = ci == 1 && dtd == CRNN_F32;                                               // block 1: an outer product, not a GEMM
    const bool blk1 = one && !(fl & CRNN_FLAG_BLOCK1_KERNELS) && c->imgw + 4 <= 255;          // ... with BatchNorm-1 folded into the neighbouring kernels (block1.hip)
    const bool wres_ok = b.pwT_off >= 0 && dtq == CRNN_BF16 && !tile_gemms;
    // ---- inference: BatchNorm + ReLU6 fold into the conv that feeds them; a pooled block on bf16 maps pools in the GEMM epilogue too (groups of 2 | 4
    // consecutive rows; for the (2,2) window the depthwise row stream writes its rows in window-major order)
    b.pool_rows = 1;
    if (pooled && wres_ok && dtd == CRNN_BF16 && al_w && crnn_pwconv_fwd_wres_folded_pool_supported(M, co, ci, ph * pw) == CRNN_OK &&
        ((ph == 1 && pw == 2 && W % 2 == 0) || (ph == 2 && pw == 2 && dws && H % 2 == 0 && W % 2 == 0)))
      b.pool_rows = ph * pw;
    b.inf_dw = dws ? DWI_STREAM : (ci % slab == 0) ? DWI_FOLDED : DWI_PLAIN;
    b.inf_fold = !pooled || b.pool_rows > 1;
    b.inf_pw = one ? PWI_ONE : (wres_ok && dtd == CRNN_BF16 && al_w && crnn_gemm_wres_bf16_supported(M, co, ci) == CRNN_OK) ? PWI_WRES : PWI_TILE;
    // ---- training forward
    const bool pro = i > 1 && S.b[i - 1].out == OUT_NEXT_BLOCK;
    if (pro || dws || dws_f32) { b.dw = pro ? DWF_PRO : DWF_STREAM; b.dw_rows = crnn_dwconv_fwd_stream_rows_ex(B, H, W, ci, dtd); }
    else if (ci % 32 == 0 && ci % slab == 0) { b.dw = DWF_TILE_STATS; b.dw_rows = crnn_dwconv_num_tiles(B, H, W); }
    else if (blk1) { b.dw = DWF_C1; b.dw_rows = crnn_dwconv_c1_stat_rows(B, H, W); }
    else { b.dw = DWF_TILE_COLREDUCE; b.dw_rows = crnn_colreduce_chunks(M); }
    const bool fuse_a = dw_bn && mode == 2 && dtd == CRNN_BF16 && dtq == CRNN_BF16 && ci % 8 == 0 && ci <= 512;
    const bool fuse_x3 = dw_bn && S.products == 2 && dtd == CRNN_F32 && dtq == CRNN_F32 && ci % 4 == 0 && ci >= 16 && ci <= 512;
    b.bn1 = blk1 ? BN1_PW1 : fuse_a ? BN1_GEMM_BF16 : (fuse_x3 && al_wp) ? BN1_GEMM_PLANES : BN1_PASS;
    b.pw_rows = crnn_pwconv_stat_rows(M);
    if (one) b.pw = blk1 ? PWF_PW1_BN : PWF_PW1;
    else if (b.bn1 == BN1_GEMM_PLANES) {
      b.pw = PWF_PLANES_TILE;
      if (!tile_gemms && ci <= 256 && crnn_gemm_wres3_supported(M, co, ci) == CRNN_OK) { b.pw = PWF_WRES3; b.pw_rows = crnn_gemm_wres3_stat_rows(M, co, ci); }
    } else if (b.bn1 == BN1_GEMM_BF16) {
      b.pw = PWF_BNRELU6_TILE;
      if (wres_ok && al_w && crnn_pwconv_fwd_wres_supported(M, co, ci) == CRNN_OK) { b.pw = PWF_WRES; b.pw_rows = crnn_pwconv_fwd_wres_rows(M, co, ci); }
    } else b.pw = PWF_TILE;
    // the block output: the shapes crnn_bn_act_pool_drop_qmax_ex / crnn_bn_bwd_qmax_ex take (whole windows, 32-bit element counter) ...
    const bool qmax_shape = b.has_qm && H % ph == 0 && W % pw == 0 && co % 4 == 0 && Mo * co + 8192L * 256 * 8 < (1L << 31);
    bool next = false;   // ... and the next block's prologue kernels (both passes: the backward has no x_i to fall back to)
    if (i <= 6 && bn2_dw && !dw_tile && dw_bwd && (!pooled || qmax_shape) && b.has_dm && (!bn2_stats || S.bn2parts > 0) && al_wp) {
      const int Hn = d.bh[i + 1], Wn = d.bw[i + 1];
      const int dtn = (mode == 2 && co % 4 == 0) ? CRNN_BF16 : CRNN_F32;
      next = dtn == dtq && crnn_dwconv_fwd_stream_pro_supported_ex(B, Hn, Wn, co, dtq) == CRNN_OK && crnn_dwconv_bwd_stream_pro_supported_ex(B, Hn, Wn, co, dtq) == CRNN_OK &&
             (dtq == CRNN_F32 || crnn_dwconv_bwd_fused_supported(Hn, Wn, co) == CRNN_OK);
      b.bn2_rows = (next && bn2_stats) ? crnn_dwconv_bwd_stream_rows_ex(B, Hn, Wn, co, dtn) : 0;
    }
    const bool qmax = qmax_shape && al_w;
    b.out = next ? OUT_NEXT_BLOCK : qmax ? OUT_QMAX : OUT_PLAIN;
    // ---- backward
    b.bn2_bwd = b.bn2_rows > 0 ? BN2_APPLY : qmax ? BN2_QMAX : BN2_PLAIN;
    const int dtx_in = i > 1 ? S.b[i - 1].dtx : CRNN_F32;
    const bool fused_bf = i > 1 && dtd == CRNN_BF16 && dtx_in == CRNN_BF16 && dw_bwd && crnn_dwconv_bwd_fused_supported(H, W, ci) == CRNN_OK;
    // the row stream (dwconv_bwd_stream.hip) where its query takes the shape and its operands -- workspace tensors and the depthwise weights -- are aligned;
    // bf16 tensors otherwise on the halo tiles (conv_bwd_fused.hip), fp32 tensors as three kernels
    const bool dbs = dw_bwd && !dw_tile && crnn_dwconv_bwd_stream_supported_ex(B, H, W, ci, dtd) == CRNN_OK && al_wp;
    const bool fused_f32 = i > 1 && dtd == CRNN_F32 && dtq == CRNN_F32 && dtx_in == CRNN_F32 && dbs;
    b.dwb = pro ? DWB_PRO : fused_f32 ? DWB_STREAM : fused_bf ? (dbs ? DWB_STREAM : DWB_TILE_FUSED) : blk1 ? DWB_C1 : DWB_THREE_KERNELS;
    b.dq_planes = fuse_x3 && S.planes_bwd == 2 && !tile_gemms && bn_stats && !(fl & CRNN_FLAG_NO_GRADIENT_PLANES) && crnn_gemm_pres_supported(M, ci, co, 2) == CRNN_OK &&
                  crnn_pwconv_wgrad_planes_stream_supported(M, co, ci) == CRNN_OK && crnn_pwconv_wgrad_planes_stream_scratch_bytes(M, co, ci) <= kGemmScratchBytes && al_wp;
    if (one) { b.wgrad = blk1 ? WG_PW1_BN : WG_PW1; b.dgrad = DG_PW1; b.dgrad_rows = blk1 ? crnn_pw1_bn_bwd_rows(M) : 0; continue; }
    b.wgrad = b.bn1 == BN1_GEMM_BF16 ? ((!tile_gemms && crnn_pwconv_wgrad_stream_supported(M, co, ci) == CRNN_OK && al_wg) ? WG_STREAM_BF16 : WG_TILE_BF16)
              : b.bn1 == BN1_GEMM_PLANES ? (b.dq_planes ? WG_PLANES_STREAM : WG_PLANES_TILE) : WG_GEMM;
    // data gradient: where the depthwise stage follows as one kernel (bf16) / in the parity mode, its epilogue also takes BatchNorm-1's backward statistics
    if (b.dq_planes) { b.dgrad = DG_PRES; b.dgrad_rows = crnn_gemm_pres_stat_rows(M, ci, co, 2); }
    else if (mode == 2 && dtq == CRNN_BF16 && dtd == CRNN_BF16 && !tile_gemms) {
      // bf16 tensors against the bf16 shadow of the block's weights: resident in registers (gemm_wres.hip) -- its storer waves also take the statistics where the
      // depthwise stage follows as one kernel --, else streamed (gemm_nt.hip); a shadow that is not 16-byte aligned: the tile GEMM and the stand-alone statistics
      const bool sh = shadow("b" + std::to_string(i) + "_pw");
      if (sh && b.dw_fused() && bn_stats && crnn_gemm_wres_bnstats_supported(M, ci, co) == CRNN_OK) { b.dgrad = DG_WRES_BF16; b.dgrad_rows = crnn_gemm_wres_bnstats_rows(M, ci, co); }
      else b.dgrad = !sh ? DG_GEMM : crnn_gemm_wres_bf16_supported(M, ci, co) == CRNN_OK ? DG_WRES_BF16 : (M <= 0x7fffffffL && crnn_gemm_nt_bf16_supported((int)M, ci, co) == CRNN_OK) ? DG_NT_BF16 : DG_GEMM;
    } else if (S.products == 2 && dtq == CRNN_F32 && dtd == CRNN_F32 && bn_stats && crnn_gemm_f32x3_bnstats_supported(M, ci, co) == CRNN_OK) {
      // the parity mode's statistics from the data gradient's epilogue: W^T planes resident for reductions of 256 channels (gemm_wres3.hip), else the plane tile GEMM
      if (!tile_gemms && co == 256 && crnn_gemm_wres3_supported(M, ci, co) == CRNN_OK && al_w) { b.dgrad = DG_WRES3; b.dgrad_rows = crnn_gemm_wres3_stat_rows(M, ci, co); }
      else if (al_wp) { b.dgrad = DG_PLANES_TILE; b.dgrad_rows = crnn_gemm_f32x3_bnstats_rows(M); }
      else b.dgrad = DG_GEMM;
    } else b.dgrad = DG_GEMM;
  }
  S.d2T_off = S.dense2_stream ? pwT : -1;
  S.d1T_off = S.dense1_stream ? pwT + 128L * 2 * u : -1;
  S.pwT_count += 128L * 2 * u + (S.dense1_stream ? (long)d.feat * d.tds : 0);
  // the dense layers' forward on the stripe stream against their W^T copies in "pwT" (dense1: and its bias)
  S.dense1_fwd_stream = S.dense1_stream && al_wp && S.d1T_off % 8 == 0;
  S.dense2_fwd_stream = S.dense2_stream && al_w && S.d2T_off % 8 == 0;
  return S;
}

Plan make_plan(const crnn_config* c, const Dims& d, const Layout& L, const Sched& S) {
  Plan P;
  const long B = d.B;
  // BatchNorm state blocks [mean|var|scale|shift] first: their offsets must stay small (int) for crnn_bn_update
  for (int i = 1; i <= 7; ++i) {
    P.add("bn1s" + std::to_string(i), 4L * d.bc[i - 1]);
    P.add("bn2s" + std::to_string(i), 4L * d.bc[i]);
  }
  // STN locnet
  P.add("pool1", B * d.Hs1 * d.Ws1);
  P.add("c1", B * d.Ho1 * d.Wo1 * 20);
  P.add("pool2", B * d.Hs2 * d.Ws2 * 20);
  P.add("flat", B * d.stn_flat);
  P.add("fc1", B * 50);
  P.add("theta", B * 6);
  P.add("x0", B * d.Hp * d.Wp);
  long maxact = 0, maxparts = 0;
  for (int i = 1; i <= 7; ++i) {
    std::string p = std::to_string(i);
    const BlockSched& b = S.b[i];
    long M = B * d.bh[i] * d.bw[i];
    int ci = d.bc[i - 1], co = d.bc[i];
    long Mo = B * (d.bh[i] / kBlocks[i - 1].ph) * (d.bw[i] / kBlocks[i - 1].pw);
    P.add("d" + p, M * ci, b.dtd); P.add("a" + p, M * ci, b.dtd); P.add("q" + p, M * co, b.dtq); P.add("x" + p, Mo * co, b.dtx);
    if (b.has_qm) P.add("qm" + p, Mo * co, b.dtq);   // q at each pool window's arg-max (training forward -> the backward's statistics pass)
    if (b.has_dm) P.add("dm" + p, (Mo * co / 8 + 3) / 4);   // dropout keep bytes of the block output (one per 8 elements) for the prologue depthwise kernels of block i+1
    maxact = lmax(maxact, M * co);
    long tiles = crnn_dwconv_num_tiles(d.B, d.bh[i], d.bw[i]);
    maxparts = lmax(maxparts, tiles * 9L * ci);
    maxparts = lmax(maxparts, (long)crnn_dwconv_bwd_fused_rows(d.B, d.bh[i], d.bw[i], ci) * 9L * ci);
    for (int dt : {CRNN_BF16, CRNN_F32}) {
      maxparts = lmax(maxparts, (long)crnn_dwconv_fwd_stream_rows_ex(d.B, d.bh[i], d.bw[i], ci, dt) * 2L * ci);
      maxparts = lmax(maxparts, (long)crnn_dwconv_bwd_stream_rows_ex(d.B, d.bh[i], d.bw[i], ci, dt) * 9L * ci);
    }
    maxparts = lmax(maxparts, (long)crnn_colreduce_chunks(M) * 2L * lmax(ci, co));
    if (ci == 1) maxparts = lmax(maxparts, lmax((long)crnn_dwconv_c1_stat_rows(d.B, d.bh[i], d.bw[i]) * 2L, (long)crnn_pw1_bn_bwd_rows(M) * (co + 2L) + 64));
    maxparts = lmax(maxparts, (long)crnn_pwconv_stat_rows(M) * 2L * co);
    maxparts = lmax(maxparts, (long)crnn_pwconv_fwd_wres_rows(M, co, ci) * 2L * co);   // one row per IO wave and stripe lane: more rows than tiles at small batches
    maxparts = lmax(maxparts, (long)crnn_bn_bwd_chunks(M) * 2L * lmax(ci, co));
    maxparts = lmax(maxparts, (long)crnn_gemm_wres_bnstats_rows(M, ci, co) * 2L * ci);
    maxparts = lmax(maxparts, (long)crnn_gemm_wres3_stat_rows(M, co, ci) * 2L * co);   // parity mode, weights-resident plane kernels (gemm_wres3.hip): forward ...
    maxparts = lmax(maxparts, (long)crnn_gemm_wres3_stat_rows(M, ci, co) * 2L * ci);   // ... and data gradient
  }
  const long TB = (long)d.T * B;
  P.add("dn1", TB * d.tds);
  for (int l = 1; l <= 2; ++l) {
    std::string p = std::to_string(l);
    for (const char* dir : {"f", "b"}) {
      P.add("xw" + p + dir, TB * d.G); P.add("cs" + p + dir, TB * d.u); P.add("gt" + p + dir, TB * d.G);
      P.add("ut" + p + dir, (long)d.G * d.u); P.add("dz" + p + dir, TB * d.G);
      P.add("dbp" + p + dir, (long)crnn_rnn_db_rows((int)B) * d.G);   // bias-gradient partials of the persistent LSTM backward (one row per 16-row batch tile)
      P.add("wt" + p + dir, (long)d.G * (l == 1 ? d.tds : d.u));   // bf16 W^T of the input projection (streaming xw kernel), oversized by 2
    }
  }
  P.add("h1f", TB * d.u); P.add("h1b", TB * d.u); P.add("r1", TB * d.u);
  P.add("h2", TB * 2 * d.u); P.add("r2d", TB * 2 * d.u);
  P.add("logits", TB * d.C); P.add("ypred", TB * d.C);
  // backward
  P.add("dlogits", TB * d.C); P.add("dr2", TB * 2 * d.u); P.add("dr1", TB * d.u);
  P.add("dcf", B * d.u); P.add("dcb", B * d.u); P.add("dhpf", B * d.u); P.add("dhpb", B * d.u);
  P.add("ddn1", TB * d.tds); P.add("gbm", TB * d.tds);
  if (S.dense1_gbm16) P.add("gbm16", TB * d.tds, CRNN_BF16);   // bf16 copy of dense1's output gradient (operand of both backward GEMMs)
  maxact = lmax(maxact, TB * d.feat);
  // gradient ping-pong buffers: sized for fp32, hold bf16 tensors in storage mode 2
  P.add("gA", maxact); P.add("gB", maxact); P.add("gC", maxact);   // conv-stack gradient buffers (three: a weight-gradient GEMM on the side stream may still read one)
  P.add("dtheta", B * 6); P.add("dfc1", B * 50); P.add("dflat", B * d.stn_flat);
  if (S.loc_fused) P.add("locterms", crnn_loc_net_bwd_scratch((int)B));   // the samples' convolution weight-gradient terms (crnn_loc_net_bwd)
  P.add("dpool2", B * d.Hs2 * d.Ws2 * 20); P.add("dc1", B * d.Ho1 * d.Wo1 * 20);
  maxparts = lmax(maxparts, (long)crnn_colreduce_chunks(TB) * lmax(d.G, lmax(d.tds, d.C)));
  maxparts = lmax(maxparts, (long)crnn_colreduce_chunks(B * d.Ho1 * d.Wo1) * 64);
  if (c->stn) {
    maxparts = lmax(maxparts, ((long)crnn_loc_conv_wgrad_chunks(d.B, d.Hs1, d.Ws1) + 1) * (25L * 20 + 20));
    maxparts = lmax(maxparts, ((long)crnn_loc_conv_wgrad_chunks(d.B, d.Hs2, d.Ws2) + 1) * (25L * 20 * 20 + 20));
  }
  P.add("partials", maxparts);
  if (S.bn2parts) P.add("bn2parts", S.bn2parts);
  // bf16 W^T copies of the pointwise-conv weights (bf16 modes) + dense2's W^T as 128 rows of 2u (rows >= num_classes are never written: the streaming
  // GEMM's columns for them are never read) + dense1's W^T [tds][feat] (dense1_stream)
  P.add("pwT", S.pwT_count, CRNN_BF16);
  if (c->mfma_bf16) P.add("lg128", TB * 128);   // dense2's raw products over the padded weight matrix
  if (S.dense2_bwd_fused) {
    P.add("d2part", (long)(crnn_dense_bwd_small_scratch_bytes(TB, 2 * d.u, d.C) / sizeof(float)));   // per-workgroup partial gradients of dense2
    P.add("keep9", (TB * 2 * d.u / 8 + 3) / 4);   // keep bytes of the Dropout(.2) under dense2 (written by the forward's dropout pass, read by the one-pass backward)
  }
  P.add("pbf", L.total, CRNN_BF16);   // bf16 shadow of the parameter buffer (GEMM B operands in the bf16 modes)
  P.add("coef", 2 * 1024);
  P.add("fold", 32 * 2 * 1024);   // chunk sums of long BatchNorm partial lists (crnn_bn_finalize_folded)
  P.add("gemm_scratch", 16L * 1024 * 1024);   // 64 MiB of split-reduction partials (main stream)
  P.add("gemm_scratch2", 16L * 1024 * 1024);  // the same for the side stream of the backward
  P.add("partials2", lmax((long)crnn_colreduce_chunks(TB) * lmax(d.G, lmax(d.tds, d.C)), 1024));
  if (S.rnn_persist) P.add("rnnx", (long)((crnn_lstm_persist_xbuf_bytes(d.T, d.B, d.u, S.dtu) + 3) / 4));   // h_t / dz_t exchange tiles
  return P;
}
Plan make_plan(const crnn_config* c) { Dims d = make_dims(c); Layout L = make_layout(c); return make_plan(c, d, L, decide(c, d, L)); }

bool aligned16(const void* a, const void* b = nullptr) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

struct Ctx {
  const crnn_config* cfg; Dims d; Layout L; Plan P; Sched S;
  const float* params; float* grads; float* ws; hipStream_t s;
  const float* p(const std::string& n) const { return params + L.off(n); }
  float* g(const std::string& n) const { return grads + L.off(n); }
  float* w(const std::string& n) const { return ws + P.off(n); }
  int gdt() const { return cfg->mfma_bf16 == 2 ? CRNN_BF16 : CRNN_F32; }   // storage of the conv-stack gradients
  bool side = false;   // side-stream context: its own split-reduction scratch and reduction partials
  float* scratch() const { return ws + P.off(side ? "gemm_scratch2" : "gemm_scratch"); }
  float* partials() const { return ws + P.off(side ? "partials2" : "partials"); }
};

// In the bf16 modes a weight operand (B of the NN / NT GEMMs, i.e. a pointer into the parameter buffer) is read from
// the bf16 shadow copy refreshed at the start of every forward: half the L2->LDS bytes, identical rounding (RNE).
const float* weight_operand(const Ctx& c, int mode, const float* B, int* dtB) {
  if (c.cfg->mfma_bf16 && mode != 2 && B >= c.params && B < c.params + c.L.total) {
    *dtB = CRNN_BF16;
    return reinterpret_cast<const float*>(reinterpret_cast<const bf16_t*>(c.ws + c.P.off("pbf")) + (B - c.params));
  }
  return B;
}
// a recurrent layer's U as the backward recurrences read it: the bf16 shadow in the bf16 modes (u % 128 == 0), else the fp32 parameter
const float* rnn_u_operand(const Ctx& c, const std::string& layer_dir, int* dtu) {
  const float* U = c.p("rnn" + layer_dir + "_u");
  return c.S.dtu == CRNN_BF16 ? weight_operand(c, 0, U, dtu) : U;
}
// One context per entry point: dimensions, layout, record and plan are built once.  The plan is the aligned record's (no workspace byte depends on the
// caller's pointers); the record the passes read is the one for the pointers they were given.
Ctx make_ctx(const crnn_config* cfg, const float* params, float* grads, float* ws, hipStream_t stream) {
  Ctx c{cfg, make_dims(cfg), make_layout(cfg), Plan(), Sched(), params, grads, ws, stream};
  c.S = decide(cfg, c.d, c.L);
  c.P = make_plan(cfg, c.d, c.L, c.S);
  const int al = (aligned16(ws) ? AL_WS : 0) | (aligned16(params) ? AL_PARAMS : 0) | (aligned16(grads) ? AL_GRADS : 0);
  if (al != AL_ALL) c.S = decide(cfg, c.d, c.L, al);
  return c;
}
// GEMMs of the conv stack / dense layers / RNN input projections: bf16 products when cfg->mfma_bf16
// planes: bf16 planes per operand of the parity mode's products (3 = fp32-accurate; 2 = 16 significant bits per factor)
int gemm(const Ctx& c, int mode, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
         const float* bias = nullptr, int act = 0, int acc = 0, int perm = 0, int planes = 3) {
  if (c.cfg->mfma_bf16) {
    int dtB = CRNN_F32;
    B = weight_operand(c, mode, B, &dtB);
    return crnn_gemm_bf16_ex(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, acc, perm, c.scratch(), kGemmScratchBytes, CRNN_F32, dtB, CRNN_F32, c.s);
  }
  // parity mode: fp32 tensors; the products from three bf16 planes per operand (fp32-level accuracy on the 16x faster bf16 matrix path,
  // crnn_gemm_f32x3).  CRNN_FLAG_F32_MFMA_GEMMS: fp32 MFMA (an fmaf chain bit for bit)
  if (c.S.products == 0)
    return crnn_gemm_f32(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, acc, perm, c.scratch(), kGemmScratchBytes, c.s);
  if (planes == 2) return crnn_gemm_f32x2(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, acc, perm, c.scratch(), kGemmScratchBytes, c.s);
  return crnn_gemm_f32x3(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, acc, perm, c.scratch(), kGemmScratchBytes, c.s);
}
// GEMM with explicit operand / result storage types (storage mode 2); falls back to the plain entry points otherwise
int gemm_t(const Ctx& c, int mode, const float* A, int dtA, const float* B, int dtB, float* C, int dtC, int M, int N, int K, int lda,
           int ldb, int ldc, const float* bias = nullptr, int act = 0, int acc = 0, int perm = 0, int planes = 3) {
  if (c.cfg->mfma_bf16 == 2) {
    B = weight_operand(c, mode, B, &dtB);
    return crnn_gemm_bf16_ex(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, acc, perm, c.scratch(), kGemmScratchBytes, dtA, dtB, dtC, c.s);
  }
  if (dtA != CRNN_F32 || dtB != CRNN_F32 || dtC != CRNN_F32) return CRNN_ERR_ARG;
  return gemm(c, mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, acc, perm, planes);
}
// the pointwise weights of block i as the forward GEMMs read them: the bf16 W^T copy in "pwT" where one was made (both operands contiguous along the
// reduction), else the bf16 shadow (bf16 modes) or the fp32 parameter
struct PwWeights { const float* w; int dt, transposed; };
PwWeights pw_weights(const Ctx& c, int i) {
  if (c.S.b[i].pwT_off >= 0) return {reinterpret_cast<const float*>(reinterpret_cast<const bf16_t*>(c.w("pwT")) + c.S.b[i].pwT_off), CRNN_BF16, 1};
  PwWeights r{nullptr, CRNN_F32, 0};
  r.w = weight_operand(c, 0, c.p("b" + std::to_string(i) + "_pw"), &r.dt);
  return r;
}
// the tensor the prologue kernels of block i + 1 form x_i from: q_i, or q_i at the pool windows' arg-max
float* pro_src(const Ctx& c, int i) { return c.w((kBlocks[i - 1].ph * kBlocks[i - 1].pw != 1 ? "qm" : "q") + std::to_string(i)); }
const float* keep_bytes(const Ctx& c, int i) { return c.cfg->dropout ? c.w("dm" + std::to_string(i)) : nullptr; }
// always-fp32 GEMM (spatial-transformer localisation net: tiny, and theta is precision-sensitive)
int gemm32(const Ctx& c, int mode, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
           const float* bias = nullptr, int act = 0, int acc = 0, int perm = 0) {
  return crnn_gemm_f32(mode, A, B, C, M, N, K, lda, ldb, ldc, bias, act, acc, perm, c.scratch(), kGemmScratchBytes, c.s);
}

int colsum(const Ctx& c, const float* x, long M, int C, int ld, float* out) {
  CRNN_TRY(crnn_colreduce_ex(x, c.partials(), M, C, ld, 1, CRNN_F32, c.s));
  return crnn_partials_sum(c.partials(), crnn_colreduce_chunks(M), C, out, 1.f, c.s);
}

int check_cfg(const crnn_config* c) {
  if (!c || c->batch <= 0) return CRNN_ERR_ARG;
  if (c->units < 64 || c->units % 64) return CRNN_ERR_UNSUPPORTED;
  if (c->mfma_bf16 < 0 || c->mfma_bf16 > 2) return CRNN_ERR_ARG;
  if (c->num_classes > 128 || c->num_classes < 2) return CRNN_ERR_UNSUPPORTED;   // two classes per lane of a wavefront (ctc.hip, beam.hip)
  if (2 * c->max_len + 1 > 64) return CRNN_ERR_UNSUPPORTED;
  if (c->tds % 4) return CRNN_ERR_UNSUPPORTED;
  Dims d = make_dims(c);
  if (c->stn && (d.Ho2 < 1 || d.Wo2 < 1)) return CRNN_ERR_UNSUPPORTED;
  if (d.T < 3 || d.feat < 1) return CRNN_ERR_UNSUPPORTED;
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
extern "C" int crnn_num_params(const crnn_config* cfg) { return (int)make_layout(cfg).params.size(); }
extern "C" long crnn_params_total(const crnn_config* cfg) { return make_layout(cfg).total; }
extern "C" int crnn_param_info(const crnn_config* cfg, int idx, char* name, int name_cap, long* offset, long* size,
                               int* ndim, int* dims) {
  Layout L = make_layout(cfg);
  if (idx < 0 || idx >= (int)L.params.size()) return CRNN_ERR_ARG;
  const Tensor& t = L.params[idx];
  if (name && name_cap > 0) { strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (offset) *offset = t.off;
  if (size) *size = t.size;
  if (ndim) *ndim = t.ndim;
  if (dims) for (int i = 0; i < 4; ++i) dims[i] = t.dims[i];
  return 0;
}
extern "C" int crnn_time_steps(const crnn_config* cfg) { return make_dims(cfg).T; }
extern "C" int crnn_bn_total(const crnn_config* cfg) {
  Dims d = make_dims(cfg); int n = 0;
  for (int i = 1; i <= 7; ++i) n += d.bc[i - 1] + d.bc[i];
  return n;
}
// idx 0..13: b1_bn1, b1_bn2, b2_bn1, ...
extern "C" int crnn_bn_info(const crnn_config* cfg, int idx, char* name, int name_cap, int* offset, int* channels, long* count) {
  if (idx < 0 || idx >= 14) return CRNN_ERR_ARG;
  Dims d = make_dims(cfg);
  int off = 0;
  for (int k = 0; k < idx; ++k) { int i = k / 2 + 1; off += (k % 2 == 0) ? d.bc[i - 1] : d.bc[i]; }
  int i = idx / 2 + 1;
  if (name && name_cap > 0) snprintf(name, name_cap, "b%d_bn%d", i, idx % 2 + 1);
  if (offset) *offset = off;
  if (channels) *channels = (idx % 2 == 0) ? d.bc[i - 1] : d.bc[i];
  if (count) *count = (long)d.B * d.bh[i] * d.bw[i];
  return 0;
}
extern "C" size_t crnn_workspace_bytes(const crnn_config* cfg) {
  if (check_cfg(cfg)) return 0;
  return (size_t)make_plan(cfg).total * sizeof(float);
}
extern "C" int crnn_ws_tensor_info(const crnn_config* cfg, const char* name, long* offset, long* count, int* dtype) {
  Plan P = make_plan(cfg);
  long o = P.off(name);
  if (o < 0) return CRNN_ERR_ARG;
  if (offset) *offset = o;
  if (count) *count = P.cnt(name);
  if (dtype) *dtype = P.dt(name);
  return 0;
}
// 1 when training does not materialise the output x_block of conv block `block` (1..7): the next block's depthwise row-stream kernels form it
// from q_block in LDS (fp32 tensors: the default; bf16 tensors: CRNN_FLAG_BN2_DW_FUSION; image width 32) -- the workspace tensor "x<block>" is
// then never written by a training forward.  (16-byte aligned parameter / workspace base pointers assumed, as torch allocations are.)
extern "C" int crnn_block_output_fused(const crnn_config* cfg, int block) {
  if (check_cfg(cfg) || block < 1 || block > 7) return 0;
  return decide(cfg, make_dims(cfg), make_layout(cfg)).b[block].out == OUT_NEXT_BLOCK ? 1 : 0;
}
// The record as text (include/crnn_mi355x.h): every field of decide()'s answer for the given alignment mask, the enum values by name
extern "C" int crnn_schedule_describe(const crnn_config* cfg, int aligned_mask, char* buf, int cap) {
  static const char* const dt[] = {"f32", "bf16"};
  static const char* const dwi[] = {"DWI_STREAM", "DWI_FOLDED", "DWI_PLAIN"}, *const pwi[] = {"PWI_ONE", "PWI_WRES", "PWI_TILE"};
  static const char* const dwf[] = {"DWF_PRO", "DWF_STREAM", "DWF_TILE_STATS", "DWF_C1", "DWF_TILE_COLREDUCE"};
  static const char* const bn1[] = {"BN1_PASS", "BN1_GEMM_BF16", "BN1_GEMM_PLANES", "BN1_PW1"};
  static const char* const pwf[] = {"PWF_PW1_BN", "PWF_PW1", "PWF_WRES3", "PWF_PLANES_TILE", "PWF_WRES", "PWF_BNRELU6_TILE", "PWF_TILE"};
  static const char* const out[] = {"OUT_NEXT_BLOCK", "OUT_QMAX", "OUT_PLAIN"}, *const bn2[] = {"BN2_APPLY", "BN2_QMAX", "BN2_PLAIN"};
  static const char* const wg[] = {"WG_PW1_BN", "WG_PW1", "WG_STREAM_BF16", "WG_TILE_BF16", "WG_PLANES_STREAM", "WG_PLANES_TILE", "WG_GEMM"};
  static const char* const dg[] = {"DG_PW1", "DG_PRES", "DG_WRES_BF16", "DG_NT_BF16", "DG_WRES3", "DG_PLANES_TILE", "DG_GEMM"};
  static const char* const dwb[] = {"DWB_PRO", "DWB_STREAM", "DWB_TILE_FUSED", "DWB_C1", "DWB_THREE_KERNELS"};
  static const char* const tn[] = {"TN_STREAM", "TN_STREAM_BF16", "TN_PLANES_STREAM", "TN_TILE"}, *const dx[] = {"DX_STREAM_BF16", "DX_PLANES_STREAM", "DX_TILE"};
  static const char* const xwn[] = {"XW_BOTH", "XW_STRIPES", "XW_TILE"};
  static_assert(sizeof dg / sizeof *dg == DG_GEMM + 1 && sizeof wg / sizeof *wg == WG_GEMM + 1 && sizeof pwf / sizeof *pwf == PWF_TILE + 1 && sizeof tn / sizeof *tn == TN_TILE + 1, "one name per value");
  CRNN_TRY(check_cfg(cfg));
  if (cap < 0 || (cap > 0 && !buf)) return CRNN_ERR_ARG;
  const Sched S = decide(cfg, make_dims(cfg), make_layout(cfg), aligned_mask & AL_ALL);
  std::string t;
  char line[768];
  for (int i = 1; i <= 7; ++i) {
    const BlockSched& b = S.b[i];
    snprintf(line, sizeof line, "block%d: dtd=%s dtq=%s dtx=%s pwT_off=%ld qm=%d dm=%d inf_dw=%s inf_pw=%s pool_rows=%d inf_fold=%d dw=%s dw_rows=%d bn1=%s pw=%s pw_rows=%d out=%s "
             "bn2_rows=%d dq_planes=%d bn2_bwd=%s wgrad=%s dgrad=%s dgrad_rows=%d dwb=%s\n", i, dt[b.dtd], dt[b.dtq], dt[b.dtx], b.pwT_off, b.has_qm, b.has_dm, dwi[b.inf_dw],
             pwi[b.inf_pw], b.pool_rows, b.inf_fold, dwf[b.dw], b.dw_rows, bn1[b.bn1], pwf[b.pw], b.pw_rows, out[b.out], b.bn2_rows, b.dq_planes, bn2[b.bn2_bwd], wg[b.wgrad],
             dg[b.dgrad], b.dgrad_rows, dwb[b.dwb]);
    t += line;
  }
  snprintf(line, sizeof line, "top: products=%d products_fwd=%d planes_fwd=%d planes_bwd=%d loc=%s bn2parts=%ld pwT_count=%ld d2T_off=%ld d1T_off=%ld dtu=%s rnn=%s rnn_uw=%d\n", S.products,
           S.products_fwd, S.planes_fwd, S.planes_bwd, S.loc_fused ? "LOC_FUSED" : "LOC_KERNELS", S.bn2parts, S.pwT_count, S.d2T_off, S.d1T_off, dt[S.dtu], S.rnn_persist ? "RNN_PERSIST" : "RNN_STEPS",
           S.rnn_uw);
  t += line;
  snprintf(line, sizeof line, "dense1: wT=%d fwd=%s gbm16=%d wgrad=%s dgrad=%s\n", S.dense1_stream, S.dense1_fwd_stream ? "D1F_STREAM" : "D1F_TILE", S.dense1_gbm16, tn[S.dense1_wgrad],
           S.dense1_dgrad_wres ? "D1G_WRES_BF16" : "D1G_TILE");
  t += line;
  for (int l = 0; l < 2; ++l) {
    snprintf(line, sizeof line, "rnn%d: xw=%s bwd=%s dw=%s du_f=%s du_b=%s dx=%s\n", l + 1, xwn[S.xw[l]],
             S.rnn_bwd_persist[l] ? "RNN_PERSIST" : "RNN_STEPS", tn[S.rnn_dw[l]], tn[S.rnn_du[l][0]], tn[S.rnn_du[l][1]], dx[S.rnn_dx[l]]);
    t += line;
  }
  snprintf(line, sizeof line, "dense2: drop=%s wT=%d fwd=%s d2part=%d bwd=%s\n", S.drop_keep_fused ? "DROP_KEEP_FUSED" : "DROP_PASSES", S.dense2_stream, S.dense2_fwd_stream ? "D2F_STREAM" : "D2F_TILE", S.dense2_bwd_fused,
           S.dense2_bwd_small ? "D2B_SMALL" : "D2B_GEMMS");
  t += line;
  if (cap > 0) { strncpy(buf, t.c_str(), cap - 1); buf[cap - 1] = 0; }
  return (int)t.size();
}
extern "C" int crnn_ws_tensor(const crnn_config* cfg, const char* name, long* offset, long* count) {
  return crnn_ws_tensor_info(cfg, name, offset, count, nullptr);
}


namespace {
constexpr int kForkMaxDevices = 64;
// The side stream an entry point may fork to: NULL (run everything on `stream`) when the caller passed none, the same stream, or a stream on a device ordinal
// beyond the fork/join event table (round 6, ADVICE: such a box used to fail the whole step with -3)
hipStream_t side_stream(hipStream_t stream, hipStream_t aux) {
  if (!aux || aux == stream) return nullptr;
  hipDevice_t d = 0;
  if (hipStreamGetDevice(aux, &d) != hipSuccess || d < 0 || d >= kForkMaxDevices) return nullptr;
  return aux;
}
// Two streams with event links (fork: the side stream continues after everything enqueued on the main stream so far; join: the reverse)
struct ForkJoin {
  // The events are created once per (host thread, device) and reused by every call (recording an event again while an earlier
  // wait on it is still queued is well defined: the wait captured the earlier record); nothing is created or destroyed
  // on the step's path.  Keyed by the streams' device: an event belongs to the device it was created on, and a second engine on
  // another GPU driven from the same host thread must not record the first one's events on its streams (invalid resource handle).
  // The events live as long as the thread (a fixed pool of 24 per device, like the runtime's own per-device pools); they are never
  // destroyed because a wait on one of them may still be queued when the thread exits.
  // A device ordinal beyond the table (more than 64 GPUs / partitions visible to one process) does not fail the step: the fork is simply not taken
  // and the side work runs on the main stream (same results; round 6, ADVICE).
  hipStream_t main, aux; int n = 0; bool on; int dev = -1;
  static constexpr int kMaxDevices = kForkMaxDevices, kEvents = 24;
  ForkJoin(hipStream_t m, hipStream_t a) : main(m), aux(a), on(a != nullptr) {
    if (on) {   // the device the side stream lives on
      hipDevice_t d = 0;
      if (hipStreamGetDevice(aux, &d) != hipSuccess || d < 0 || d >= kMaxDevices) on = false; else dev = d;
    }
  }
  int event(int i, hipEvent_t* out) {
    static thread_local hipEvent_t ev[kMaxDevices][kEvents] = {};
    if (i >= kEvents || dev < 0) return CRNN_ERR_ARG;
    hipEvent_t& e = ev[dev][i];
    if (!e) { hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming); if (r != hipSuccess) return (int)r; }
    *out = e;
    return CRNN_OK;
  }
  int link(hipStream_t from, hipStream_t to) {   // `to` continues after everything enqueued on `from` so far
    if (!on) return CRNN_OK;
    hipEvent_t e; CRNN_TRY(event(n++, &e));
    hipError_t r = hipEventRecord(e, from); if (r != hipSuccess) return (int)r;
    r = hipStreamWaitEvent(to, e, 0); return r == hipSuccess ? CRNN_OK : (int)r;
  }
  int fork() { return link(main, aux); }
  int join() { return link(aux, main); }
  // split form of a join: mark the side stream's progress now, make the main stream wait for that point later
  int mark(hipEvent_t* e) {
    if (!on) return CRNN_OK;
    CRNN_TRY(event(n++, e));
    hipError_t r = hipEventRecord(*e, aux); return r == hipSuccess ? CRNN_OK : (int)r;
  }
  int wait(hipEvent_t e) {
    if (!on || !e) return CRNN_OK;
    hipError_t r = hipStreamWaitEvent(main, e, 0); return r == hipSuccess ? CRNN_OK : (int)r;
  }
};

}  // namespace

// ---------------------------------------------------------------------------------------------------
extern "C" int crnn_forward(const crnn_config* cfg, const float* params, const float* bn_mean, const float* bn_var,
                            const float* x, float* ws, size_t ws_bytes, float* y_pred, int train, uint64_t seed,
                            hipStream_t stream) {
  return crnn_forward_ex(cfg, params, bn_mean, bn_var, x, ws, ws_bytes, y_pred, train, seed, stream, nullptr);
}
namespace {
// one Bidirectional layer's recurrences, both directions: a persistent kernel or one launch per timestep; "cs" holds r * h_prev for the GRU (cell state for the LSTM)
int rnn_fwd(const Ctx& c, const char* layer, float* hf, float* hb, int ldh) {
  const Sched& S = c.S;
  const int T = c.d.T, B = c.d.B, u = c.d.u;
  const std::string f = std::string(layer) + "f", b = std::string(layer) + "b";
  float *xf = c.w("xw" + f), *xb = c.w("xw" + b), *uf = c.w("ut" + f), *ub = c.w("ut" + b);
  float *csf = c.w("cs" + f), *csb = c.w("cs" + b), *gtf = c.w("gt" + f), *gtb = c.w("gt" + b);
  if (!S.rnn_persist)
    return c.cfg->gru ? crnn_gru_fwd_ex(xf, xb, uf, ub, hf, hb, ldh, gtf, gtb, csf, csb, T, B, u, S.dtu, c.s)
                      : crnn_lstm_fwd_ex(xf, xb, uf, ub, hf, hb, ldh, csf, csb, gtf, gtb, T, B, u, S.dtu, c.s);
  const size_t xbytes = crnn_lstm_persist_xbuf_bytes(T, B, u, S.dtu);
  return c.cfg->gru ? crnn_gru_fwd_persist(xf, xb, uf, ub, hf, hb, ldh, gtf, gtb, csf, csb, T, B, u, S.dtu, c.w("rnnx"), xbytes, S.rnn_uw, c.s)
                    : crnn_lstm_fwd_persist(xf, xb, uf, ub, hf, hb, ldh, csf, csb, gtf, gtb, T, B, u, S.dtu, c.w("rnnx"), xbytes, 0, S.rnn_uw, c.s);
}
}  // namespace

// aux_stream != NULL (and != stream): work that nothing at the head of the forward waits for runs there next to the spatial transformer's
// small kernels -- today the dropout keep bytes of the block outputs that only exist inside the next depthwise kernels (a function of
// (seed, site, index), 0.1 ms of VALU work at batch 256), joined before block 2's depthwise kernel.  Same results.
extern "C" int crnn_forward_ex(const crnn_config* cfg, const float* params, const float* bn_mean, const float* bn_var,
                               const float* x, float* ws, size_t ws_bytes, float* y_pred, int train, uint64_t seed,
                               hipStream_t stream, hipStream_t aux_stream) {
  CRNN_TRY(check_cfg(cfg));
  const Ctx c = make_ctx(cfg, params, nullptr, ws, stream);
  if (ws_bytes < (size_t)c.P.total * sizeof(float)) return CRNN_ERR_ARG;
  const Dims& d = c.d;
  const Sched& S = c.S;
  const int B = d.B;
  const bool mfma_bf16 = cfg->mfma_bf16 != 0;
  const float drop_block = cfg->dropout ? kDropBlock : 0.f;
  aux_stream = side_stream(stream, aux_stream);
  ForkJoin fj(stream, aux_stream);
  bool keep_pending = false;
  if (train && cfg->dropout) {   // the dropout decisions of the block outputs that only exist inside the next depthwise kernels (OUT_NEXT_BLOCK)
    void* outs[CRNN_KEEP_BATCH_MAX]; long ng[CRNN_KEEP_BATCH_MAX]; uint32_t lay[CRNN_KEEP_BATCH_MAX]; int n = 0;
    for (int i = 1; i <= 6; ++i)
      if (S.b[i].out == OUT_NEXT_BLOCK) { outs[n] = c.w("dm" + std::to_string(i)); ng[n] = (long)B * d.bh[i + 1] * d.bw[i + 1] * d.bc[i] / 8; lay[n] = (uint32_t)i; ++n; }   // (block i + 1's map = block i's output, pooled or not)
    if (n) {
      CRNN_TRY(fj.fork());
      CRNN_TRY(crnn_dropout_keep_bytes_batch(n, outs, ng, lay, kDropBlock, seed, fj.on ? aux_stream : stream));
      keep_pending = fj.on;
    }
  }
  if (mfma_bf16) CRNN_TRY(crnn_convert_f32_to_bf16(params, c.ws + c.P.off("pbf"), c.L.total, stream));
  // ---- spatial transformer (utils.py:247-258) + ZeroPadding2D (utils.py:63)
  if (S.loc_fused) {   // the localisation net as one workgroup per sample (stn.hip) where a sample's maps fit
    CRNN_TRY(crnn_loc_net_fwd(x, c.p("stn_c1_k"), c.p("stn_c1_b"), c.p("stn_c2_k"), c.p("stn_c2_b"), c.p("stn_d1_w"), c.p("stn_d1_b"), c.p("stn_d2_w"),
                              c.p("stn_d2_b"), c.w("pool1"), c.w("c1"), c.w("pool2"), c.w("flat"), c.w("fc1"), c.w("theta"), B, d.H0, d.W0, stream));
    CRNN_TRY(crnn_sampler_fwd(x, c.w("theta"), c.w("x0"), B, d.H0, d.W0, 2, stream));
  } else if (cfg->stn) {
    CRNN_TRY(crnn_maxpool_fwd(x, c.w("pool1"), B, d.H0, d.W0, 1, 2, 2, stream));
    CRNN_TRY(crnn_loc_conv_fwd(c.w("pool1"), c.p("stn_c1_k"), c.p("stn_c1_b"), c.w("c1"), B, d.Hs1, d.Ws1, 1, stream));
    CRNN_TRY(crnn_maxpool_fwd(c.w("c1"), c.w("pool2"), B, d.Ho1, d.Wo1, 20, 2, 2, stream));
    CRNN_TRY(crnn_loc_conv_fwd(c.w("pool2"), c.p("stn_c2_k"), c.p("stn_c2_b"), c.w("flat"), B, d.Hs2, d.Ws2, 20, stream));
    CRNN_TRY(crnn_loc_fc_fwd(c.w("flat"), c.p("stn_d1_w"), c.p("stn_d1_b"), c.p("stn_d2_w"), c.p("stn_d2_b"), c.w("fc1"), c.w("theta"), B,
                             d.stn_flat, stream));
    CRNN_TRY(crnn_sampler_fwd(x, c.w("theta"), c.w("x0"), B, d.H0, d.W0, 2, stream));
  } else {
    CRNN_TRY(crnn_pad_copy(x, c.w("x0"), B, d.H0, d.W0, 2, stream));
  }
  if (mfma_bf16) {   // bf16 modes: W^T (bf16) copies of the pointwise weights of blocks 2..7 and of the streamed dense layers, one launch
    long in_off[8], out_off[8]; int R[8], Cc[8]; int n = 0;
    for (int i = 2; i <= 7; ++i)
      if (S.b[i].pwT_off >= 0) { in_off[n] = c.L.off("b" + std::to_string(i) + "_pw"); out_off[n] = S.b[i].pwT_off; R[n] = d.bc[i - 1]; Cc[n] = d.bc[i]; ++n; }
    if (S.dense2_stream) { in_off[n] = c.L.off("dense2_w"); out_off[n] = S.d2T_off; R[n] = 2 * d.u; Cc[n] = d.C; ++n; }   // W [2u][C] -> W^T rows 0..C-1 of a 128-row matrix
    if (S.dense1_stream) { in_off[n] = c.L.off("dense1_w"); out_off[n] = S.d1T_off; R[n] = d.feat; Cc[n] = d.tds; ++n; }   // W [feat][tds] -> W^T [tds][feat] behind it
    if (n) CRNN_TRY(crnn_transpose_batch(params, c.w("pwT"), n, in_off, out_off, R, Cc, CRNN_BF16, stream));
  }
  // ---- 7 depthwise-separable blocks (utils.py:43-56, 64-70)
  const float* in = c.w("x0");
  if (!train) {   // inference: every BatchNorm's [mean|var|scale|shift] is known before the first conv -- one launch for all 14
    const float *mm[14], *mv[14], *gg[14], *bb[14]; float* st[14]; int cc[14]; int n = 0, off = 0;
    for (int i = 1; i <= 7; ++i) {
      const std::string bp = "b" + std::to_string(i);
      for (int h = 0; h < 2; ++h) {
        const int ch = h ? d.bc[i] : d.bc[i - 1];
        mm[n] = bn_mean + off; mv[n] = bn_var + off; gg[n] = c.p(bp + (h ? "_bn2_g" : "_bn1_g")); bb[n] = c.p(bp + (h ? "_bn2_b" : "_bn1_b"));
        st[n] = c.w((h ? "bn2s" : "bn1s") + std::to_string(i)); cc[n] = ch; off += ch; ++n;
      }
    }
    CRNN_TRY(crnn_bn_infer_state_batch(n, mm, mv, gg, bb, cc, st, stream));
  }
  for (int i = 1; i <= 7; ++i) {
    std::string p = std::to_string(i), bp = "b" + p;
    const BlockSched& b = S.b[i];
    const int H = d.bh[i], W = d.bw[i], ci = d.bc[i - 1], co = d.bc[i];
    const long M = (long)B * H * W;
    float* dd = c.w("d" + p); float* aa = c.w("a" + p); float* qq = c.w("q" + p); float* xo = c.w("x" + p);
    float* s1 = c.w("bn1s" + p); float* s2 = c.w("bn2s" + p);
    float* parts = c.w("partials");
    const float* kdw = c.p(bp + "_dw"); const float* kpw = c.p(bp + "_pw");
    const int dtd = b.dtd, dtq = b.dtq;
    const int ph = kBlocks[i - 1].ph, pw = kBlocks[i - 1].pw;
    const PwWeights wq = pw_weights(c, i);
    if (!train) {
      // inference (learning_phase 0): the BatchNorm scale/shift are known up front, so BN + ReLU6 fold into the
      // epilogue of the conv that feeds them -- the depthwise kernel writes `a` directly and, when the block has no
      // pooling (or pools in the GEMM epilogue: the un-pooled map q never exists), the pointwise GEMM writes the block output directly
      switch (b.inf_dw) {
        case DWI_STREAM: CRNN_TRY(crnn_dwconv3x3_fwd_stream_ex(in, kdw, aa, nullptr, s1, B, H, W, ci, 0, b.pool_rows == 4 ? 1 : 0, stream)); break;
        case DWI_FOLDED: CRNN_TRY(crnn_dwconv3x3_bn_relu6_fwd(in, kdw, s1, aa, B, H, W, ci, dtd, stream)); break;
        default:
          CRNN_TRY(crnn_dwconv3x3_fwd_ex(in, kdw, dd, nullptr, B, H, W, ci, 0, dtd, stream));
          CRNN_TRY(crnn_bn_act_pool_drop_ex(dd, s1, aa, 1, 1, (int)M, ci, 1, 1, 0.f, 0, 0, dtd, dtd, stream));
      }
      const bool fold = b.inf_fold;
      if (b.inf_pw == PWI_ONE) CRNN_TRY(fold ? crnn_pw1_fwd_folded(aa, kpw, xo, M, co, s2, dtq, stream) : crnn_pw1_fwd(aa, kpw, qq, M, co, nullptr, dtq, stream));
      else if (b.pool_rows > 1) CRNN_TRY(crnn_pwconv_fwd_wres_folded_pool(aa, wq.w, xo, M, co, ci, s2, b.pool_rows, stream));
      else if (b.inf_pw == PWI_WRES)   // bf16 tensors + W^T: the weights-resident kernel (folded BatchNorm in its MFMA waves' epilogue, or the plain product)
        CRNN_TRY(fold ? crnn_pwconv_fwd_wres_folded(aa, wq.w, xo, M, co, ci, s2, stream) : crnn_gemm_wres_bf16(aa, wq.w, qq, (int)M, co, ci, stream));
      else CRNN_TRY(crnn_pwconv_fwd(aa, wq.w, fold ? xo : qq, M, co, ci, nullptr, fold ? s2 : nullptr, S.products_fwd, dtd, wq.dt, dtq, wq.transposed, stream));
      if (!fold) CRNN_TRY(crnn_bn_act_pool_drop_ex(qq, s2, xo, B, H, W, co, ph, pw, 0.f, seed, (uint32_t)i, dtq, b.dtx, stream));
      in = xo;
      continue;
    }
    // depthwise conv; its epilogue also produces the batch statistics of BatchNorm-1
    const float* g1 = c.p(bp + "_bn1_g"); const float* b1 = c.p(bp + "_bn1_b");
    switch (b.dw) {
      case DWF_PRO:   // the previous block's output was not materialised: its BatchNorm-2 + ReLU6 + dropout run inside this depthwise kernel
        if (keep_pending) { CRNN_TRY(fj.join()); keep_pending = false; }   // the keep bytes are complete
        CRNN_TRY(crnn_dwconv3x3_fwd_stream_pro_ex(pro_src(c, i - 1), c.w("bn2s" + std::to_string(i - 1)), drop_block, keep_bytes(c, i - 1), kdw, dd, parts, B, H, W, ci, dtd, stream));
        break;
      case DWF_STREAM: CRNN_TRY(crnn_dwconv3x3_fwd_stream_dt(in, kdw, dd, parts, B, H, W, ci, 0, dtd, stream)); break;
      case DWF_TILE_STATS: CRNN_TRY(crnn_dwconv3x3_fwd_ex(in, kdw, dd, parts, B, H, W, ci, 0, dtd, stream)); break;
      case DWF_C1: CRNN_TRY(crnn_dwconv3x3_c1_fwd(in, kdw, dd, parts, B, H, W, stream)); break;   // block 1: the one-channel kernel takes its own statistics
      default:
        CRNN_TRY(crnn_dwconv3x3_fwd_ex(in, kdw, dd, nullptr, B, H, W, ci, 0, dtd, stream));
        CRNN_TRY(crnn_colreduce_ex(dd, parts, M, ci, ci, 2, dtd, stream));
    }
    if (b.dw == DWF_C1 || b.dw == DWF_TILE_COLREDUCE) CRNN_TRY(crnn_bn_finalize(parts, b.dw_rows, ci, M, g1, b1, s1, stream));
    else CRNN_TRY(crnn_bn_finalize_folded(parts, b.dw_rows, ci, M, g1, b1, s1, c.w("fold"), stream));
    if (b.bn1 == BN1_PASS) CRNN_TRY(crnn_bn_act_pool_drop_ex(dd, s1, aa, 1, 1, (int)M, ci, 1, 1, 0.f, 0, 0, dtd, dtd, stream));
    // pointwise conv; its epilogue also produces the batch statistics of BatchNorm-2
    switch (b.pw) {
      case PWF_PW1_BN: CRNN_TRY(crnn_pw1_bn_fwd(dd, s1, kpw, qq, M, co, parts, dtq, stream)); break;   // block 1: outer product of relu6(BN(d))
      case PWF_PW1: CRNN_TRY(crnn_pw1_fwd(aa, kpw, qq, M, co, parts, dtq, stream)); break;
      case PWF_WRES3:   // the weights' planes resident in registers, the pixel rows streamed once (gemm_wres3.hip)
        CRNN_TRY(crnn_pwconv_bnrelu6_fwd_wres3(dd, s1, kpw, qq, M, co, ci, S.planes_fwd, parts, stream)); break;
      case PWF_PLANES_TILE:   // the tile kernel, splitting the weights while staging
        CRNN_TRY((S.planes_fwd == 2 ? crnn_pwconv_bnrelu6_fwd_f32x2 : crnn_pwconv_bnrelu6_fwd_f32x3)(dd, s1, kpw, qq, M, co, ci, parts, stream)); break;
      case PWF_WRES:   // weights resident in registers, IO waves transform / drain / take the statistics (gemm_wres.hip)
        CRNN_TRY(crnn_pwconv_bnrelu6_fwd_wres(dd, s1, wq.w, qq, M, co, ci, parts, stream)); break;
      case PWF_BNRELU6_TILE: CRNN_TRY(crnn_pwconv_bnrelu6_fwd(dd, s1, wq.w, qq, M, co, ci, parts, dtq, wq.transposed, stream)); break;
      default: CRNN_TRY(crnn_pwconv_fwd(aa, wq.w, qq, M, co, ci, parts, nullptr, S.products_fwd, dtd, wq.dt, dtq, wq.transposed, stream));
    }
    CRNN_TRY(crnn_bn_finalize_folded(parts, b.pw_rows, co, M, c.p(bp + "_bn2_g"), c.p(bp + "_bn2_b"), s2, c.w("fold"), stream));
    switch (b.out) {
      case OUT_NEXT_BLOCK:   // x_i is formed by block i+1's depthwise kernel from q_i (and again by its backward): not written
        if (ph * pw != 1)    // pooled: from q at each window's arg-max, which one pass over q selects (no BatchNorm output is written)
          CRNN_TRY(crnn_bn_act_pool_drop_qmax_ex(qq, s2, nullptr, pro_src(c, i), B, H, W, co, ph, pw, 0.f, seed, (uint32_t)i, dtq, dtq, stream));
        in = nullptr;
        break;
      case OUT_QMAX:
        CRNN_TRY(crnn_bn_act_pool_drop_qmax_ex(qq, s2, xo, c.w("qm" + p), B, H, W, co, ph, pw, drop_block, seed, (uint32_t)i, dtq, b.dtx, stream));
        in = xo;
        break;
      default:
        CRNN_TRY(crnn_bn_act_pool_drop_ex(qq, s2, xo, B, H, W, co, ph, pw, drop_block, seed, (uint32_t)i, dtq, b.dtx, stream));
        in = xo;
    }
  }
  if (keep_pending) { CRNN_TRY(fj.join()); keep_pending = false; }
  // ---- Reshape + dense1 (relu) + Dropout(.4) (utils.py:72-75); output time-major [T][B][tds]
  const int T = d.T, TB = T * B, u = d.u, G = d.G;
  const bf16_t* pwT = reinterpret_cast<const bf16_t*>(c.w("pwT"));
  if (S.dense1_fwd_stream)   // the 64-row stripe stream (gemm_wgrad.hip): x7 bf16 against a bf16 W1^T, bias + ReLU + the rows to time-major + Dropout(.4) in the epilogue
    CRNN_TRY(crnn_dense_fwd_stream(in, pwT + S.d1T_off, c.p("dense1_b"), c.w("dn1"), TB, d.tds, d.feat, d.feat, d.feat, 1, T,
                                   (train && cfg->dropout) ? kDropDense1 : 0.f, seed, kLayerDense1, stream));
  else {
    CRNN_TRY(gemm_t(c, 0, in, S.b[7].dtx, c.p("dense1_w"), CRNN_F32, c.w("dn1"), CRNN_F32, TB, d.tds, d.feat, d.feat, d.tds, d.tds, c.p("dense1_b"), 1, 0, T));
    if (train && cfg->dropout) CRNN_TRY(crnn_dropout(c.w("dn1"), c.w("dn1"), TB, d.tds, d.tds, d.tds, kDropDense1, seed, kLayerDense1, stream));
  }
  // ---- 2 x Bidirectional(LSTM) (utils.py:78-79)
  // bf16 modes: the recurrent products run on the bf16 MFMA from a bf16 U^T (u % 128 == 0); parity mode: fp32.  bf16 U^T: the input projections stream
  // too (64-row stripes of X against a bf16 W^T through LDS, gemm_wgrad.hip) unless the tile schedule is asked for
  {  // U -> U^T for the four recurrences (and W -> W^T for the streamed input projections), one launch
    long in_off[8], out_off[8]; int R[8], Cc[8]; int n = 0;
    const char* names[4] = {"1f", "1b", "2f", "2b"};
    const long esz = (S.dtu == CRNN_BF16) ? 2 : 4;
    for (const char* nm : names) {
      in_off[n] = c.L.off(std::string("rnn") + nm + "_u");
      // element offset of ut<nm> from ut1f in the destination type (the workspace offsets are in floats)
      out_off[n] = (c.P.off(std::string("ut") + nm) - c.P.off("ut1f")) * 4 / esz;
      R[n] = u; Cc[n] = G; ++n;
    }
    if (S.xw_stream)
      for (const char* nm : names) {
        in_off[n] = c.L.off(std::string("rnn") + nm + "_w");
        out_off[n] = (c.P.off(std::string("wt") + nm) - c.P.off("ut1f")) * 4 / esz;
        R[n] = nm[0] == '1' ? d.tds : u; Cc[n] = G; ++n;
      }
    CRNN_TRY(crnn_transpose_batch(params, c.w("ut1f"), n, in_off, out_off, R, Cc, S.dtu, stream));
  }
  auto xw = [&](const float* xin, int din, const std::string& s, bool stripes) -> int {
    if (stripes)
      return crnn_gemm_nt_f32_stream_bias(xin, c.w("wt" + s), nullptr, nullptr, c.w("xw" + s), c.p("rnn" + s + "_b"), TB, G, din, din, din, G, stream);
    return gemm(c, 0, xin, c.p("rnn" + s + "_w"), c.w("xw" + s), TB, G, din, din, G, G, c.p("rnn" + s + "_b"));
  };
  // both directions of a layer in one launch of persistent workgroups (crnn_rnn_input_proj; bit-identical to the two stripe launches)
  auto xw2 = [&](const float* xin, int din, int layer) -> int {
    const std::string f = std::to_string(layer) + "f", b = std::to_string(layer) + "b";
    if (S.xw[layer - 1] == XW_BOTH)
      return crnn_rnn_input_proj(xin, c.w("wt" + f), c.w("wt" + b), c.p("rnn" + f + "_b"), c.p("rnn" + b + "_b"), c.w("xw" + f), c.w("xw" + b), TB, G, din, din, din, G, stream);
    CRNN_TRY(xw(xin, din, f, S.xw[layer - 1] == XW_STRIPES));
    return xw(xin, din, b, S.xw[layer - 1] == XW_STRIPES);
  };
  CRNN_TRY(xw2(c.w("dn1"), d.tds, 1));
  CRNN_TRY(rnn_fwd(c, "1", c.w("h1f"), c.w("h1b"), u));
  CRNN_TRY(crnn_add(c.w("h1f"), c.w("h1b"), c.w("r1"), (long)TB * u, stream));  // merge_mode='sum'
  CRNN_TRY(xw2(c.w("r1"), u, 2));
  CRNN_TRY(rnn_fwd(c, "2", c.w("h2"), c.w("h2") + u, 2 * u));                    // merge_mode='concat'
  const float* r2 = c.w("h2");
  if (train) {  // Dropout(.2) (utils.py:83)
    // dense2's one-pass backward reads the decisions as keep bytes: written with the dropped activations in one pass, else by a pass of their own
    if (S.drop_keep_fused) CRNN_TRY(crnn_dropout_keep(c.w("h2"), c.w("r2d"), c.w("keep9"), TB, 2 * u, 2 * u, 2 * u, kDropRnn, seed, kLayerRnn, stream));
    else {
      CRNN_TRY(crnn_dropout(c.w("h2"), c.w("r2d"), TB, 2 * u, 2 * u, 2 * u, cfg->dropout ? kDropRnn : 0.f, seed, kLayerRnn, stream));
      if (cfg->dropout && S.dense2_bwd_fused) CRNN_TRY(crnn_dropout_keep_bytes(c.w("keep9"), (long)TB * 2 * u / 8, kDropRnn, seed, kLayerRnn, stream));
    }
    r2 = c.w("r2d");
  }
  // ---- dense2 + softmax (utils.py:85-86); back to batch-major [B][T][C]
  // round 5: the product on the streaming kernel (64-row stripes against the 128-row padded bf16 W^T through LDS; the tile GEMM ran 104 workgroups for 35 us), bias +
  // row permutation + softmax + the y_pred copy in one pass over its output: dropout aside, four launches (56 us) -> two (18 us)
  if (S.dense2_fwd_stream) {
    CRNN_TRY(crnn_gemm_nt_f32_stream_bias(r2, pwT + S.d2T_off, nullptr, nullptr, c.w("lg128"), nullptr, TB, 128, 2 * u, 2 * u, 2 * u, 128, stream));
    return crnn_softmax_rows_perm(c.w("lg128"), 128, c.p("dense2_b"), c.w("logits"), c.w("ypred"), y_pred, TB, d.C, B, stream);   // (writes y_pred too)
  }
  CRNN_TRY(gemm(c, 0, r2, c.p("dense2_w"), c.w("logits"), TB, d.C, 2 * u, 2 * u, d.C, d.C, c.p("dense2_b"), 0, 0, B));
  CRNN_TRY(crnn_softmax_rows(c.w("logits"), c.w("ypred"), TB, d.C, stream));
  if (y_pred && y_pred != c.w("ypred")) {
    hipError_t e = hipMemcpyAsync(y_pred, c.w("ypred"), (size_t)TB * d.C * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return (int)e;
  }
  return CRNN_OK;
}

// ---------------------------------------------------------------------------------------------------
// One Bidirectional layer's backward in three pieces so that the caller can put the weight-gradient GEMMs on a second
// stream: (1) the BPTT chain (T dependent step launches, latency-bound), (2) dW/dU/db from the finished dz (throughput
// work nobody downstream of the chain waits for), (3) dX = dZ W^T (what the layer below needs).
// Sched::rnn_bwd_persist: the persistent backward of the layer runs and leaves the bias-gradient partials "dbp<layer>f/b", which rnn_bwd_wgrads sums
// instead of reading dz once more (LSTM or GRU: whichever cell the configuration has)
static int rnn_bwd_chain(const Ctx& c, int layer, const float* hf, const float* hb, int ldh, const float* doutf, const float* doutb, int ldo) {
  const Dims& d = c.d;
  const int T = d.T, B = d.B, u = d.u;
  std::string l = std::to_string(layer);
  float* dzf = c.w("dz" + l + "f"); float* dzb = c.w("dz" + l + "b");
  float *gtf = c.w("gt" + l + "f"), *gtb = c.w("gt" + l + "b"), *csf = c.w("cs" + l + "f"), *csb = c.w("cs" + l + "b");
  // bf16 modes: U is read from the bf16 shadow of the parameter buffer (refreshed by the forward)
  int dtu = CRNN_F32;
  const float* uf = rnn_u_operand(c, l + "f", &dtu); const float* ub = rnn_u_operand(c, l + "b", &dtu);
  if (!c.S.rnn_bwd_persist[layer - 1])
    return c.cfg->gru ? crnn_gru_bwd_ex(uf, ub, hf, hb, ldh, gtf, gtb, doutf, doutb, ldo, dzf, dzb, c.w("dcf"), c.w("dcb"), c.w("dhpf"), c.w("dhpb"), T, B, u, dtu, c.s)
                      : crnn_lstm_bwd_ex(uf, ub, csf, csb, gtf, gtb, doutf, doutb, ldo, dzf, dzb, c.w("dcf"), c.w("dcb"), T, B, u, dtu, c.s);
  const size_t xbytes = crnn_lstm_persist_xbuf_bytes(T, B, u, dtu);
  float *dbf = c.w("dbp" + l + "f"), *dbb = c.w("dbp" + l + "b");
  return c.cfg->gru ? crnn_gru_bwd_persist_db(uf, ub, hf, hb, ldh, gtf, gtb, doutf, doutb, ldo, dzf, dzb, dbf, dbb, T, B, u, dtu, c.w("rnnx"), xbytes, c.S.rnn_uw, c.s)
                    : crnn_lstm_bwd_persist_db(uf, ub, csf, csb, gtf, gtb, doutf, doutb, ldo, dzf, dzb, dbf, dbb, T, B, u, dtu, c.w("rnnx"), xbytes, 0, c.S.rnn_uw, c.s);
}
// C[M][N] = A^T B over K rows (weight gradients of the recurrent layers): the streaming kernel in the bf16 modes (gemm_wgrad.hip, fp32 operands rounded to
// bf16 on the way in like the tile GEMM does), the pixel-stream form of the two-plane weight gradient in the parity mode (gemm_wgrad3.hip), else the tile GEMM
static int gemm_tn(const Ctx& c, int kernel, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc) {
  switch (kernel) {
    case TN_STREAM: return crnn_gemm_tn_stream(A, lda, B, ldb, C, ldc, M, N, K, c.scratch(), kGemmScratchBytes, c.s);
    case TN_PLANES_STREAM: return crnn_gemm_tn_planes_stream(A, lda, B, ldb, C, ldc, M, N, K, c.scratch(), kGemmScratchBytes, c.s);
    default: return gemm(c, 2, A, B, C, M, N, K, lda, ldb, ldc, nullptr, 0, 0, 0, c.S.planes_bwd);
  }
}
static int rnn_bwd_wgrads(const Ctx& c, int layer, const float* xin, int ldx, int din, const float* hf, const float* hb, int ldh) {
  const Dims& d = c.d;
  const Sched& S = c.S;
  const int T = d.T, B = d.B, TB = T * B, u = d.u, G = d.G;
  std::string l = std::to_string(layer);
  float* dzf = c.w("dz" + l + "f"); float* dzb = c.w("dz" + l + "b");
  // dW = X^T dZ ; dU = Hprev^T dZ ; db = colsum(dZ)
  CRNN_TRY(gemm_tn(c, S.rnn_dw[layer - 1], xin, dzf, c.g("rnn" + l + "f_w"), din, G, TB, ldx, G, G));
  CRNN_TRY(gemm_tn(c, S.rnn_dw[layer - 1], xin, dzb, c.g("rnn" + l + "b_w"), din, G, TB, ldx, G, G));
  const int K1 = (T - 1) * B;
  // forward direction: h_{t-1} pairs with dz_t ; backward direction: h_{t+1} pairs with dz_t
  const int Nh = c.cfg->gru ? 2 * u : G;   // GRU: only the z,r columns see h_prev; the candidate sees r*h_prev
  CRNN_TRY(gemm_tn(c, S.rnn_du[layer - 1][0], hf, dzf + (long)B * G, c.g("rnn" + l + "f_u"), u, Nh, K1, ldh, G, G));
  CRNN_TRY(gemm_tn(c, S.rnn_du[layer - 1][1], hb + (long)B * ldh, dzb, c.g("rnn" + l + "b_u"), u, Nh, K1, ldh, G, G));
  if (c.cfg->gru) {
    CRNN_TRY(gemm(c, 2, c.w("cs" + l + "f"), dzf + 2 * u, c.g("rnn" + l + "f_u") + 2 * u, u, u, TB, u, G, G, nullptr, 0, 0, 0, c.S.planes_bwd));
    CRNN_TRY(gemm(c, 2, c.w("cs" + l + "b"), dzb + 2 * u, c.g("rnn" + l + "b_u") + 2 * u, u, u, TB, u, G, G, nullptr, 0, 0, 0, c.S.planes_bwd));
  }
  if (c.S.rnn_bwd_persist[layer - 1]) {    // the persistent backward summed dz over time per 16-row batch tile: the tiles in a fixed order
    CRNN_TRY(crnn_partials_sum(c.w("dbp" + l + "f"), crnn_rnn_db_rows(B), G, c.g("rnn" + l + "f_b"), 1.f, c.s));
    return crnn_partials_sum(c.w("dbp" + l + "b"), crnn_rnn_db_rows(B), G, c.g("rnn" + l + "b_b"), 1.f, c.s);
  }
  CRNN_TRY(colsum(c, dzf, TB, G, G, c.g("rnn" + l + "f_b")));
  return colsum(c, dzb, TB, G, G, c.g("rnn" + l + "b_b"));
}
static int rnn_bwd_dx(const Ctx& c, int layer, int din, float* dxin) {
  const Dims& d = c.d;
  const int TB = d.T * d.B, G = d.G;
  std::string l = std::to_string(layer);
  float *dzf = c.w("dz" + l + "f"), *dzb = c.w("dz" + l + "b");
  const float *wf = c.p("rnn" + l + "f_w"), *wb = c.p("rnn" + l + "b_w");
  // both directions in one stripe-stream launch: bf16 modes (gemm_wgrad.hip, the weights' bf16 shadows) / parity mode, two-plane backward (gemm_wgrad3.hip)
  switch (c.S.rnn_dx[layer - 1]) {
    case DX_STREAM_BF16: {
      int dtf = CRNN_F32, dtb = CRNN_F32;
      const float* sf = weight_operand(c, 1, wf, &dtf);
      const float* sb = weight_operand(c, 1, wb, &dtb);
      return crnn_gemm_nt_f32_stream(dzf, sf, dzb, sb, dxin, TB, din, G, G, G, din, c.s);
    }
    case DX_PLANES_STREAM: return crnn_gemm_nt_f32x2_stream(dzf, wf, dzb, wb, dxin, TB, din, G, G, G, din, c.s);
    default:
      CRNN_TRY(gemm(c, 1, dzf, wf, dxin, TB, din, G, G, G, din, nullptr, 0, 0, 0, c.S.planes_bwd));
      return gemm(c, 1, dzb, wb, dxin, TB, din, G, G, G, din, nullptr, 0, 1, 0, c.S.planes_bwd);
  }
}

// The backward runs in two stages so that a data-parallel host can start the gradient all-reduce of the upper
// layers (dense1, the recurrent layers, dense2: the tail of the flat buffer, 75 % of its bytes) while the
// conv-stack / STN stage is still running.
namespace {
int backward_top(const Ctx& c, const int* labels, const int* input_length, const int* label_length, float* loss, uint64_t seed, hipStream_t aux);
int backward_bottom(const Ctx& c, const float* x, uint64_t seed, hipStream_t aux);
// top / bottom: which stages run; aux: the side stream (NULL: none)
int backward_stages(const crnn_config* cfg, const float* params, float* grads, const float* x, const int* labels, const int* input_length, const int* label_length,
                    float* ws, size_t ws_bytes, float* loss, uint64_t seed, hipStream_t stream, hipStream_t aux, bool top, bool bottom) {
  CRNN_TRY(check_cfg(cfg));
  const Ctx c = make_ctx(cfg, params, grads, ws, stream);
  if (ws_bytes < (size_t)c.P.total * sizeof(float)) return CRNN_ERR_ARG;
  aux = side_stream(stream, aux);
  if (top) CRNN_TRY(backward_top(c, labels, input_length, label_length, loss, seed, aux));
  return bottom ? backward_bottom(c, x, seed, aux) : CRNN_OK;
}
}  // namespace
extern "C" long crnn_grad_split_offset(const crnn_config* cfg) { return make_layout(cfg).off("dense1_w"); }
extern "C" int crnn_backward_top_ex(const crnn_config* cfg, const float* params, float* grads, const int* labels,
                                    const int* input_length, const int* label_length, float* ws, size_t ws_bytes, float* loss,
                                    uint64_t seed, hipStream_t stream, hipStream_t aux_stream) {
  return backward_stages(cfg, params, grads, nullptr, labels, input_length, label_length, ws, ws_bytes, loss, seed, stream, aux_stream, true, false);
}
extern "C" int crnn_backward_top(const crnn_config* cfg, const float* params, float* grads, const int* labels,
                                 const int* input_length, const int* label_length, float* ws, size_t ws_bytes, float* loss,
                                 uint64_t seed, hipStream_t stream) {
  return crnn_backward_top_ex(cfg, params, grads, labels, input_length, label_length, ws, ws_bytes, loss, seed, stream, nullptr);
}
extern "C" int crnn_backward_bottom_ex(const crnn_config* cfg, const float* params, float* grads, const float* x, float* ws,
                                       size_t ws_bytes, uint64_t seed, hipStream_t stream, hipStream_t aux_stream) {
  return backward_stages(cfg, params, grads, x, nullptr, nullptr, nullptr, ws, ws_bytes, nullptr, seed, stream, aux_stream, false, true);
}
extern "C" int crnn_backward_bottom(const crnn_config* cfg, const float* params, float* grads, const float* x, float* ws,
                                    size_t ws_bytes, uint64_t seed, hipStream_t stream) {
  return crnn_backward_bottom_ex(cfg, params, grads, x, ws, ws_bytes, seed, stream, nullptr);
}
extern "C" int crnn_backward_ex(const crnn_config* cfg, const float* params, float* grads, const float* x, const int* labels,
                                const int* input_length, const int* label_length, float* ws, size_t ws_bytes, float* loss,
                                uint64_t seed, hipStream_t stream, hipStream_t aux_stream) {
  return backward_stages(cfg, params, grads, x, labels, input_length, label_length, ws, ws_bytes, loss, seed, stream, aux_stream, true, true);
}
extern "C" int crnn_backward(const crnn_config* cfg, const float* params, float* grads, const float* x, const int* labels,
                             const int* input_length, const int* label_length, float* ws, size_t ws_bytes, float* loss,
                             uint64_t seed, hipStream_t stream) {
  return crnn_backward_ex(cfg, params, grads, x, labels, input_length, label_length, ws, ws_bytes, loss, seed, stream, nullptr);
}

namespace {
// aux != nullptr: a second stream takes the weight-gradient GEMMs that nothing on the critical path waits for (dense2's
// during the layer-2 BPTT chain, layer 2's during the layer-1 chain).  The chains are T dependent launches of a few
// microseconds each and leave the GPU almost idle; the GEMMs fill it.  Only the aux stream touches the split-reduction
// scratch and the reduction partials between the fork and the join, and every gradient tensor still has a single
// writer in a fixed order, so the result is bit-identical to the serial schedule.
int backward_top(const Ctx& c, const int* labels, const int* input_length, const int* label_length, float* loss, uint64_t seed, hipStream_t aux) {
  const crnn_config* cfg = c.cfg; float* grads = c.grads; hipStream_t stream = c.s;
  const Dims& d = c.d;
  const Sched& S = c.S;
  const int B = d.B, T = d.T, TB = T * B, u = d.u, planes = S.planes_bwd;
  ForkJoin fj(stream, aux);
  Ctx ca = c; if (aux) { ca.s = aux; ca.side = true; }   // same tensors, side stream, its own reduction scratch
  hipError_t e = hipMemsetAsync(grads, 0, (size_t)c.L.total * sizeof(float), stream);
  if (e != hipSuccess) return (int)e;
  // ---- CTC (utils.py:98-103): loss per sample + d mean(loss)/d logits (time-major)
  CRNN_TRY(crnn_ctc_loss_grad(c.w("ypred"), labels, input_length, label_length, loss, c.w("dlogits"), B, T, d.C, d.L, 2, 1.0f / (float)B, stream));
  // ---- dense2: weight / bias gradients on the side stream, the data gradient feeds the recurrent layers
  const float* r2 = c.w("r2d");
  if (S.dense2_bwd_small)   // one pass over r2 / dlogits: dW, db, and the data gradient with the forward's dropout multiplier (dense.hip, weights in registers)
    CRNN_TRY(crnn_dense_bwd_small(r2, c.w("dlogits"), c.p("dense2_w"), c.w("dr2"), c.g("dense2_w"), c.g("dense2_b"), c.w("d2part"),
                                  (size_t)c.P.cnt("d2part") * sizeof(float), TB, 2 * u, d.C, 2 * u, 2 * u, cfg->dropout ? c.w("keep9") : nullptr,
                                  cfg->dropout ? kDropRnn : 0.f, seed, kLayerRnn, stream));
  CRNN_TRY(fj.fork());
  if (!S.dense2_bwd_small) {
    CRNN_TRY(gemm(ca, 2, r2, c.w("dlogits"), c.g("dense2_w"), 2 * u, d.C, TB, 2 * u, d.C, d.C, nullptr, 0, 0, 0, planes));
    CRNN_TRY(colsum(ca, c.w("dlogits"), TB, d.C, d.C, c.g("dense2_b")));
    CRNN_TRY(gemm(c, 1, c.w("dlogits"), c.p("dense2_w"), c.w("dr2"), TB, 2 * u, d.C, d.C, d.C, 2 * u, nullptr, 0, 0, 0, planes));
    if (cfg->dropout) CRNN_TRY(crnn_dropout(c.w("dr2"), c.w("dr2"), TB, 2 * u, 2 * u, 2 * u, kDropRnn, seed, kLayerRnn, stream));
  }
  // ---- Bidirectional LSTM / GRU x2
  CRNN_TRY(rnn_bwd_chain(c, 2, c.w("h2"), c.w("h2") + u, 2 * u, c.w("dr2"), c.w("dr2") + u, 2 * u));
  CRNN_TRY(fj.fork());                               // dz of layer 2 is complete: its weight gradients go to the side stream
  CRNN_TRY(rnn_bwd_wgrads(ca, 2, c.w("r1"), u, u, c.w("h2"), c.w("h2") + u, 2 * u));
  CRNN_TRY(rnn_bwd_dx(c, 2, u, c.w("dr1")));
  CRNN_TRY(rnn_bwd_chain(c, 1, c.w("h1f"), c.w("h1b"), u, c.w("dr1"), c.w("dr1"), u));
  CRNN_TRY(fj.join());                               // the scratch buffers are the main stream's again
  CRNN_TRY(rnn_bwd_wgrads(c, 1, c.w("dn1"), d.tds, d.tds, c.w("h1f"), c.w("h1b"), u));
  CRNN_TRY(rnn_bwd_dx(c, 1, d.tds, c.w("ddn1")));
  // ---- Dropout(.4) + relu of dense1, rows back to batch-major
  // (bf16 tensors: both of dense1's backward GEMMs read a bf16 copy of its output gradient)
  CRNN_TRY(crnn_relu_bwd_ex(c.w("dn1"), c.w("ddn1"), c.w("gbm"), S.dense1_gbm16 ? c.w("gbm16") : nullptr, TB, d.tds, cfg->dropout ? 1.0f / (1.0f - kDropDense1) : 1.0f, B, stream));
  const float* feat = c.w("x7");
  // weight gradient on the pixel streams, 36 feature tiles x 7 row ranges: both operands bf16 (gemm_wgrad.hip) / parity mode, two-plane backward (gemm_wgrad3.hip)
  switch (S.dense1_wgrad) {
    case TN_STREAM_BF16: CRNN_TRY(crnn_gemm_tn_bf16_stream(feat, d.feat, c.w("gbm16"), d.tds, c.g("dense1_w"), d.tds, d.feat, d.tds, TB, c.scratch(), kGemmScratchBytes, stream)); break;
    case TN_PLANES_STREAM: CRNN_TRY(crnn_gemm_tn_planes_stream(feat, d.feat, c.w("gbm"), d.tds, c.g("dense1_w"), d.tds, d.feat, d.tds, TB, c.scratch(), kGemmScratchBytes, stream)); break;
    default: CRNN_TRY(gemm_t(c, 2, feat, S.b[7].dtx, c.w("gbm"), CRNN_F32, c.g("dense1_w"), CRNN_F32, d.feat, d.tds, TB, d.feat, d.tds, d.tds, nullptr, 0, 0, 0, planes));
  }
  CRNN_TRY(colsum(c, c.w("gbm"), TB, d.tds, d.tds, c.g("dense1_b")));
  // data gradient gA [T*B][feat] = gbm [T*B][tds] . W1^T: the weights-resident GEMM (gemm_wres.hip) against the bf16 shadow of W1, or the tile GEMM
  if (S.dense1_dgrad_wres) return crnn_gemm_wres_bf16(c.w("gbm16"), reinterpret_cast<const bf16_t*>(c.w("pbf")) + c.L.off("dense1_w"), c.w("gA"), TB, d.feat, d.tds, stream);
  return gemm_t(c, 1, c.w("gbm"), CRNN_F32, c.p("dense1_w"), CRNN_F32, c.w("gA"), c.gdt(), TB, d.feat, d.tds, d.tds, d.tds, d.feat, nullptr, 0, 0, 0, planes);
}

// aux != nullptr: the pointwise weight-gradient GEMM of every block runs on the side stream next to the rest of the block's
// backward (data-gradient GEMM, BatchNorm statistics pass, fused depthwise stage -- HBM- and VALU-bound kernels that leave the
// matrix cores and most of the vector-memory path idle).  The GEMM reads the BatchNorm-2 input gradient of its block, so the
// gradient buffers rotate over three allocations and the main stream waits for GEMM i before the buffer it reads is written
// again (by the depthwise stage of block i-1).  One writer per gradient tensor, fixed order: bit-identical to the serial schedule.
int backward_bottom(const Ctx& c, const float* x, uint64_t seed, hipStream_t aux) {
  const crnn_config* cfg = c.cfg; hipStream_t stream = c.s;
  const Dims& d = c.d;
  const Sched& S = c.S;
  const int B = d.B, planes = S.planes_bwd;
  const float drop_block = cfg->dropout ? kDropBlock : 0.f;
  ForkJoin fj(stream, aux);
  Ctx ca = c; if (aux) { ca.s = aux; ca.side = true; }
  float* gA = c.w("gA"); float* gB = c.w("gB"); float* gC = c.w("gC");   // gA holds d loss / d x7 (written by backward_top)
  float* parts = c.w("partials"); float* coef = c.w("coef");
  hipEvent_t gB_free = nullptr, gC_free = nullptr;     // side-stream GEMMs still reading gB / gC (null: none)
  // ---- conv stack
  for (int i = 7; i >= 1; --i) {
    std::string p = std::to_string(i), bp = "b" + p;
    const BlockSched& b = S.b[i];
    const int H = d.bh[i], W = d.bw[i], ci = d.bc[i - 1], co = d.bc[i], ph = kBlocks[i - 1].ph, pw = kBlocks[i - 1].pw;
    const long M = (long)B * H * W;
    const int dtd = b.dtd, dtq = b.dtq;   // dtq == storage of the incoming gradient (gdt)
    float* dd = c.w("d" + p); float* qq = c.w("q" + p); float* s1 = c.w("bn1s" + p); float* s2 = c.w("bn2s" + p);
    const float* kdw = c.p(bp + "_dw"); const float* kpw = c.p(bp + "_pw");
    float* gpw = c.g(bp + "_pw"); float* g1g = c.g(bp + "_bn1_g"); float* g1b = c.g(bp + "_bn1_b"); float* g2g = c.g(bp + "_bn2_g"); float* g2b = c.g(bp + "_bn2_b");
    // ---- BatchNorm-2 + ReLU6 (+ pool, dropout) backward: gA -> dq in gB.  dq_planes (parity mode, two-plane backward): dq -- read only by this block's two pointwise
    // GEMMs -- is WRITTEN as its two bf16 planes (the bytes of the fp32 tensor), so that neither GEMM splits it: the data gradient runs from the planes by LDS-DMA
    // with the weight planes resident (gemm_pres.hip), the weight gradient's IO waves copy them (gemm_wgrad3.hip).  Same words, same products.
    CRNN_TRY(fj.wait(gB_free)); gB_free = nullptr;        // gB is written next
    switch (b.bn2_bwd) {
      case BN2_APPLY:   // the depthwise-stage backward of block i+1 took this BatchNorm's statistics pass: finalize, then pass 2 alone
        CRNN_TRY(crnn_bn_bwd_finalize(c.w("bn2parts"), b.bn2_rows, co, M, g2g, g2b, coef, stream));
        if (b.dq_planes) CRNN_TRY(crnn_bn_bwd_apply_planes_ex(qq, gA, s2, coef, gB, M * co, 2, B, H, W, co, ph, pw, drop_block, seed, (uint32_t)i, stream));
        else CRNN_TRY(crnn_bn_bwd_apply_ex(qq, gA, s2, coef, gB, B, H, W, co, ph, pw, drop_block, seed, (uint32_t)i, dtq, stream));
        break;
      case BN2_QMAX:    // pooled block: the statistics pass reads the forward's arg-max values
        CRNN_TRY(crnn_bn_bwd_qmax_ex(qq, c.w("qm" + p), gA, s2, c.p(bp + "_bn2_g"), b.dq_planes ? nullptr : gB, b.dq_planes ? gB : nullptr, M * co,
                                     b.dq_planes ? 2 : 0, g2g, g2b, parts, coef, B, H, W, co, ph, pw, drop_block, seed, (uint32_t)i, dtq, stream));
        break;
      default:
        if (b.dq_planes) CRNN_TRY(crnn_bn_bwd_planes_ex(qq, gA, s2, c.p(bp + "_bn2_g"), gB, M * co, 2, g2g, g2b, parts, coef, B, H, W, co, ph, pw, drop_block, seed, (uint32_t)i, stream));
        else CRNN_TRY(crnn_bn_bwd_ex(qq, gA, s2, c.p(bp + "_bn2_g"), gB, g2g, g2b, parts, coef, B, H, W, co, ph, pw, drop_block, seed, (uint32_t)i, dtq, stream));
    }
    // ---- pointwise conv backward: weight gradient from dq and a = ReLU6(BatchNorm-1(d)) -- re-formed from d while staging where the forward never wrote it
    // (Sched::bn1) --, on the side stream where the depthwise stage is one kernel; data gradient da in gA
    const int bn1_rows = b.dgrad_rows;                       // > 0: the data-gradient kernel leaves BatchNorm-1's backward statistics in `partials`
    const bool side = fj.on && b.dw_fused();
    const Ctx& cw = side ? ca : c;
    if (side) CRNN_TRY(fj.fork());
    switch (b.wgrad) {
      case WG_PW1_BN:   // block 1: weight gradient, data gradient and BatchNorm-1's backward statistics from one pass over dq
        // ([rows][2] statistics for the finalize below; the weight-gradient partials behind them)
        CRNN_TRY(crnn_pw1_bn_bwd(dd, s1, kpw, gB, gA, gpw, parts + ((2L * bn1_rows + 63) & ~63L), parts, M, co, dtq, stream)); break;
      case WG_PW1: CRNN_TRY(crnn_pw1_bwd(c.w("a" + p), kpw, gB, gA, gpw, parts, M, co, dtq, stream)); break;   // block 1: outer-product weight / data gradients
      case WG_STREAM_BF16: CRNN_TRY(crnn_pwconv_bnrelu6_wgrad_stream(dd, s1, gB, gpw, M, co, ci, cw.scratch(), kGemmScratchBytes, cw.s)); break;   // pixel stream (gemm_wgrad.hip)
      case WG_TILE_BF16: CRNN_TRY(crnn_pwconv_bnrelu6_wgrad(dd, s1, gB, gpw, M, co, ci, cw.scratch(), kGemmScratchBytes, cw.s)); break;
      case WG_PLANES_STREAM:   // two-plane operands on the pixel stream (gemm_wgrad3.hip): one workgroup per 128 x 128 tile and pixel range; dq from its planes
        CRNN_TRY(crnn_pwconv_bnrelu6_wgrad_planes_stream_gp(dd, s1, gB, M * co, gpw, M, co, ci, cw.scratch(), kGemmScratchBytes, cw.s)); break;
      case WG_PLANES_TILE:
        CRNN_TRY((planes == 2 ? crnn_pwconv_bnrelu6_wgrad_f32x2 : crnn_pwconv_bnrelu6_wgrad_f32x3)(dd, s1, gB, gpw, M, co, ci, cw.scratch(), kGemmScratchBytes, cw.s)); break;
      default: CRNN_TRY(gemm_t(cw, 2, c.w("a" + p), dtd, gB, dtq, gpw, CRNN_F32, ci, co, (int)M, ci, co, co, nullptr, 0, 0, 0, planes));
    }
    if (side) CRNN_TRY(fj.mark(&gB_free));
    // data gradient da[M][ci] = dq[M][co] . W[ci][co]^T
    switch (b.dgrad) {
      case DG_PW1: break;   // (block 1: done above)
      case DG_PRES: CRNN_TRY(crnn_gemm_pres_bnstats(gB, M * co, kpw, gA, M, ci, co, 2, dd, s1, parts, nullptr, 0, 0, stream)); break;
      case DG_WRES_BF16:
      case DG_NT_BF16: {
        // the weights' bf16 shadow resident in registers (gemm_wres.hip); with dgrad_rows, the storer waves also take the statistics pass of the depthwise BatchNorm's
        // backward (they hold the finished da stripe: the stand-alone pass would read da and d again).  DG_NT_BF16: the shadow streamed (gemm_nt.hip)
        int dtw = CRNN_F32;
        const float* wsh = weight_operand(c, 1, kpw, &dtw);
        if (b.dgrad == DG_NT_BF16) CRNN_TRY(crnn_gemm_nt_bf16(gB, wsh, gA, (int)M, ci, co, stream));
        else if (bn1_rows > 0) CRNN_TRY(crnn_gemm_wres_bf16_bnstats(gB, wsh, gA, M, ci, co, dd, s1, parts, stream));
        else CRNN_TRY(crnn_gemm_wres_bf16(gB, wsh, gA, (int)M, ci, co, stream));
        break;
      }
      case DG_WRES3:   // W^T planes resident, dq streamed once (gemm_wres3.hip)
        CRNN_TRY(crnn_gemm_wres3_bnstats(gB, kpw, gA, M, ci, co, planes, dd, s1, parts, stream)); break;
      case DG_PLANES_TILE:   // the plane GEMM's epilogue takes the statistics (it holds the finished da tile)
        CRNN_TRY((planes == 2 ? crnn_gemm_f32x2_bnstats : crnn_gemm_f32x3_bnstats)(gB, kpw, gA, M, ci, co, dd, s1, parts, stream)); break;
      default: CRNN_TRY(gemm_t(c, 1, gB, dtq, kpw, CRNN_F32, gA, dtd, (int)M, ci, co, co, co, ci, nullptr, 0, 0, 0, planes));
    }
    // ---- BatchNorm-1 + ReLU6 and depthwise conv backward: statistics (finalize alone where the data gradient took them), then pass 2 + both depthwise gradients
    const float* xin = (i == 1) ? c.w("x0") : c.w("x" + std::to_string(i - 1));
    const bool three = b.dwb == DWB_THREE_KERNELS;
    if (bn1_rows > 0 && dtd == CRNN_F32)     // (one row per GEMM tile row: folded first)
      CRNN_TRY(crnn_bn_bwd_finalize_folded(parts, bn1_rows, ci, M, g1g, g1b, coef, c.w("fold"), stream));
    else if (bn1_rows > 0)
      CRNN_TRY(crnn_bn_bwd_finalize(parts, bn1_rows, ci, M, g1g, g1b, coef, stream));
    else
      CRNN_TRY(crnn_bn_bwd_ex(dd, gA, s1, c.p(bp + "_bn1_g"), three ? gB : nullptr, g1g, g1b, parts, coef, B, H, W, ci, 1, 1, 0.f, 0, 0, dtd, stream));
    if (b.dw_fused()) {   // one kernel
      CRNN_TRY(fj.wait(gC_free)); gC_free = nullptr;      // gC is written next
      switch (b.dwb) {
        case DWB_PRO: {   // the forward did not keep x_{i-1}: re-formed from q_{i-1} in LDS, with the keep bytes the forward of this step left in the workspace;
          // where Sched::bn2_rows, the kernel also takes the statistics pass of that block's BatchNorm-2 backward
          const BlockSched& prev = S.b[i - 1];
          CRNN_TRY(crnn_dwconv3x3_bwd_stream_pro_ex(dd, gA, s1, coef, pro_src(c, i - 1), c.w("bn2s" + std::to_string(i - 1)), drop_block, keep_bytes(c, i - 1), kdw, gC,
                                                    c.g(bp + "_dw"), parts, prev.bn2_rows > 0 ? c.w("bn2parts") : nullptr, B, H, W, ci, dtd, stream));
          break;
        }
        case DWB_STREAM: CRNN_TRY(crnn_dwconv3x3_bwd_stream_ex(dd, gA, s1, coef, xin, kdw, gC, c.g(bp + "_dw"), parts, B, H, W, ci, dtd, stream)); break;
        default: CRNN_TRY(crnn_dwconv3x3_bwd_fused(dd, gA, s1, coef, xin, kdw, gC, c.g(bp + "_dw"), parts, B, H, W, ci, stream));
      }
      // the block below finds its incoming gradient in gA, writes gB; this block's side-stream GEMM may still read the old gB
      float* t = gA; gA = gC; gC = gB; gB = t;
      gC_free = gB_free; gB_free = nullptr;
    } else if (b.dwb == DWB_C1) {   // block 1: pass 2 + both depthwise gradients in one kernel
      CRNN_TRY(crnn_dwconv3x3_c1_bwd(dd, gA, s1, coef, xin, kdw, (i > 1 || cfg->stn) ? gB : nullptr, c.g(bp + "_dw"), parts, B, H, W, stream));
      if (i > 1 || cfg->stn) { float* t = gA; gA = gB; gB = t; }   // (the spatial transformer's backward finds d loss / d x0 in gA)
    } else {
      if (bn1_rows > 0) CRNN_TRY(crnn_bn_bwd_apply_ex(dd, gA, s1, coef, gB, B, H, W, ci, 1, 1, 0.f, 0, 0, dtd, stream));   // (pass 2 alone)
      CRNN_TRY(crnn_dwconv3x3_wgrad_ex(xin, gB, c.g(bp + "_dw"), parts, B, H, W, ci, dtd, stream));
      if (i > 1 || cfg->stn) CRNN_TRY(crnn_dwconv3x3_fwd_ex(gB, kdw, gA, nullptr, B, H, W, ci, 1, dtd, stream));
    }
  }
  CRNN_TRY(fj.join());                                   // every weight gradient is complete in the main stream's order
  // ---- spatial transformer
  if (cfg->stn) {
    CRNN_TRY(crnn_sampler_bwd(x, c.w("theta"), gA, c.w("dtheta"), B, d.H0, d.W0, 2, stream));
    if (S.loc_fused)
      return crnn_loc_net_bwd(c.w("dtheta"), c.w("flat"), c.w("fc1"), c.w("pool1"), c.w("c1"), c.w("pool2"), c.p("stn_d1_w"), c.p("stn_d2_w"), c.p("stn_c2_k"),
                              c.w("dfc1"), c.w("locterms"), c.g("stn_c1_k"), c.g("stn_c1_b"), c.g("stn_c2_k"), c.g("stn_c2_b"), c.g("stn_d1_w"), c.g("stn_d1_b"),
                              c.g("stn_d2_w"), c.g("stn_d2_b"), B, d.H0, d.W0, stream);
    CRNN_TRY(crnn_loc_fc_bwd(c.w("flat"), c.w("fc1"), c.w("dtheta"), c.p("stn_d1_w"), c.p("stn_d2_w"), c.w("dfc1"), c.w("dflat"),
                             c.g("stn_d1_w"), c.g("stn_d1_b"), c.g("stn_d2_w"), c.g("stn_d2_b"), B, d.stn_flat, stream));
    CRNN_TRY(crnn_loc_conv_wgrad(c.w("pool2"), c.w("dflat"), c.g("stn_c2_k"), c.g("stn_c2_b"), c.w("partials"), B, d.Hs2, d.Ws2, 20, stream));
    CRNN_TRY(crnn_loc_conv_dgrad(c.w("dflat"), c.p("stn_c2_k"), c.w("dpool2"), B, d.Hs2, d.Ws2, stream));
    CRNN_TRY(crnn_maxpool_bwd(c.w("c1"), c.w("dpool2"), c.w("dc1"), B, d.Ho1, d.Wo1, 20, 2, 2, stream));
    CRNN_TRY(crnn_loc_conv_wgrad(c.w("pool1"), c.w("dc1"), c.g("stn_c1_k"), c.g("stn_c1_b"), c.w("partials"), B, d.Hs1, d.Ws1, 1, stream));
  }
  return CRNN_OK;
}
}  // namespace


extern "C" int crnn_train_step_adam(const crnn_config* cfg, float* params, float* grads, float* m, float* v, float* bn_mean, float* bn_var,
                                    const float* x, const int* labels, const int* input_length, const int* label_length, float* ws,
                                    size_t ws_bytes, float* y_pred, float* loss, void* norm_scratch, float* norm_out, float lr_t,
                                    float beta1, float beta2, float eps, float clipnorm, uint64_t seed, hipStream_t stream) {
  CRNN_TRY(crnn_forward_ex(cfg, params, bn_mean, bn_var, x, ws, ws_bytes, y_pred, 1, seed, stream, nullptr));
  CRNN_TRY(crnn_backward(cfg, params, grads, x, labels, input_length, label_length, ws, ws_bytes, loss, seed, stream));
  const long n = make_layout(cfg).total;
  CRNN_TRY(crnn_global_norm(grads, n, clipnorm, norm_scratch, norm_out, stream));
  CRNN_TRY(crnn_adam_step(params, grads, m, v, n, lr_t, beta1, beta2, eps, norm_out, stream));
  return crnn_bn_update(cfg, bn_mean, bn_var, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------
// BatchNorm moving statistics (momentum .99): m <- .99 m + .01 mean ;
// v <- .99 v + .01 var * n/(n-1) * n/(n-(1+eps))   (TF fused-BN Bessel correction x Keras 2.2.2 factor)
struct BnTable { int state_off[14]; int C[14]; int cum[15]; float count[14]; };
__global__ void bn_moving_kernel(BnTable tab, float* __restrict__ mmean, float* __restrict__ mvar, const float* __restrict__ ws,
                                 int total, float momentum, float eps) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int k = 0;
  while (k < 13 && i >= tab.cum[k + 1]) ++k;
  int ch = i - tab.cum[k];
  float n = tab.count[k];
  float mean = ws[tab.state_off[k] + ch], var = ws[tab.state_off[k] + tab.C[k] + ch];
  float vhat = var * (n / (n - 1.f)) * (n / (n - (1.f + eps)));
  mmean[i] = momentum * mmean[i] + (1.f - momentum) * mean;
  mvar[i] = momentum * mvar[i] + (1.f - momentum) * vhat;
}

extern "C" int crnn_bn_update(const crnn_config* cfg, float* bn_mean, float* bn_var, float* ws, size_t ws_bytes, hipStream_t stream) {
  CRNN_TRY(check_cfg(cfg));
  Dims d = make_dims(cfg);
  Plan P = make_plan(cfg);
  if (ws_bytes < (size_t)P.total * sizeof(float)) return CRNN_ERR_ARG;
  BnTable tab;
  int k = 0, cum = 0;
  for (int i = 1; i <= 7; ++i)
    for (int j = 1; j <= 2; ++j, ++k) {
      int C = (j == 1) ? d.bc[i - 1] : d.bc[i];
      tab.state_off[k] = (int)P.off(std::string("bn") + (j == 1 ? "1s" : "2s") + std::to_string(i));
      tab.C[k] = C; tab.cum[k] = cum; tab.count[k] = (float)((long)d.B * d.bh[i] * d.bw[i]);
      cum += C;
    }
  tab.cum[14] = cum;
  hipLaunchKernelGGL(bn_moving_kernel, dim3(cdiv(cum, 256)), dim3(256), 0, stream, tab, bn_mean, bn_var, ws, cum, 0.99f, BN_EPS);
  CRNN_LAUNCH_CHECK();
  return CRNN_OK;
}
