"""-m gpu tests of alphabets of 65..128 classes: the softmax, CTC and beam kernels hold two classes per lane of a wavefront there (lane l owns
classes l and l + 64).  Operators against the CPU oracle at the tolerances of the 38 / 64-class operator tests, the whole model in the parity
mode and on the streamed dense2 of the bf16 modes, and the Python surface (train, predict, decode, score) over a 96-character alphabet.  Every
test checks that its data reaches the upper half (ids >= 64): none can pass on the lower half alone."""
import numpy as np
import pytest
import torch

import utils as U
from oracle import ops, ctc, model as M
from gpu_util import L, dev, zeros, P, S, ok, host, assert_close
from crnn_mi355x.engine import Engine
from test_gpu_model import run_case, check_case

pytestmark = pytest.mark.gpu


def _bf16_round(a):
    """round-to-nearest-even to bfloat16, returned as float64"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("rows,C,ldz,P_", [(12, 65, 128, 4), (64, 97, 128, 0), (52 * 8, 128, 128, 8)])
def test_softmax_rows_two_classes_per_lane(rows, C, ldz, P_, two):
    """crnn_softmax_rows and crnn_softmax_rows_perm above 64 classes against ops.softmax_fwd; the permuted logits are z + bias exactly, the two
    entry points agree bit for bit, padding columns (NaN) are never read and the memory behind every output stays as it was."""
    rs = np.random.RandomState(rows + C)
    z = rs.normal(size=(rows, ldz)).astype(np.float32) * 3; z[:, C:] = np.nan
    z[0, :C] = 0.0; z[0, C - 1] = 9.0                        # a row whose maximum is the last class (upper half)
    bias = rs.normal(size=C).astype(np.float32)
    zd, bd = dev(z), dev(bias)
    n = rows * C
    lg = torch.full((n + 16,), 5.0, device="cuda"); p1 = torch.full((n + 16,), 6.0, device="cuda"); p2 = torch.full((n + 16,), 7.0, device="cuda")
    ok(L().crnn_softmax_rows_perm(P(zd), ldz, P(bd), P(lg), P(p1), P(p2) if two else None, rows, C, P_, S()))
    want = z[:, :C] + bias
    if P_:
        m = np.arange(rows); orow = (m % P_) * (rows // P_) + m // P_
        perm = np.empty_like(want); perm[orow] = want; want = perm
    assert np.array_equal(host(lg[:n]).reshape(rows, C), want)
    oracle = ops.softmax_fwd(want.astype(np.float64))
    assert_close(host(p1[:n]).reshape(rows, C), oracle, rtol=1e-5, atol=1e-7, what="crnn_softmax_rows_perm vs oracle")
    ref = torch.full((n + 16,), 8.0, device="cuda")
    ok(L().crnn_softmax_rows(P(dev(want)), P(ref), rows, C, S()))
    assert_close(host(ref[:n]).reshape(rows, C), oracle, rtol=1e-5, atol=1e-7, what="crnn_softmax_rows vs oracle")
    assert torch.equal(p1[:n], ref[:n])
    if two:
        assert torch.equal(p2[:n], p1[:n])
    else:
        assert bool((p2 == 7.0).all())
    assert bool((lg[n:] == 5.0).all()) and bool((p1[n:] == 6.0).all()) and bool((p2[n:] == 7.0).all()) and bool((ref[n:] == 8.0).all())
    assert abs(host(p1[:n]).reshape(rows, C).sum(1) - 1).max() < 1e-5
    assert L().crnn_softmax_rows(P(zd), P(ref), 1, 129, S()) == -3
    assert L().crnn_softmax_rows_perm(P(zd), 256, P(bd), P(lg), P(p1), None, 1, 129, 0, S()) == -3


# ------------------------------------------------------------------------------------------------ CTC
def _wide_ctc_case(B, T, C, Lmax, seed):
    """Labels from [0, C - 1) with one forced repeat; sample 0: ids >= 64 only (C >= 97), sample 1: a short input, sample 2: an empty label."""
    rs = np.random.RandomState(seed)
    y = ops.softmax_fwd(rs.normal(size=(B, T, C)) * 2)
    ll = rs.randint(2, Lmax + 1, size=B)
    labels = np.full((B, Lmax), C - 1, dtype=np.int64)
    for b in range(B):
        labels[b, :ll[b]] = rs.randint(0, C - 1, size=ll[b])
        labels[b, 1] = labels[b, 0]                          # a repeated character
    if C >= 97:
        labels[0, :ll[0]] = rs.randint(64, C - 1, size=ll[0]); labels[0, 1] = labels[0, 0]
    il = np.full(B, T - 2, dtype=np.int64)
    il[1] = 2 * ll[1] + 1                                    # short, and feasible whatever repeats the draw holds
    ll[2] = 0; labels[2, :] = C - 1
    return y, labels, il, ll.astype(np.int64)


@pytest.mark.parametrize("B,T,C,Lmax", [(6, 14, 65, 5), (6, 14, 97, 5), (6, 14, 128, 5), (4, 102, 128, 31)])
def test_ctc_loss_and_logit_gradient_above_64_classes(B, T, C, Lmax):
    """crnn_ctc_loss_grad against ctc.ctc_loss_and_grad + ops.softmax_bwd; (4, 102, 128, 31) is the largest case the 160 KB of LDS hold."""
    y, labels, il, ll = _wide_ctc_case(B, T, C, Lmax, 17 + C + T)
    if C >= 97:
        used = np.concatenate([labels[b, :ll[b]] for b in range(B)])
        assert ((used >= 64) & (used < C - 1)).any() and (labels[0, :ll[0]] >= 64).all() and (used < 64).any()
    assert il[1] < T - 2 and ll[2] == 0
    loss_ref, gy = ctc.ctc_loss_and_grad(y, labels, il, ll)
    gl_ref = ops.softmax_bwd(y, gy / B)
    assert np.isfinite(loss_ref).all()
    yd = dev(y)
    loss = zeros(B); dl = torch.full((T, B, C), 9.0, device="cuda")
    args = (P(dev(labels, np.int32)), P(dev(il, np.int32)), P(dev(ll, np.int32)), P(loss), P(dl))
    ok(L().crnn_ctc_loss_grad(P(yd), *args, B, T, C, Lmax, 2, 1.0 / B, S()))
    assert_close(host(loss), loss_ref, rtol=1e-4, atol=1e-3, what="ctc loss at C=%d" % C)
    got = np.swapaxes(host(dl), 0, 1)                        # [B][T][C]
    assert_close(got, gl_ref, rtol=1e-3, atol=2e-6, what="dlogits at C=%d" % C)
    for b in range(B):
        assert (got[b, :2] == 0).all() and (got[b, 2 + il[b]:] == 0).all(), b
    assert np.abs(got[:, :, 64:]).max() > 0
    assert L().crnn_ctc_loss_grad(P(yd), *args, B, T, 129, Lmax, 2, 1.0 / B, S()) == -3


# ------------------------------------------------------------------------------------------------ decoders
_POST = {}


def _posteriors(C):
    """(y float32 [12][20][C], input_length): peaked and flat samples, one of exactly uniform rows (every class ties, across the two halves), at
    C = 66 one peaked on class 64 -- the only label of the upper half there -- in several frames; input lengths 1 and 2 included."""
    if C not in _POST:
        rs = np.random.RandomState(C)
        B, T = 12, 20
        logits = rs.normal(size=(B, T, C)) * rs.choice([0.7, 2.0, 6.0], size=(B, 1, 1))
        if C == 66:
            logits[2, 3:6, 64] += 30.0; logits[2, 9, 64] += 30.0; logits[2, 14:16, 64] += 30.0
        yp = ops.softmax_fwd(logits).astype(np.float32)
        yp[1] = np.float32(1.0 / C)
        il = np.full(B, T); il[3] = 1; il[4] = 2; il[5] = 13
        yp.setflags(write=False); il.setflags(write=False)
        _POST[C] = (yp, il)
    return _POST[C]


def _reaches_upper_half(ref, C):
    if C >= 97:
        assert (ref >= 64).any()
    if C == 66:
        assert 64 in ref
    assert ref.max() < C - 1


@pytest.mark.parametrize("C", [65, 66, 97, 128])
def test_greedy_decode_above_64_classes(C):
    yp, il = _posteriors(C)
    B, T = yp.shape[:2]
    ref, rl = ctc.ctc_greedy_decode(yp, il)
    _reaches_upper_half(ref, C)
    out = torch.full((B, T), 7, dtype=torch.int32, device="cuda"); ln = zeros(B, dtype=torch.int32)
    ok(L().crnn_ctc_greedy_decode(P(dev(np.array(yp))), P(dev(il, np.int32)), P(out), P(ln), B, T, C, S()))
    assert np.array_equal(host(ln), rl) and np.array_equal(host(out), ref)


@pytest.mark.parametrize("bw,merge", [(1, 1), (10, 1), (10, 0), (64, 1)])
@pytest.mark.parametrize("C", [65, 66, 97, 128])
def test_beam_decode_above_64_classes(C, bw, merge):
    """Indices and lengths bit-exact against the oracle's restatement of TF's beam search, scores to rtol 1e-4 / atol 1e-3.  C = 65: the blank
    sits alone in the upper half; C = 66: class 64 is its only label."""
    yp, il = _posteriors(C)
    B, T = yp.shape[:2]
    ref, rl, rsc = ctc.ctc_beam_decode(yp, beam_width=bw, merge_repeated=bool(merge), input_length=il)
    _reaches_upper_half(ref, C)
    out = torch.full((B, T), 7, dtype=torch.int32, device="cuda"); ln = zeros(B, dtype=torch.int32); sc = zeros(B)
    ok(L().crnn_ctc_beam_decode(P(dev(np.array(yp))), P(dev(il, np.int32)), P(out), P(ln), P(sc), B, T, C, bw, merge, S()))
    assert np.array_equal(host(ln), rl)
    assert np.array_equal(host(out), ref)
    assert_close(host(sc), rsc, rtol=1e-4, atol=1e-3, what="beam score")
    assert L().crnn_ctc_beam_decode(P(dev(np.array(yp))), None, P(out), P(ln), P(sc), B, T, 129, bw, merge, S()) == -3


# ------------------------------------------------------------------------------------------------ model, parity mode
def _labels_reach_upper_half(res, C):
    x, lab, il, ll = res[4]
    used = np.concatenate([lab[b, :ll[b]] for b in range(len(ll))])
    assert ((used >= 64) & (used < C - 1)).any(), used


def test_small_model_with_97_classes():
    res = run_case(B=4, imgh=40, imgw=32, u=64, tds=32, max_len=6, stn=True, dropout=True, num_classes=97)
    _labels_reach_upper_half(res, 97)
    check_case(res, "small-97")


def test_small_gru_model_with_128_classes():
    res = run_case(B=4, imgh=40, imgw=32, u=64, tds=32, max_len=6, stn=True, dropout=True, gru=True, num_classes=128)
    _labels_reach_upper_half(res, 128)
    check_case(res, "small-gru-128")


# ------------------------------------------------------------------------------------------------ model, bf16s: the streamed dense2
def test_bf16s_streamed_dense2_writes_all_97_columns():
    """T * B = 22 * 32 = 704 rows are whole 64-row stripes: dense2 runs on the stripe stream against the 128-row padded W^T and crnn_softmax_rows_perm
    reads 97 of its 128 columns.  The logits equal the fp64 product of the bf16-rounded operands the device used, plus the bias, at the tolerance of
    test_gemm_bf16_mode_equals_fp32_accumulation_of_bf16_rounded_operands (rtol 2e-5 of the largest value + 1e-4)."""
    B, C, u = 32, 97, 64
    cfg = M.Config(imgh=40, imgw=32, num_classes=C, max_len=6, time_dense_size=32, n_units=u)
    p, bn = M.init_params(cfg, seed=7, dtype=np.float64)
    p = M.randomize_params(cfg, p)
    x, lab, il, ll = M.synthetic_batch(cfg, B, seed=1, dtype=np.float64)
    eng = Engine(B, 40, 32, C, 6, 32, u, precision="bf16s", dropout=False)
    T = eng.T
    assert T * B == 704
    eng.set_params(p, bn)
    eng.ws_tensor("lg128").fill_(-7.0)
    y = eng.forward(x.astype(np.float32), train=True, seed=0)
    torch.cuda.synchronize()
    r2 = eng.ws_tensor("r2d").float().cpu().numpy().reshape(T, B, 2 * u)         # dense2's input, time-major
    W = np.asarray(p["dense2_w"], dtype=np.float32); b = np.asarray(p["dense2_b"], dtype=np.float32)
    ref = _bf16_round(r2) @ _bf16_round(W) + b.astype(np.float64)                # [T][B][C]
    ref = np.swapaxes(ref, 0, 1)                                                 # batch-major, as the epilogue writes them
    logits = eng.ws_tensor("logits").cpu().numpy().reshape(B, T, C)
    assert_close(logits, ref, rtol=2e-5, atol=1e-4, what="streamed dense2, 97 columns")
    # the stream was taken: its raw products are what the epilogue read
    lg128 = eng.ws_tensor("lg128").cpu().numpy().reshape(T, B, 128)
    assert np.array_equal(np.swapaxes(lg128[:, :, :C] + b, 0, 1), logits)
    yh = y.cpu().numpy()
    assert yh.shape == (B, T, C) and np.abs(yh.sum(-1) - 1).max() < 1e-5
    assert_close(yh, ops.softmax_fwd(logits.astype(np.float64)), rtol=1e-5, atol=1e-7, what="y_pred")
    loss = eng.backward(lab, il, ll, seed=0).cpu().numpy()
    g = eng.get_grads()
    assert np.isfinite(loss).all()
    assert g["dense2_w"].shape == (128, 97) and g["dense2_b"].shape == (97,)
    assert all(np.isfinite(v).all() for v in g.values())
    assert np.abs(g["dense2_w"][:, 64:]).max() > 0 and np.abs(g["rnn1f_u"]).max() > 0 and np.abs(g["b1_dw"]).max() > 0


# ------------------------------------------------------------------------------------------------ surface
_CHARS = [chr(33 + i) for i in range(96)]                    # 96 distinct one-character strings


def _surface_batch(B, T, max_len, seed):
    rs = np.random.RandomState(seed)
    x = rs.normal(size=(B, 100, 32, 1)).astype(np.float32) if T == 52 else None
    ll = rs.randint(1, 9, size=B)
    lab = np.full((B, max_len), 96, dtype=np.int64)
    for b in range(B):
        lab[b, :ll[b]] = rs.randint(0, 96, size=ll[b])
    lab[0, :ll[0]] = rs.randint(64, 96, size=ll[0])
    return x, lab, np.full((B, 1), T - 2, dtype=np.int64), ll.reshape(B, 1).astype(np.int64)


def test_97_class_model_trains_predicts_and_decodes_through_utils():
    B = 4
    model = U.CRNN(num_classes=97, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()
    model.compile(loss={"ctc": lambda y_true, y_pred: y_pred}, optimizer=U.optimizers.Adam(lr=1e-3, beta_1=0.5, beta_2=0.999, clipnorm=5))
    x, lab, il, ll = _surface_batch(B, 52, 23, 5)
    assert (lab[lab != 96] >= 64).any()
    w0 = model.get_weights()[-2].copy()
    loss = model.train_on_batch(x, lab, il, ll)
    assert np.isfinite(loss) and loss > 0
    w1 = model.get_weights()[-2]
    assert w1.shape == (128, 97) and np.abs(w1 - w0)[:, 64:].max() > 0        # the step moved the columns of the upper half
    y = U.init_predictor(model).predict_on_batch(x)
    assert y.shape == (B, 52, 97) and np.abs(y.sum(-1) - 1).max() < 1e-5
    dec = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=dict(enumerate(_CHARS)))
    rows = dec.decode_labels(y)
    ref, rl, _ = ctc.ctc_beam_decode(y, beam_width=10, merge_repeated=True)
    assert np.array_equal(rows, ref)
    assert list(dec.decode(y)) == [ctc.labels_to_text(r, dict(enumerate(_CHARS))) for r in ref]
    # posteriors peaked on the upper half decode to its characters: nothing on the way narrows the ids
    want = [[64, 95, 70], [3, 64, 90, 64], [95], [80, 1, 81]]
    yp = np.full((B, 52, 97), 1e-4, dtype=np.float32)
    for b, w in enumerate(want):
        for k, c in enumerate(w):
            yp[b, 2 * k:2 * k + 2, c] = 1.0
        yp[b, 2 * len(w):, 96] = 1.0
    yp /= yp.sum(-1, keepdims=True)
    assert dec.decode(yp) == ["".join(_CHARS[c] for c in w) for w in want]
    assert U.DecodeCTCPred(inverse_classes=dict(enumerate(_CHARS)), greedy=True).decode(yp) == dec.decode(yp)


def test_device_scoring_of_label_rows_with_ids_above_63():
    rs = np.random.RandomState(9)
    n = 37
    pred = np.full((n, 52), -1, dtype=np.int64); truth = np.full((n, 23), 96, dtype=np.int64)
    for i in range(n):
        t = rs.randint(60, 96, size=rs.randint(1, 20))
        p_ = [c for c in t if rs.rand() > 0.2]
        p_ = [int(rs.randint(0, 96)) if rs.rand() < 0.2 else int(c) for c in p_] + rs.randint(64, 96, size=rs.randint(0, 3)).tolist()
        truth[i, :len(t)] = t; pred[i, :len(p_)] = p_
    assert (truth[truth != 96] >= 64).any() and (pred >= 64).any()
    d, pl, tl = U.device_edit_distances(pred, truth, (96, -1))
    score = U.Score(pred, d.cpu().numpy(), pl.cpu().numpy(), tl.cpu().numpy())
    dec = U.DecodeCTCPred(inverse_classes=dict(enumerate(_CHARS)))
    pt, tt = [dec.labels_to_text(r) for r in pred], [dec.labels_to_text(r) for r in truth]
    assert score.texts(dec) == pt
    assert score.distances.tolist() == [int(U.levenshtein(a, b)) for a, b in zip(pt, tt)] and score.distances.max() > 0
    assert score.pred_lengths.tolist() == [len(a) for a in pt] and score.true_lengths.tolist() == [len(b) for b in tt]
    assert score.edit_distance == U.edit_distance(pt, tt)
    assert score.normalized_edit_distance == U.normalized_edit_distance(pt, tt)


def test_crnn_with_nothing_but_its_defaults_runs():
    """U.CRNN() as the reference constructs it: 97 classes, shape (40, 40, 1), 23 characters, 128 / 256 units."""
    B = 2
    model = U.CRNN().get_model()
    assert model.config["num_classes"] == 97
    model.compile(loss={"ctc": lambda y_true, y_pred: y_pred}, optimizer=U.optimizers.Adam(lr=1e-3, clipnorm=5))
    T = (40 + 4) // 2
    _, lab, il, ll = _surface_batch(B, T, 23, 6)
    x = np.random.RandomState(2).normal(size=(B, 40, 40, 1)).astype(np.float32)
    loss = model.train_on_batch(x, lab, il, ll)
    assert np.isfinite(loss)
    y = U.init_predictor(model).predict_on_batch(x)
    assert y.shape == (B, T, 97) and np.abs(y.sum(-1) - 1).max() < 1e-5
    texts = U.DecodeCTCPred(beam_width=10, inverse_classes=dict(enumerate(_CHARS))).decode(y)
    assert len(texts) == B and all(isinstance(t, str) for t in texts)
