"""-m gpu tests of lexicon decoding (csrc/lexicon.hip, crnn_mi355x/lexicon.py): the CTC log-probability of every word of a table under every
sample's posterior map against the fp64 reference of tests/lexicon_ref.py (pinned to the CTC oracle and to torch in tests/test_lexicon_cpu.py)
and against the loss kernel, the independence of a pair's score from whatever shares its wavefront, the candidates mode, the top-k kernel, the
validation of untrusted tables, the refusals, and the Python surface (LexiconDecoder as a drop-in decoder, predict.py --lexicon).
The shapes are the smallest at which the kernel takes every path: word lengths on both sides of the 16- and 32-lane segment limits, tables
shorter than and longer than a workgroup's tile (64 words; rows of fewer words are dealt evenly to the four waves, at least 4 each), alphabets on
both sides of 64 classes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import utils as U
from gpu_util import L, dev, zeros, P, S, ok, host
from lexicon_ref import _ref_scores, posteriors, input_lengths, make_words, table, SEGMENT_LENGTHS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
NEG_INF = float("-inf")


def _scores(y, words, il=None, skip=0, cand=None, width=31, lab=None, ll=None, fill=None):
    """One call of crnn_ctc_lexicon_score -> scores as an ndarray (B, M); y (B, T, C) float32 ndarray, words a list of id sequences (or lab / ll:
    a ready table), cand (B, K) or None."""
    B, T, C = y.shape
    if lab is None:
        lab, ll = table(words, width=width)
    N, Lmax = lab.shape
    M = cand.shape[1] if cand is not None else N
    out = torch.full((B, M), 7.0 if fill is None else fill, device="cuda")
    nbytes = L().crnn_ctc_lexicon_workspace_bytes(B, T, C, skip)
    assert nbytes == B * (T - skip) * C * 4
    ws = zeros(nbytes // 4)
    ok(L().crnn_ctc_lexicon_score(P(dev(y)), P(dev(il, np.int32)) if il is not None else None, P(dev(lab, np.int32)), P(dev(ll, np.int32)),
                                  P(dev(cand, np.int32)) if cand is not None else None, P(out), P(ws), nbytes, B, T, C, skip, N, Lmax,
                                  M if cand is not None else 0, S()))
    return host(out)


def _assert_scores(got, ref, what):
    """The project's CTC tolerance (rtol 1e-4, atol 1e-3, as the loss tests) on the finite entries; the -inf pattern must be equal."""
    assert got.shape == ref.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), "%s: -inf pattern differs at %s" % (what, np.argwhere(np.isneginf(got) != np.isneginf(ref))[:5])
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all() and not np.isnan(got).any()
    err = np.abs(got[fin] - ref[fin])
    print("%s: %d finite, %d -inf, max |diff| %.3e at reference %.3f" % (what, fin.sum(), (~fin).sum(), err.max(), ref[fin][err.argmax()]))
    assert (err <= 1e-3 + 1e-4 * np.abs(ref[fin])).all(), "%s: max|diff| %.3e" % (what, err.max())


# ---- 1. scores against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [0, 2])
@pytest.mark.parametrize("C", [38, 66, 97, 128])
def test_scores_equal_the_reference(C, skip):
    B, T, N = 6, 20, 40
    y = posteriors(C, T)
    il = input_lengths(T, skip)
    assert sorted(il.tolist()) == sorted([0, 1, 2, 13, T - skip, T - skip])
    words = make_words(C, n=N, seed=0)
    words[9] = [3, 3, 3]                                     # tripled: 5 frames -- impossible for the samples with 1 or 2
    assert sorted(set(len(w) for w in words if w != [3, 3, 3])) == sorted(SEGMENT_LENGTHS)
    assert any(len(w) >= 2 and w[0] == w[1] for w in words) and any(len(w) >= 3 and w[0] == w[1] == w[2] for w in words)
    if C >= 66:
        used = np.concatenate([w for w in words if w])
        assert (used >= 64).any() and (used < 64).any() and used.max() <= C - 2
    ref = _ref_scores(y, words, il, skip)
    assert np.isfinite(ref).any() and np.isneginf(ref).any()
    assert np.isfinite(ref[0, 9]) and np.isneginf(ref[2, 9]) and np.isneginf(ref[4, 9])      # the same word: possible in T - skip frames, not in 2 or 1
    assert np.isfinite(ref[:, [n for n, w in enumerate(words) if len(w) == 16]]).any()      # the 64-lane form has finite results to get right
    got = _scores(np.array(y), words, il, skip)
    _assert_scores(got, ref, "C=%d skip=%d" % (C, skip))
    assert got[5, [n for n, w in enumerate(words) if not w][0]] == 0.0                       # Tb = 0: exactly 0 for the empty word
    # NULL input lengths: the whole window
    _assert_scores(_scores(np.array(y), words, None, skip), _ref_scores(y, words, None, skip), "C=%d skip=%d, no lengths" % (C, skip))


def test_longest_words_have_finite_scores_when_the_frames_allow():
    """T = 20 leaves every word of 31 letters impossible; with 66 frames all 63 states of the longest word carry a finite value."""
    C, T = 38, 66
    y = posteriors(C, T)
    words = make_words(C, n=14, seed=4)
    words[6] = list(range(31))                               # no repeats: 31 frames are enough
    il = np.array([T, 40, 31, T, 62, 63])
    ref = _ref_scores(y, words, il, 0)
    assert np.isfinite(ref[:, 6]).all() and sum(len(w) == 31 for w in words) == 2
    _assert_scores(_scores(np.array(y), words, il, 0), ref, "T=66")


# ---- 2. against the loss kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [38, 128])
def test_scores_equal_the_negated_loss_of_the_loss_kernel(C):
    B, T, N, skip = 6, 20, 40, 2
    y = np.array(posteriors(C, T))
    il = input_lengths(T, skip)
    words = make_words(C, n=N, seed=0)
    got = _scores(y, words, il, skip)
    rs = np.random.RandomState(C)
    pairs = [(int(b), int(n)) for b, n in zip(rs.randint(0, B, 32), rs.permutation(N)[:32])]
    pairs[:6] = [(b, [n for n, w in enumerate(words) if len(w) == (0, 1, 7, 8, 15, 16)[b]][0]) for b in range(6)]
    lab, ll = table([words[n] for _, n in pairs], width=31, pad=C - 1)
    yb = np.stack([y[b] for b, _ in pairs])
    ilb = np.array([il[b] for b, _ in pairs], dtype=np.int32)
    loss = zeros(32); dl = zeros(T, 32, C)
    ok(L().crnn_ctc_loss_grad(P(dev(yb)), P(dev(lab, np.int32)), P(dev(ilb, np.int32)), P(dev(ll, np.int32)), P(loss), P(dl), 32, T, C, 31, skip,
                              1.0, S()))
    want = -host(loss)
    mine = np.array([got[b, n] for b, n in pairs])
    fin = np.isfinite(want)
    assert fin.sum() >= 5 and (~fin).sum() >= 5
    assert np.array_equal(np.isneginf(mine), np.isneginf(want))
    print("C=%d: scores bit-identical to -loss of crnn_ctc_loss_grad on %d pairs: %s (max |diff| %.3e)"
          % (C, len(pairs), np.array_equal(mine, want), np.abs(mine[fin] - want[fin]).max()))
    np.testing.assert_allclose(mine[fin], want[fin], rtol=1e-6, atol=0)


# ---- 3. independence from the neighbours -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C", [(1, 5, 38), (1, 131, 97), (65, 131, 38), (6, 63, 128)])
def test_a_pairs_score_does_not_depend_on_its_neighbours(B, N, C):
    """The table in its given order, reversed, sorted by length (how Lexicon uploads it: the packed forms) and each word alone (N = 1: the
    one-word-per-wave form) -- every pair's score bit-equal.  N = 5 and 63 are less than a tile (4 and 16 words per wave), 131 is two tiles and
    3 words, odd."""
    T = 20
    base = posteriors(C, T)
    y = np.stack([base[b % 6] for b in range(B)]).copy()
    if B > 6:
        y = (y * np.random.RandomState(B).uniform(0.5, 1.0, size=(B, T, 1))).astype(np.float32)      # (not normalised: the kernel re-normalises)
    il = np.array([(T, 13, 7, T, 16, 9)[b % 6] for b in range(B)])
    words = make_words(C, n=N, seed=N, lengths=(0, 1, 3, 7, 8, 5, 15, 16, 2, 31, 7, 4))
    given = _scores(y, words, il)
    assert np.isfinite(given).any() and (N <= 5 or np.isneginf(given).any()) and given.shape == (B, N)
    rev = _scores(y, words[::-1], il)[:, ::-1]
    assert np.array_equal(given, rev)
    by_len = np.argsort([len(w) for w in words], kind="stable")
    srt = _scores(y, [words[k] for k in by_len], il)
    assert np.array_equal(given[:, by_len], srt)
    alone = np.concatenate([_scores(y, [w], il) for w in words], 1)
    assert np.array_equal(given, alone)


def test_a_long_table_scores_the_same_whole_and_in_slices():
    """257 samples x 1021 words (15 whole tiles of 64 and 61 words; a tile count that shares no factor with the 8 XCDs, the rotation of the tiles by
    the sample index in play) equals, bit for bit, its scores in slices of 100 words (16 words per wave) and of 30 (8 per wave) -- and the
    reference on a sample of the pairs."""
    B, N, C, T = 257, 1021, 38, 20
    base = posteriors(C, T)
    y = (np.stack([base[b % 6] for b in range(B)]) * np.random.RandomState(1).uniform(0.5, 1.0, size=(B, T, 1))).astype(np.float32)
    il = np.array([(T, 13, 7, T, 16, 9)[b % 6] for b in range(B)])
    words = make_words(C, n=N, seed=2, lengths=(0, 1, 3, 7, 8, 5, 15, 16, 2, 31, 7, 4))
    words.sort(key=len)                                      # as Lexicon uploads it
    whole = _scores(y, words, il)
    for width in (100, 30):
        parts = np.concatenate([_scores(y, words[lo:lo + width], il) for lo in range(0, N, width)], 1)
        assert np.array_equal(whole, parts), width
    pick = np.arange(0, N, 17)
    _assert_scores(whole[:12, pick], _ref_scores(y[:12], [words[n] for n in pick], il[:12], 0), "257 x 1021")


# ---- 4. candidates -------------------------------------------------------------------------------------------------------------------------------
def test_candidate_lists_equal_the_gather_of_the_dense_scores():
    C, T, N, K = 97, 20, 40, 5
    y = np.array(posteriors(C, T))
    il = input_lengths(T, 0)
    words = make_words(C, n=N, seed=0)
    dense = _scores(y, words, il)
    cand = np.array([[3, 17, 39, 0, 8],                      # every slot live
                     [-1, 5, -1, 5, 12],                     # empty slots in front and between, a word twice
                     [-1, -1, -1, -1, -1],                   # nothing
                     [40, 1, 1000000, -7, 2],                # N, far outside, negative: -inf, nothing indexed
                     [39, -1, -1, -1, -1],
                     [0, 1, 2, 3, -1]], dtype=np.int32)
    got = _scores(y, words, il, cand=cand)
    want = np.full((6, K), NEG_INF, dtype=np.float32)
    inside = (cand >= 0) & (cand < N)
    for b in range(6):
        want[b, inside[b]] = dense[b, cand[b, inside[b]]]
    assert np.isfinite(want).any() and np.array_equal(got, want)
    assert np.isneginf(got[2]).all() and np.isneginf(got[3, [0, 2, 3]]).all()


# ---- 5. top k ----------------------------------------------------------------------------------------------------------------------------------------
def _topk(scores, k, cand=None):
    B, M = scores.shape
    sd = dev(scores)
    cd = dev(cand, np.int32) if cand is not None else None
    outs = []
    for _ in range(2):
        idx = torch.full((B, k), 77, dtype=torch.int32, device="cuda"); val = torch.full((B, k), 5.0, device="cuda")
        ok(L().crnn_ctc_lexicon_topk(P(sd), P(cd), P(idx), P(val), B, M, k, S()))
        outs.append((host(idx), host(val)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))      # two launches: the same bits
    return outs[0]


def _topk_ref(scores, k, cand=None):
    """A stable argsort of the device's own scores: descending, equal scores to the lower position; only finite entries count."""
    B, M = scores.shape
    idx = np.full((B, k), -1, dtype=np.int32); val = np.full((B, k), NEG_INF, dtype=np.float32)
    for b in range(B):
        order = [j for j in np.argsort(-scores[b].astype(np.float64), kind="stable") if np.isfinite(scores[b, j])][:k]
        idx[b, :len(order)] = [j if cand is None else cand[b, j] for j in order]
        val[b, :len(order)] = scores[b, order]
    return idx, val


@pytest.mark.parametrize("k", [1, 3, 8])
def test_topk_equals_a_stable_sort_of_the_scores(k):
    C, T = 38, 20
    y = np.array(posteriors(C, T))
    il = input_lengths(T, 0)
    words = make_words(C, n=40, seed=0)
    words[30] = list(words[4]); words[12] = list(words[4])            # one word three times: its score ties with itself
    scores = _scores(y, words, il)
    assert np.array_equal(scores[:, 4], scores[:, 12]) and np.array_equal(scores[:, 4], scores[:, 30])
    idx, val = _topk(scores, k)
    ri, rv = _topk_ref(scores, k)
    assert np.array_equal(idx, ri) and np.array_equal(val, rv)
    for b in range(6):                                                # the tie goes to the lower index
        row = idx[b].tolist()
        if 12 in row:
            assert 4 in row and row.index(4) < row.index(12)
    # images with fewer than k finite scores: a table without the empty word leaves the sample with no frame nothing, the one with one frame two words
    short = _scores(y, [[1, 2, 3], [5], [6, 6], [7], [8, 9]], il)
    finite = np.isfinite(short).sum(1)
    assert finite.tolist() == [5, 5, 3, 5, 2, 0]
    idx, val = _topk(short, k)
    ri, rv = _topk_ref(short, k)
    assert np.array_equal(idx, ri) and np.array_equal(val, rv)
    for b in range(6):
        assert (idx[b, finite[b]:] == -1).all() and np.isneginf(val[b, finite[b]:]).all() and (idx[b, :finite[b]] >= 0).all()
    # fewer words than k
    few = scores[:, :2].copy()
    idx, val = _topk(few, k)
    ri, rv = _topk_ref(few, k)
    assert np.array_equal(idx, ri) and np.array_equal(val, rv) and (k <= 2 or ((idx[:, 2:] == -1).all() and np.isneginf(val[:, 2:]).all()))
    # through candidate lists: idx are table indices
    cand = np.array([[3, 17, 39, 4, 12, 30, -1, 8, 9]] * 6, dtype=np.int32); cand[1, :3] = -1; cand[3] = -1
    cs = _scores(y, words, il, cand=cand)
    idx, val = _topk(cs, k, cand)
    ri, rv = _topk_ref(cs, k, cand)
    assert np.array_equal(idx, ri) and np.array_equal(val, rv) and (idx[3] == -1).all()


def test_topk_over_long_rows_with_many_ties():
    """Rows longer than the workgroup has threads (every thread's list fills and overflows), values quantised so that ties are everywhere, -inf and
    NaN entries never chosen."""
    rs = np.random.RandomState(3)
    scores = -np.round(rs.exponential(3.0, size=(5, 5003)) * 4).astype(np.float32) / 4
    scores[:, ::7] = NEG_INF
    scores[1, 5::11] = np.nan
    scores[2] = NEG_INF; scores[2, [4000, 17, 4999]] = [-1.0, -1.0, -9.0]
    scores[3, :] = -2.5                                               # one value everywhere: positions 0..7
    scores[4, 256 * np.arange(12) + 3] = 0.0                              # twelve ties in ONE thread's strided share: its list keeps the first eight
    for k in (1, 8):
        idx, val = _topk(scores, k)
        ri, rv = _topk_ref(np.where(np.isnan(scores), NEG_INF, scores), k)
        assert np.array_equal(idx, ri) and np.array_equal(val, rv), k
    assert idx[3].tolist() == list(range(8)) and idx[2].tolist() == [17, 4000, 4999, -1, -1, -1, -1, -1]


# ---- 6. untrusted tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [38, 128])
def test_untrusted_table_entries_score_minus_infinity_and_leave_their_neighbours_alone(C):
    """Validation of inputs: lengths and labels outside their ranges score -inf and index nothing; the guard words around them keep their scores."""
    T, Lmax = 20, 31
    y = np.array(posteriors(C, T))
    il = np.array([T, 13, T, T, 16, 9])
    words = make_words(C, n=24, seed=7, lengths=(1, 3, 7, 5, 15, 2))
    lab, ll = table(words, width=Lmax)
    clean = _scores(y, None, il, lab=lab, ll=ll)
    assert np.isfinite(clean).any()
    bad = {2: ("len", -1), 5: ("len", Lmax + 1), 9: ("len", 1 << 30), 10: ("id", C - 1), 13: ("id", C), 14: ("id", -1), 19: ("id", 1 << 30),
           23: ("len", -(1 << 31))}
    lab2, ll2 = lab.copy(), ll.copy()
    for n, (kind, v) in bad.items():
        if kind == "len":
            ll2[n] = v
        else:
            assert ll2[n] >= 1
            lab2[n, ll2[n] - 1] = v
    got = _scores(y, None, il, lab=lab2, ll=ll2)
    good = [n for n in range(24) if n not in bad]
    assert np.isneginf(got[:, sorted(bad)]).all() and np.isfinite(clean[:, sorted(bad)]).sum() >= 8      # (they had scores to lose)
    assert np.array_equal(got[:, good], clean[:, good])
    # the same through a candidate list
    cand = np.tile(np.arange(24, dtype=np.int32), (6, 1))
    assert np.array_equal(_scores(y, None, il, lab=lab2, ll=ll2, cand=cand), got)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    B, T, C, N = 6, 20, 38, 40
    y = dev(np.array(posteriors(C, T)))
    lab, ll = table(make_words(C, n=N, seed=0), width=31)
    labd, lld = dev(lab, np.int32), dev(ll, np.int32)
    out = torch.full((B, N), 7.0, device="cuda")
    ws = torch.full((B * T * 129,), 3.0, device="cuda")
    big = ws.numel() * 4

    def call(y_=y, words=labd, wl=lld, scores=out, ws_=ws, nbytes=big, C_=C, Lmax=31):
        return L().crnn_ctc_lexicon_score(P(y_), None, P(words), P(wl), None, P(scores), P(ws_), nbytes, B, T, C_, 0, N, Lmax, 0, S())
    assert call(C_=129) == -3 and call(Lmax=32) == -3
    assert call(y_=None) == -2 and call(words=None) == -2 and call(wl=None) == -2 and call(scores=None) == -2 and call(ws_=None) == -2
    assert call(nbytes=B * T * C * 4 - 4) == -2
    idx = torch.full((B, 3), 77, dtype=torch.int32, device="cuda"); val = torch.full((B, 3), 5.0, device="cuda")
    assert L().crnn_ctc_lexicon_topk(P(out), None, P(idx), P(val), B, N, 0, S()) == -2
    assert L().crnn_ctc_lexicon_topk(P(out), None, P(idx), P(val), B, N, 9, S()) == -2
    assert L().crnn_ctc_lexicon_topk(None, None, P(idx), P(val), B, N, 3, S()) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 3.0).all()) and bool((idx == 77).all()) and bool((val == 5.0).all())
    assert call(nbytes=B * T * C * 4) == 0                    # the exact size is enough
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ---- 8. surface --------------------------------------------------------------------------------------------------------------------------------------------
_CHARS = [chr(33 + i) for i in range(96)]


def _tol(v):
    return 1e-3 + 1e-4 * abs(v)


def _assert_best(words_chosen, ref, texts, what):
    """`words_chosen[b]` must be the reference's arg-max (first maximum: the earlier table index); where the reference's runner-up is within the
    scores' tolerance of the best, any word that close to the best is accepted."""
    for b, w in enumerate(words_chosen):
        best = int(np.argmax(ref[b]))
        near = [texts[n] for n in range(len(texts)) if ref[b, n] >= ref[b, best] - 2 * _tol(ref[b, best])]
        assert w == texts[best] or w in near, (what, b, w, texts[best])


def test_lexicon_decoder_on_a_models_own_posteriors():
    model = U.init_predictor(U.CRNN(num_classes=97, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model())
    x = np.random.RandomState(5).normal(size=(8, 100, 32, 1)).astype(np.float32)
    y = model.predict_on_batch(x)
    assert y.shape == (8, 52, 97)
    rs = np.random.RandomState(6)
    ids = [rs.randint(0, 96, size=rs.randint(0, 9)).tolist() for _ in range(70)] + [rs.randint(64, 96, size=4).tolist(), list(range(64, 95))]
    caller = ["".join(_CHARS[c] for c in w) for w in ids] + ["not\tspellable"]
    with pytest.warns(UserWarning):
        lex = U.Lexicon(caller, dict(enumerate(_CHARS)))
    assert len(lex) == 72 and len(lex.rejected) == 1 and lex.labels.max() >= 64
    ref = _ref_scores(y, [lex.labels[i, :lex.lengths[i]].tolist() for i in range(len(lex))], None, 0)      # in table order
    dec = U.LexiconDecoder(lex, top_paths=3)
    best = dec.decode(y)
    _assert_best(best, ref, lex.words, "decode")
    assert dec.decode(torch.from_numpy(y).cuda()) == best                  # a device tensor or an ndarray
    assert U.LexiconDecoder(lex, top_paths=3, score_bytes=3 * 72 * 4).decode(y) == best       # chunks of three images
    words, lp = dec.decode_topk(y)
    assert [w[0] for w in words] == best and lp.shape == (8, 3) and (np.diff(lp, axis=1) <= 0).all()
    for b in range(8):
        for j in range(3):
            n = lex.words.index(words[b][j])
            assert abs(lp[b, j] - ref[b, n]) <= _tol(ref[b, n])
        assert lp[b, 2] >= np.sort(ref[b])[-3] - _tol(ref[b].max())
    # label rows: DecodeCTCPred.decode_labels' contract
    rows = dec.decode_labels(y)
    assert rows.dtype == np.int32 and rows.shape == (8, lex.labels.shape[1]) and [dec.labels_to_text(r) for r in rows] == best
    drows, dlens = dec.decode_labels(torch.from_numpy(y).cuda(), device=True)
    assert drows.is_cuda and dlens.is_cuda and drows.dtype == torch.int32 and dlens.dtype == torch.int32
    assert np.array_equal(host(drows), rows) and host(dlens).tolist() == [len(w) for w in best]
    # candidates, as caller positions: image b may only be words b .. b + 3 of the caller's list (and the unspellable one)
    cands = [[b, b + 1, b + 2, b + 3, 72] for b in range(8)]
    got = dec.decode(y, candidates=cands)
    for b in range(8):
        tab = [int(lex.index_of[p]) for p in cands[b][:4]]
        sub = ref[b, tab]
        assert got[b] in [lex.words[t] for t, v in zip(tab, sub) if v >= sub.max() - 2 * _tol(sub.max())]
    assert dec.decode(y, candidates=[[72]] * 8) == [""] * 8 and dec.decode(y, candidates=[[]] * 8) == [""] * 8
    w2, lp2 = dec.decode_topk(y, candidates=np.full((8, 2), -1))
    assert w2 == [["", "", ""]] * 8 and np.isneginf(lp2).all()
    # the confidence of a transcription: the exact CTC log-probability of the beam decoder's own result
    beam = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=dict(enumerate(_CHARS)))
    beam_rows = beam.decode_labels(y)
    texts = [beam.labels_to_text(r) for r in beam_rows]
    conf = dec.log_prob(y, texts)
    want = np.array([_ref_scores(y[b:b + 1], [[int(c) for c in beam_rows[b] if c != -1]], None, 0)[0, 0] for b in range(8)])
    assert conf.shape == (8,) and np.array_equal(np.isneginf(conf), np.isneginf(want))
    fin = np.isfinite(want)
    assert fin.any() and (np.abs(conf[fin] - want[fin]) <= 1e-3 + 1e-4 * np.abs(want[fin])).all()
    assert np.isneginf(dec.log_prob(y, ["not\tspellable"] * 8)).all() and np.isneginf(dec.log_prob(y, ["!" * 32] * 8)).all()
    # an empty lexicon decodes everything to ""
    with pytest.warns(UserWarning):
        none = U.LexiconDecoder(U.Lexicon(["\t"], dict(enumerate(_CHARS))))
    assert none.decode(y) == [""] * 8 and (none.decode_labels(y) == -1).all()


def _make_dataset(folder, n, seed=0):
    from PIL import Image, ImageDraw
    rs = np.random.RandomState(seed)
    alphabet = "abcdefghij0123"
    names = []
    for i in range(n):
        word = "".join(rs.choice(list(alphabet), size=rs.randint(2, 6)))
        img = Image.new("L", (20 + 12 * len(word), 28), color=235 if i % 3 else 30)
        ImageDraw.Draw(img).text((4, 6), word, fill=20 if i % 3 else 230)
        names.append(os.path.join(folder, "%d_%s_%d.png" % (i, word, i)))
        img.save(names[-1])
    return names


def _classes():
    return {ch: i for i, ch in enumerate(U.get_lexicon())}


def test_validation_with_a_lexicon_decoder_and_the_cli(tmp_path, capsys):
    """Model.score_generator and metrics.Score with a LexiconDecoder, unmodified; predict.py --lexicon in this process (both scoring routes print the
    same report) and in a fresh one."""
    inv = {v: k for k, v in _classes().items()}
    m = U.CRNN(num_classes=38, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()
    model = U.init_predictor(m)
    fdir = tmp_path / "files"
    os.makedirs(fdir)
    names = _make_dataset(str(fdir), n=21)
    truth_words = [os.path.basename(n).split("_")[1] for n in names]
    caller = sorted(set(truth_words)) + ["zebra", "", "0", "Unspellable"]
    with pytest.warns(UserWarning):
        lex = U.Lexicon(caller, inv)
    dec = U.LexiconDecoder(lex)
    kw = dict(img_size=(100, 32, 1), normed=True, batch_size=8, classes=_classes(), max_len=23, transform_p=0.)
    reader = U.Readf(**kw)
    y = model.predict_generator(reader.run_generator(names), steps=3)[:21]
    true_texts = [dec.labels_to_text(r) for r in reader.get_labels(names)]
    assert true_texts == truth_words
    texts = dec.decode(y)
    ref = _ref_scores(y, [lex.labels[i, :lex.lengths[i]].tolist() for i in range(len(lex))], None, 0)
    _assert_best(texts, ref, lex.words, "validation")
    score = model.score_generator(U.Readf(**kw).run_generator(names), steps=3, decoder=dec, length=21)
    assert isinstance(score, U.Score) and len(score) == 21 and score.texts(dec) == texts
    assert score.distances.tolist() == [int(U.levenshtein(p, t)) for p, t in zip(texts, true_texts)]
    assert score.edit_distance == U.edit_distance(texts, true_texts) and score.normalized_edit_distance == U.normalized_edit_distance(texts, true_texts)
    # the reference's own verdict on "a lexicon of the truth words helps": whatever it says, the device says the same
    ref_texts = [lex.words[int(np.argmax(ref[b]))] for b in range(21)]
    beam = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=inv)
    beam_ed = U.edit_distance(beam.decode(y), true_texts)
    ref_ed = U.edit_distance(ref_texts, true_texts)
    print("mean edit distance: lexicon (reference scores) %.4f, lexicon (device) %.4f, beam %.4f" % (ref_ed, score.edit_distance, beam_ed))
    if texts == ref_texts:                                    # (no near-tie was resolved the other way: _assert_best above allows only those)
        assert score.edit_distance == ref_ed and (score.edit_distance <= beam_ed) == (ref_ed <= beam_ed)
    # the command line
    mdir = tmp_path / "models" / "m1"
    os.makedirs(mdir)
    U.save_model_json(m, str(tmp_path / "models"), "m1")
    m.save_weights(str(mdir / "final_weights.h5"))
    lexfile = tmp_path / "words.txt"
    lexfile.write_text("\n".join(caller) + "\n")
    sys.path.insert(0, PKG)
    import predict as predict_cli
    base = ["--model_path", str(mdir), "--image_path", str(fdir), "--batch_size", "8", "--G", "0", "--validate", "--train_portion", "0.5",
            "--lexicon", str(lexfile)]
    seen = []
    for flags in ([], ["--device_score"], ["--device_score", "--device_ingest"]):
        res = tmp_path / ("res%d" % len(flags))
        os.makedirs(res)
        capsys.readouterr()
        predict_cli.main(base + ["--result_path", str(res)] + flags)
        out = capsys.readouterr().out
        line = [l for l in out.splitlines() if "mean edit distance" in l]
        assert len(line) == 1 and len([l for l in out.splitlines() if "rejected" in l]) == 1 and "%d words, 1 rejected" % len(lex) in out
        import pandas as pd
        df = pd.read_csv(res / "prediction.csv", dtype=str, keep_default_na=False)
        assert len(df) == 11 and set(df["prediction"]) <= set(lex.words)
        seen.append((line[0], df["prediction"].tolist()))
    assert seen[0] == seen[1] and seen[2][0] == seen[0][0]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    res = tmp_path / "fresh"
    os.makedirs(res)
    done = subprocess.run([sys.executable, os.path.join(PKG, "predict.py")] + base + ["--device_score", "--result_path", str(res)], env=env,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:]
    assert [l for l in done.stdout.splitlines() if "mean edit distance" in l] == [seen[0][0]]
    assert open(res / "prediction.csv").read() == open(tmp_path / "res1" / "prediction.csv").read()
