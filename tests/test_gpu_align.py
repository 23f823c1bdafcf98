"""-m gpu tests of the character alignment (csrc/align.hip, crnn_mi355x/align.py): the best CTC path of one transcription per sample, its states,
character spans and per-character sums, bit for bit against the np.float32 replay of tests/align_ref.py run over the lsm map the device's own
pre-pass wrote (the uniform sample of lexicon_ref.posteriors makes that a test of the tie rule), and within the project's CTC tolerance of the
fp64 Viterbi (pinned to a brute-force enumeration in tests/test_align_cpu.py); the workspace against the lexicon kernel's; the longest words and
the 16-frame boundaries of the backpointer words; a planted path; invariants; untrusted input and refusals; the Python surface and
predict.py --align.  The shapes are the smallest at which the kernel takes every path."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import utils as U
from gpu_util import L, dev, zeros, P, S, ok, host
from lexicon_ref import _ref_scores, posteriors, input_lengths, make_words, table, SEGMENT_LENGTHS
from align_ref import viterbi_f64, viterbi_f32_replay, path_is_valid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
NEG_INF = float("-inf")
KEYS = ("score", "states", "start", "end", "char_logp")
FILL = {"score": 7.0, "states": 77, "start": 78, "end": 79, "char_logp": 5.0}


def _align(y, words=None, il=None, skip=0, width=31, lab=None, ll=None, want=KEYS, pad=-1):
    """One call of crnn_ctc_align -> ({name: ndarray}, lsm (B, T - skip, C) as the pre-pass left it in the workspace).  y (B, T, C) float32 ndarray;
    words: one id sequence per sample (or lab / ll: ready rows).  Outputs not in `want` are passed as NULL; all are pre-filled with FILL."""
    B, T, C = y.shape
    if lab is None:
        lab, ll = table(words, width=width, pad=pad)
    Lmax = lab.shape[1]
    shapes = {"score": (B,), "states": (B, T - skip), "start": (B, Lmax), "end": (B, Lmax), "char_logp": (B, Lmax)}
    out = {k: torch.full(shapes[k], FILL[k], dtype=torch.float32 if k in ("score", "char_logp") else torch.int32, device="cuda") for k in KEYS}
    nbytes = L().crnn_ctc_align_workspace_bytes(B, T, C, skip)
    assert nbytes == B * (T - skip) * C * 4
    ws = zeros(nbytes // 4)
    ptr = lambda k: P(out[k]) if k in want else None
    ok(L().crnn_ctc_align(P(dev(y)), P(dev(il, np.int32)) if il is not None else None, P(dev(lab, np.int32)), P(dev(ll, np.int32)), ptr("score"),
                          ptr("states"), ptr("start"), ptr("end"), ptr("char_logp"), P(ws), nbytes, B, T, C, skip, Lmax, S()))
    return {k: host(out[k]) for k in KEYS}, host(ws).reshape(B, T - skip, C)


def _assert_equals_replay(got, lsm, words, il, width, what):
    """Bit for bit, the -inf and -1 patterns included.  -> the replay"""
    ref = dict(zip(KEYS, viterbi_f32_replay(lsm, words, il, width=width)))
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(got[k], ref[k]), "%s: %s differs at %s" % (what, k, np.argwhere(got[k] != ref[k])[:5].tolist())
    return ref


def _assert_scores(got, ref, what):
    """The project's CTC tolerance (rtol 1e-4, atol 1e-3, as the loss tests) on the finite entries; the -inf pattern must be equal."""
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), "%s: -inf pattern differs" % what
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all() and not np.isnan(got).any()
    if fin.any():
        err = np.abs(got[fin] - ref[fin])
        assert (err <= 1e-3 + 1e-4 * np.abs(ref[fin])).all(), "%s: max|diff| %.3e" % (what, err.max())


# ---- 1. bit-exact against the replay ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [0, 2])
@pytest.mark.parametrize("C", [38, 66, 97, 128])
def test_alignment_equals_the_replay_bit_for_bit(C, skip):
    B, T, N = 6, 20, 21
    y = np.array(posteriors(C, T))
    il = input_lengths(T, skip)
    words = make_words(C, n=N, seed=0)
    words[9] = [3, 3, 3]                                     # tripled: 5 frames
    assert sorted(set(len(w) for w in words if w != [3, 3, 3])) == sorted(SEGMENT_LENGTHS)
    assert any(len(w) >= 2 and w[0] == w[1] for w in words) and any(len(w) >= 3 and w[0] == w[1] == w[2] for w in words)
    if C >= 66:
        used = np.concatenate([w for w in words if w])
        assert (used >= 64).any() and (used < 64).any() and used.max() <= C - 2 and any(w and min(w) >= 64 for w in words)
    fin = inf = ties = 0
    for call in range(N):                                    # one word per sample; over the calls every sample meets every word
        per_sample = [words[(call + b) % N] for b in range(B)]
        got, lsm = _align(y, per_sample, il, skip)
        ref = _assert_equals_replay(got, lsm, per_sample, il, 31, "C=%d skip=%d call %d" % (C, skip, call))
        fin += np.isfinite(got["score"]).sum(); inf += np.isneginf(got["score"]).sum()
        ties += int(np.isfinite(got["score"][1]) and len(per_sample[1]) >= 1)       # sample 1 is exactly uniform: every choice there is a tie
        assert (got["states"] == -1).any() and (got["states"] >= 0).any() and (got["start"] == -1).any() and np.isneginf(got["char_logp"]).any()
        _assert_scores(got["score"].astype(np.float64), viterbi_f64(y, per_sample, il, skip, width=31)[0], "C=%d skip=%d call %d" % (C, skip, call))
        assert got["score"][5] == (0.0 if not per_sample[5] else NEG_INF)            # Tb = 0: exactly 0 for the empty word
        for b in range(B):
            if np.isfinite(ref["score"][b]):
                assert path_is_valid(got["states"][b, :min(il[b], T - skip)].tolist(), per_sample[b], C - 1)
    assert fin >= 20 and inf >= 20 and ties >= 5
    # NULL input lengths: the whole window
    per_sample = [words[(3 + b) % N] for b in range(B)]
    got, lsm = _align(y, per_sample, None, skip)
    _assert_equals_replay(got, lsm, per_sample, None, 31, "C=%d skip=%d, no lengths" % (C, skip))
    assert np.isfinite(got["score"]).sum() >= 3 and (got["states"][np.isfinite(got["score"])] >= 0).all()


# ---- 2. the workspace -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,skip", [(38, 0), (38, 2), (128, 2)])
def test_workspace_is_the_lexicon_kernels_bit_for_bit(C, skip):
    B, T = 6, 20
    y = np.array(posteriors(C, T))
    words = make_words(C, n=6, seed=0)
    _, lsm = _align(y, words, None, skip)
    lab, ll = table(words, width=31)
    nbytes = L().crnn_ctc_lexicon_workspace_bytes(B, T, C, skip)
    ws = zeros(nbytes // 4)
    scores = zeros(B, 6)
    ok(L().crnn_ctc_lexicon_score(P(dev(y)), None, P(dev(lab, np.int32)), P(dev(ll, np.int32)), None, P(scores), P(ws), nbytes, B, T, C, skip, 6, 31, 0, S()))
    other = host(ws).reshape(B, T - skip, C)
    assert np.isfinite(lsm).all() and np.array_equal(lsm.view(np.uint32), other.view(np.uint32))


# ---- 3. longest words, backpointer word boundaries ------------------------------------------------------------------------------------------------
def test_longest_words_and_backpointer_word_boundaries():
    """Input lengths on both sides of every 16-frame backpointer word up to four words and a partial fifth; 31 letters fill all 63 states."""
    C, T, B = 38, 66, 9
    base = posteriors(C, T)
    y = np.stack([base[b % 6] for b in range(B)])
    il = np.array([15, 16, 17, 31, 32, 33, 62, 63, 66])
    plain = list(range(31))
    doubled = list(range(30)); doubled.insert(7, 7)             # 31 letters, one doubled: 32 frames at least
    assert len(doubled) == 31 and doubled[7] == doubled[8]
    for word, first in ((plain, 31), (doubled, 32), (list(range(7)), 7), ([], 0)):
        got, lsm = _align(y, [word] * B, il, 0)
        _assert_equals_replay(got, lsm, [word] * B, il, 31, "T=66, %d letters" % len(word))
        assert np.array_equal(np.isfinite(got["score"]), il >= first), (len(word), got["score"])
        _assert_scores(got["score"].astype(np.float64), viterbi_f64(y, [word] * B, il, 0, width=31)[0], "T=66")
    assert (got["states"][8] == 0).all()                      # the empty word: every frame in state 0


# ---- 4. a planted path ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [38, 128])
def test_a_planted_path_is_recovered(C):
    hi = 100 if C == 128 else 30
    word = [4, 4, 9, hi]                                     # a doubled letter; one label >= 64 at C = 128
    # leading blanks, 'a', the blank between the doubled letters, 'a' held three frames, then b and c with no blank between distinct letters, trailing blanks
    planted = [0, 0, 1, 2, 3, 3, 3, 5, 7, 8, 8]
    assert path_is_valid(planted, word, C - 1)
    T = len(planted)
    ext = [C - 1 if s % 2 == 0 else word[s // 2] for s in range(9)]
    y = np.full((2, T + 3, C), 0.1 / (C - 1), dtype=np.float32)
    for t, s in enumerate(planted):
        y[0, t, ext[s]] = 0.9
        y[1, t + 2, ext[s]] = 0.9                            # the same through skip = 2
    for skip, b in ((0, 0), (2, 1)):
        got, lsm = _align(y[b:b + 1], [word], np.array([T]), skip, width=6)
        assert got["states"][0, :T].tolist() == planted and (got["states"][0, T:] == -1).all()
        assert got["start"][0].tolist() == [2, 4, 7, 8, -1, -1] and got["end"][0].tolist() == [3, 7, 8, 9, -1, -1]
        assert np.isfinite(got["char_logp"][0, :4]).all() and np.isneginf(got["char_logp"][0, 4:]).all()
        assert abs(got["score"][0] - T * np.log(0.9)) < 1e-3
        assert abs(got["char_logp"][0, 1] - 3 * np.log(0.9)) < 1e-3
        _assert_equals_replay(got, lsm, [word], np.array([T]), 6, "planted")


# ---- 5. invariants -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [38, 97])
def test_invariants_of_the_best_path(C):
    B, T, skip = 6, 20, 0
    y = np.array(posteriors(C, T))
    il = np.array([T, 13, 7, T, 16, 9])
    words = make_words(C, n=12, seed=3, lengths=(0, 1, 3, 7, 2, 5))
    total = _ref_scores(y, words, il, skip)
    checked = 0
    for call in range(12):
        per_sample = [words[(call + b) % 12] for b in range(B)]
        got, lsm = _align(y, per_sample, il, skip)
        lab, ll = table(per_sample, width=31)
        nbytes = L().crnn_ctc_lexicon_workspace_bytes(B, T, C, skip)
        lex, lex_ws = zeros(B, 1), zeros(nbytes // 4)
        cand = np.arange(B, dtype=np.int32).reshape(B, 1)     # sample b against word b: log_prob's way
        ok(L().crnn_ctc_lexicon_score(P(dev(y)), P(dev(il, np.int32)), P(dev(lab, np.int32)), P(dev(ll, np.int32)), P(dev(cand, np.int32)), P(lex),
                                      P(lex_ws), nbytes, B, T, C, skip, B, 31, 1, S()))
        lex = host(lex)[:, 0]
        for b in range(B):
            w, Tb = per_sample[b], int(il[b])
            sc = got["score"][b]
            assert np.isneginf(sc) == np.isneginf(lex[b]) == np.isneginf(total[b, (call + b) % 12])
            if not np.isfinite(sc):
                continue
            checked += 1
            path = got["states"][b, :Tb].tolist()
            assert path_is_valid(path, w, C - 1) and (got["states"][b, Tb:] == -1).all()
            assert sc <= lex[b] + 1e-3 + 1e-4 * abs(lex[b])              # the best path never above the total probability
            blanks = sum(float(lsm[b, t, C - 1]) for t in range(Tb) if path[t] % 2 == 0)
            chars = float(got["char_logp"][b, :len(w)].astype(np.float64).sum())
            assert abs(chars + blanks - sc) <= 1e-4 * abs(sc) + 1e-6
            st, en = got["start"][b, :len(w)], got["end"][b, :len(w)]
            assert (st < en).all() and (st[1:] >= en[:-1]).all() and (len(w) == 0 or (st[0] >= 0 and en[-1] <= Tb))
    assert checked >= 30


# ---- 6. untrusted input, refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [38, 128])
def test_untrusted_rows_get_no_alignment_and_leave_their_neighbours_alone(C):
    T, Lmax, B = 20, 8, 12
    base = posteriors(C, T)
    y = np.stack([base[(0, 2, 4)[b % 3]] for b in range(B)])
    words = make_words(C, n=B, seed=7, lengths=(3, 5, 7, 2, 8, 4))
    lab, ll = table(words, width=Lmax, pad=-5)
    il = np.full(B, T, dtype=np.int32)
    clean, _ = _align(y, None, il, 0, lab=lab, ll=ll)
    assert np.isfinite(clean["score"]).all()
    bad = {1: ("len", -1), 3: ("len", 32), 4: ("len", Lmax + 1), 6: ("id", -1), 7: ("id", C - 1), 9: ("len", 1 << 30), 10: ("id", 1 << 30)}
    lab2, ll2, il2 = lab.copy(), ll.copy(), il.copy()
    for b, (kind, v) in bad.items():
        if kind == "len":
            ll2[b] = v
        else:
            lab2[b, ll2[b] - 1] = v
    il2[0] = T + 1000; il2[5] = 1 << 30                      # beyond the map: clamped to the window (the header's contract), nothing read past it
    got, _ = _align(y, None, il2, 0, lab=lab2, ll=ll2)
    rows = sorted(bad)
    good = [b for b in range(B) if b not in bad]
    assert np.isneginf(got["score"][rows]).all() and (got["states"][rows] == -1).all() and (got["start"][rows] == -1).all()
    assert (got["end"][rows] == -1).all() and np.isneginf(got["char_logp"][rows]).all()
    for k in KEYS:                                           # the neighbours: as in the launch without the bad rows
        assert np.array_equal(got[k][good], clean[k][good]), k
    # slots past the length: -1 / -inf over the sentinel, every one written
    for b in good:
        n = ll[b]
        assert (got["start"][b, :n] >= 0).all() and (got["start"][b, n:] == -1).all() and (got["end"][b, n:] == -1).all()
        assert np.isfinite(got["char_logp"][b, :n]).all() and np.isneginf(got["char_logp"][b, n:]).all()
    # a row stride as large as T, any padding; NULL optional outputs
    wide, _ = _align(y, words, il, 0, width=T, pad=1 << 20)
    for k in ("start", "end", "char_logp"):
        assert np.array_equal(wide[k][:, :Lmax], clean[k]) and (wide[k][:, Lmax:] == (NEG_INF if k == "char_logp" else -1)).all()
    assert np.array_equal(wide["score"], clean["score"]) and np.array_equal(wide["states"], clean["states"])
    only, _ = _align(y, None, il, 0, lab=lab, ll=ll, want=("score",))
    assert np.array_equal(only["score"], clean["score"]) and all((only[k] == FILL[k]).all() for k in KEYS[1:])
    some, _ = _align(y, None, il, 0, lab=lab, ll=ll, want=("score", "start", "char_logp"))
    assert np.array_equal(some["start"], clean["start"]) and np.array_equal(some["char_logp"], clean["char_logp"])
    assert (some["states"] == FILL["states"]).all() and (some["end"] == FILL["end"]).all()


@pytest.mark.parametrize("C", [38, 128])
def test_a_map_that_is_no_softmax_map_gets_no_alignment_and_leaves_its_neighbours_alone(C):
    """A NaN frame, an infinite or a negative entry (a diverged model) makes the whole lsm row NaN and with it every state's value: no alignment,
    every slot -1 / -inf, and nothing read through a span that the path never marked.  Beyond input_len such a frame is never looked at."""
    T, Lmax, B = 20, 8, 12
    base = posteriors(C, T)
    y = np.stack([base[(0, 2, 4)[b % 3]] for b in range(B)])
    words = make_words(C, n=B, seed=7, lengths=(3, 5, 7, 2, 8, 4))
    il = np.array([T, T, T, 13, T, T, 13, T, T, T, T, T], dtype=np.int32)
    clean, _ = _align(y, words, il, 0, width=Lmax)
    assert np.isfinite(clean["score"]).all()
    y2 = y.copy()
    y2[1, 7, :] = np.nan                                     # a whole frame
    y2[2, 0, 3] = np.nan                                     # one entry of the first frame
    y2[4, T - 1, C - 1] = np.inf
    y2[7, 5, 0] = -0.5                                       # log of a negative number
    y2[8, :, :] = np.nan
    y2[10, 11, 2] = -np.inf
    y2[3, 15, :] = np.nan; y2[6, 13, 1] = -1.0               # beyond input_len = 13: not part of the window's path
    bad = [1, 2, 4, 7, 8, 10]
    good = [b for b in range(B) if b not in bad]
    for _ in range(2):                                       # twice: the second launch meets whatever the first left in LDS
        got, lsm = _align(y2, words, il, 0, width=Lmax)
        assert np.isnan(lsm[bad]).any(axis=(1, 2)).all() and np.isfinite(lsm[good][:, :13]).all()
        assert np.isneginf(got["score"][bad]).all() and (got["states"][bad] == -1).all() and (got["start"][bad] == -1).all()
        assert (got["end"][bad] == -1).all() and np.isneginf(got["char_logp"][bad]).all()
        for k in KEYS:
            assert np.array_equal(got[k][good], clean[k][good]), k


def test_the_frame_limit_is_512():
    C, B, skip = 38, 2, 2
    rs = np.random.RandomState(11)
    logits = rs.normal(size=(B, 514, C)) * 2.0
    e = np.exp(logits - logits.max(-1, keepdims=True))
    y = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    words = [rs.randint(0, C - 1, size=31).tolist(), [5, 5, 5, 1, 2, 3, 4]]
    il = np.array([512, 499])
    got, lsm = _align(y, words, il, skip)
    assert lsm.shape == (B, 512, C)
    _assert_equals_replay(got, lsm, words, il, 31, "512 frames")
    assert np.isfinite(got["score"]).all() and (got["states"][0] >= 0).all() and got["states"][0, 511] in (61, 62) and (got["states"][1, 499:] == -1).all()
    _assert_scores(got["score"].astype(np.float64), viterbi_f64(y, words, il, skip, width=31)[0], "512 frames")


def test_refusals_write_nothing():
    B, T, C = 6, 20, 38
    y = dev(np.array(posteriors(C, T)))
    lab, ll = table(make_words(C, n=B, seed=0), width=31)
    labd, lld = dev(lab, np.int32), dev(ll, np.int32)
    out = {k: torch.full((B, T if k == "states" else 31) if k != "score" else (B,), FILL[k], dtype=torch.float32 if k in ("score", "char_logp") else torch.int32,
                         device="cuda") for k in KEYS}
    ws = torch.full((B * 520 * 129,), 3.0, device="cuda")
    big = ws.numel() * 4

    def call(y_=y, labels=labd, wl=lld, score=out["score"], ws_=ws, nbytes=big, B_=B, T_=T, C_=C, skip=0, Lmax=31):
        return L().crnn_ctc_align(P(y_), None, P(labels), P(wl), P(score), P(out["states"]), P(out["start"]), P(out["end"]), P(out["char_logp"]),
                                  P(ws_), nbytes, B_, T_, C_, skip, Lmax, S())
    assert call(C_=129) == -3 and call(T_=513) == -3 and call(T_=515, skip=2) == -3
    assert call(y_=None) == -2 and call(labels=None) == -2 and call(wl=None) == -2 and call(score=None) == -2 and call(ws_=None) == -2
    assert call(B_=-1) == -2 and call(C_=1) == -2 and call(T_=2, skip=2) == -2 and call(Lmax=0) == -2 and call(skip=-1) == -2
    assert call(nbytes=B * T * C * 4 - 4) == -2
    assert call(B_=0) == 0
    torch.cuda.synchronize()
    assert all(bool((out[k] == FILL[k]).all()) for k in KEYS) and bool((ws == 3.0).all())
    assert call(nbytes=B * T * C * 4) == 0                    # the exact size is enough
    torch.cuda.synchronize()
    assert not bool((out["score"] == FILL["score"]).any()) and not bool((out["states"] == FILL["states"]).any())


# ---- 7. surface ---------------------------------------------------------------------------------------------------------------------------------
_CHARS = [chr(33 + i) for i in range(96)]


def test_align_decoded_after_beam_greedy_and_lexicon_decoders():
    model = U.init_predictor(U.CRNN(num_classes=97, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model())
    x = np.random.RandomState(5).normal(size=(8, 100, 32, 1)).astype(np.float32)
    y = model.predict_on_batch(x)
    assert y.shape == (8, 52, 97)
    inv = dict(enumerate(_CHARS))
    rs = np.random.RandomState(6)
    lexicon = U.Lexicon(["".join(_CHARS[c] for c in rs.randint(0, 96, size=rs.randint(0, 9))) for _ in range(70)], inv)
    scorer = U.LexiconDecoder(lexicon)
    aligner = U.CTCAligner(inv)
    yd = torch.from_numpy(y).cuda()
    for decoder in (U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=inv), U.DecodeCTCPred(inverse_classes=inv, greedy=True), scorer):
        res = aligner.align_decoded(yd, decoder)
        texts = decoder.decode(y)
        assert [a.text for a in res] == texts and all(isinstance(a, U.Alignment) for a in res)
        total = scorer.log_prob(y, texts)
        aligned = 0
        for a, t, lp in zip(res, texts, total):
            assert a.states.shape == (52,) and np.isneginf(a.log_prob) == np.isneginf(lp)
            if np.isneginf(lp):
                assert a.chars == [] and len(t) > 31
                continue
            aligned += 1
            assert a.log_prob <= lp + 1e-3 + 1e-4 * abs(lp)
            assert [c.char for c in a.chars] == list(t) and all(isinstance(c, U.CharSpan) for c in a.chars)
            spans = [(c.start, c.end) for c in a.chars]
            assert all(0 <= s < e <= 52 for s, e in spans) and all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
            assert all(np.isfinite(c.log_prob) and c.log_prob <= 0 for c in a.chars)
        assert aligned >= 1
        again = aligner.align(y, texts)                      # the same through texts, from an ndarray
        assert [(a.text, a.log_prob, a.chars) for a in again] == [(a.text, a.log_prob, a.chars) for a in res]
    # the window of the training loss: spans come back in frames of the map
    texts = scorer.decode(y)
    a0 = aligner.align(y, texts)
    a2 = U.CTCAligner(inv, skip=2).align(y, texts)
    assert all(len(a.states) == 50 for a in a2) and all(c.start >= 2 for a in a2 for c in a.chars)
    out = aligner.align_labels(yd, *scorer.decode_labels(yd, device=True))
    assert all(out[k].is_cuda for k in KEYS) and np.array_equal(host(out["score"]), np.array([a.log_prob for a in a0], dtype=np.float32))
    # what cannot be spelled or is too long: no alignment
    odd = aligner.align(y, ["not\tspellable", "!" * 32] + texts[2:])
    assert odd[0].log_prob == NEG_INF and odd[0].chars == [] and odd[1].log_prob == NEG_INF and odd[1].chars == [] and odd[2].log_prob == a0[2].log_prob


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


def test_predict_cli_writes_alignment_csv(tmp_path, capsys):
    """predict.py --align in a fresh process writes alignment.csv, one row per prediction; prediction.csv and the report are those of a run without
    the flag (this process)."""
    m = U.CRNN(num_classes=38, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()
    fdir = tmp_path / "files"
    os.makedirs(fdir)
    _make_dataset(str(fdir), n=13)
    mdir = tmp_path / "models" / "m1"
    os.makedirs(mdir)
    U.save_model_json(m, str(tmp_path / "models"), "m1")
    m.save_weights(str(mdir / "final_weights.h5"))
    base = ["--model_path", str(mdir), "--image_path", str(fdir), "--batch_size", "8", "--G", "0", "--validate", "--train_portion", "0."]
    sys.path.insert(0, PKG)
    import predict as predict_cli
    plain = tmp_path / "plain"
    os.makedirs(plain)
    capsys.readouterr()
    predict_cli.main(base + ["--result_path", str(plain)])
    want = capsys.readouterr().out
    flagged = tmp_path / "flagged"
    os.makedirs(flagged)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    done = subprocess.run([sys.executable, os.path.join(PKG, "predict.py")] + base + ["--align", "--result_path", str(flagged)], env=env,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:]
    report = lambda text, folder: [l.replace(str(folder), "<result>") for l in text.splitlines() if " sec. " not in l]      # (all but the stopwatch lines)
    assert report(done.stdout, flagged) == report(want, plain) and any("mean edit distance" in l for l in report(want, plain))
    assert open(flagged / "prediction.csv", "rb").read() == open(plain / "prediction.csv", "rb").read()
    assert not os.path.exists(plain / "alignment.csv")
    rows = list(csv.reader(open(flagged / "alignment.csv", newline="")))
    pred = list(csv.reader(open(flagged / "prediction.csv", newline="")))
    assert rows[0] == ["fname", "prediction", "path_log_prob", "chars"] and len(rows) == len(pred) == 14
    for row, p in zip(rows[1:], pred[1:]):
        assert row[0] == p[1] and row[1] == p[2]
        lp = float(row[2])
        items = row[3].split(" ") if row[3] else []
        if not np.isfinite(lp):                              # a prediction longer than 31 characters has no alignment
            assert lp == NEG_INF and items == [] and len(row[1]) > 31
            continue
        assert lp <= 0 and len(items) == len(row[1])
        last = 0
        for item, ch in zip(items, row[1]):
            c, s, e, v = item.rsplit(":", 3)
            assert c == ch and last <= int(s) < int(e) <= 52 and float(v) <= 0
            last = int(e)
