"""CPU tests (no GPU) of lexicon decoding's host half: Lexicon's encoding, rejection list, stable length sort and its maps; predict.py's
--lexicon flag; the entry points' declarations, export and argument checks (those return before anything is launched); and the fp64 reference
the GPU tests use (tests/lexicon_ref.py), pinned to the CTC oracle and to torch.nn.functional.ctc_loss."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import utils as U
from crnn_mi355x import lexicon as LX
from crnn_mi355x import native
from oracle import ctc
from lexicon_ref import _ref_scores, log_softmax_of_log, posteriors, input_lengths, make_words, table, SEGMENT_LENGTHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
_CHARS = [chr(33 + i) for i in range(96)]                    # the 96-character alphabet of tests/test_gpu_alphabet.py


# ---- Lexicon -------------------------------------------------------------------------------------------------------------------------------
def test_lexicon_encodes_sorts_by_length_and_maps_back():
    inv = {i: ch for i, ch in enumerate(U.get_lexicon())}
    classes = {ch: i for i, ch in inv.items()}
    words = ["hello", "a", "", "world", "b", "be", "ab", "a", "x" * 31]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # nothing rejected: no warning
        lex = U.Lexicon(words, inv)
    assert U.Lexicon is LX.Lexicon and U.LexiconDecoder is LX.LexiconDecoder
    assert len(lex) == 9 and lex.rejected == []
    # stable: equal lengths keep the caller's order ("a" at 1 before "b" at 4 before the second "a" at 7)
    assert lex.words == ["", "a", "b", "a", "be", "ab", "hello", "world", "x" * 31]
    assert lex.order.tolist() == [2, 1, 4, 7, 5, 6, 0, 3, 8]
    assert [words[p] for p in lex.order] == lex.words
    assert lex.index_of.tolist() == [6, 1, 0, 7, 2, 4, 5, 3, 8] and all(lex.order[lex.index_of[p]] == p for p in range(9))
    assert lex.lengths.tolist() == [0, 1, 1, 1, 2, 2, 5, 5, 31] and lex.lengths.dtype == np.int32
    assert lex.labels.shape == (9, 31) and lex.labels.dtype == np.int32
    for i, w in enumerate(lex.words):
        assert lex.labels[i, :len(w)].tolist() == [classes[c] for c in w] and (lex.labels[i, len(w):] == -1).all()
    dec = U.LexiconDecoder(lex)
    assert dec.inverse_classes is inv and [dec.labels_to_text(r) for r in lex.labels] == lex.words
    assert dec.labels_to_text([classes["o"], 37, classes["k"], -1]) == "ok"


def test_lexicon_rejects_what_the_alphabet_cannot_spell_and_warns_once():
    inv = {i: ch for i, ch in enumerate(U.get_lexicon())}
    words = ["good", "Bad", "y" * 32, "also good".replace(" ", "-"), "café", ""]
    with pytest.warns(UserWarning) as rec:
        lex = U.Lexicon(words, inv)
    assert len(rec) == 1 and "3 of 6" in str(rec[0].message)
    assert lex.rejected == [(1, "Bad"), (2, "y" * 32), (4, "café")]
    assert lex.words == ["", "good", "also-good"] and lex.order.tolist() == [5, 0, 3]
    assert lex.index_of.tolist() == [1, -1, -1, 2, -1, 0]
    assert lex.encode("Bad") is None and lex.encode("y" * 32) is None and lex.encode("") == [] and len(lex.encode("y" * 31)) == 31
    # nothing accepted: an empty table with one column, and a decoder can still be built
    with pytest.warns(UserWarning):
        none = U.Lexicon(["A", "B"], inv)
    assert len(none) == 0 and none.labels.shape == (0, 1) and none.order.shape == (0,) and none.index_of.tolist() == [-1, -1]
    U.LexiconDecoder(none)


def test_lexicon_over_a_96_character_alphabet_reaches_the_upper_half():
    lex = U.Lexicon(["".join(_CHARS[c] for c in w) for w in ([95, 64, 3], [64], [0, 1], [])], _CHARS)          # a list as the alphabet
    assert lex.rejected == [] and lex.lengths.tolist() == [0, 1, 2, 3]
    assert lex.labels[1, 0] == 64 and lex.labels[3].tolist() == [95, 64, 3] and lex.labels.max() == 95
    assert U.Lexicon(["ab"], dict(enumerate(_CHARS))).labels.tolist() == [[ord("a") - 33, ord("b") - 33]]


def test_decoder_arguments_and_candidate_mapping():
    inv = {i: ch for i, ch in enumerate(U.get_lexicon())}
    with pytest.warns(UserWarning):
        lex = U.Lexicon(["ccc", "a", "NO", "bb"], inv)
    assert lex.words == ["a", "bb", "ccc"]
    for bad in (0, 9):
        with pytest.raises(ValueError):
            U.LexiconDecoder(lex, top_paths=bad)
    dec = U.LexiconDecoder(lex, top_paths=8, skip=2, score_bytes=1 << 20)
    assert (dec.top_paths, dec.skip, dec.score_bytes) == (8, 2, 1 << 20) and U.LexiconDecoder(lex).score_bytes == LX.SCORE_BYTES
    # caller positions -> table indices in ascending order; rejected, empty and out-of-range positions -> -1, last
    got = dec._candidates([[0, 1], [2], [], [3, 3, 7]], 4)
    assert got.dtype == np.int32 and got.tolist() == [[0, 2, -1], [-1, -1, -1], [-1, -1, -1], [1, 1, -1]]
    assert dec._candidates(np.array([[3, -1], [0, 9]]), 2).tolist() == [[1, -1], [2, -1]]
    assert dec._candidates(np.array([[-1, 0, 2, 3, 1]]), 1).tolist() == [[0, 1, 2, -1, -1]]
    with pytest.raises(ValueError):
        dec._candidates([[0]], 2)


def test_predict_cli_takes_a_lexicon_file():
    sys.path.insert(0, PKG)
    import predict as predict_cli
    base = ["--model_path", "m", "--image_path", "i"]
    assert predict_cli.parse_args(base).lexicon is None
    assert predict_cli.parse_args(base + ["--lexicon", "words.txt"]).lexicon == "words.txt"
    args = predict_cli.parse_args(base + ["--lexicon", "w.txt", "--validate", "--device_score", "--device_ingest"])
    assert args.lexicon == "w.txt" and args.validate and args.device_score and args.device_ingest
    with pytest.raises(SystemExit):
        predict_cli.parse_args(base + ["--lexicon"])


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    decl = native.parse_header()
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert decl["crnn_ctc_lexicon_workspace_bytes"] == (Z, [I, I, I, I])
    assert decl["crnn_ctc_lexicon_score"] == (I, [P] * 7 + [Z] + [I] * 7 + [P])
    assert decl["crnn_ctc_lexicon_topk"] == (I, [P] * 4 + [I] * 3 + [P])
    lib = ctypes.CDLL(native.LIB_PATH)
    assert all(hasattr(lib, n) for n in ("crnn_ctc_lexicon_workspace_bytes", "crnn_ctc_lexicon_score", "crnn_ctc_lexicon_topk"))
    assert "lexicon.hip" in native.SOURCES


def test_entry_points_reject_bad_arguments_before_launching():
    """Every check runs on the host before a launch, so the rejections need no GPU (the pointers are never followed)."""
    L = native.lib()
    fake = ctypes.c_void_p(1 << 20)
    assert L.crnn_ctc_lexicon_workspace_bytes(6, 20, 38, 2) == 6 * 18 * 38 * 4 and L.crnn_ctc_lexicon_workspace_bytes(1024, 52, 38, 0) == 1024 * 52 * 38 * 4
    assert L.crnn_ctc_lexicon_workspace_bytes(4, 2, 38, 2) == 0

    def score(y=fake, il=None, words=fake, wl=fake, cand=None, scores=fake, ws=fake, ws_bytes=1 << 30, B=6, T=20, C=38, skip=0, N=40, Lmax=31, K=0):
        return L.crnn_ctc_lexicon_score(y, il, words, wl, cand, scores, ws, ws_bytes, B, T, C, skip, N, Lmax, K, None)
    for name in ("y", "words", "wl", "scores", "ws"):
        assert score(**{name: None}) == -2, name
    assert score(B=-1) == -2 and score(N=-1) == -2 and score(Lmax=-1) == -2 and score(skip=-1) == -2 and score(T=2, skip=2) == -2 and score(C=1) == -2
    assert score(cand=fake, K=-1) == -2
    assert score(ws_bytes=6 * 20 * 38 * 4 - 1) == -2 and score(skip=2, ws_bytes=6 * 18 * 38 * 4 - 1) == -2
    assert score(C=129) == -3 and score(Lmax=32) == -3 and score(C=129, ws_bytes=0) == -3
    assert score(T=129, C=128) == -3 and score(T=131, C=128, skip=2) == -3                              # 128 frames x 128 classes = 64 KiB: the budget
    assert score(T=128, C=128, B=0) == 0 and score(T=130, C=128, skip=2, B=0) == 0 and score(T=129, C=128, B=0) == -3
    assert score(B=0) == 0 and score(N=0) == 0 and score(cand=fake, K=0) == 0                           # nothing to do: nothing launched
    assert score(B=0, y=None) == -2                                                                     # a null pointer is a bad argument whatever B is

    def topk(scores=fake, cand=None, idx=fake, val=fake, B=0, M=40, k=1):
        return L.crnn_ctc_lexicon_topk(scores, cand, idx, val, B, M, k, None)
    for name in ("scores", "idx", "val"):
        assert topk(**{name: None}) == -2, name
    assert topk(k=0) == -2 and topk(k=9) == -2 and topk(B=-1) == -2 and topk(M=-1) == -2
    assert topk(k=8) == 0 and topk(k=1, cand=fake) == 0


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def _pairs_for_the_oracle(C, T, skip):
    """(b, word) pairs with Tb >= 1 (the oracle indexes frame 0): every sample with a frame x a spread of lengths, the impossible ones included."""
    il = input_lengths(T, skip)
    words = make_words(C, n=21, seed=3)
    words[3] = [5, 5, 5, 5]                                  # four equal letters need 7 frames
    return [(b, w) for b in range(6) if il[b] >= 1 for w in words], il


@pytest.mark.parametrize("C,skip", [(38, 0), (38, 2), (97, 2)])
def test_reference_equals_the_ctc_oracle(C, skip):
    T = 20
    y = posteriors(C, T).astype(np.float64)
    pairs, il = _pairs_for_the_oracle(C, T, skip)
    assert len(pairs) >= 20 and len(pairs) <= 120
    words = [w for _, w in pairs]
    lab, ll = table(words, width=31, pad=C - 1)
    yb = np.stack([y[b] for b, _ in pairs])
    ilb = np.array([il[b] for b, _ in pairs])
    loss, _ = ctc.ctc_loss_and_grad(yb, lab.astype(np.int64), ilb, ll.astype(np.int64), skip=skip)
    uniq = sorted(set(map(tuple, words)))
    ref = _ref_scores(y, [list(w) for w in uniq], il, skip)
    got = np.array([ref[b, uniq.index(tuple(w))] for b, w in pairs])
    want = -loss.astype(np.float64)
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert fin.sum() >= 10 and (~fin).sum() >= 10            # possible and impossible pairs
    b2 = [i for i, (b, w) in enumerate(pairs) if il[b] == 13 and w == [5, 5, 5, 5]]
    b1 = [i for i, (b, w) in enumerate(pairs) if il[b] == 2 and w == [5, 5, 5, 5]]
    assert b2 and fin[b2[0]] and b1 and not fin[b1[0]]       # the same word: possible in 13 frames, not in 2
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=1e-10)


def test_reference_handles_no_frames_and_equals_torch_ctc_loss():
    C, T, skip = 38, 20, 0
    y = posteriors(C, T)
    words = make_words(C, n=28, seed=5)
    assert sorted(set(len(w) for w in words)) == sorted(SEGMENT_LENGTHS)
    il = input_lengths(T, skip)
    ref = _ref_scores(y, words, il, skip)
    assert ref.shape == (6, 28)
    # Tb = 0 (sample 5): 0 for the empty word, -inf otherwise, as the loss kernel decides it
    assert il[5] == 0 and all(ref[5, n] == (0.0 if len(w) == 0 else -np.inf) for n, w in enumerate(words))
    # clamping: lengths past the window are the window
    assert np.array_equal(_ref_scores(y, words, np.array([99, 13, 2, 20, 1, -4]), skip), ref)
    assert np.array_equal(_ref_scores(y, words, None, skip)[0], ref[0])
    lp = torch.from_numpy(log_softmax_of_log(y, skip)).permute(1, 0, 2).contiguous()             # (T, B, C) fp64
    for b in range(5):                                        # torch needs at least one frame
        tgt = torch.tensor([v for w in words for v in w], dtype=torch.long)
        tl = torch.tensor([len(w) for w in words], dtype=torch.long)
        loss = torch.nn.functional.ctc_loss(lp[:, b:b + 1].expand(-1, len(words), -1), tgt, torch.full((len(words),), int(il[b]), dtype=torch.long), tl,
                                            blank=C - 1, reduction="none", zero_infinity=False).numpy()
        want = -loss
        assert np.array_equal(np.isneginf(ref[b]), np.isinf(loss)), b
        fin = np.isfinite(want)
        np.testing.assert_allclose(ref[b][fin], want[fin], rtol=1e-10, atol=1e-9)
    assert np.isfinite(ref).any() and np.isneginf(ref).any()
    # probabilities: over all words of length <= 1 plus ... the scores of one sample never exceed 0, and the empty word on a
    # uniform map of Tb frames is Tb * log(1 / C) up to the epsilon
    assert (ref <= 1e-12).all()
    empty = [n for n, w in enumerate(words) if not w][0]
    assert abs(ref[1, empty] - 13 * np.log(1.0 / C)) < 1e-3
