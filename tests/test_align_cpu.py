"""CPU tests (no GPU) of the character alignment's host half and of the references the GPU tests use (tests/align_ref.py): the fp64 Viterbi pinned
to a brute-force enumeration of every CTC path, the np.float32 replay against it, the best path never above the total probability, CTCAligner's
encoding / rejection / span offsets, predict.py's --align flag, and the entry point's declaration, export and argument checks (those return
before anything is launched)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import utils as U
from crnn_mi355x import align as AL
from crnn_mi355x import native
from lexicon_ref import _ref_scores, log_softmax_of_log, posteriors, input_lengths, make_words
from align_ref import viterbi_f64, viterbi_f32_replay, brute_force, path_is_valid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")


# ---- the references --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 5, 6])
def test_viterbi_f64_equals_the_enumeration_of_every_path(T):
    C = 5
    rs = np.random.RandomState(T)
    y = rs.dirichlet(np.ones(C) * 0.6, size=(1, T))
    lsm = log_softmax_of_log(y, 0)[0]
    words = [[], [2], [0, 3], [1, 1], [3, 0]]                # L <= 2, a doubled letter among them
    seen_inf = seen_fin = 0
    for w in words:
        score, states, start, end, char = viterbi_f64(y, [w], None, 0, width=2)
        best, arg = brute_force(lsm, w)
        if not arg:
            assert score[0] == -np.inf and (states[0] == -1).all() and (start[0] == -1).all() and (end[0] == -1).all() and np.isneginf(char[0]).all()
            seen_inf += 1
            continue
        seen_fin += 1
        assert abs(score[0] - best) <= 1e-12, (w, score[0], best)
        assert states[0].tolist() in arg, (w, states[0].tolist(), arg)
        assert path_is_valid(states[0].tolist(), w, C - 1)
        for l, c in enumerate(w):
            run = [t for t in range(T) if states[0, t] == 2 * l + 1]
            assert run and (start[0, l], end[0, l]) == (run[0], run[-1] + 1)
            assert abs(char[0, l] - sum(lsm[t, c] for t in run)) <= 1e-12
        assert (start[0, len(w):] == -1).all() and (end[0, len(w):] == -1).all() and np.isneginf(char[0, len(w):]).all()
    assert seen_fin >= 1 and (T >= 3 or seen_inf >= 1)          # [1, 1] needs three frames, the two-letter words two


def test_tie_rule_on_a_uniform_map():
    """Every choice is a tie: the path ends in the last state and, going back, stays wherever staying was possible -- so it reaches every state as
    early as the word allows."""
    C, T = 5, 7
    y = np.full((1, T, C), 1.0 / C)
    score, states, start, end, _ = viterbi_f64(y, [[0, 1]], None, 0)
    assert states[0].tolist() == [1, 3, 4, 4, 4, 4, 4] and start[0].tolist() == [0, 1] and end[0].tolist() == [1, 2]
    lsm32 = log_softmax_of_log(y, 0).astype(np.float32)
    assert viterbi_f32_replay(lsm32, [[0, 1]])[1][0].tolist() == states[0].tolist()
    assert viterbi_f64(y, [[2, 2]], None, 0)[1][0].tolist() == [1, 2, 3, 4, 4, 4, 4]
    assert viterbi_f64(y, [[]], None, 0)[1][0].tolist() == [0] * 7


@pytest.mark.parametrize("skip", [0, 2])
def test_f32_replay_agrees_with_f64_where_nothing_ties(skip):
    C, T = 38, 20
    y = posteriors(C, T)
    words = make_words(C, n=21, seed=0)
    lsm32 = log_softmax_of_log(y, skip).astype(np.float32)
    fin = 0
    for n in range(0, 21, 3):
        per_sample = [words[(n + b) % 21] for b in range(6)]
        a = viterbi_f64(y, per_sample, None, skip, width=31)
        r = viterbi_f32_replay(lsm32, per_sample, None, width=31)
        assert r[0].dtype == np.float32 and r[4].dtype == np.float32
        for b in (0, 2, 4):                                  # samples without ties (1 is uniform, 3 and 5 hold exact zeros: equal floors)
            assert np.isneginf(a[0][b]) == np.isneginf(r[0][b])
            if np.isfinite(a[0][b]):
                fin += 1
                np.testing.assert_allclose(r[0][b], a[0][b], rtol=1e-6)
                assert np.array_equal(a[1][b], r[1][b]) and np.array_equal(a[2][b], r[2][b]) and np.array_equal(a[3][b], r[3][b])
                m = np.isfinite(a[4][b])
                np.testing.assert_allclose(r[4][b][m], a[4][b][m], rtol=1e-5)
    assert fin >= 10


@pytest.mark.parametrize("C,skip", [(38, 0), (38, 2), (97, 0)])
def test_best_path_never_exceeds_the_total_probability(C, skip):
    T = 20
    y = posteriors(C, T)
    il = input_lengths(T, skip)
    words = make_words(C, n=21, seed=1)
    total = _ref_scores(y, words, il, skip)                   # (6, 21)
    fin = 0
    for n, w in enumerate(words):
        score = viterbi_f64(y, [w] * 6, il, skip, width=31)[0]
        assert np.array_equal(np.isneginf(score), np.isneginf(total[:, n])), n      # a path exists exactly where the probability is not zero
        m = np.isfinite(score)
        fin += m.sum()
        assert (score[m] <= total[m, n] + 1e-9).all()
    assert fin >= 20


def test_no_frames_and_clamped_lengths():
    C, T = 38, 20
    y = posteriors(C, T)
    words = [[], [3], [], [1, 2], [5], []]
    score, states, start, end, char = viterbi_f64(y, words, np.array([0, 0, 99, -3, 1, 5]), 2)
    assert score[0] == 0.0 and score[1] == -np.inf and score[3] == -np.inf and np.isfinite(score[[2, 4, 5]]).all()
    assert states.shape == (6, 18) and (states[0] == -1).all() and (states[2] == 0).all() and states[4].tolist() == [1] + [-1] * 17
    assert states[5].tolist() == [0] * 5 + [-1] * 13 and (start[4, 0], end[4, 0]) == (0, 1)
    # what the library does not trust: no alignment
    s2 = viterbi_f64(y, [None, [37], [-1], list(range(32)), [1], [1, 2]], None, 0, width=1)[0]
    assert np.isneginf(s2[[0, 1, 2, 3, 5]]).all() and np.isfinite(s2[4])


# ---- CTCAligner -------------------------------------------------------------------------------------------------------------------------------
def _inv():
    return {i: ch for i, ch in enumerate(U.get_lexicon())}


def test_aligner_encodes_and_rejects_as_the_lexicon_does():
    inv = _inv()
    assert U.CTCAligner is AL.CTCAligner and U.Alignment is AL.Alignment and U.CharSpan is AL.CharSpan
    al = U.CTCAligner(inv, skip=2)
    lex = U.Lexicon(["ok"], inv)
    for text in ("hello", "", "y" * 31, "y" * 32, "Bad", "café", "a-b"):
        assert al.encode(text) == lex.encode(text), text
    assert al.encode("y" * 32) is None and al.encode("Bad") is None and al.encode("") == []
    table, lens = al._table(["ab", "Bad", "", "y" * 32, "hello"])
    assert table.dtype == np.int32 and lens.dtype == np.int32 and table.shape == (5, 5)
    assert lens.tolist() == [2, -1, 0, -1, 5] and (table[1] == -1).all() and (table[3] == -1).all()
    assert table[0].tolist() == [al.classes["a"], al.classes["b"], -1, -1, -1]
    assert U.CTCAligner(list("xyz")).encode("zx") == [2, 0] and U.CTCAligner(inv).skip == 0
    with pytest.raises(ValueError):
        al.align(np.zeros((3, 20, 38), dtype=np.float32), ["a", "b"])            # raised before anything touches a device
    with pytest.raises(ValueError):
        al.align(np.zeros((1, 20, 38), dtype=np.float32), [])


def test_too_many_frames_raise_before_anything_is_launched():
    import torch
    lab, ln = torch.zeros((1, 4), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    assert AL.MAX_FRAMES == 512
    for T, skip in ((513, 0), (515, 2), (2, 2)):
        with pytest.raises(ValueError):
            AL.ctc_align(torch.zeros((1, T, 38)), lab, ln, skip=skip)             # host tensors: nothing reaches a device


def test_aligner_moves_spans_by_skip_and_drops_chars_without_an_alignment():
    al = U.CTCAligner(_inv(), skip=2)
    ninf = float("-inf")
    fake = {"score": np.array([-3.5, ninf, 0.0], dtype=np.float32),
            "states": np.array([[0, 1, 1, 3, 4], [-1] * 5, [0] * 5], dtype=np.int32),
            "start": np.array([[1, 3], [-1, -1], [-1, -1]], dtype=np.int32),
            "end": np.array([[3, 4], [-1, -1], [-1, -1]], dtype=np.int32),
            "char_logp": np.array([[-1.25, -0.5], [ninf, ninf], [ninf, ninf]], dtype=np.float32)}
    a, b, c = al._alignments(fake, ["hi", "zz", ""])
    assert isinstance(a, U.Alignment) and a.text == "hi" and a.log_prob == -3.5 and a.states.tolist() == [0, 1, 1, 3, 4]
    assert a.chars == [U.CharSpan("h", 3, 5, -1.25), U.CharSpan("i", 5, 6, -0.5)]                # window frames 1..3 and 3..4, plus skip
    assert b.text == "zz" and b.log_prob == ninf and b.chars == []
    assert c.text == "" and c.log_prob == 0.0 and c.chars == []
    a0 = U.CTCAligner(_inv())._alignments(fake, ["hi", "zz", ""])[0]
    assert [(s.start, s.end) for s in a0.chars] == [(1, 3), (3, 4)]


def test_alignment_csv_columns(tmp_path):
    import csv
    rows = [U.Alignment("hi", -3.5, [U.CharSpan("h", 3, 5, -1.25), U.CharSpan("i", 5, 6, -0.5)], None), U.Alignment("a,b", float("-inf"), [], None)]
    AL.write_alignment_csv(str(tmp_path / "alignment.csv"), ["x.png", "y.png"], rows)
    got = list(csv.reader(open(tmp_path / "alignment.csv", newline="")))
    assert got == [["fname", "prediction", "path_log_prob", "chars"], ["x.png", "hi", "-3.5", "h:3:5:-1.25 i:5:6:-0.5"], ["y.png", "a,b", "-inf", ""]]


def test_predict_cli_align_flag():
    sys.path.insert(0, PKG)
    import predict as predict_cli
    base = ["--model_path", "m", "--image_path", "i"]
    assert predict_cli.parse_args(base).align is False
    assert predict_cli.parse_args(base + ["--align", "--result_path", "r"]).align is True
    assert predict_cli.parse_args(base + ["--align", "--result_path", "r", "--validate", "--lexicon", "w.txt"]).align is True
    with pytest.raises(SystemExit):
        predict_cli.parse_args(base + ["--align"])                                                     # needs --result_path
    with pytest.raises(SystemExit):
        predict_cli.parse_args(base + ["--align", "--result_path", "r", "--validate", "--device_score"])   # that path never materialises the maps


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    decl = native.parse_header()
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert decl["crnn_ctc_align_workspace_bytes"] == (Z, [I, I, I, I])
    assert decl["crnn_ctc_align"] == (I, [P] * 10 + [Z] + [I] * 5 + [P])
    lib = ctypes.CDLL(native.LIB_PATH)
    assert hasattr(lib, "crnn_ctc_align") and hasattr(lib, "crnn_ctc_align_workspace_bytes")
    assert "align.hip" in native.SOURCES and os.path.exists(os.path.join(native.CSRC, "align.hip"))


def test_entry_point_rejects_bad_arguments_before_launching():
    """Every check runs on the host before a launch, so the rejections need no GPU (the pointers are never followed)."""
    L = native.lib()
    fake = ctypes.c_void_p(1 << 20)
    for args in ((6, 20, 38, 2), (1024, 52, 38, 0), (4, 2, 38, 2), (2, 514, 128, 2)):
        assert L.crnn_ctc_align_workspace_bytes(*args) == L.crnn_ctc_lexicon_workspace_bytes(*args)
    assert L.crnn_ctc_align_workspace_bytes(6, 20, 38, 2) == 6 * 18 * 38 * 4

    def align(y=fake, il=None, labels=fake, ll=fake, score=fake, states=fake, start=fake, end=fake, char=fake, ws=fake, ws_bytes=1 << 30, B=6, T=20,
              C=38, skip=0, Lmax=31):
        return L.crnn_ctc_align(y, il, labels, ll, score, states, start, end, char, ws, ws_bytes, B, T, C, skip, Lmax, None)
    for name in ("y", "labels", "ll", "score", "ws"):
        assert align(**{name: None}) == -2, name
    assert align(B=-1) == -2 and align(T=-1) == -2 and align(C=1) == -2 and align(C=-5) == -2 and align(skip=-1) == -2 and align(Lmax=0) == -2 and align(Lmax=-1) == -2
    assert align(T=2, skip=2) == -2 and align(T=1, skip=2) == -2
    assert align(ws_bytes=6 * 20 * 38 * 4 - 1) == -2 and align(skip=2, ws_bytes=6 * 18 * 38 * 4 - 1) == -2
    assert align(C=129) == -3 and align(T=513) == -3 and align(T=515, skip=2) == -3 and align(C=129, ws_bytes=0) == -3
    assert align(B=0) == 0 and align(B=0, T=512, C=128) == 0 and align(B=0, T=514, skip=2) == 0 and align(B=0, Lmax=512) == 0      # nothing to do: nothing launched
    assert align(B=0, T=513) == -3 and align(B=0, y=None) == -2
