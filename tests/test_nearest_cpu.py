"""CPU tests (no GPU) of lexicon shortlists' host half: the plain-Python reference of crnn_lexicon_nearest (tests/nearest_ref.py) pinned to
crnn_mi355x.metrics.levenshtein, its selection rule on hand-made ties, the decoder's and the command line's argument checks, the entry points'
declarations, export and refusals (those return before anything is launched), and the property of the constructed fixture that lets the GPU test
demand equality with the exhaustive decoder: on all 48 images the exhaustive best word is among the 16 nearest to the beam decode."""
import ctypes
import os
import sys

import numpy as np
import pytest

import utils as U
from crnn_mi355x import lexicon as LX
from crnn_mi355x import native
from oracle import ctc
from lexicon_ref import _ref_scores, table
import nearest_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def test_reference_levenshtein_equals_the_metrics_module():
    rs = np.random.RandomState(0)
    chars = "abcd"                                          # a small alphabet: matches, repeats and transpositions are common
    for _ in range(300):
        a = "".join(rs.choice(list(chars), size=rs.randint(0, 12)))
        b = "".join(rs.choice(list(chars), size=rs.randint(0, 12)))
        assert NR.levenshtein(a, b) == U.levenshtein(a, b) == NR.levenshtein(b, a)
    assert NR.levenshtein("", "") == 0 and NR.levenshtein("abc", "") == 3 and NR.levenshtein("kitten", "sitting") == 3


def test_reference_filters_truncates_and_takes_the_minimum_over_the_rows():
    C = 38
    assert NR.filter_query([-1, 3, 37, 3, 99, -5, 36, 0, -1], C) == [3, 3, 36, 0]
    assert NR.filter_query([37] * 5 + [-1] * 5, C) == [] and NR.filter_query(list(range(30)) * 3, C) == (list(range(30)) * 3)[:64]
    lab, ll = table([[1, 2, 3], [], [4, 5], [1, 2, 3, 4, 5, 6]], width=8)
    q = np.array([[[1, 37, 2, -1, 3, -1], [4, 5, -1, -1, -1, -1]],           # rows "123" and "45": each word takes the nearer one
                  [[-1] * 6, [37] * 6]])                                      # two empty queries: the distance is the word's length
    d = NR.distances(q, lab, ll, C)
    assert d.tolist() == [[0, 2, 0, 3], [3, 0, 2, 6]]
    assert NR.distances(q[:, 0], lab, ll, C).tolist() == [[0, 3, 3, 3], [3, 0, 2, 6]]          # (B, qcols): one row per sample
    # what cannot be trusted: a length outside [0, Lmax], a label outside [0, C - 2] inside the length (one past it does not matter)
    lab2, ll2 = lab.copy(), ll.copy()
    ll2[0] = -1; ll2[2] = 9; lab2[3, 5] = 37
    lab2[1, 0] = 1000
    assert NR.distances(q, lab2, ll2, C).tolist() == [[255, 2, 255, 255], [255, 0, 255, 255]]
    # 65 kept symbols: the 65th is not read
    long_q = np.array([[list(range(13)) * 5]])
    assert long_q.shape[2] == 65
    w, wl = table([list(range(13)) * 2 + [0, 1, 2, 3, 4]], width=31)
    assert NR.distances(long_q, w, wl, C)[0, 0] == 64 - 31 == NR.distances(long_q[:, :, :64], w, wl, C)[0, 0]


def test_reference_selects_by_distance_then_index_and_writes_ascending_indices():
    d = np.array([[3, 1, 2, 1, 255, 1, 0, 2],
                  [255, 255, 4, 255, 255, 255, 255, 255],
                  [5, 5, 5, 5, 5, 5, 5, 5]])
    idx, dist = NR.select(d, 4)
    assert idx.tolist() == [[1, 3, 5, 6], [2, -1, -1, -1], [0, 1, 2, 3]] and idx.dtype == np.int32
    assert dist.tolist() == [[1, 1, 1, 0], [4, -1, -1, -1], [5, 5, 5, 5]]
    idx, dist = NR.select(d, 3)                              # the threshold bin (d = 1) holds three and two fit: the lowest indices win
    assert idx[0].tolist() == [1, 3, 6] and dist[0].tolist() == [1, 1, 0]
    idx, dist = NR.select(d, 9)                              # K > N: the untrusted entry is never taken, the tail is -1
    assert idx[0].tolist() == [0, 1, 2, 3, 5, 6, 7, -1, -1] and dist[0].tolist() == [3, 1, 2, 1, 1, 0, 2, -1, -1]
    assert NR.select(d, 1)[0].tolist() == [[6], [2], [0]]


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------
def test_names_import_from_utils_and_decoder_arguments_are_checked():
    assert U.lexicon_nearest is LX.lexicon_nearest and hasattr(U.Lexicon, "nearest")
    inv = {i: ch for i, ch in enumerate(U.get_lexicon())}
    lex = U.Lexicon(["ccc", "a", "bb"], inv)
    assert lex.num_classes == 38
    for kw in (dict(shortlist=0), dict(shortlist=1025), dict(shortlist=8, paths=9, beam_width=64), dict(shortlist=8, paths=0),
               dict(shortlist=8, paths=5, beam_width=4)):
        with pytest.raises(ValueError):
            U.LexiconDecoder(lex, **kw)
    dec = U.LexiconDecoder(lex, shortlist=1024, paths=8, beam_width=8)
    assert (dec.shortlist, dec.paths, dec.beam_width) == (1024, 8, 8)
    plain = U.LexiconDecoder(lex)
    assert plain.shortlist is None and (plain.paths, plain.beam_width) == (1, 10)
    with pytest.raises(ValueError) as err:                  # a string the alphabet cannot spell is named (raised before anything touches a device)
        lex.nearest(["fine", "Not fine"], k=2, device="cpu")
    assert "Not fine" in str(err.value)
    with pytest.raises(ValueError):
        lex.nearest(["a"], k=0, device="cpu")


def test_predict_cli_shortlist_flags_need_a_lexicon(capsys):
    sys.path.insert(0, PKG)
    import predict as predict_cli
    base = ["--model_path", "m", "--image_path", "i"]
    args = predict_cli.parse_args(base)
    assert args.lexicon_shortlist is None and args.lexicon_paths is None
    args = predict_cli.parse_args(base + ["--lexicon", "w.txt", "--lexicon_shortlist", "50", "--lexicon_paths", "3"])
    assert (args.lexicon_shortlist, args.lexicon_paths) == (50, 3)
    for bad in (["--lexicon_shortlist", "8"], ["--lexicon_paths", "2"], ["--lexicon", "w.txt", "--lexicon_paths", "2"],
                ["--lexicon", "w.txt", "--lexicon_shortlist", "0"], ["--lexicon", "w.txt", "--lexicon_shortlist", "1025"],
                ["--lexicon", "w.txt", "--lexicon_shortlist", "8", "--lexicon_paths", "9"]):
        with pytest.raises(SystemExit) as err:
            predict_cli.parse_args(base + bad)
        assert err.value.code == 2 and "error:" in capsys.readouterr().err, bad


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    decl = native.parse_header()
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert decl["crnn_lexicon_nearest_workspace_bytes"] == (Z, [I, I])
    assert decl["crnn_lexicon_nearest"] == (I, [P, I, I, P, P, P, P, P, Z] + [I] * 5 + [P])
    lib = ctypes.CDLL(native.LIB_PATH)
    assert hasattr(lib, "crnn_lexicon_nearest_workspace_bytes") and hasattr(lib, "crnn_lexicon_nearest")
    assert "lexicon_nearest.hip" in native.SOURCES


def test_entry_point_rejects_bad_arguments_before_launching():
    """Every check runs on the host before a launch, so the rejections need no GPU (the pointers are never followed)."""
    L = native.lib()
    fake = ctypes.c_void_p(1 << 20)
    assert L.crnn_lexicon_nearest_workspace_bytes(1024, 88000) == 1024 * (1024 + 88000)
    assert L.crnn_lexicon_nearest_workspace_bytes(3, 65) == 3 * (1024 + 68) and L.crnn_lexicon_nearest_workspace_bytes(0, 5) == 0

    def near(q=fake, P=1, qcols=24, words=fake, wl=fake, idx=fake, dist=fake, ws=fake, ws_bytes=1 << 30, B=6, C=38, N=40, Lmax=31, K=5):
        return L.crnn_lexicon_nearest(q, P, qcols, words, wl, idx, dist, ws, ws_bytes, B, C, N, Lmax, K, None)
    for name in ("q", "words", "wl", "idx", "dist", "ws"):
        assert near(**{name: None}) == -2, name
    assert near(B=-1) == -2 and near(N=-1) == -2 and near(ws_bytes=6 * (1024 + 40) - 1) == -2
    for kw in (dict(C=1), dict(C=129), dict(Lmax=0), dict(Lmax=32), dict(P=0), dict(P=9), dict(qcols=0), dict(qcols=1025), dict(K=0), dict(K=1025)):
        assert near(**kw) == -3, kw
    assert near(B=0) == 0 and near(B=0, N=0) == 0 and near(B=0, K=1024, P=8, qcols=1024, C=128, ws_bytes=0) == 0        # nothing launched
    assert near(B=0, q=None) == -2                          # a null pointer is a bad argument whatever B is


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------
def test_fixture_keeps_the_exhaustive_best_word_in_every_shortlist():
    """With the references alone: fp64 scores of all 400 words per image, the oracle's beam decode (width 10, no merging) as the query, the 16
    nearest words by the reference selection -- the best-scoring word is among them on all 48 images, so the GPU test may demand equality."""
    y, words = NR.fixture()
    assert y.shape == (NR.FIX_IMAGES, NR.FIX_T, NR.FIX_C) and len(words) == NR.FIX_N == len(set(map(tuple, words)))
    assert [len(w) for w in words] == sorted(len(w) for w in words) and {len(w) for w in words} == set(range(2, 11))
    assert max(max(w) for w in words) <= 11 and abs(float(y[0, 0].max()) - 0.9) < 1e-6 and np.allclose(y.sum(-1), 1.0, atol=1e-5)
    ref = _ref_scores(y, words, None, 0)
    best = ref.argmax(1)
    assert np.isfinite(ref[np.arange(len(best)), best]).all()
    q, _, _ = ctc.ctc_beam_decode(np.array(y), beam_width=10, merge_repeated=False)
    lab, ll = table(words, width=10)
    d = NR.distances(q, lab, ll, NR.FIX_C)
    idx, _ = NR.select(d, NR.FIX_K)
    miss = [b for b in range(len(best)) if best[b] not in idx[b]]
    print("exhaustive best outside the %d nearest: %d of %d images; distance of the best word: %s" % (NR.FIX_K, len(miss), len(best), np.bincount(d[np.arange(len(best)), best]).tolist()))
    assert not miss
    # not trivially safe: the best word is not always the nearest one's bin alone, and the clean third decodes to its word
    assert (d[np.arange(len(best)), best] > 0).sum() >= 16 and (d.min(1) == 0).sum() >= 16
