"""CPU tests (no GPU) of the device scoring's host half: the entry point's declaration, export and argument checks (those return before anything
is launched), metrics.Score's two means against the host functions -- equal as floats, no tolerance --, the one-character-per-class guard and
predict.py's --device_score flag."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import utils as U
from crnn_mi355x import metrics as M
from crnn_mi355x import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "helpers_golden.json")))


def test_header_declares_and_library_exports_the_entry_point():
    decl = native.parse_header()
    assert "crnn_edit_distance" in decl
    ret, args = decl["crnn_edit_distance"]
    assert ret is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(native.LIB_PATH), "crnn_edit_distance")
    assert "score.hip" in native.SOURCES
    assert U.Score is M.Score and U.device_edit_distances is M.device_edit_distances and U.check_label_metric is M.check_label_metric
    assert hasattr(U.Model, "score_generator")


def test_entry_point_rejects_bad_arguments_before_launching():
    """Every check of crnn_edit_distance runs on the host before the launch, so the rejections need no GPU (the pointers are never followed)."""
    L = native.lib()
    fake = ctypes.c_void_p(1 << 20)         # stands for a device pointer

    def call(pred=fake, pred_cols=52, truth=fake, truth_cols=23, dist=fake, pred_len=fake, truth_len=fake, n=8):
        return L.crnn_edit_distance(pred, pred_cols, truth, truth_cols, 37, -1, dist, pred_len, truth_len, n, None)
    for name in ("pred", "truth", "dist", "pred_len", "truth_len"):
        assert call(**{name: None}) == -2, name
    assert call(n=-1) == -2 and call(pred_cols=0) == -2 and call(truth_cols=0) == -2 and call(pred_cols=-3) == -2
    assert call(n=0, pred=None) == -2                                    # a null pointer is a bad argument whatever n is
    assert call(truth_cols=65) == -3 and call(pred_cols=1025) == -3 and call(truth_cols=65, pred_cols=64) == -3
    assert call(n=0) == 0 and call(n=0, truth_cols=64, pred_cols=1024) == 0
    with pytest.raises(native.CrnnError):
        native.check(call(truth_cols=65), "edit_distance")


def _score_of(pairs):
    """A Score built from integers alone: what the device brings back for these pairs."""
    d = [int(U.levenshtein(a, b)) for a, b in pairs]
    return M.Score(np.zeros((len(pairs), 1), np.int32), np.array(d, np.int32), np.array([len(a) for a, _ in pairs], np.int32),
                   np.array([len(b) for _, b in pairs], np.int32))


def test_score_means_equal_the_host_functions_on_the_reference_pairs():
    pairs = [(a, b) for a, b, _ in GOLD["levenshtein"] if b]
    assert len(pairs) >= 5
    s = _score_of(pairs)
    pred, true = [a for a, _ in pairs], [b for _, b in pairs]
    assert s.distances.tolist() == [int(d) for a, b, d in GOLD["levenshtein"] if b]
    assert s.edit_distance == U.edit_distance(pred, true) and isinstance(s.edit_distance, float)
    assert s.normalized_edit_distance == U.normalized_edit_distance(pred, true)
    assert s.edit_distance == pytest.approx(GOLD["edit_distance"], rel=1e-12)
    assert s.normalized_edit_distance == pytest.approx(GOLD["normalized_edit_distance"], rel=1e-12)
    assert s.exact == sum(1 for a, b in pairs if a == b) and len(s) == len(pairs)
    assert s.cer == sum(s.distances.tolist()) / sum(len(b) for b in true)


def test_score_means_equal_the_host_functions_on_1000_random_pairs():
    rs = np.random.RandomState(0)
    alphabet = list("abcdefghij0123456789-")

    def word(lo):
        return "".join(rs.choice(alphabet, size=rs.randint(lo, 24)))
    pairs = [(word(0), word(1)) for _ in range(1000)]
    s = _score_of(pairs)
    pred, true = [a for a, _ in pairs], [b for _, b in pairs]
    assert s.edit_distance == U.edit_distance(pred, true)
    assert s.normalized_edit_distance == U.normalized_edit_distance(pred, true)
    assert 0 < s.exact + 1 and s.distances.max() > 5
    empty = M.Score(np.zeros((0, 0), np.int32), [], [], [])
    assert empty.edit_distance == U.edit_distance([], []) == 0 and empty.normalized_edit_distance == 0 and empty.exact == 0


def test_empty_truth_raises_zero_division_as_the_host_does():
    pairs = [("abc", "abd"), ("x", ""), ("", "q")]
    with pytest.raises(ZeroDivisionError):
        U.normalized_edit_distance([a for a, _ in pairs], [b for _, b in pairs])
    s = _score_of(pairs)
    with pytest.raises(ZeroDivisionError):
        s.normalized_edit_distance
    assert s.edit_distance == U.edit_distance([a for a, _ in pairs], [b for _, b in pairs])


def test_texts_are_the_decoders():
    inv = {i: ch for i, ch in enumerate(U.get_lexicon())}
    dec = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=inv)
    rows = np.array([[10, 11, -1, -1], [37, 12, 37, 0], [-1, -1, -1, -1]], np.int32)
    s = M.Score(rows, [0, 1, 2], [2, 2, 0], [2, 1, 2])
    assert s.texts(dec) == ["ab", "c0", ""] == [dec.labels_to_text(r) for r in rows]


def test_guard_wants_one_distinct_character_per_class():
    lex = U.get_lexicon()
    M.check_label_metric(lex)
    M.check_label_metric({i: ch for i, ch in enumerate(lex)})
    with pytest.raises(ValueError, match="class 2"):
        M.check_label_metric({0: "a", 1: "b", 2: "ch", 3: "d"})          # a two-character class
    with pytest.raises(ValueError, match="class 3"):
        M.check_label_metric({0: "a", 1: "b", 2: "c", 3: "a"})           # a duplicated character
    with pytest.raises(ValueError, match="class 1"):
        M.check_label_metric(["a", "", "c"])                             # a class that decodes to nothing
    M.check_label_metric({0: 7, 1: 8})                                   # labels_to_text joins str(value)

    class _Gen:                                                          # the guard runs before anything touches the generator or the GPU
        def __next__(self):
            raise AssertionError("the generator was advanced")
    model = U.CRNN(num_classes=5, max_string_len=4, shape=(100, 32, 1), time_dense_size=8, n_units=64).get_model()
    dec = U.DecodeCTCPred(inverse_classes={0: "a", 1: "b", 2: "ch", 3: "d"})
    with pytest.raises(ValueError, match="class 2"):
        model.score_generator(_Gen(), 3, dec)


def test_device_score_flag_needs_validate(capsys):
    sys.path.insert(0, os.path.join(ROOT, "crnn-ocr-lite_amd"))
    import predict as predict_cli
    base = ["--model_path", "m", "--image_path", "i"]
    args = predict_cli.parse_args(base + ["--validate", "--device_score"])
    assert args.device_score and args.validate
    assert not predict_cli.parse_args(base + ["--validate"]).device_score and not predict_cli.parse_args(base).device_score
    with pytest.raises(SystemExit) as e:
        predict_cli.parse_args(base + ["--device_score"])
    assert e.value.code == 2 and "--validate" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        predict_cli.main(base + ["--device_score"])
