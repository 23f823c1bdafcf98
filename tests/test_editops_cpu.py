"""CPU tests (no GPU) of the edit scripts' host half: crnn_edit_ops' declaration, export and argument checks (those return before anything is
launched); metrics.edit_ops -- the definition the device is held to -- against the literal cases of the contract and against the test-local
restatement tests/editops_ref.py, with the identities every script obeys; metrics.Confusions; Score's two new arguments; predict.py's
--confusions flag."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import utils as U
from crnn_mi355x import metrics as M
from crnn_mi355x import native

import editops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "helpers_golden.json")))

# (truth, prediction, (match, sub, del, ins), truth_map, pred_map): the contract's table, derived by hand
LITERAL = [("ab", "b", (1, 0, 1, 0), [-1, 0], [1]),
           ("ab", "ba", (0, 2, 0, 0), [0, 1], [0, 1]),                    # two substitutions, not a deletion and an insertion
           ("aa", "a", (1, 0, 1, 0), [-1, 0], [1]),                       # the first of a doubled letter is the dropped one
           ("a", "aa", (1, 0, 0, 1), [1], [-1, 0]),                       # the first is the spurious one
           ("kitten", "sitting", (4, 2, 0, 1), [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5, -1])]


def test_header_declares_and_library_exports_the_entry_point():
    decl = native.parse_header()
    assert "crnn_edit_ops" in decl
    ret, args = decl["crnn_edit_ops"]
    assert ret is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 7 + \
        [ctypes.c_int, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(native.LIB_PATH), "crnn_edit_ops")
    assert "editops.hip" in native.SOURCES and os.path.exists(os.path.join(native.CSRC, "editops.hip"))
    assert U.edit_ops is M.edit_ops and U.confusion_matrix is M.confusion_matrix and U.device_edit_ops is M.device_edit_ops
    assert U.Confusions is M.Confusions


def test_entry_point_rejects_bad_arguments_before_launching():
    """Every check of crnn_edit_ops runs on the host before the launch, so the rejections need no GPU (the pointers are never followed)."""
    L = native.lib()
    fake = ctypes.c_void_p(1 << 20)         # stands for a device pointer

    def call(pred=fake, pred_cols=52, truth=fake, truth_cols=23, C=37, ops=fake, dist=fake, pred_len=fake, truth_len=fake, truth_map=fake,
             pred_map=fake, conf=fake, n=8):
        return L.crnn_edit_ops(pred, pred_cols, truth, truth_cols, 37, -1, C, ops, dist, pred_len, truth_len, truth_map, pred_map, conf, n, None)
    for name in ("pred", "truth", "ops", "dist", "pred_len", "truth_len"):
        assert call(**{name: None}) == -2, name
        assert call(**{name: None, "n": 0}) == -2, name                  # a null pointer is a bad argument whatever n is
    assert call(n=-1) == -2 and call(pred_cols=0) == -2 and call(truth_cols=0) == -2 and call(pred_cols=-3) == -2 and call(C=0) == -2 and call(C=-1) == -2
    assert call(truth_cols=65) == -3 and call(pred_cols=1025) == -3 and call(C=129) == -3 and call(truth_cols=65, pred_cols=64) == -3
    assert call(n=0) == 0 and call(n=0, truth_cols=64, pred_cols=1024, C=128) == 0 and call(n=0, C=1, truth_cols=1, pred_cols=1) == 0
    assert call(n=0, truth_map=None) == 0 and call(n=0, pred_map=None) == 0 and call(n=0, conf=None) == 0     # the optional pointers
    assert call(n=0, truth_map=None, pred_map=None, conf=None) == 0
    assert call(truth_map=None, pred_map=None, conf=None, truth_cols=65) == -3
    with pytest.raises(native.CrnnError):
        native.check(call(C=129), "edit_ops")


@pytest.mark.parametrize("truth,pred,ops,truth_map,pred_map", LITERAL)
def test_literal_cases_of_the_contract(truth, pred, ops, truth_map, pred_map):
    assert M.edit_ops(pred, truth) == (ops, truth_map, pred_map)
    assert R.edit_ops(pred, truth) == (ops, truth_map, pred_map)
    assert M.edit_ops(list(map(ord, pred)), list(map(ord, truth))) == (ops, truth_map, pred_map)       # label rows, as the device sees them


def _random_pairs():
    rs = np.random.RandomState(7)
    pairs = []
    for k in range(2000):
        alpha = (2, 3, 36)[k % 3]                                         # small alphabets are where the ties are
        m = (0, 1, 2, 5, 63, 64)[(k // 3) % 6]
        n = int(rs.randint(0, 81))
        if k % 7 == 0 and m:                                              # a prediction that is a corrupted copy of the truth
            t = rs.randint(0, alpha, m).tolist()
            p = [v for v in t if rs.rand() > 0.2]
            pairs.append((p, t))
        else:
            pairs.append((rs.randint(0, alpha, n).tolist(), rs.randint(0, alpha, m).tolist()))
    return pairs


def _replay(truth, truth_map, pred, pred_map):
    """The prediction rebuilt from the truth by the script: walk both maps in order; only inserted and substituted symbols come from `pred`,
    and every prediction position is produced exactly once, in order."""
    out, j = [], 0
    for k, b in enumerate(truth):
        if truth_map[k] < 0:
            continue                                                      # deleted
        while j < truth_map[k]:
            assert pred_map[j] == -1                                      # inserted before this pair
            out.append(pred[j])
            j += 1
        assert pred_map[j] == k
        out.append(b if pred[j] == b else pred[j])                        # kept (the truth's own symbol), or substituted
        j += 1
    out += pred[j:]
    assert all(v == -1 for v in pred_map[j:])
    return out


def test_host_definition_equals_the_reference_on_2000_random_pairs():
    pairs = _random_pairs()
    kinds, ties = np.zeros(4, np.int64), 0
    for pred, truth in pairs:
        got = M.edit_ops(pred, truth)
        steps, tie = R.script(pred, truth)
        assert got == R.edit_ops(pred, truth, steps), (pred, truth)
        (match, sub, dele, ins), tm, pm = got
        m, n = len(truth), len(pred)
        assert sub + dele + ins == int(M.levenshtein(pred, truth)) and match + sub + dele == m and match + sub + ins == n
        assert len(tm) == m and len(pm) == n
        paired_t = [(k, j) for k, j in enumerate(tm) if j >= 0]
        paired_p = [(i, k) for k, i in enumerate(pm) if i >= 0]
        assert paired_t == paired_p                                       # mutually inverse
        assert all(x[1] < y[1] for x, y in zip(paired_t, paired_t[1:]))    # strictly increasing: an alignment never crosses
        assert all(v >= -1 for v in tm + pm) and sum(v == -1 for v in tm) == dele and sum(v == -1 for v in pm) == ins
        assert sum(truth[k] == pred[j] for k, j in paired_t) == match
        assert _replay(truth, tm, pred, pm) == pred
        kinds += (match, sub, dele, ins)
        ties += tie
    assert (kinds > 1000).all() and ties > 200                            # the pairs reach every kind of step and the tie of rules 1 and 2


def test_reference_run_pairs_have_the_recorded_distance():
    for pred, truth, d in GOLD["levenshtein"]:
        (match, sub, dele, ins), tm, pm = M.edit_ops(pred, truth)
        assert sub + dele + ins == int(d) and (match, sub, dele, ins) == R.edit_ops(pred, truth)[0]


def test_confusion_matrix_equals_the_reference_and_guards_its_labels():
    pairs = [(p, t) for p, t in _random_pairs()[:300] if max(p + t + [0]) < 3]
    assert len(pairs) > 100
    conf = M.confusion_matrix(pairs, 3)
    assert conf.dtype == np.int64 and conf.shape == (4, 4) and np.array_equal(conf, R.confusion(pairs, 3)) and conf[3, 3] == 0
    assert conf[:3].sum() == sum(len(t) for _, t in pairs) and conf[:, :3].sum() == sum(len(p) for p, _ in pairs)
    for bad in ([([0, 3], [0])], [([0], [-1])]):
        with pytest.raises(ValueError, match="pair 0"):
            M.confusion_matrix(bad, 3)


def _confusions():
    m = np.zeros((5, 5), np.int64)              # classes a b c d, index 4 = nothing; class d never occurs
    m[0, 0], m[1, 1], m[2, 2] = 50, 40, 0
    m[0, 1] = 7                                 # a read as b
    m[1, 0] = 7                                 # b read as a: the same count, the lower truth index first
    m[0, 2] = 7                                 # the same count and truth: the lower prediction index first
    m[1, 4] = 9                                 # b dropped
    m[4, 2] = 3                                 # a spurious c
    m[2, 0] = 1
    return M.Confusions(m, {0: "a", 1: "b", 2: "c", 3: "d"})


def test_confusions_totals_top_and_per_class():
    c = _confusions()
    assert c.matrix.dtype == np.int64 and c.num_classes == 4
    assert (c.matches, c.substitutions, c.deletions, c.insertions) == (90, 22, 9, 3)
    want = [("b", "", 9), ("a", "b", 7), ("a", "c", 7), ("b", "a", 7), ("", "c", 3), ("c", "a", 1)]
    assert c.top(20) == want and c.top(3) == want[:3] and c.top(0) == []
    per = c.per_class()
    assert [p[0] for p in per] == ["a", "b", "c", "d"] and [p[1] for p in per] == [64, 56, 1, 0]
    assert per[0][2] == 50 / 64 and per[0][3] == 50 / 58 and per[1][2] == 40 / 56 and per[1][3] == 40 / 47
    assert per[2][2] == 0.0 and per[2][3] == 0.0                          # a class that is never right
    assert per[3][2] is None and per[3][3] is None                        # an empty row and an empty column
    lone = M.Confusions(np.array([[0, 0, 0], [0, 0, 0], [2, 0, 0]]), ["x", "y"])      # x only ever inserted: no support, precision 0
    assert lone.per_class() == [("x", 0, None, 0.0), ("y", 0, None, None)] and lone.insertions == 2
    with pytest.raises(ValueError):
        M.Confusions(np.zeros((3, 4)), ["x", "y"])


def test_confusions_add_report_and_csv_round_trip(tmp_path):
    c = _confusions()
    two = c + c
    assert np.array_equal(two.matrix, 2 * c.matrix) and two.top(1) == [("b", "", 18)] and np.array_equal(c.matrix, _confusions().matrix)
    with pytest.raises(TypeError):
        c + M.Confusions(np.zeros((3, 3)), ["x", "y"])
    text = c.report(2).splitlines()
    assert len(text) == 3 and "90 matches, 22 substitutions, 9 deletions, 3 insertions" in text[0]
    assert "'b' read as nothing: 9" in text[1] and "'a' read as 'b': 7" in text[2]
    assert "nothing read as 'c': 3" in c.report(20)
    path = str(tmp_path / "confusions.csv")
    c.to_csv(path)
    lines = open(path).read().splitlines()
    assert lines[0] == "truth,predicted,count" and len(lines) == 1 + int((c.matrix != 0).sum()) and "b,,9" in lines and ",c,3" in lines
    back = M.Confusions.from_csv(path, c.inverse_classes)
    assert np.array_equal(back.matrix, c.matrix)


def test_score_built_the_old_way_is_unchanged():
    s = M.Score(np.zeros((3, 2), np.int32), [0, 1, 2], [2, 2, 1], [2, 1, 3])
    assert s.ops is None and s.confusions is None and s.truth_maps is None and s.pred_maps is None
    assert len(s) == 3 and s.exact == 1 and s.cer == 3 / 6 and s.edit_distance == sum(float(d) / 3 for d in (0, 1, 2))
    assert s.normalized_edit_distance == sum(float(d) / (t * 3) for d, t in ((0, 2), (1, 1), (2, 3)))
    with_ops = M.Score(np.zeros((2, 2), np.int32), [0, 1], [2, 2], [2, 1], ops=[[2, 0, 0, 0], [1, 0, 0, 1]], confusions=_confusions())
    assert with_ops.ops.shape == (2, 4) and with_ops.ops.dtype == np.int32 and with_ops.confusions.matches == 90 and with_ops.exact == 1


def test_confusions_flag_needs_validate(capsys):
    sys.path.insert(0, PKG)
    import predict as predict_cli
    base = ["--model_path", "m", "--image_path", "i"]
    assert predict_cli.parse_args(base + ["--validate", "--confusions"]).confusions == 20
    assert predict_cli.parse_args(base + ["--validate", "--confusions", "5", "--device_score"]).confusions == 5
    assert predict_cli.parse_args(base + ["--validate"]).confusions is None and predict_cli.parse_args(base).confusions is None
    for flags in (["--confusions"], ["--confusions", "3"], ["--validate", "--confusions", "-1"]):
        with pytest.raises(SystemExit) as e:
            predict_cli.parse_args(base + flags)
        assert e.value.code == 2 and "--confusions" in capsys.readouterr().err
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))           # a fresh process: the error comes before anything is loaded
    done = subprocess.run([sys.executable, os.path.join(PKG, "predict.py")] + base + ["--confusions"], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 2 and "--validate" in done.stderr and "--confusions" in done.stderr
