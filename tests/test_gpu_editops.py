"""-m gpu tests of the edit scripts on the device (csrc/editops.hip through metrics.device_edit_ops, Model.score_generator(confusions=True) and
predict.py --confusions): the four counts, the distance and lengths, both alignment maps and the confusion matrix equal the test-local
restatement of the contract (tests/editops_ref.py) as integers -- np.array_equal throughout, no tolerance, no excluded case -- over a case list
that is itself checked to reach every kind of step, over random pairs at 3, 38 and 128 classes and batch sizes around the wavefront / workgroup
/ pairs-per-workgroup boundaries, and at the widest prediction; launches accumulate into one matrix; out-of-range labels index nothing."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import utils as U
from crnn_mi355x import metrics as M
from crnn_mi355x import native

import editops_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "helpers_golden.json")))
C, BLANK, PAD = 37, 37, -1                      # the 38-class model: 37 characters, the blank's index stands for "nothing"
PRED_COLS, TRUTH_COLS = 80, 64
KEYS = ("ops", "dist", "pred_len", "truth_len", "truth_map", "pred_map", "conf")
LITERAL = [("ab", "b"), ("ab", "ba"), ("aa", "a"), ("a", "aa"), ("kitten", "sitting")]      # (truth, prediction): the contract's table


def _rows(lists, cols, fill=PAD):
    out = np.full((len(lists), cols), fill, np.int64)
    for k, r in enumerate(lists):
        assert len(r) <= cols
        out[k, :len(r)] = r
    return out


def _launch(pred, truth, num_classes=C, skip=(BLANK, PAD), conf=None, maps=True, with_conf=True):
    """One launch, nothing checked on the way (metrics.launch_edit_ops) -> dict of ndarrays, conf = what the launch added to a zeroed matrix
    (or to `conf`, a device tensor that is updated in place)."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    if conf is None and with_conf:
        conf = torch.zeros((num_classes + 1, num_classes + 1), dtype=torch.int32, device="cuda")
    outs = M.launch_edit_ops(dev(pred), dev(truth), skip, num_classes, conf, maps)
    got = {k: (None if t is None else t.cpu().numpy()) for k, t in zip(KEYS, outs)}
    got["conf"] = None if conf is None else conf.cpu().numpy()
    return got


def _assert_equal(got, want, what="", keys=KEYS):
    for k in keys:
        g, w = got[k], want[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
            raise AssertionError("%s %s: rows %s, got %s, want %s" % (what, k, bad[:6].tolist(), g[bad[:3]].tolist(), w[bad[:3]].tolist()))


def _cases():
    """[(pred row, truth row)] as lists, skip values included where a case wants them (the list of tests/test_gpu_score.py and the contract's own)."""
    rs = np.random.RandomState(1)
    word = lambda n, k=36: rs.randint(0, k, n).tolist()
    table = {ch: i for i, ch in enumerate(GOLD["lexicon"])}               # test-local: characters -> ints
    cases = []
    add = lambda p, t: cases.append((list(p), list(t)))
    add([], [])                                                           # both sides empty
    add(word(7), [])                                                      # one side empty
    add([], word(9))
    add(word(70), [])
    w = word(12)
    add(w, w)                                                             # equal rows
    w = word(64)
    add(w, w)
    for m in (1, 63, 64):                                                 # truth length exactly 1, 63, 64
        t = word(m, 3)
        add(word(5, 3), t)
        add(t[:m // 2] + word(3, 3) + t[m // 2:], t)
        add(word(PRED_COLS, 2), word(m, 2))                               # prediction longer than 64, of pred_cols exactly
        add(word(65, 3), t)
        add([v for k, v in enumerate(t) if k % 5 != 2], t)                # characters dropped from the truth
    add(word(PRED_COLS), word(20))
    a, b = word(10), word(8)
    add([BLANK, PAD] + a, [PAD, BLANK, BLANK] + b)                        # skip values at the start
    add(a[:4] + [BLANK] + a[4:6] + [PAD, PAD] + a[6:], b[:3] + [PAD] + b[3:])    # in the middle
    add(a + [BLANK, PAD, BLANK], b + [BLANK])                             # at the end (beyond the padding that every short row has)
    add([BLANK] + a[:5] + [PAD] * 60 + a[5:] + [BLANK], [PAD] * 40 + b + [BLANK] * 10)   # kept symbols in two 64-column chunks
    add([BLANK] * PRED_COLS, word(6))                                     # rows consisting only of skip values
    add(word(6), [PAD, BLANK] * (TRUTH_COLS // 2))
    add([PAD] * PRED_COLS, [BLANK] * TRUTH_COLS)
    for t, p in LITERAL:                                                  # the contract's table
        add([table[c] for c in p], [table[c] for c in t])
    for p, t, _ in GOLD["levenshtein"]:                                   # the reference-run pairs
        add([table[c] for c in p], [table[c] for c in t])
    return cases


def test_case_list_equals_the_reference_and_reaches_every_kind_of_step():
    cases = _cases()
    pred, truth = _rows([p for p, _ in cases], PRED_COLS), _rows([t for _, t in cases], TRUTH_COLS)
    want = R.batch(pred, truth, (BLANK, PAD), C)
    # the list is itself checked: each kind of step, a symbol without a counterpart on either side, a tie of rules 1 and 2, every length class
    assert (want["ops"].sum(0) > 0).all() and (want["truth_map"] == -1).any() and (want["pred_map"] == -1).any()
    assert any(R.script(R.filtered(p, (BLANK, PAD)), R.filtered(t, (BLANK, PAD)))[1] for p, t in cases)
    assert {0, 1, 63, 64} <= set(want["truth_len"].tolist()) and {0, 65, PRED_COLS} <= set(want["pred_len"].tolist())
    assert ((want["truth_len"] == 0) & (want["pred_len"] == 0)).any() and (want["dist"] == 0).sum() >= 4
    assert want["conf"][C, C] == 0 and want["conf"][C].sum() > 0 and want["conf"][:, C].sum() > 0
    got = _launch(pred, truth)
    _assert_equal(got, want)
    lit = len(cases) - len(GOLD["levenshtein"]) - len(LITERAL)                            # the table's rows, as literals
    assert got["ops"][lit:lit + 5].tolist() == [[1, 0, 1, 0], [0, 2, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1], [4, 2, 0, 1]]
    assert got["truth_map"][lit:lit + 5, :6].tolist() == [[-1, 0, -2, -2, -2, -2], [0, 1, -2, -2, -2, -2], [-1, 0, -2, -2, -2, -2],
                                                          [1, -2, -2, -2, -2, -2], [0, 1, 2, 3, 4, 5]]
    assert got["pred_map"][lit:lit + 5, :7].tolist() == [[1] + [-2] * 6, [0, 1] + [-2] * 5, [1] + [-2] * 6, [-1, 0] + [-2] * 5, [0, 1, 2, 3, 4, 5, -1]]
    assert (got["ops"][-len(GOLD["levenshtein"]):, 1:].sum(1)).tolist() == [int(d) for _, _, d in GOLD["levenshtein"]]
    # the three integers of crnn_edit_distance, from its own launch on the same tensors
    d, pl, tl = U.device_edit_distances(pred, truth, (BLANK, PAD))
    assert np.array_equal(d.cpu().numpy(), got["dist"]) and np.array_equal(pl.cpu().numpy(), got["pred_len"]) and np.array_equal(tl.cpu().numpy(), got["truth_len"])
    # the public wrapper: ndarrays of any integer dtype or device tensors in, int32 device tensors out
    outs = U.device_edit_ops(torch.from_numpy(pred).cuda().to(torch.int32), truth.astype(np.int16), (BLANK, PAD), C)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in outs) and tuple(outs[0].shape) == (len(cases), 4)
    assert tuple(outs[4].shape) == truth.shape and tuple(outs[5].shape) == pred.shape
    _assert_equal(dict(zip(KEYS, [t.cpu().numpy() for t in outs])), want, "wrapper", KEYS[:6])
    with pytest.raises(ValueError, match="64"):                                           # not symmetric: never swapped
        U.device_edit_ops(pred[:, :64], _rows([t for _, t in cases], 65), (BLANK, PAD), C)
    e = U.device_edit_ops(np.zeros((0, 5), np.int32), np.zeros((0, 3), np.int32), (BLANK, PAD), C)
    assert tuple(e[0].shape) == (0, 4) and tuple(e[1].shape) == (0,) and tuple(e[4].shape) == (0, 3)


def _random_pairs(n, seed, num_classes, pred_cols, truth_cols, full_every=4):
    """Rows with skip values sprinkled in; alphabets of 2, 3 and all `num_classes` symbols in turn (the small ones are where the ties are); every
    `full_every`-th pair uses the full widths.  skip = (num_classes, -1)."""
    rs = np.random.RandomState(seed)
    pred, truth = np.full((n, pred_cols), PAD, np.int64), np.full((n, truth_cols), num_classes, np.int64)
    for k in range(n):
        alpha = (min(2, num_classes), min(3, num_classes), num_classes)[k % 3]
        full = k % full_every == 0
        for row, cols in ((pred[k], pred_cols), (truth[k], truth_cols)):
            used = rs.randint(0, (cols if full else min(cols, 24)) + 1)
            vals = rs.randint(0, alpha, used) if k % 2 else num_classes - 1 - rs.randint(0, alpha, used)      # the top of the alphabet too
            holes = rs.rand(used) < (0.15 if k % 4 < 2 else 0.0)
            row[:used] = np.where(holes, rs.choice([num_classes, PAD], used), vals)
    return pred, truth


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 257])
@pytest.mark.parametrize("num_classes", [3, 38, 128])
def test_random_pairs_over_alphabets_and_batch_sizes_and_rows_past_n_untouched(num_classes, n):
    pred, truth = _random_pairs(n, 1000 * num_classes + n, num_classes, 52, 23)
    pred[0, :3], truth[0, :3] = [num_classes - 1, 0, num_classes - 1], [num_classes - 1, num_classes - 1, 0]      # the last real row of the matrix
    want = R.batch(pred, truth, (num_classes, PAD), num_classes)
    assert want["conf"][num_classes - 1].sum() > 0 and want["conf"][:, num_classes - 1].sum() > 0 and (want["ops"] >= 0).all()
    dp, dt = torch.from_numpy(pred.astype(np.int32)).cuda(), torch.from_numpy(truth.astype(np.int32)).cuda()
    fills = (-7, -8, -9, -10, -11, -12)
    outs = [torch.full((n + 9,) + tail, s, dtype=torch.int32, device="cuda") for s, tail in zip(fills, ((4,), (), (), (), (23,), (52,)))]
    conf = torch.zeros((num_classes + 1, num_classes + 1), dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = native.lib().crnn_edit_ops(p(dp), 52, p(dt), 23, num_classes, PAD, num_classes, *[p(o) for o in outs], p(conf), n,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    got = dict(zip(KEYS, [o.cpu().numpy() for o in outs] + [conf.cpu().numpy()]))
    _assert_equal({k: (v if k == "conf" else v[:n]) for k, v in got.items()}, want, "C = %d, n = %d" % (num_classes, n))
    for k, s in zip(KEYS, fills):
        assert (got[k][n:] == s).all(), k
    rc = native.lib().crnn_edit_ops(p(dp), 52, p(dt), 23, num_classes, PAD, num_classes, *[p(o) for o in outs], p(conf), 0, None)   # n == 0: nothing launched
    torch.cuda.synchronize()
    assert rc == 0 and all(np.array_equal(o.cpu().numpy(), got[k]) for o, k in zip(outs + [conf], KEYS))


def test_widest_prediction_with_kept_symbols_in_the_first_and_the_last_chunk():
    rs = np.random.RandomState(5)
    pred, truth = np.full((5, 1024), PAD, np.int64), np.full((5, 64), 128, np.int64)
    pred[0] = rs.randint(0, 3, 1024)                                      # every column kept, against a full truth word
    truth[0] = rs.randint(0, 3, 64)
    pred[1, :7], pred[1, 1020:] = rs.randint(0, 128, 7), [127, 0, 127, 5]        # the first and the last chunk only
    truth[1, :9] = list(pred[1, :7]) + [127, 5]
    pred[2, 960:] = rs.randint(0, 2, 64)                                  # the last chunk alone
    truth[2, :40] = rs.randint(0, 2, 40)
    keep = rs.rand(1024) < 0.3                                            # about 300 kept symbols over all sixteen chunks
    pred[3] = np.where(keep, rs.randint(0, 4, 1024), rs.choice([128, PAD], 1024))
    truth[3, 10:60] = rs.randint(0, 4, 50)
    truth[4, :5] = [1, 2, 3, 4, 5]                                        # an empty prediction
    want = R.batch(pred, truth, (128, PAD), 128)
    assert want["pred_len"].tolist()[:3] == [1024, 11, 64] and want["pred_len"][3] > 250 and want["pred_len"][4] == 0
    _assert_equal(_launch(pred, truth, 128, (128, PAD)), want)


def test_launches_accumulate_and_the_optional_outputs_change_nothing_else():
    pred, truth = _random_pairs(90, 11, 38, 60, 30)
    half = 41
    whole = _launch(pred, truth, 38, (38, PAD))
    _assert_equal(whole, R.batch(pred, truth, (38, PAD), 38))
    conf = torch.zeros((39, 39), dtype=torch.int32, device="cuda")
    first = _launch(pred[:half], truth[:half], 38, (38, PAD), conf=conf)
    alone = first["conf"].copy()
    second = _launch(pred[half:], truth[half:], 38, (38, PAD), conf=conf)                 # adds to what is there
    assert np.array_equal(second["conf"], whole["conf"])
    assert np.array_equal(second["conf"] - alone, _launch(pred[half:], truth[half:], 38, (38, PAD))["conf"])
    no_conf = _launch(pred, truth, 38, (38, PAD), with_conf=False)                        # conf = NULL: the same ops and maps
    assert no_conf["conf"] is None
    _assert_equal(no_conf, whole, "without the matrix", KEYS[:6])
    no_maps = _launch(pred, truth, 38, (38, PAD), maps=False)                             # maps = NULL: the same ops and matrix
    assert no_maps["truth_map"] is None and no_maps["pred_map"] is None
    _assert_equal(no_maps, whole, "without the maps", KEYS[:4] + KEYS[6:])
    again = _launch(pred, truth, 38, (38, PAD))                                           # the same launch twice: the same bits
    _assert_equal(again, whole, "second run")
    with pytest.raises(ValueError, match="confusion"):
        U.device_edit_ops(pred, truth, (38, PAD), 38, confusion=torch.zeros((38, 38), dtype=torch.int32, device="cuda"))


def test_labels_outside_the_alphabet_index_nothing():
    num_classes, skip = 12, (13, PAD)                                     # the skips are C + 1 and -1, so C and -5 are KEPT labels
    pred, truth = _random_pairs(21, 3, num_classes, 40, 20)
    pred[pred == num_classes], truth[truth == num_classes] = 13, 13
    pred[4, 2], truth[9, 0], pred[17, 39], truth[17, 19] = num_classes, -5, 1 << 20, -(1 << 30)
    bad = [4, 9, 17]
    good = [r for r in range(21) if r not in bad]
    want = R.batch(pred, truth, skip, num_classes)
    assert (want["ops"][bad] == -1).all() and (want["ops"][good] >= 0).all() and want["pred_len"][4] >= 1 and want["truth_len"][9] >= 1
    got = _launch(pred, truth, num_classes, skip)
    _assert_equal(got, want)
    assert (got["truth_map"][bad] == -2).all() and (got["pred_map"][bad] == -2).all()
    assert np.array_equal(got["conf"], _launch(pred[good], truth[good], num_classes, skip)["conf"])      # the matrix of the other rows alone
    with pytest.raises(ValueError, match="row 4"):
        U.device_edit_ops(pred, truth, skip, num_classes)


# ---- validation pass and CLI ----------------------------------------------------------------------------------------------------------------
def _tiny_generator(batches, batch, seed):
    """Batches of the tiny engine shape (40 x 32, max_len 6) as a Readf would yield them; the last two rows of the last batch are stale."""
    rs = np.random.RandomState(seed)
    for k in range(batches):
        x = rs.rand(batch, 40, 32, 1).astype(np.float32) * 2 - 1
        lab = np.full((batch, 6), -1, np.int64)
        for r in range(batch):
            used = rs.randint(1, 7)
            lab[r, :used] = rs.randint(0, 37, used)
        yield ({"the_input": x, "the_labels": lab}, None)


def test_score_generator_counts_the_real_pairs_of_a_short_tail_batch():
    inv = {i: ch for i, ch in enumerate(U.get_lexicon())}
    classes = {ch: i for i, ch in inv.items()}
    model = U.init_predictor(U.CRNN(num_classes=38, max_string_len=6, shape=(40, 32, 1), time_dense_size=32, n_units=64).get_model())
    dec = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=inv)
    plain = model.score_generator(_tiny_generator(3, 4, 0), steps=3, decoder=dec, length=10)
    assert plain.ops is None and plain.confusions is None and len(plain) == 10
    score = model.score_generator(_tiny_generator(3, 4, 0), steps=3, decoder=dec, length=10, confusions=True, maps=True)
    assert len(score) == 10 and score.ops.shape == (10, 4) and isinstance(score.confusions, U.Confusions)
    for name in ("labels", "distances", "pred_lengths", "true_lengths"):
        assert np.array_equal(getattr(score, name), getattr(plain, name)), name
    texts = score.texts(dec)
    truths = [dec.labels_to_text(lab) for batch, _ in _tiny_generator(3, 4, 0) for lab in batch["the_labels"]][:10]
    pairs = [([classes[c] for c in p], [classes[c] for c in t]) for p, t in zip(texts, truths)]
    print("decoded:", texts, "truth:", truths)
    assert np.array_equal(score.confusions.matrix, M.confusion_matrix(pairs, 37)) and score.confusions.matrix.shape == (38, 38)
    assert score.ops.tolist() == [list(M.edit_ops(p, t)[0]) for p, t in pairs]
    assert score.confusions.matrix[:37].sum() == sum(len(t) for t in truths)              # every real truth symbol once, no stale one
    for r, (p, t) in enumerate(pairs):
        _, tm, pm = M.edit_ops(p, t)
        assert score.truth_maps[r].tolist() == tm + [-2] * (6 - len(tm)) and score.pred_maps[r, :len(pm)].tolist() == pm
        assert (score.pred_maps[r, len(pm):] == -2).all()
    whole = model.score_generator(_tiny_generator(3, 4, 0), steps=3, decoder=dec, confusions=True)       # without `length`: 12 pairs count
    assert len(whole) == 12 and whole.ops[:10].tolist() == score.ops.tolist() and whole.truth_maps is None
    assert whole.confusions.matrix.sum() > score.confusions.matrix.sum()
    with pytest.raises(ValueError, match="confusions=True"):
        model.score_generator(_tiny_generator(1, 4, 0), steps=1, decoder=dec, maps=True)


def _make_dataset(folder, n, seed=0):
    from PIL import Image, ImageDraw
    rs = np.random.RandomState(seed)
    alphabet = "abcdefghij0123"
    for i in range(n):
        word = "".join(rs.choice(list(alphabet), size=rs.randint(2, 6)))
        img = Image.new("L", (20 + 12 * len(word), 28), color=235 if i % 3 else 30)
        ImageDraw.Draw(img).text((4, 6), word, fill=20 if i % 3 else 230)
        img.save(os.path.join(folder, "%d_%s_%d.png" % (i, word, i)))


def test_predict_cli_confusions_are_the_same_on_the_host_and_on_the_device(tmp_path, capsys):
    sys.path.insert(0, PKG)
    import predict as predict_cli
    mdir = tmp_path / "models" / "m1"
    os.makedirs(mdir)
    m = U.CRNN(num_classes=38, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()
    U.save_model_json(m, str(tmp_path / "models"), "m1")
    m.save_weights(str(mdir / "final_weights.h5"))
    fdir = tmp_path / "files"
    os.makedirs(fdir)
    _make_dataset(str(fdir), n=27)
    base = ["--model_path", str(mdir), "--image_path", str(fdir), "--batch_size", "4", "--G", "0", "--validate", "--train_portion", "0.5"]
    seen = []
    for flags in (["--confusions"], ["--confusions", "--device_score"], ["--confusions", "3", "--device_score"]):
        res = tmp_path / ("res_%d" % len(seen))
        os.makedirs(res)
        capsys.readouterr()
        predict_cli.main(base + ["--result_path", str(res)] + flags)
        out = capsys.readouterr().out.splitlines()
        assert len([l for l in out if "mean edit distance" in l]) == 1
        seen.append(([l for l in out if "aligned symbols" in l or " read as " in l], open(res / "confusions.csv").read()))
    assert seen[0] == seen[1] and seen[0][1] == seen[2][1]                                # 14 files (a tail batch of 2): the same lines, the same bytes
    assert len(seen[0][0]) >= 2 and seen[0][0][0].count("aligned symbols") == 1 and seen[2][0] == seen[0][0][:4]
    assert seen[0][1].splitlines()[0] == "truth,predicted,count" and len(seen[0][1].splitlines()) > 1
