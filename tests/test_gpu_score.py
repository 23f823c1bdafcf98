"""-m gpu tests of the device scoring (csrc/score.hip through crnn_mi355x/metrics.py, Model.score_generator and predict.py --device_score): the
kernel's distances and filtered lengths equal metrics.levenshtein on the filtered rows as integers -- no tolerance, no excluded case -- over a
case list that is itself checked to reach every class of input, over random pairs on small and large alphabets and over batch sizes around the
wavefront / workgroup boundaries; the validation pass and the CLI report what the host path reports."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "helpers_golden.json")))
BLANK, PAD = 37, -1
PRED_COLS, TRUTH_COLS = 80, 64


def _filtered(row, skip=(BLANK, PAD)):
    return [int(v) for v in row if int(v) not in skip]


def _host(pred, truth, skip=(BLANK, PAD)):
    """(distances, pred lengths, truth lengths) by metrics.levenshtein on the filtered rows, as integers."""
    a, b = [_filtered(r, skip) for r in pred], [_filtered(r, skip) for r in truth]
    d = [M.levenshtein(x, y) for x, y in zip(a, b)]
    assert all(v == int(v) for v in d)
    return np.array([int(v) for v in d]), np.array([len(x) for x in a]), np.array([len(y) for y in b])


def _rows(lists, cols, fill=PAD):
    out = np.full((len(lists), cols), fill, np.int64)
    for k, r in enumerate(lists):
        assert len(r) <= cols
        out[k, :len(r)] = r
    return out


def _device(pred, truth, skip=(BLANK, PAD)):
    d, pl, tl = U.device_edit_distances(pred, truth, skip)
    assert all(t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (len(pred),) for t in (d, pl, tl))
    return d.cpu().numpy(), pl.cpu().numpy(), tl.cpu().numpy()


def _assert_equal(got, want, what=""):
    for g, w, name in zip(got, want, ("distance", "prediction length", "truth length")):
        bad = np.nonzero(g != w)[0]
        assert not len(bad), "%s %s: rows %s, got %s, want %s" % (what, name, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def _cases():
    """[(pred row, truth row)] as full-width rows (PRED_COLS / TRUTH_COLS), skip values included where a case wants them."""
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
    add(word(PRED_COLS), word(20))
    a, b = word(10), word(8)
    add([BLANK, PAD] + a, [PAD, BLANK, BLANK] + b)                        # skip values at the start
    add(a[:4] + [BLANK] + a[4:6] + [PAD, PAD] + a[6:], b[:3] + [PAD] + b[3:] )   # in the middle
    add(a + [BLANK, PAD, BLANK], b + [BLANK])                             # at the end (beyond the padding that every short row has)
    add([BLANK] + a[:5] + [PAD] * 60 + a[5:] + [BLANK], [PAD] * 40 + b + [BLANK] * 10)   # kept symbols in two 64-column chunks
    add([BLANK] * PRED_COLS, word(6))                                     # a row consisting only of skip values
    add(word(6), [PAD, BLANK] * (TRUTH_COLS // 2))
    add([PAD] * PRED_COLS, [BLANK] * TRUTH_COLS)
    for p, t, _ in GOLD["levenshtein"]:                                   # the reference-run pairs
        add([table[c] for c in p], [table[c] for c in t])
    return cases


def _classes_of(p, t):
    a, b = _filtered(p), _filtered(t)
    is_skip = lambda v: v in (BLANK, PAD)
    out = set()
    if not a and not b:
        out.add("both empty")
    if bool(a) != bool(b):
        out.add("one side empty")
    if a and a == b:
        out.add("equal rows")
    if len(b) in (1, 63, 64):
        out.add("truth length %d" % len(b))
    if len(a) > 64:
        out.add("prediction longer than 64")
    if len(a) == PRED_COLS:
        out.add("prediction of pred_cols exactly")
    for r, f in ((p, a), (t, b)):
        if f and r and is_skip(r[0]):
            out.add("skip at the start")
        kept = [k for k, v in enumerate(r) if not is_skip(v)]
        if kept and any(is_skip(v) for v in r[kept[0]:kept[-1]]):
            out.add("skip in the middle")
        if kept and len(r) > kept[-1] + 1:
            out.add("skip at the end")
        if r and not f:
            out.add("only skip values")
    return out


def test_kernel_equals_levenshtein_over_every_class_of_input():
    cases = _cases()
    want_classes = {"both empty", "one side empty", "equal rows", "truth length 1", "truth length 63", "truth length 64", "prediction longer than 64",
                    "prediction of pred_cols exactly", "skip at the start", "skip in the middle", "skip at the end", "only skip values"}
    seen = set().union(*[_classes_of(p, t) for p, t in cases])
    assert seen >= want_classes, "the case list never reaches %s" % sorted(want_classes - seen)
    gold = [(p, t, d) for p, t, d in GOLD["levenshtein"]]
    pred, truth = _rows([p for p, _ in cases], PRED_COLS), _rows([t for _, t in cases], TRUTH_COLS)
    got, want = _device(pred, truth), _host(pred, truth)
    _assert_equal(got, want)
    assert got[0][-len(gold):].tolist() == [int(d) for _, _, d in gold]    # the reference's own results for its pairs
    assert got[0].max() > 64 and (got[0] == 0).sum() >= 4
    _assert_equal(_device(torch.from_numpy(pred).cuda().to(torch.int32), truth.astype(np.int16)), want, "device tensor / int16 truth")
    _assert_equal(_device(pred[:, :64], _rows([t for _, t in cases], 100)), _host(pred[:, :64], truth), "swapped operands")   # only the prediction fits 64
    with pytest.raises(native.CrnnError):
        U.device_edit_distances(pred, _rows([t for _, t in cases], 65), (BLANK, PAD))
    e = U.device_edit_distances(np.zeros((0, 5), np.int32), np.zeros((0, 3), np.int32), (BLANK, PAD))
    assert all(tuple(t.shape) == (0,) for t in e)


def _random_pairs(n, seed, long_every=4, pred_cols=130, truth_cols=64):
    """Rows with skip values sprinkled in; alphabets of 2, 3 and 37 symbols in turn; every `long_every`-th pair uses the full widths."""
    rs = np.random.RandomState(seed)
    pred, truth = np.full((n, pred_cols), PAD, np.int64), np.full((n, truth_cols), BLANK, np.int64)
    for k in range(n):
        alpha = (2, 3, 37)[k % 3]
        full = k % long_every == 0
        for row, cols in ((pred[k], pred_cols), (truth[k], truth_cols)):
            used = rs.randint(0, (cols if full else min(cols, 24)) + 1)
            vals = rs.randint(0, alpha, used)
            holes = rs.rand(used) < (0.15 if k % 2 else 0.0)
            row[:used] = np.where(holes, rs.choice([BLANK, PAD], used), vals)
    return pred, truth


def test_4096_random_pairs_over_small_and_large_alphabets():
    pred, truth = _random_pairs(4096, 2)
    want = _host(pred, truth)
    assert want[2].max() == 64 and want[1].max() > 120 and (want[2] == 0).any() and (want[2] == 63).any()
    _assert_equal(_device(pred, truth), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 4097])
def test_batch_sizes_and_rows_past_n_untouched(n):
    pred, truth = _random_pairs(n, 100 + n, long_every=16, pred_cols=52, truth_cols=23)
    want = _host(pred, truth)
    dp, dt = torch.from_numpy(pred.astype(np.int32)).cuda(), torch.from_numpy(truth.astype(np.int32)).cuda()
    outs = [torch.full((n + 9,), s, dtype=torch.int32, device="cuda") for s in (-7, -8, -9)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = native.lib().crnn_edit_distance(p(dp), 52, p(dt), 23, BLANK, PAD, p(outs[0]), p(outs[1]), p(outs[2]), n,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    got = [o.cpu().numpy() for o in outs]
    _assert_equal([g[:n] for g in got], want, "n = %d" % n)
    for g, s in zip(got, (-7, -8, -9)):
        assert (g[n:] == s).all()
    rc = native.lib().crnn_edit_distance(p(dp), 52, p(dt), 23, BLANK, PAD, p(outs[0]), p(outs[1]), p(outs[2]), 0, None)     # n == 0: nothing launched
    torch.cuda.synchronize()
    assert rc == 0 and all(np.array_equal(o.cpu().numpy(), g) for o, g in zip(outs, got))


# ---- validation pass and CLI (the helpers follow tests/test_gpu_ingest.py) ---------------------------------------------------------------
def _make_dataset(folder, n=48, seed=0):
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


def _small_model():
    return U.CRNN(num_classes=38, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()


@pytest.fixture(scope="module")
def model():
    return U.init_predictor(_small_model())


@pytest.mark.parametrize("reader", ["Readf", "DeviceReadf"])
@pytest.mark.parametrize("greedy", [False, True])
def test_score_generator_equals_predict_decode_and_host_metrics(tmp_path, model, greedy, reader):
    names = _make_dataset(str(tmp_path), n=21)                          # batches of 8: two full ones and a tail of 5
    kw = dict(img_size=(100, 32, 1), normed=True, batch_size=8, classes=_classes(), max_len=23, transform_p=0.)
    dec = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes={v: k for k, v in _classes().items()}, greedy=greedy)
    host_reader = U.Readf(**kw)
    y = model.predict_generator(host_reader.run_generator(names), steps=3)
    ref_labels = dec.decode_labels(y)[:21]
    ref_texts = [dec.labels_to_text(r) for r in ref_labels]
    y_true = host_reader.get_labels(names)
    true_texts = [dec.labels_to_text(r) for r in y_true]
    assert all(true_texts) and true_texts[0] == os.path.basename(names[0]).split("_")[1]

    score = model.score_generator(getattr(U, reader)(**kw).run_generator(names), steps=3, decoder=dec, length=21)
    assert isinstance(score, U.Score) and len(score) == 21
    assert score.labels.dtype == np.int32 and np.array_equal(score.labels, ref_labels)
    assert score.texts(dec) == ref_texts
    assert score.distances.tolist() == [int(U.levenshtein(p, t)) for p, t in zip(ref_texts, true_texts)]
    assert score.pred_lengths.tolist() == [len(p) for p in ref_texts] and score.true_lengths.tolist() == [len(t) for t in true_texts]
    assert score.edit_distance == U.edit_distance(ref_texts, true_texts)
    assert score.normalized_edit_distance == U.normalized_edit_distance(ref_texts, true_texts)
    assert score.exact == sum(p == t for p, t in zip(ref_texts, true_texts))
    whole = model.score_generator(getattr(U, reader)(**kw).run_generator(names), steps=3, decoder=dec)        # without `length`: 24 rows
    assert len(whole) == 24 and np.array_equal(whole.labels[:21], ref_labels) and whole.distances[:21].tolist() == score.distances.tolist()
    dev_labels, dev_len = dec.decode_labels(torch.from_numpy(y).cuda(), device=True)                          # device in, device out
    assert dev_labels.is_cuda and dev_len.is_cuda and np.array_equal(dev_labels.cpu().numpy()[:21], ref_labels)
    assert np.array_equal(dec.decode_labels(torch.from_numpy(y).cuda())[:21], ref_labels)                     # the default: an ndarray
    assert dev_len.cpu().numpy()[:21].tolist() == [int((r != -1).sum()) for r in ref_labels]


def test_predict_cli_device_score_prints_the_same_metrics_and_writes_the_same_csv(tmp_path, capsys):
    sys.path.insert(0, PKG)
    import predict as predict_cli
    mdir = tmp_path / "models" / "m1"
    os.makedirs(mdir)
    m = _small_model()
    U.save_model_json(m, str(tmp_path / "models"), "m1")
    m.save_weights(str(mdir / "final_weights.h5"))
    fdir = tmp_path / "files"
    os.makedirs(fdir)
    _make_dataset(str(fdir), n=27)
    base = ["--model_path", str(mdir), "--image_path", str(fdir), "--batch_size", "4", "--G", "0", "--validate", "--train_portion", "0.5"]
    for ingest in ([], ["--device_ingest"]):
        seen = []
        for flag in ([], ["--device_score"]):
            res = tmp_path / ("res_%d_%d" % (len(ingest), len(flag)))
            os.makedirs(res)
            capsys.readouterr()
            predict_cli.main(base + ["--result_path", str(res)] + ingest + flag)
            out = capsys.readouterr().out
            line = [l for l in out.splitlines() if "mean edit distance" in l]
            pairs = [l for l in out.splitlines() if l.startswith(" [('") or l.startswith(" [(\"")]
            info = [l.split(" in ")[0] for l in out.splitlines() if "[INFO]" in l and " sec." in l]
            assert len(line) == 1 and "normalized edit distance score" in line[0]
            seen.append((line[0], open(res / "prediction.csv").read(), pairs, info))
        assert seen[0] == seen[1], ingest
        assert len(seen[0][1].splitlines()) == 15 and len(seen[0][3]) == 3       # 14 of the 27 files, and the three timed [INFO] lines
