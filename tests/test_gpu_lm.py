"""-m gpu tests of the beam search with a character language model and N-best output (csrc/beam.hip, crnn_mi355x/lm.py): without a table both
entry points give the bits recorded from the plain decoder's former kernel (tests/golden/beam_bits.npz, written by tests/golden/make_beam_bits.py;
the two entry points run one kernel, so comparing them with each other alone would see no mistake in it), also at the plain decoder's capacity
edge, where the labels are the oracle's too; with one it follows the fp32 reference of tests/lm_beam_ref.py (pinned on the CPU by
tests/test_lm_cpu.py, which also names the near-tie rows -- the only rows not compared) on alphabets on both sides of 64 classes and on a
context that wraps; a language model changes what is read; N-best order and padding; refusals; determinism; the Python surface and
predict.py --lm --nbest."""
import csv
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import utils as U
from gpu_util import L, dev, zeros, P, S, ok, host
import lm_beam_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
NEG_INF = float("-inf")


def _decode(y, il, table, order, bw, top, merge):
    """one call of crnn_ctc_beam_decode_lm on ndarrays -> (labels (B, top, T), lengths (B, top), scores (B, top)) ndarrays; outputs pre-filled"""
    B, T, C = y.shape
    out = torch.full((B, top, T), 77, dtype=torch.int32, device="cuda")
    ln = torch.full((B, top), 78, dtype=torch.int32, device="cuda")
    sc = torch.full((B, top), 7.0, device="cuda")
    ok(L().crnn_ctc_beam_decode_lm(P(dev(y)), P(dev(il, np.int32)) if il is not None else None, P(dev(table)) if table is not None else None, order,
                                   P(out), P(ln), P(sc), B, T, C, bw, top, int(merge), S()))
    return host(out), host(ln), host(sc)


# ---- 1. the default scorer ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _recorded():
    """-> (tests/golden/make_beam_bits.py as a module, {name: int32 ndarray} of tests/golden/beam_bits.npz, the `hipcc --version` it was recorded with)"""
    spec = importlib.util.spec_from_file_location("make_beam_bits", os.path.join(ROOT, "tests", "golden", "make_beam_bits.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return (gen,) + gen.load()


def _assert_recorded(tag, entry, lab, lens, score_bits):
    """labels, lengths and score bits of one entry point equal the fixture's.  The fixture belongs to the compiler it was recorded with: another one
    may round logf / expf differently, and then it is to be recorded again from a commit known to be good -- not skipped."""
    gen, gold, recorded_with = _recorded()
    differ = [name for name, a in zip(gen.names(tag), (lab, lens, score_bits)) if a.dtype != np.int32 or not np.array_equal(a, gold[name])]
    here = gen.hipcc_version()
    assert not differ, "%s differs from tests/golden/beam_bits.npz in: %s\n%s\nfixture recorded with:\n%s\nthis machine:\n%s" % (
        entry, "; ".join(differ), "`hipcc --version` differs from the fixture's" if here != recorded_with else "same `hipcc --version` as the fixture",
        recorded_with, here)


@pytest.mark.parametrize("merge", [0, 1])
@pytest.mark.parametrize("bw", [1, 10, 64])
@pytest.mark.parametrize("C", [38, 97])
def test_without_a_table_it_is_the_plain_beam_search_bit_for_bit(C, bw, merge):
    y, il = R.plain_case_inputs(C, bw)
    B, T = R.PLAIN_B, R.PLAIN_T
    out = zeros(B, T, dtype=torch.int32); ln = zeros(B, dtype=torch.int32); sc = zeros(B)
    ok(L().crnn_ctc_beam_decode(P(dev(y)), P(dev(il, np.int32)), P(out), P(ln), P(sc), B, T, C, bw, merge, S()))
    lab, lens, scores = _decode(y, il, None, 1, bw, 1, merge)
    tag = _recorded()[0].case_tag(C, bw, merge)
    _assert_recorded(tag, "crnn_ctc_beam_decode", host(out), host(ln), host(sc).view(np.int32))
    _assert_recorded(tag, "crnn_ctc_beam_decode_lm", lab[:, 0], lens[:, 0], np.ascontiguousarray(scores[:, 0]).view(np.int32))
    assert np.array_equal(lab[:, 0], host(out)) and np.array_equal(lens[:, 0], host(ln))
    assert np.array_equal(scores[:, 0].view(np.uint32), host(sc).view(np.uint32))
    assert (lens[4:, 0] > 5).all()
    # an all-zero order-1 table: the same labels
    zl, zn, zs = _decode(y, il, np.zeros((1, C), np.float32), 1, bw, 1, merge)
    assert np.array_equal(zl, lab) and np.array_equal(zn, lens)
    assert np.allclose(zs, scores, rtol=1e-4, atol=1e-3)


def test_the_plain_decoder_keeps_its_capacity_edge():
    """T = 251 at width 64 takes 4 * (1 + 251 * 64) + 64 * 16 + 64 = 65348 of the 65536 bytes of LDS: the plain entry point still accepts it (the
    node table is far past its register copy: the LDS walk), T = 252 is refused by both, and a table's row cache no longer fits at T = 251."""
    from oracle import ctc
    C, B, T, bw = R.EDGE_C, R.EDGE_B, R.EDGE_T, R.EDGE_BW
    assert (C, B, T, bw, R.EDGE_MERGE) == (38, 2, 251, 64, 1)
    y = R.edge_inputs()
    out = torch.full((B, T), 1000, dtype=torch.int32, device="cuda"); ln = torch.full((B,), -5, dtype=torch.int32, device="cuda"); sc = zeros(B)
    ok(L().crnn_ctc_beam_decode(P(dev(y)), None, P(out), P(ln), P(sc), B, T, C, bw, 1, S()))
    out, ln, sc_bits = host(out), host(ln), host(sc).view(np.int32)
    want, want_len, _ = ctc.ctc_beam_decode(y, bw, True)      # neither row is a near-tie: tests/test_lm_cpu.py
    assert np.array_equal(out, want) and np.array_equal(ln, want_len) and (ln > 100).all()
    _assert_recorded(_recorded()[0].EDGE_TAG, "crnn_ctc_beam_decode", out, ln, sc_bits)
    # without a table crnn_ctc_beam_decode_lm has the same bound and gives the same bits
    lab, lens, scores = _decode(y, None, None, 1, bw, 1, 1)
    _assert_recorded(_recorded()[0].EDGE_TAG, "crnn_ctc_beam_decode_lm", lab[:, 0], lens[:, 0], np.ascontiguousarray(scores[:, 0]).view(np.int32))
    assert np.array_equal(lab[:, 0], out) and np.array_equal(lens[:, 0], ln) and np.array_equal(scores[:, 0].view(np.int32), sc_bits)
    # refusals: nothing is written
    o = torch.full((B, T + 1), 77, dtype=torch.int32, device="cuda"); n = torch.full((B,), 78, dtype=torch.int32, device="cuda")
    s = torch.full((B,), 7.0, device="cuda")
    y252, table = zeros(B, T + 1, C), zeros(1, C)
    assert L().crnn_ctc_beam_decode(P(y252), None, P(o), P(n), P(s), B, T + 1, C, bw, 1, S()) == -3
    assert L().crnn_ctc_beam_decode_lm(P(y252), None, None, 1, P(o), P(n), P(s), B, T + 1, C, bw, 1, 1, S()) == -3
    assert L().crnn_ctc_beam_decode_lm(P(dev(y)), None, P(table), 1, P(o), P(n), P(s), B, T, C, bw, 1, 1, S()) == -3
    torch.cuda.synchronize()
    assert bool((o == 77).all()) and bool((n == 78).all()) and bool((s == 7.0).all())


def test_the_plain_entry_point_checks_its_arguments():
    B, T, C = 4, 20, 38
    y = dev(R.posteriors(np.random.RandomState(0), B, T, C))
    out = torch.full((B, T), 77, dtype=torch.int32, device="cuda"); ln = torch.full((B,), 78, dtype=torch.int32, device="cuda")
    sc = torch.full((B,), 7.0, device="cuda")

    def call(y_=y, out_=out, ln_=ln, sc_=sc, B_=B, T_=T):
        return L().crnn_ctc_beam_decode(P(y_), None, P(out_), P(ln_), P(sc_), B_, T_, C, 10, 1, S())
    assert call(out_=None) == -2 and call(y_=None) == -2 and call(ln_=None) == -2 and call(sc_=None) == -2
    assert call(B_=-1) == -2 and call(T_=-1) == -2
    assert call(B_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((ln == 78).all()) and bool((sc == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 77).any()) and not bool((ln == 78).any()) and not bool((sc == 7.0).any())


# ---- 2. with a table, against the fp32 reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", R.CASE_WIDTHS)
@pytest.mark.parametrize("order,C,T", R.CASES)
def test_with_a_table_it_follows_the_fp32_reference(order, C, T, width):
    (ref_lab, ref_len, ref_sc, raw), near = R.case_reference(order, C, T, width)
    assert near.sum() <= R.NEAR_TIE_CAP
    rows = np.nonzero(~near)[0]                               # the skipped rows are exactly the near-tie rows
    y, table, il = R.case_inputs(order, C, T)
    merges = (False, True) if (order, C) == (2, 38) else (False,)
    for merge in merges:
        want_lab, want_len = R.remerge(raw, T, merge)
        if merge:
            assert (want_len < ref_len).any()                # the planted doubled letter: merge_repeated deletes something
        for top in (1, R.CASE_TOP):
            lab, lens, scores = _decode(y, il, table, order, width, top, merge)
            err = np.abs(scores[rows] - ref_sc[rows, :top])
            fin = np.isfinite(ref_sc[rows, :top])
            print("order %d C %d T %d width %d top %d merge %d: %d rows, max score error %.3e" % (order, C, T, width, top, merge, len(rows), err[fin].max()))
            assert np.array_equal(lens[rows], want_len[rows, :top])
            assert np.array_equal(lab[rows], want_lab[rows, :top])
            assert np.array_equal(np.isneginf(scores[rows]), np.isneginf(ref_sc[rows, :top]))
            assert (err[fin] <= 1e-3 + 1e-4 * np.abs(ref_sc[rows, :top][fin])).all()
    if C == 97:                                              # both halves of the two-classes-per-lane layout are read (at 66 classes the upper half is one label and the blank)
        assert (ref_lab >= 64).any() and ((ref_lab >= 0) & (ref_lab < 64)).any()
    # the table was read: without it the answers differ
    plain, _, _ = _decode(y, il, None, 1, width, 1, False)
    assert not np.array_equal(plain[:, 0], ref_lab[:, 0])


# ---- 3. the language model changes the answer -----------------------------------------------------------------------------------------------------
def test_a_language_model_changes_what_is_read():
    inv = {0: "a", 1: "b", 2: "c"}
    y = np.full((1, 4, 4), 0.02, dtype=np.float32)
    y[0, 0, 0] = 0.94                                        # a
    y[0, 1, 3] = 0.94                                        # blank
    y[0, 2] = [0.03, 0.50, 0.44, 0.03]                       # b, narrowly, or c
    y[0, 3, 3] = 0.94                                        # blank
    plain = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=inv)
    assert plain.decode(y) == ["ab"]
    assert U.LMDecoder(None, beam_width=10, inverse_classes=inv).decode(y) == ["ab"]
    lm = U.CharLM.from_words(["ac"] * 20 + ["ca"], inv, order=2)
    dec = U.LMDecoder(lm, alpha=1.0, beta=0.0, beam_width=10, top_paths=3)
    assert dec.decode(y) == ["ac"]
    top = dec.decode_topk(y)[0]
    assert top[0][0] == "ac" and top[0][1] > top[1][1] >= top[2][1] and len({t for t, _ in top}) == 3
    # the score: the beam's log-score of the string plus the model's weights, to the beam tolerance
    (seq, sc), = R.beam_lm_one(np.log(y[0] + np.float32(1e-7)), 10, (1.0 * lm.logp).astype(np.float32), 2, 1)
    assert seq == [0, 2] and abs(top[0][1] - sc) <= 1e-3 + 1e-4 * abs(sc)
    # weight 0 switches the model off
    assert U.LMDecoder(lm, alpha=0.0, beam_width=10).decode(y) == ["ab"]


# ---- 4. N-best ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,C", [(1, 38), (2, 38), (2, 97)])
def test_nbest_is_sorted_and_its_head_is_the_single_best(order, C):
    B, T = 24, 27
    rs = np.random.RandomState(order + C)
    y, table = R.posteriors(rs, B, T, C), (R.lm_table(rs, C, order) if order > 1 else None)
    il = np.full(B, T); il[:3] = [0, 1, 2]
    lab5, len5, sc5 = _decode(y, il, table, order, 10, 5, 0)
    lab1, len1, sc1 = _decode(y, il, table, order, 10, 1, 0)
    assert np.array_equal(lab5[:, 0], lab1[:, 0]) and np.array_equal(len5[:, 0], len1[:, 0])
    assert np.array_equal(sc5[:, 0].view(np.uint32), sc1[:, 0].view(np.uint32))
    assert (sc5[:, :-1] >= sc5[:, 1:]).all() and np.isfinite(sc5[3:]).all()
    for b in range(B):                                       # five different strings, each padded with -1 past its length
        seqs = [tuple(lab5[b, k, :len5[b, k]]) for k in range(5) if np.isfinite(sc5[b, k])]
        assert len(set(seqs)) == len(seqs) and all((lab5[b, k, len5[b, k]:] == -1).all() and (lab5[b, k, :len5[b, k]] >= 0).all() for k in range(5))
    # no frame: the root alone; its score is the end-of-word weight of the start context
    assert len5[0].tolist() == [0] * 5 and sc5[0, 0] == (table[-1, C - 1] if table is not None else 0.0) and np.isneginf(sc5[0, 1:]).all()
    assert (lab5[0] == -1).all()


def test_unused_paths_are_empty():
    """beam_width 3, one frame, one letter: the root and its only child are all the leaves there are; no frame: the root alone"""
    B, T, C = 6, 20, 2
    y = R.posteriors(np.random.RandomState(3), B, T, C)
    lab, lens, sc = _decode(y, np.ones(B, dtype=np.int64), None, 1, 3, 3, 0)
    assert np.isfinite(sc[:, :2]).all() and (np.sort(lens[:, :2], axis=1) == [0, 1]).all()
    assert (lens[:, 2] == 0).all() and np.isneginf(sc[:, 2]).all() and (lab[:, 2] == -1).all()
    assert (lab[:, :2, 1:] == -1).all() and (np.sort(lab[:, :2, 0], axis=1) == [-1, 0]).all()
    table = R.lm_table(np.random.RandomState(4), C, 2)
    lab, lens, sc = _decode(y, np.zeros(B, dtype=np.int64), table, 2, 3, 3, 0)
    assert (lens == 0).all() and (sc[:, 0] == table[1, 1]).all() and np.isneginf(sc[:, 1:]).all() and (lab == -1).all()
    # a 38-class map fills all three paths after one frame (the root may be among them or not)
    lab, lens, sc = _decode(R.posteriors(np.random.RandomState(3), B, T, 38), np.ones(B, dtype=np.int64), None, 1, 3, 3, 0)
    assert np.isfinite(sc).all() and (lens <= 1).all() and (lens.sum(1) >= 2).all()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    B, T, C = 4, 20, 38
    y = dev(R.posteriors(np.random.RandomState(0), B, T, C))
    table = zeros(38 * 38, 38)
    out = torch.full((B, 5, T), 77, dtype=torch.int32, device="cuda")
    ln = torch.full((B, 5), 78, dtype=torch.int32, device="cuda")
    sc = torch.full((B, 5), 7.0, device="cuda")

    def call(y_=y, lm=table, order=3, bw=10, top=5, C_=C, B_=B, T_=T, out_=out):
        return L().crnn_ctc_beam_decode_lm(P(y_), None, P(lm), order, P(out_), P(ln), P(sc), B_, T_, C_, bw, top, 0, S())
    assert call(bw=65) == -3 and call(bw=0) == -3 and call(bw=4, top=5) == -3 and call(top=0) == -3 and call(order=0) == -3
    assert call(order=5) == -3                                # 38 ** 4 * 38 * 4 bytes = 317 MB, above the cap
    assert call(C_=129) == -3 and call(C_=1) == -3
    assert call(bw=64, T_=300) == -3                          # the node table alone is past the LDS budget
    assert call(y_=None) == -2 and call(out_=None) == -2 and call(B_=-1) == -2
    assert call(B_=0) == 0
    assert L().crnn_ctc_lm_rows(38, 1) == 1 and L().crnn_ctc_lm_rows(38, 3) == 1444 and L().crnn_ctc_lm_rows(38, 4) == 54872
    assert L().crnn_ctc_lm_rows(38, 5) == 0 and L().crnn_ctc_lm_rows(128, 3) == 16384 and L().crnn_ctc_lm_rows(128, 4) == 0
    assert L().crnn_ctc_lm_rows(129, 1) == 0 and L().crnn_ctc_lm_rows(38, 0) == 0
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((ln == 78).all()) and bool((sc == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 77).any()) and not bool((ln == 78).any()) and not bool((sc == 7.0).any())
    with pytest.raises(ValueError):
        from crnn_mi355x import engine
        engine.beam_decode_lm(y, zeros(38, 37), order=2)


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit():
    order, C, T = 2, 97, 27
    y, table, il = R.case_inputs(order, C, T)
    a = _decode(y, il, table, order, 16, 3, 0)
    b = _decode(y, il, table, order, 16, 3, 0)
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))


# ---- 7. surface ---------------------------------------------------------------------------------------------------------------------------------
def _classes():
    return {ch: i for i, ch in enumerate(U.get_lexicon())}


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


def test_lm_decoder_in_validation_alignment_and_the_cli(tmp_path):
    inv = {v: k for k, v in _classes().items()}
    m = U.CRNN(num_classes=38, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()
    model = U.init_predictor(m)
    fdir = tmp_path / "files"
    os.makedirs(fdir)
    names = _make_dataset(str(fdir), n=13)
    words = [os.path.basename(n).split("_")[1] for n in names]
    lm = U.CharLM.from_words(words + ["Unspellable"], inv, order=3)
    assert lm.rejected == [(13, "Unspellable")]
    dec = U.LMDecoder(lm, alpha=0.8, beta=0.5, beam_width=10, top_paths=3)
    kw = dict(img_size=(100, 32, 1), normed=True, batch_size=8, classes=_classes(), max_len=23, transform_p=0.)
    reader = U.Readf(**kw)
    y = model.predict_generator(reader.run_generator(names), steps=2)[:13]
    texts = dec.decode(y)
    topk = dec.decode_topk(y)
    assert len(topk) == 13 and all(len(p) == 3 for p in topk) and [p[0][0] for p in topk] == texts
    assert all(p[0][1] >= p[1][1] >= p[2][1] > NEG_INF for p in topk)
    # Model.score_generator with the decoder, unmodified
    score = model.score_generator(U.Readf(**kw).run_generator(names), steps=2, decoder=dec, length=13)
    true_texts = [dec.labels_to_text(r) for r in reader.get_labels(names)]
    assert isinstance(score, U.Score) and len(score) == 13 and score.texts(dec) == texts and true_texts == words
    assert score.distances.tolist() == [int(U.levenshtein(p, t)) for p, t in zip(texts, true_texts)]
    # decode_labels(device=True) feeds the aligner
    labels, lengths = dec.decode_labels(torch.from_numpy(y).cuda(), device=True)
    assert labels.is_cuda and lengths.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == (13, 52)
    aligned = U.CTCAligner(inv).align_decoded(torch.from_numpy(y).cuda(), dec)
    assert [a.text for a in aligned] == texts
    # plain N-best: its head is DecodeCTCPred's answer
    plain = U.LMDecoder(None, beam_width=10, top_paths=3, merge_repeated=True, inverse_classes=inv)
    assert plain.decode(y) == U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes=inv).decode(y)
    # the command line, in a fresh process
    mdir = tmp_path / "models" / "m1"
    os.makedirs(mdir)
    U.save_model_json(m, str(tmp_path / "models"), "m1")
    m.save_weights(str(mdir / "final_weights.h5"))
    wl = tmp_path / "words.txt"
    wl.write_text("".join("%s\t%d\n" % (w, 1 + i % 3) for i, w in enumerate(words)) + "Unspellable\n")
    res = tmp_path / "res"
    os.makedirs(res)
    base = ["--model_path", str(mdir), "--image_path", str(fdir), "--batch_size", "8", "--G", "0"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    done = subprocess.run([sys.executable, os.path.join(PKG, "predict.py")] + base + ["--lm", str(wl), "--nbest", "3", "--result_path", str(res)], env=env,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:]
    assert "Language model: order 3 from 14 words, 1 rejected" in done.stdout
    pred = list(csv.reader(open(res / "prediction.csv", newline="")))
    rows = list(csv.reader(open(res / "nbest.csv", newline="")))
    assert rows[0] == ["", "fname", "rank", "text", "score"] and len(pred) == 14 and len(rows) == 1 + 3 * 13
    for i, p in enumerate(pred[1:]):
        mine = rows[1 + 3 * i:4 + 3 * i]
        assert [r[1] for r in mine] == [p[1]] * 3 and [r[2] for r in mine] == ["0", "1", "2"] and mine[0][3] == p[2]
        assert float(mine[0][4]) >= float(mine[1][4]) >= float(mine[2][4])
    # argument errors
    sys.path.insert(0, PKG)
    import predict as predict_cli
    for bad in (["--nbest", "3"], ["--lm", str(wl), "--lexicon", str(wl)], ["--nbest", "0", "--result_path", str(res)]):
        with pytest.raises(SystemExit):
            predict_cli.parse_args(base + bad)
