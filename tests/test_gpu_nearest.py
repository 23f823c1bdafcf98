"""-m gpu tests of lexicon shortlists (csrc/lexicon_nearest.hip, crnn_mi355x/lexicon.py): distances and selected rows of crnn_lexicon_nearest
against the plain-Python reference of tests/nearest_ref.py (pinned to metrics.levenshtein in tests/test_nearest_cpu.py), the selection rule around
the tile and wavefront sizes, untrusted table entries, the refusals, and the surface: a shortlist LexiconDecoder against the exhaustive one
(equal whenever the exhaustive best word is in the shortlist: always for K >= N, and on all 48 images of the constructed fixture),
Lexicon.nearest, Model.score_generator and predict.py --lexicon_shortlist.
Shapes are the smallest at which the kernels take every path: queries on both sides of the 32-bit / 64-bit word and of the 64-symbol cut, query
rows of one and of several 64-column chunks, tables on both sides of a wavefront, of the selection sweep's 1024 entries and of the distance
kernel's tile (1024 words), rows with and without 16-byte alignment."""
import os
import sys

import numpy as np
import pytest
import torch

import utils as U
from gpu_util import L, dev, P, S, ok, host
from lexicon_ref import posteriors, make_words, table
import nearest_ref as NR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
TILE = 1024                                                  # NEAR_TILE of csrc/lexicon_nearest.hip


def _near(q, lab, ll, C, K):
    """Two calls of crnn_lexicon_nearest on pre-filled outputs -> (idx, dist) ndarrays (B, K); the calls must agree bit for bit."""
    q = np.asarray(q)
    if q.ndim == 2:
        q = q[:, None, :]
    B, Pn, qcols = q.shape
    N, Lmax = lab.shape
    qd, labd, lld = dev(q, np.int32), dev(lab, np.int32), dev(ll, np.int32)
    nbytes = L().crnn_lexicon_nearest_workspace_bytes(B, N)
    assert nbytes == B * (1024 + (N + 3) // 4 * 4)
    outs = []
    for fill in (77, -9):
        idx = torch.full((B, K), fill, dtype=torch.int32, device="cuda"); dist = torch.full((B, K), fill, dtype=torch.int32, device="cuda")
        ws = torch.full((max(1, nbytes // 4),), 0x5a5a5a5a, dtype=torch.int32, device="cuda")      # the entry point clears what it counts in
        ok(L().crnn_lexicon_nearest(P(qd), Pn, qcols, P(labd), P(lld), P(idx), P(dist), P(ws), nbytes, B, C, N, Lmax, K, S()))
        outs.append((host(idx), host(dist)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


def _scatter(rs, syms, qcols, C):
    """`syms` in order at random columns of a row of qcols, everything between them something the filter drops: -1, the blank, ids far outside"""
    row = rs.choice([-1, C - 1, C, 10000, -5], size=qcols)
    at = np.sort(rs.permutation(qcols)[:len(syms)])
    row[at] = syms
    return row


def _query_pool(rs, qcols, C, words, base, lo):
    """Query rows of `qcols` columns: nothing kept (three ways), table words and the hand query between dropped elements, and queries of
    m = 31, 32, 33, 64, 65 kept symbols where the row holds them (both machine words, and one symbol past the cut): random ones, and repetitions
    of `base`, a 31-letter word of the table, whose distances stay below m."""
    pool = [np.full(qcols, -1), np.full(qcols, C - 1), _scatter(rs, [], qcols, C)]
    for w in words:
        if 1 <= len(w) <= qcols:
            pool.append(_scatter(rs, w, qcols, C))
    for m in (31, 32, 33, 64, 65):
        if m <= qcols:
            pool.append(_scatter(rs, rs.randint(lo, C - 1, size=m), qcols, C))
            pool.append(_scatter(rs, (base + base + base)[:m], qcols, C))
    return pool


# ---- 1. distances and rows against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Pn", [1, 3])
@pytest.mark.parametrize("C", [38, 128])
def test_distances_and_rows_equal_the_reference(C, Pn):
    rs = np.random.RandomState(C + Pn)
    lo = 64 if C == 128 else 0
    words = make_words(C, n=21, seed=1)
    if C == 128:                                             # every letter from the upper half of the alphabet: the second class of a lane
        words = [[64 + v % 63 for v in w] for w in words]
    hand = [lo + 3, lo + 1, lo + 4, lo + 1, lo + 5, lo + 9, lo + 2, lo + 6]
    words += [[], list(hand), hand[::-1]]                    # the empty word, the query itself, the query reversed
    assert sorted(set(len(w) for w in words)) == [0, 1, 7, 8, 15, 16, 31] and min(min(w) for w in words if w) >= lo and len(words[6]) == 31
    assert any(len(w) >= 3 and w[0] == w[1] == w[2] for w in words)
    lab, ll = table(words, width=31)
    N = len(words)
    seen_m, split = set(), 0
    for qcols in (1, 64, 65, 200):
        pool = _query_pool(rs, qcols, C, [hand, words[2], words[5], words[-1]], words[6], lo)
        n = len(pool)
        q = np.stack([np.stack([pool[(i + 5 * p) % n] for p in range(Pn)]) for i in range(n)])      # sample i: rows i, i + 5, i + 10 of the pool
        assert q.shape == (n, Pn, qcols)
        seen_m |= {len([v for v in row if 0 <= v <= C - 2]) for row in pool}
        ref = NR.distances(q, lab, ll, C)
        assert ref.max() < 255
        idx, dist = _near(q, lab, ll, C, N)                  # K = N: every word's distance, in table order
        assert np.array_equal(idx, np.tile(np.arange(N, dtype=np.int32), (n, 1))), qcols
        assert np.array_equal(dist, ref), (qcols, np.argwhere(dist != ref)[:5])
        for K in (1, 5):
            ri, rd = NR.select(ref, K)
            idx, dist = _near(q, lab, ll, C, K)
            assert np.array_equal(idx, ri) and np.array_equal(dist, rd), (qcols, K)
        if Pn == 3:                                          # the minimum sits at a different row for different words of one sample
            per_row = np.stack([NR.distances(q[:, p], lab, ll, C) for p in range(Pn)])
            assert np.array_equal(per_row.min(0), ref)
            split += int((np.array([len(set(per_row[:, b, :].argmin(0).tolist())) for b in range(n)]) > 1).sum())
    assert {0, 8, 31, 32, 33, 64, 65} <= seen_m
    assert Pn == 1 or split >= 8


def test_rows_of_any_width_read_the_same_words():
    """Lmax = 8 (16-byte rows), 9, 10, 11 (no alignment) and 31: the same words in tables of different widths give the same rows."""
    C = 38
    rs = np.random.RandomState(3)
    words = [rs.randint(0, 12, size=rs.randint(0, 9)).tolist() for _ in range(70)]
    q = np.stack([_scatter(rs, rs.randint(0, 12, size=m), 24, C) for m in (0, 3, 5, 8, 8, 12)])
    want = None
    for width in (8, 9, 10, 11, 31):
        lab, ll = table(words, width=width)
        got = _near(q, lab, ll, C, 70)
        want = want or (NR.distances(q, lab, ll, C), got)
        assert np.array_equal(got[1], want[0]) and np.array_equal(got[0], want[1][0]), width


# ---- 2. selection --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, TILE + 1])
def test_selection_takes_the_lowest_indices_of_the_threshold_bin(N):
    """Tables of short words over three letters: many equal words, so the threshold bin holds far more than K.  K = 1, a few, N and past N."""
    C = 38
    rs = np.random.RandomState(N)
    words = [rs.randint(0, 3, size=rs.randint(0, 5)).tolist() for _ in range(N)]
    lab, ll = table(words, width=4)
    q = np.stack([_scatter(rs, rs.randint(0, 3, size=m), 12, C) for m in (0, 1, 2, 3, 4, 7)])
    ref = NR.distances(q, lab, ll, C)
    for K in sorted({1, 7, min(N, 1024), min(N + 3, 1024)}):
        ri, rd = NR.select(ref, K)
        idx, dist = _near(q, lab, ll, C, K)
        assert np.array_equal(idx, ri) and np.array_equal(dist, rd), K
        live = idx >= 0
        assert (live.sum(1) == min(K, N)).all() and (np.diff(np.where(live, idx, (1 << 30) + np.arange(K)), axis=1) > 0).all()      # ascending, the -1 tail last
        if K == 7 and N > 7:
            assert max(np.bincount(ref[b])[rd[b].max()] for b in range(6)) > K                      # (a threshold bin larger than the row)


def test_selection_over_65_samples_and_two_tiles():
    """B = 65, N = 2 tiles and 50 words, P = 2: every sample has its own query and its own row."""
    C, N, B = 38, 2 * TILE + 50, 65
    rs = np.random.RandomState(9)
    words = [rs.randint(0, 3, size=rs.randint(0, 5)).tolist() for _ in range(N)]
    lab, ll = table(words, width=5)
    q = np.stack([np.stack([_scatter(rs, rs.randint(0, 3, size=rs.randint(0, 7)), 10, C) for _ in range(2)]) for _ in range(B)])
    ri, rd = NR.nearest(q, lab, ll, C, 20)
    idx, dist = _near(q, lab, ll, C, 20)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd)
    assert len({tuple(r) for r in idx.tolist()}) > 20


def test_an_empty_table_fills_the_outputs_with_minus_one():
    q, lab, ll = dev(np.zeros((3, 1, 5)), np.int32), dev(np.zeros((1, 4)), np.int32), dev(np.zeros(1), np.int32)
    idx = torch.full((3, 4), 77, dtype=torch.int32, device="cuda"); dist = torch.full((3, 4), 77, dtype=torch.int32, device="cuda")
    ws = torch.zeros(3 * 256, dtype=torch.int32, device="cuda")
    ok(L().crnn_lexicon_nearest(P(q), 1, 5, P(lab), P(ll), P(idx), P(dist), P(ws), 3 * 1024, 3, 38, 0, 4, 4, S()))
    assert bool((idx == -1).all()) and bool((dist == -1).all())


# ---- 3. untrusted tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [38, 128])
def test_untrusted_entries_are_never_selected_and_leave_their_neighbours_alone(C):
    Lmax = 31
    rs = np.random.RandomState(C)
    words = make_words(C, n=24, seed=7, lengths=(1, 3, 7, 5, 15, 2))
    lab, ll = table(words, width=Lmax)
    q = np.stack([_scatter(rs, w, 40, C) for w in (words[2], words[9], words[14], [], words[19])])
    clean_i, clean_d = _near(q, lab, ll, C, 24)
    assert np.array_equal(clean_d, NR.distances(q, lab, ll, C))
    bad = {2: ("len", -1), 5: ("len", Lmax + 1), 9: ("len", 1 << 30), 10: ("id", C - 1), 13: ("id", 10000), 14: ("id", -5), 19: ("id", 1 << 30),
           23: ("len", -(1 << 31))}
    lab2, ll2 = lab.copy(), ll.copy()
    for n, (kind, v) in bad.items():
        if kind == "len":
            ll2[n] = v
        else:
            assert ll2[n] >= 1
            lab2[n, rs.randint(0, ll2[n])] = v
    good = [n for n in range(24) if n not in bad]
    idx, dist = _near(q, lab2, ll2, C, 24)
    assert np.array_equal(idx[:, :16], np.tile(np.array(good, dtype=np.int32), (5, 1))) and (idx[:, 16:] == -1).all() and (dist[:, 16:] == -1).all()
    assert np.array_equal(dist[:, :16], clean_d[:, good])
    ri, rd = NR.nearest(q, lab2, ll2, C, 3)
    idx, dist = _near(q, lab2, ll2, C, 3)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd) and not set(idx.ravel().tolist()) & set(bad)
    # a table of nothing but such entries: every slot unused
    idx, dist = _near(q, lab2[[2, 10, 13]], ll2[[2, 10, 13]], C, 2)
    assert (idx == -1).all() and (dist == -1).all()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    B, C, N, K, qcols = 6, 38, 40, 5, 24
    lab, ll = table(make_words(C, n=N, seed=0), width=31)
    q, labd, lld = dev(np.zeros((B, 1, qcols)), np.int32), dev(lab, np.int32), dev(ll, np.int32)
    idx = torch.full((B, K), 77, dtype=torch.int32, device="cuda"); dist = torch.full((B, K), 55, dtype=torch.int32, device="cuda")
    need = L().crnn_lexicon_nearest_workspace_bytes(B, N)
    ws = torch.full((need // 4 + 64,), 3, dtype=torch.int32, device="cuda")

    def call(q_=q, Pn=1, qc=qcols, words=labd, wl=lld, idx_=idx, dist_=dist, ws_=ws, nbytes=need, C_=C, Lmax=31, K_=K, B_=B, N_=N):
        return L().crnn_lexicon_nearest(P(q_), Pn, qc, P(words), P(wl), P(idx_), P(dist_), P(ws_), nbytes, B_, C_, N_, Lmax, K_, S())
    for kw in (dict(C_=1), dict(C_=129), dict(Lmax=0), dict(Lmax=32), dict(Pn=0), dict(Pn=9), dict(qc=0), dict(qc=1025), dict(K_=0), dict(K_=1025)):
        assert call(**kw) == -3, kw
    for kw in (dict(q_=None), dict(words=None), dict(wl=None), dict(idx_=None), dict(dist_=None), dict(ws_=None), dict(B_=-1), dict(N_=-1),
               dict(nbytes=need - 1), dict(nbytes=0)):
        assert call(**kw) == -2, kw
    torch.cuda.synchronize()
    assert bool((idx == 77).all()) and bool((dist == 55).all()) and bool((ws == 3).all())
    assert call() == 0                                       # the exact size is enough
    torch.cuda.synchronize()
    assert not bool((idx == 77).any()) and not bool((dist == 55).any()) and bool((ws[need // 4:] == 3).all())


# ---- 5. the decoder ----------------------------------------------------------------------------------------------------------------------------------
_INV = {i: ch for i, ch in enumerate(U.get_lexicon())}


def _lexicon_of(words):
    return U.Lexicon(["".join(_INV[c] for c in w) for w in words], _INV)


def _bits(t):
    return host(t).view(np.uint32)


@pytest.mark.parametrize("skip", [0, 2])
def test_a_shortlist_of_the_whole_table_decodes_as_the_exhaustive_decoder(skip):
    C, T = 38, 20
    y = torch.from_numpy(np.array(posteriors(C, T))).cuda()
    lex = _lexicon_of(sorted(make_words(C, n=40, seed=0), key=len))
    assert len(lex) == 40 and lex.num_classes == C
    ei, ev = U.LexiconDecoder(lex, top_paths=3, skip=skip)._topk(y, None, 3)
    assert bool((ei >= 0).any())
    for K, paths in ((40, 1), (1024, 3)):
        si, sv = U.LexiconDecoder(lex, top_paths=3, skip=skip, shortlist=K, paths=paths)._topk(y, None, 3)
        assert np.array_equal(host(si), host(ei)) and np.array_equal(_bits(sv), _bits(ev)), (K, paths)
    short = U.LexiconDecoder(lex, top_paths=3, skip=skip, shortlist=1024, score_bytes=2 * 40 * 4)      # chunks of two images
    assert short.decode(y) == U.LexiconDecoder(lex, skip=skip).decode(y)
    rows, lens = short.decode_labels(y, device=True)
    erows, elens = U.LexiconDecoder(lex, skip=skip).decode_labels(y, device=True)
    assert rows.is_cuda and np.array_equal(host(rows), host(erows)) and np.array_equal(host(lens), host(elens))
    # an explicit candidate list wins over the shortlist
    cands = [[b, b + 1, b + 2] for b in range(6)]
    assert short.decode(y, candidates=cands) == U.LexiconDecoder(lex, skip=skip).decode(y, candidates=cands)


@pytest.mark.parametrize("K,paths", [(1, 1), (4, 1), (4, 3), (16, 3)])
def test_where_the_best_word_is_shortlisted_both_decoders_agree_bit_for_bit(K, paths):
    """The fixture's maps against its 400 words.  The clean third of the images decodes to its own word, the only one at distance 0 and (the fp64
    reference in test_nearest_cpu.py) the best: at least those 16 images are hits for every K."""
    ynp, words = NR.fixture()
    y = torch.from_numpy(np.array(ynp)).cuda()
    lex = _lexicon_of(words)
    assert lex.labels[:, :10].tolist() == table(words, width=10)[0].tolist()          # already sorted by length: the table is the list
    ei, ev = U.LexiconDecoder(lex)._topk(y, None, 1)
    dec = U.LexiconDecoder(lex, shortlist=K, paths=paths)
    si, sv = dec._topk(y, None, 1)
    labels, lengths = lex.device(y.device)
    rows = host(dec._shortlist(y, labels, lengths, K))
    best = host(ei)[:, 0]
    hit = np.array([best[b] in rows[b] for b in range(len(best))])
    print("K = %d, %d paths: the exhaustive best is shortlisted on %d of %d images" % (K, paths, hit.sum(), len(hit)))
    assert hit.sum() >= 16
    assert np.array_equal(host(si)[hit], host(ei)[hit]) and np.array_equal(_bits(sv)[hit], _bits(ev)[hit])
    assert (host(sv)[~hit] <= host(ev)[~hit]).all()          # elsewhere the shortlist's best is some other word: never a better score


def test_the_constructed_fixture_decodes_as_the_exhaustive_decoder_on_all_48_images():
    ynp, words = NR.fixture()
    y = torch.from_numpy(np.array(ynp)).cuda()
    lex = _lexicon_of(words)
    ei, ev = U.LexiconDecoder(lex)._topk(y, None, 1)
    si, sv = U.LexiconDecoder(lex, shortlist=NR.FIX_K, paths=1)._topk(y, None, 1)
    assert ei.shape == (NR.FIX_IMAGES, 1) and bool((ei >= 0).all())
    assert np.array_equal(host(si), host(ei)) and np.array_equal(_bits(sv), _bits(ev))
    # the shortlist rows are the reference's rows for the device's own beam paths
    from crnn_mi355x.engine import beam_decode_lm
    paths, _, _ = beam_decode_lm(y, None, beam_width=10, top_paths=1, merge_repeated=False)
    labels, lengths = lex.device(y.device)
    idx, dist = U.lexicon_nearest(paths, labels, lengths, NR.FIX_K, NR.FIX_C)
    ri, rd = NR.nearest(host(paths), lex.labels, lex.lengths, NR.FIX_C, NR.FIX_K)
    assert np.array_equal(host(idx), ri) and np.array_equal(host(dist), rd)


# ---- 6. through the surface --------------------------------------------------------------------------------------------------------------------------
def test_lexicon_nearest_words_of_a_string():
    caller = ["string", "strong", "sting", "strung", "spring", "stringy", "ring", "", "text", "like", "string-like", "strnig", "a" * 31]
    lex = U.Lexicon(caller, _INV)
    queries = ["strnig-like text".replace(" ", "-"), "strnig", "", "zzzz"]
    words, dists = lex.nearest(queries, k=3)
    for qtext, w, d in zip(queries, words, dists):
        want = sorted((U.levenshtein(qtext, t), i) for i, t in enumerate(lex.words))[:3]
        assert w == [lex.words[i] for _, i in want] and d == [int(v) for v, _ in want], qtext
    assert words[1][0] == "strnig" and dists[1][0] == 0 and words[2][0] == "" and dists[0] == sorted(dists[0])
    # label rows, as a decoder returns them (the blank and -1 anywhere), and k past the lexicon
    row = np.array([[37, lex.classes["r"], -1, lex.classes["i"], lex.classes["n"], 37, lex.classes["g"], -1]])
    w, d = lex.nearest(row, k=20)
    assert w[0][0] == "ring" and d[0][0] == 0 and len(w[0]) == len(lex) and d[0] == sorted(d[0])
    assert lex.nearest(torch.from_numpy(row).cuda(), k=20) == (w, d)


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


def test_validation_and_the_cli_with_a_shortlist_of_the_whole_list(tmp_path, capsys):
    """Model.score_generator with a shortlist decoder reports what the exhaustive decoder reports when K >= N, and predict.py --lexicon_shortlist
    writes the same prediction.csv as predict.py --lexicon alone."""
    classes = {ch: i for i, ch in _INV.items()}
    m = U.CRNN(num_classes=38, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()
    model = U.init_predictor(m)
    fdir = tmp_path / "files"
    os.makedirs(fdir)
    names = _make_dataset(str(fdir), n=21)
    caller = sorted(set(os.path.basename(n).split("_")[1] for n in names)) + ["zebra", "", "0"]
    lex = U.Lexicon(caller, _INV)
    assert len(lex) < 64
    kw = dict(img_size=(100, 32, 1), normed=True, batch_size=8, classes=classes, max_len=23, transform_p=0.)
    scores = []
    for dec in (U.LexiconDecoder(lex), U.LexiconDecoder(lex, shortlist=64, paths=3)):
        s = model.score_generator(U.Readf(**kw).run_generator(names), steps=3, decoder=dec, length=21)
        assert isinstance(s, U.Score) and len(s) == 21
        scores.append((s.texts(dec), s.distances.tolist(), s.edit_distance, s.normalized_edit_distance))
    assert scores[0] == scores[1] and set(scores[0][0]) <= set(lex.words)
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
    for flags in ([], ["--lexicon_shortlist", "64"], ["--lexicon_shortlist", "64", "--lexicon_paths", "3", "--device_score"]):
        res = tmp_path / ("res%d" % len(flags))
        os.makedirs(res)
        capsys.readouterr()
        predict_cli.main(base + ["--result_path", str(res)] + flags)
        out = capsys.readouterr().out
        info = [l for l in out.splitlines() if "[INFO] Lexicon:" in l]
        assert len(info) == 1 and ("shortlist of the 64 words nearest" in info[0]) == bool(flags) and ("every word scored" in info[0]) == (not flags)
        line = [l for l in out.splitlines() if "mean edit distance" in l]
        assert len(line) == 1
        seen.append((line[0], open(res / "prediction.csv").read()))
    assert seen[0] == seen[1] == seen[2]
