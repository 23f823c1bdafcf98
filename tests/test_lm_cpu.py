"""CPU tests of the language-model beam search's reference (tests/lm_beam_ref.py) and of crnn_mi355x.lm.CharLM: the reference is tied to the pinned
oracle (oracle.ctc) where the two overlap and to a brute-force enumeration where the search is exhaustive; the inputs of the GPU tests are
numerically stable (fp32 and fp64 runs of the reference agree on the label sequences, near-ties counted and capped)."""
import itertools

import numpy as np
import pytest

from oracle import ctc
from oracle.ctc import _logsumexp2, EPS, NEG_INF
import lm_beam_ref as R
from crnn_mi355x.lm import CharLM, read_word_list


# ---- 1. ties to the pinned oracle ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_maps():
    B, T, C = 24, 52, 38
    y = R.plant_double(R.posteriors(np.random.RandomState(7), B, T, C), 5, 3)
    il = np.full(B, T); il[:4] = [1, 2, 17, 51]
    return y, il


@pytest.mark.parametrize("bw", [10, 3, 25])
def test_reference_without_a_table_and_with_a_zero_table_is_the_pinned_oracle(oracle_maps, bw):
    y, il = oracle_maps
    B, T, C = y.shape
    runs = [R.beam_lm_decode(y, bw, None, 1, 1, False, il), R.beam_lm_decode(y, bw, np.zeros((1, C), np.float32), 1, 1, False, il)]
    for merge in (False, True):
        ref, rl, rsc = ctc.ctc_beam_decode(y, beam_width=bw, merge_repeated=merge, input_length=il)
        for out, lens, scores, raw in runs:
            lab, ln = R.remerge(raw, T, merge)
            assert np.array_equal(lab[:, 0], ref) and np.array_equal(ln[:, 0], rl)
            assert np.array_equal(scores[:, 0], rsc)
    assert np.array_equal(runs[0][0], R.remerge(runs[0][3], T, False)[0])
    assert (rl < runs[0][1][:, 0]).any()                     # merge_repeated did delete something: both settings were told apart


# ---- 2. brute force --------------------------------------------------------------------------------------------------------------------------------
def _enumerate(logits, table, order):
    """every alignment of T frames over C classes -> {labelling: log sum of its alignments + its LM weights + its end weight}, fp64"""
    T, C = logits.shape
    V, rows = C - 1, R.lm_rows(C, order)
    inp = logits - logits.max(1, keepdims=True)
    total = {}
    for path in itertools.product(range(C), repeat=T):
        lab = tuple(k for i, k in enumerate(path) if k != V and (i == 0 or k != path[i - 1]))
        total[lab] = _logsumexp2(total.get(lab, NEG_INF), float(sum(inp[t, k] for t, k in enumerate(path))))
    for lab in total:
        ctx = rows - 1
        for k in lab:
            total[lab] += table[ctx, k]
            ctx = (ctx * C + k) % rows
        total[lab] += table[ctx, V]
    return total


@pytest.mark.parametrize("order", [1, 2, 3])
def test_exhaustive_search_equals_the_enumeration_of_all_alignments(order):
    C, T = 4, 3
    rs = np.random.RandomState(order)
    for trial in range(4):
        y = R.posteriors(rs, 1, T, C)[0]
        table = R.lm_table(rs, C, order).astype(np.float64)
        logits = np.log(y.astype(np.float64) + EPS)
        got = R.beam_lm_one(logits, 64, table, order, 5, np.float64)
        want = sorted(_enumerate(logits, table, order).items(), key=lambda kv: -kv[1])[:5]
        assert len(want) == 5 and [tuple(s) for s, _ in got] == [k for k, _ in want]
        assert np.allclose([v for _, v in got], [v for _, v in want], rtol=0, atol=1e-9)
    # the table matters: without it another order
    plain = R.beam_lm_one(logits, 64, None, 1, 5, np.float64)
    assert [s for s, _ in plain] != [s for s, _ in got] or not np.allclose([v for _, v in plain], [v for _, v in got])


# ---- 3. numerical stability of the GPU inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", R.CASE_WIDTHS)
@pytest.mark.parametrize("order,C,T", R.CASES)
def test_gpu_inputs_are_stable_between_fp32_and_fp64(order, C, T, width):
    (lab, lens, scores, raw), near = R.case_reference(order, C, T, width)
    print("order %d C %d T %d width %d: %d of %d rows are near-ties" % (order, C, T, width, near.sum(), R.CASE_B))
    assert near.sum() <= R.NEAR_TIE_CAP
    assert np.isfinite(scores[4:]).all() and (lens[4:, 0] > 0).any()
    if order == 3 and C == 12:                               # contexts beyond rows: the wrap is exercised
        assert max(len(p[0]) for p in raw) >= 3


def test_capacity_edge_input_is_stable_between_fp32_and_fp64():
    """the T = 251, width 64 map that tests/golden/make_beam_bits.py records and the GPU test holds against oracle.ctc.ctc_beam_decode: neither row is a near-tie"""
    y = R.edge_inputs()
    assert y.shape == (2, 251, 38) and R.EDGE_BW == 64
    raw32 = R.beam_lm_decode(y, R.EDGE_BW, None, 1, 1, False, None, np.float32)[3]
    raw64 = R.beam_lm_decode(y, R.EDGE_BW, None, 1, 1, False, None, np.float64)[3]
    assert raw32 == raw64 and min(len(p[0]) for p in raw32) > 100


# ---- 4. CharLM -----------------------------------------------------------------------------------------------------------------------------------
ALPHA = list("abcdefghijklmnopqrstuvwxyz0123456789_")


def test_charlm_rows_sum_to_one_and_log_prob_walks_the_table():
    rs = np.random.RandomState(0)
    words = ["".join(rs.choice(ALPHA[:12], size=rs.randint(0, 7))) for _ in range(200)]
    for order in (1, 2, 3):
        lm = CharLM.from_words(words, ALPHA, order=order)
        assert lm.logp.shape == (38 ** (order - 1), 38) and lm.logp.dtype == np.float64 and np.isfinite(lm.logp).all()
        assert np.allclose(np.exp(lm.logp).sum(1), 1.0, atol=1e-12)
        for w in ("", "a", "abba", "zzz9"):
            ids = [ALPHA.index(ch) for ch in w]
            ctx, lp = lm.rows - 1, 0.0
            for i in ids:
                lp += lm.logp[ctx, i]; ctx = (ctx * 38 + i) % lm.rows
            assert lm.log_prob(w) == pytest.approx(lp + lm.logp[ctx, 37], abs=1e-12)
        assert lm.log_prob("A") == NEG_INF
    assert lm.log_prob(words[0]) > lm.log_prob("zzz9")        # seen text above unseen text


def test_charlm_tiny_corpus_by_hand():
    """["aa", "ab"] over {a, b}, order 2, mu = 1.  Unigrams: a 3, b 1, end 2 of 6 -> P1 = (n + 1/3) / 7.  Bigrams, P2 = (n(h, c) + P1(c)) / (n(h) + 1):
    after the start a 2 of 2; after a: a 1, b 1, end 1 of 3; after b: end 1 of 1."""
    lm = CharLM.from_words(["aa", "ab"], ["a", "b"], order=2, mu=1.0)
    p1 = np.array([10 / 21, 4 / 21, 7 / 21])
    want = np.array([(np.array([1, 1, 1]) + p1) / 4,         # row 0: after a
                     (np.array([0, 0, 1]) + p1) / 2,         # row 1: after b
                     (np.array([2, 0, 0]) + p1) / 3])        # row 2: at the start
    assert np.allclose(np.exp(lm.logp), want, atol=1e-15)
    assert lm.log_prob("ab") == pytest.approx(np.log(want[2, 0] * want[0, 1] * want[1, 2]))
    assert np.allclose(np.exp(CharLM.from_words(["aa", "ab"], ["a", "b"], order=1).logp), p1[None])
    # counts weigh the words
    twice = CharLM.from_words(["aa", "ab"], ["a", "b"], order=1, counts=[2, 0])
    assert np.allclose(np.exp(twice.logp), (np.array([4, 0, 2]) + 1 / 3) / 7)


def test_charlm_save_load_rejected_and_limits(tmp_path):
    lm = CharLM.from_words(["abc", "a-b", "Abc", "", "c"], {0: "a", 1: "b", 2: "c"}, order=3)
    assert lm.rejected == [(1, "a-b"), (2, "Abc")]
    path = str(tmp_path / "model.npz")
    lm.save(path)
    back = CharLM.load(path)
    assert back.order == 3 and back.classes == lm.classes and np.array_equal(back.logp, lm.logp)
    assert back.log_prob("abc") == lm.log_prob("abc")
    with pytest.raises(ValueError):
        CharLM(4, ALPHA + list("ABCDEFGHIJKLMNOPQRSTUVWXYZ"))       # 64 ** 3 rows * 64 * 4 bytes = 67 MB
    with pytest.raises(ValueError):
        CharLM(0, ALPHA)
    with pytest.raises(ValueError):
        CharLM(1, ["a", "b"], logp=np.array([[0.0, -np.inf, 0.0]]))
    assert np.allclose(CharLM(2, ["a", "b"]).logp, -np.log(3))
    wl = tmp_path / "words.txt"
    wl.write_text("abc\t3\nb\n\ncab\t0.5\n")
    assert read_word_list(str(wl)) == (["abc", "b", "", "cab"], [3.0, 1.0, 1.0, 0.5])


def test_charlm_table_layout_on_the_host():
    """table(): label columns alpha * logp + beta, the end column without the bonus; float32; cached per (alpha, beta)"""
    lm = CharLM.from_words(["abba", "ab"], ["a", "b"], order=2)
    t = lm.table(0.7, 0.25, device="cpu")
    assert t.dtype.is_floating_point and t.element_size() == 4 and tuple(t.shape) == (3, 3)
    want = 0.7 * lm.logp
    want[:, :2] += 0.25
    assert np.array_equal(t.numpy(), want.astype(np.float32))
    assert lm.table(0.7, 0.25, device="cpu") is t and lm.table(0.7, 0.0, device="cpu") is not t
    assert np.array_equal(lm.table(0.7, 0.0, device="cpu").numpy()[:, 2], t.numpy()[:, 2])
