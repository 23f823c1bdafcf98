"""Shared by tests/test_lexicon_cpu.py and tests/test_gpu_lexicon.py: the fp64 reference of the lexicon scores and the fixed inputs both use.

_ref_scores is alpha-only and vectorised over (sample, word); test_lexicon_cpu.py pins it to oracle.ctc.ctc_loss_and_grad (score = -loss) and to
torch.nn.functional.ctc_loss, so the GPU tests can afford thousands of pairs where the pure-Python oracle affords hundreds."""
import numpy as np

EPS = 1e-7
SEGMENT_LENGTHS = (0, 1, 7, 8, 15, 16, 31)        # S = 2L + 1 = 1, 3, 15 | 17, 31 | 33, 63: both sides of the 16- and 32-lane segment limits, and the longest


def log_softmax_of_log(y, skip):
    """Keras ctc_batch_cost's input to TF: log(y + eps), and TF's own log-softmax on top; fp64.  -> (B, T - skip, C)"""
    z = np.log(np.asarray(y)[:, skip:, :].astype(np.float64) + EPS)
    m = z.max(-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))


def _ref_scores(y, words, input_len=None, skip=0):
    """y (B, T, C) softmax; words: list of label-id sequences (ids in [0, C - 2]); input_len (B,) or None (= T - skip), clamped to [0, T - skip].
    -> (B, N) float64: log p(word | y[b, skip : skip + Tb]); -inf where no path exists; Tb = 0: 0 for the empty word, -inf otherwise."""
    lsm = log_softmax_of_log(y, skip)
    B, Tmax, C = lsm.shape
    blank = C - 1
    N = len(words)
    Smax = 2 * max([len(w) for w in words] + [0]) + 1
    ext = np.full((N, Smax), blank, dtype=np.int64)
    S = np.zeros(N, dtype=np.int64)
    for n, w in enumerate(words):
        w = [int(v) for v in w]
        assert all(0 <= v < blank for v in w), w
        ext[n, 1:2 * len(w):2] = w
        S[n] = 2 * len(w) + 1
    s = np.arange(Smax)
    live = s[None, :] < S[:, None]                                         # (N, Smax)
    skip_ok = np.zeros((N, Smax), dtype=bool)
    skip_ok[:, 2:] = (ext[:, 2:] != blank) & (ext[:, 2:] != ext[:, :-2])
    skip_ok &= live
    Tb = np.full(B, Tmax, dtype=np.int64) if input_len is None else np.clip(np.asarray(input_len).reshape(-1).astype(np.int64), 0, Tmax)
    alpha = np.full((B, N, Smax), -np.inf)
    if Tmax > 0:
        alpha[:, :, 0] = lsm[:, 0, blank][:, None]
        if Smax > 1:
            alpha[:, :, 1] = np.where(S[None, :] > 1, lsm[:, 0, :][:, ext[:, 1]], -np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(1, Tmax):
            a1 = np.full_like(alpha, -np.inf); a1[:, :, 1:] = alpha[:, :, :-1]
            a2 = np.full_like(alpha, -np.inf); a2[:, :, 2:] = alpha[:, :, :-2]
            a2 = np.where(skip_ok[None], a2, -np.inf)
            new = np.logaddexp(np.logaddexp(alpha, a1), a2) + lsm[:, t, :][:, ext]       # (B, N, Smax)
            new = np.where(live[None], new, -np.inf)
            alpha = np.where((t < Tb)[:, None, None], new, alpha)
        last = np.take_along_axis(alpha, np.broadcast_to((S - 1)[None, :, None], (B, N, 1)), 2)[:, :, 0]
        prev = np.take_along_axis(alpha, np.broadcast_to(np.maximum(S - 2, 0)[None, :, None], (B, N, 1)), 2)[:, :, 0]
        out = np.where(S[None, :] > 1, np.logaddexp(last, prev), last)
    empty = np.where(S == 1, 0.0, -np.inf)
    return np.where((Tb == 0)[:, None], empty[None, :], out)


# ---- fixed inputs ---------------------------------------------------------------------------------------------------------------------------
_POST = {}


def posteriors(C, T=20):
    """y float32 (6, T, C): 0 peaked, 1 exactly uniform rows, 2 flat, 3 rows with exact zeros (a third of the classes, the blank in some frames),
    4 moderately peaked, 5 so peaked that most classes underflow to exact zeros in fp32.  Read-only, built once per (C, T)."""
    if (C, T) not in _POST:
        rs = np.random.RandomState(1000 + C + T)
        logits = rs.normal(size=(6, T, C)) * np.array([6.0, 0.0, 0.7, 2.0, 2.0, 60.0]).reshape(6, 1, 1)
        e = np.exp(logits - logits.max(-1, keepdims=True))
        y = e / e.sum(-1, keepdims=True)
        y[3][:, rs.permutation(C)[:C // 3]] = 0.0
        y[3][::4, C - 1] = 0.0
        y[3] /= y[3].sum(-1, keepdims=True)
        y = y.astype(np.float32)
        y[1] = np.float32(1.0 / C)
        assert (y[3] == 0).any() and (y[5] == 0).any()
        y.setflags(write=False)
        _POST[(C, T)] = y
    return _POST[(C, T)]


def input_lengths(T, skip):
    """0, 1, 2, 13 and T - skip (twice): one per sample of posteriors()."""
    return np.array([T - skip, 13, 2, T - skip, 1, 0], dtype=np.int64)


def make_words(C, n=40, seed=0, lengths=SEGMENT_LENGTHS):
    """n label sequences with lengths cycling through `lengths`, in no particular order of length; every third one doubles its first letter, every
    fifth one triples it; with C >= 66 every other word draws from the upper half of the alphabet (ids >= 64) only."""
    rs = np.random.RandomState(seed + C)
    words = []
    for i in range(n):
        L = lengths[i % len(lengths)]
        lo = 64 if (C >= 66 and i % 2) else 0
        w = rs.randint(lo, C - 1, size=L).tolist()
        if L >= 2 and i % 3 == 0:
            w[1] = w[0]
        if L >= 3 and i % 5 == 0:
            w[2] = w[1] = w[0]
        words.append(w)
    return words


def table(words, width=None, pad=-1):
    """-> (labels (N, width) int32 padded with `pad`, lengths (N,) int32)"""
    width = width or max([len(w) for w in words] + [1])
    lab = np.full((len(words), width), pad, dtype=np.int32)
    for i, w in enumerate(words):
        lab[i, :len(w)] = w
    return lab, np.array([len(w) for w in words], dtype=np.int32)
