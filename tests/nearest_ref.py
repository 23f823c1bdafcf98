"""Shared by tests/test_nearest_cpu.py and tests/test_gpu_nearest.py: the plain-Python reference of crnn_lexicon_nearest (the query filter, the
64-symbol truncation, Levenshtein, the minimum over the P rows, the distance 255 of an entry that cannot be trusted, the (distance, index) selection
with its ascending-index output) and the constructed fixture on which a shortlist decoder must equal the exhaustive one.  test_nearest_cpu.py pins
the Levenshtein here to crnn_mi355x.metrics.levenshtein."""
import numpy as np

MAX_QUERY = 64
UNTRUSTED = 255


def filter_query(row, C):
    """Elements inside [0, C - 2] in their order, the first 64 of them."""
    return [int(v) for v in row if 0 <= int(v) <= C - 2][:MAX_QUERY]


def levenshtein(a, b):
    """Unit costs, the two-row table."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[len(b)]


def distances(queries, labels, lengths, C):
    """queries (B, P, qcols) or (B, qcols) ints, labels (N, Lmax), lengths (N,) -> (B, N) int: min over p of the distance; 255 for an entry whose
    length is outside [0, Lmax] or that has a label outside [0, C - 2] inside its length."""
    q = np.asarray(queries)
    if q.ndim == 2:
        q = q[:, None, :]
    labels, lengths = np.asarray(labels), np.asarray(lengths)
    N, Lmax = labels.shape
    out = np.full((q.shape[0], N), UNTRUSTED, dtype=np.int64)
    words = []
    for j in range(N):
        L = int(lengths[j])
        w = [int(v) for v in labels[j, :L]] if 0 <= L <= Lmax else None
        words.append(w if w is not None and all(0 <= v <= C - 2 for v in w) else None)
    for b in range(q.shape[0]):
        qs = [filter_query(row, C) for row in q[b]]
        memo = {}
        for j, w in enumerate(words):
            if w is None:
                continue
            key = tuple(w)
            if key not in memo:
                memo[key] = min(levenshtein(x, w) for x in qs)
            out[b, j] = memo[key]
    return out


def select(d, K):
    """d (B, N) -> (idx (B, K), dist (B, K)) int32: the K entries smallest by (d, index) among d < 255, written in ascending index order, -1 after."""
    d = np.asarray(d)
    B, N = d.shape
    idx = np.full((B, K), -1, dtype=np.int32)
    dist = np.full((B, K), -1, dtype=np.int32)
    for b in range(B):
        order = sorted((int(d[b, j]), j) for j in range(N) if d[b, j] < UNTRUSTED)[:K]
        chosen = sorted(j for _, j in order)
        idx[b, :len(chosen)] = chosen
        dist[b, :len(chosen)] = d[b, chosen]
    return idx, dist


def nearest(queries, labels, lengths, C, K):
    return select(distances(queries, labels, lengths, C), K)


# ---- the constructed fixture -------------------------------------------------------------------------------------------------------------------
FIX_C, FIX_T, FIX_N, FIX_K, FIX_IMAGES, FIX_PEAK, FIX_SEED = 38, 24, 400, 16, 48, 0.9, 0
_FIX = {}


def fixture(C=FIX_C, N=FIX_N, images=FIX_IMAGES, seed=FIX_SEED, peak=FIX_PEAK):
    """-> (y (images, 24, C) float32 softmax maps, words: N distinct label sequences of lengths 2..10 over ids 0..11, sorted by length (stable)).
    Image i spells table word rs-chosen as character frame / blank frame and then blanks, the spelled class `peak` per frame and the rest spread
    evenly; i % 3 == 0: one character substituted, 1: one deleted, 2: clean.  Read-only, built once per argument set."""
    key = (C, N, images, seed, peak)
    if key not in _FIX:
        rs = np.random.RandomState(seed)
        seen, words = set(), []
        while len(words) < N:
            w = tuple(rs.randint(0, 12, size=rs.randint(2, 11)).tolist())
            if w not in seen:
                seen.add(w); words.append(list(w))
        words.sort(key=len)
        y = np.full((images, FIX_T, C), (1.0 - peak) / (C - 1), dtype=np.float64)
        for i in range(images):
            w = list(words[rs.randint(0, N)])
            if i % 3 == 0:
                k = rs.randint(0, len(w))
                w[k] = (w[k] + 1 + rs.randint(0, 11)) % 12
            elif i % 3 == 1:
                del w[rs.randint(0, len(w))]
            frames = [C - 1] * FIX_T
            for k, c in enumerate(w):
                frames[2 * k] = c
            y[i, np.arange(FIX_T), frames] = peak
        y = y.astype(np.float32)
        y.setflags(write=False)
        _FIX[key] = (y, words)
    return _FIX[key]
