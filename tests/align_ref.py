"""Shared by tests/test_align_cpu.py and tests/test_gpu_align.py: the references of the character alignment (csrc/align.hip).

viterbi_f64         the best CTC path of one word per sample in fp64 over lexicon_ref.log_softmax_of_log, with the library's tie rule;
                    test_align_cpu.py pins it to a brute-force enumeration of every CTC path.
viterbi_f32_replay  the same recursion in np.float32, operation for operation, over the lsm map the device's pre-pass wrote: max and add are exactly
                    rounded, so this is what the device must reproduce bit for bit.
Tie rule: equal values go to the higher state index -- stay beats s - 1 beats s - 2 (strict > in that order); at the end S - 1 beats S - 2 unless
v[S - 2] > v[S - 1]."""
import numpy as np

from lexicon_ref import log_softmax_of_log

MAX_LABEL_LEN = 31


def extended(word, blank):
    """-> (ext (S,), can_skip (S,) bool)"""
    S = 2 * len(word) + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = word
    can_skip = np.zeros(S, dtype=bool)
    can_skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return ext, can_skip


def _one(lsm, word, Tb, ft):
    """lsm (Tmax, C) of dtype ft -> (score, path (Tb,) or None)"""
    ninf = ft(-np.inf)
    blank = lsm.shape[1] - 1
    ext, can_skip = extended(word, blank)
    S = len(ext)
    if Tb == 0:
        return (ft(0.0) if S == 1 else ninf), (np.zeros(0, dtype=np.int32) if S == 1 else None)
    v = np.full(S, ninf, dtype=ft)
    v[0] = lsm[0, blank]
    if S > 1:
        v[1] = lsm[0, ext[1]]
    bp = np.zeros((Tb, S), dtype=np.int32)
    for t in range(1, Tb):
        v1 = np.full(S, ninf, dtype=ft); v1[1:] = v[:-1]
        v2 = np.full(S, ninf, dtype=ft); v2[2:] = v[:-2]; v2[~can_skip] = ninf
        best = v.copy()
        m = v1 > best; best[m] = v1[m]; bp[t][m] = 1
        m = v2 > best; best[m] = v2[m]; bp[t][m] = 2
        v = best + lsm[t, ext]
        assert v.dtype == ft
    fin = S - 1
    if S > 1 and v[S - 2] > v[S - 1]:
        fin = S - 2
    if v[fin] == ninf:
        return ninf, None
    path = np.zeros(Tb, dtype=np.int32)
    s = fin
    for t in range(Tb - 1, 0, -1):
        path[t] = s
        s -= bp[t, s]
    path[0] = s
    return v[fin], path


def _viterbi(lsm, words, input_len, width, ft):
    B, Tmax, C = lsm.shape
    assert lsm.dtype == ft and len(words) == B
    width = width or max([len(w) for w in words if w is not None] + [1])
    Tb = np.full(B, Tmax, dtype=np.int64) if input_len is None else np.clip(np.asarray(input_len).reshape(-1).astype(np.int64), 0, Tmax)
    score = np.full(B, -np.inf, dtype=ft)
    states = np.full((B, Tmax), -1, dtype=np.int32)
    start = np.full((B, width), -1, dtype=np.int32)
    end = np.full((B, width), -1, dtype=np.int32)
    char = np.full((B, width), -np.inf, dtype=ft)
    for b, w in enumerate(words):
        if w is None or len(w) > min(width, MAX_LABEL_LEN) or any(not 0 <= int(c) <= C - 2 for c in w):
            continue                                          # what the library does not trust: no alignment
        sc, path = _one(lsm[b], [int(c) for c in w], int(Tb[b]), ft)
        score[b] = sc
        if path is None:
            continue
        states[b, :len(path)] = path
        for l, c in enumerate(w):
            ts = np.nonzero(path == 2 * l + 1)[0]
            assert len(ts) and (np.diff(ts) == 1).all()
            start[b, l], end[b, l] = ts[0], ts[-1] + 1
            acc = lsm[b, ts[0], c]
            for t in ts[1:]:
                acc = acc + lsm[b, t, c]
            char[b, l] = acc
    return score, states, start, end, char


def viterbi_f64(y, words, input_len=None, skip=0, width=None):
    """y (B, T, C) softmax; words: ONE label-id sequence per sample (None, a sequence longer than min(width, 31) or with an id outside [0, C - 2]:
    no alignment); input_len (B,) or None (= T - skip), clamped to [0, T - skip]; width: columns of start / end / char sums.
    -> (score (B,), states (B, T - skip) int32, start, end (B, width) int32 in window frames, char sums (B, width)); fp64."""
    return _viterbi(log_softmax_of_log(y, skip), words, input_len, width, np.float64)


def viterbi_f32_replay(lsm, words, input_len=None, width=None):
    """The same over a float32 lsm map (B, T - skip, C) -- the one the device's pre-pass left in the workspace -- in np.float32 throughout."""
    return _viterbi(np.ascontiguousarray(lsm, dtype=np.float32), words, input_len, width, np.float32)


def path_is_valid(path, word, blank):
    """A CTC path of `word` in extended-label states: starts in {0, 1}, ends in {S - 2, S - 1}, moves by 0, 1 or 2, skips only where allowed."""
    ext, can_skip = extended(word, blank)
    S = len(ext)
    if len(path) == 0:
        return S == 1
    if path[0] not in (0, 1) or path[-1] not in (S - 1, S - 2) or min(path) < 0 or max(path) >= S:
        return False
    for a, b in zip(path[:-1], path[1:]):
        d = b - a
        if d not in (0, 1, 2) or (d == 2 and not can_skip[b]):
            return False
    return True


def brute_force(lsm, word):
    """Every CTC path of `word` through lsm (T, C), by enumeration: -> (best value, list of the paths that reach it), fp64."""
    import itertools
    T, C = lsm.shape
    ext, _ = extended(word, C - 1)
    best, arg = -np.inf, []
    for p in itertools.product(range(len(ext)), repeat=T):
        if not path_is_valid(p, word, C - 1):
            continue
        val = sum(lsm[t, ext[s]] for t, s in enumerate(p))
        if val > best + 1e-12:
            best, arg = val, [list(p)]
        elif abs(val - best) <= 1e-12:
            arg.append(list(p))
    return best, arg
