"""Test-local restatement of the edit-script contract (include/crnn_mi355x.h: crnn_edit_ops), written independently of metrics.edit_ops: the full
Levenshtein matrix, the three rules in their order, the two maps and the confusion counts.  Both the host path and the device are compared with it."""
import numpy as np


def matrix(a, b):
    """D[i][j], i over the truth b, j over the prediction a: plain lists, the textbook recurrence."""
    D = [[0] * (len(a) + 1) for _ in range(len(b) + 1)]
    for i in range(len(b) + 1):
        for j in range(len(a) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (0 if b[i - 1] == a[j - 1] else 1), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D


def script(pred, truth):
    """-> [(kind, truth position or None, prediction position or None)] from the END of the words to their start: the backtrace itself.
    kind: 'match' / 'sub' / 'del' / 'ins'.  Also returns whether rules 1 and 2 both applied at some cell (a tie the priority decided)."""
    a, b = list(pred), list(truth)
    D = matrix(a, b)
    i, j, steps, tie = len(b), len(a), [], False
    while (i, j) != (0, 0):
        rule1 = i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (1 if b[i - 1] != a[j - 1] else 0)
        rule2 = i > 0 and D[i][j] == D[i - 1][j] + 1
        tie = tie or (rule1 and rule2)
        if rule1:
            steps.append(("match" if b[i - 1] == a[j - 1] else "sub", i - 1, j - 1))
            i, j = i - 1, j - 1
        elif rule2:
            steps.append(("del", i - 1, None))
            i -= 1
        else:
            assert j > 0 and D[i][j] == D[i][j - 1] + 1
            steps.append(("ins", None, j - 1))
            j -= 1
    return steps, tie


def edit_ops(pred, truth, steps=None):
    """-> ((matches, substitutions, deletions, insertions), truth_map, pred_map), the shape of metrics.edit_ops (`steps`: the pair's script, if the
    caller has it already)."""
    if steps is None:
        steps, _ = script(pred, truth)
    truth_map, pred_map = [-1] * len(truth), [-1] * len(pred)
    count = {"match": 0, "sub": 0, "del": 0, "ins": 0}
    for kind, ti, pj in steps:
        count[kind] += 1
        if kind in ("match", "sub"):
            truth_map[ti], pred_map[pj] = pj, ti
    return (count["match"], count["sub"], count["del"], count["ins"]), truth_map, pred_map


def confusion(pairs, C):
    """(C + 1, C + 1) int64 of the scripts of [(pred, truth)]: row = truth class, column = predicted class, index C = nothing."""
    conf = np.zeros((C + 1, C + 1), np.int64)
    for pred, truth in pairs:
        for kind, ti, pj in script(pred, truth)[0]:
            conf[C if ti is None else truth[ti], C if pj is None else pred[pj]] += 1
    return conf


def filtered(row, skip):
    return [int(v) for v in row if int(v) not in skip]


def batch(pred_rows, truth_rows, skip, C):
    """What one launch over full-width rows must write: dict of ops (N, 4), dist, pred_len, truth_len (N,), truth_map (N, Q), pred_map (N, P)
    (-2 past the filtered length) and conf.  A row with a kept label outside [0, C): ops -1, maps -2, nothing added to conf."""
    pred_rows, truth_rows = np.asarray(pred_rows), np.asarray(truth_rows)
    N, P, Q = len(pred_rows), pred_rows.shape[1], truth_rows.shape[1]
    out = dict(ops=np.zeros((N, 4), np.int64), dist=np.zeros(N, np.int64), pred_len=np.zeros(N, np.int64), truth_len=np.zeros(N, np.int64),
               truth_map=np.full((N, Q), -2, np.int64), pred_map=np.full((N, P), -2, np.int64), conf=np.zeros((C + 1, C + 1), np.int64))
    for r in range(N):
        a, b = filtered(pred_rows[r], skip), filtered(truth_rows[r], skip)
        out["dist"][r], out["pred_len"][r], out["truth_len"][r] = matrix(a, b)[len(b)][len(a)], len(a), len(b)
        if any(not 0 <= v < C for v in a + b):
            out["ops"][r] = -1
            continue
        ops, tm, pm = edit_ops(a, b)
        out["ops"][r] = ops
        out["truth_map"][r, :len(b)] = tm
        out["pred_map"][r, :len(a)] = pm
        out["conf"] += confusion([(a, b)], C)
    return out
