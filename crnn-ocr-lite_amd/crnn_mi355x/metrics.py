"""Edit-distance metrics with the reference's names and return conventions (utils.py:262-298):
levenshtein -> float, edit_distance -> mean over pairs, normalized_edit_distance -> mean of d/len(truth)."""
import numpy as np

from .labels import class_items


def levenshtein(seq1, seq2):
    """Two-row dynamic programme (the reference fills the full matrix; same result, returned as float)."""
    n2 = len(seq2)
    prev = np.arange(n2 + 1, dtype=np.float64)
    for i, a in enumerate(seq1, 1):
        cur = np.empty(n2 + 1, dtype=np.float64)
        cur[0] = i
        for j, b in enumerate(seq2, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if a == b else 1))
        prev = cur
    return float(prev[n2])


def edit_distance(y_pred, y_true):
    total = len(y_true)
    return sum(levenshtein(p, t) / total for p, t in zip(y_pred, y_true)) if total else 0


def normalized_edit_distance(y_pred, y_true):
    total = len(y_true)
    return sum(levenshtein(p, t) / (len(t) * total) for p, t in zip(y_pred, y_true)) if total else 0


def edit_ops(pred, truth):
    """The edit script of `pred` against `truth` (two sequences of comparable symbols) -> (ops, truth_map, pred_map): the definition
    crnn_edit_ops (csrc/editops.hip) is held to.  D is the full Levenshtein matrix, i over the truth b, j over the prediction a; the script is
    the backtrace from (m, n) to (0, 0), at each cell the first rule that applies: 1. diagonal when i > 0, j > 0 and
    D[i][j] == D[i-1][j-1] + (b[i-1] != a[j-1]) -- a match or a substitution; 2. deletion of b[i-1] when i > 0 and D[i][j] == D[i-1][j] + 1;
    3. insertion of a[j-1].  ops = (matches, substitutions, deletions, insertions); truth_map[k] = the prediction position aligned to truth
    symbol k or -1 (deleted); pred_map[k] = the truth position aligned to prediction symbol k or -1 (inserted)."""
    a, b = list(pred), list(truth)
    n, m = len(a), len(b)
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    D[:, 0] = np.arange(m + 1)
    D[0, :] = np.arange(n + 1)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i, j] = min(D[i - 1, j - 1] + (b[i - 1] != a[j - 1]), D[i - 1, j] + 1, D[i, j - 1] + 1)
    truth_map, pred_map = [-1] * m, [-1] * n
    matches = subs = dels = ins = 0
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (b[i - 1] != a[j - 1]):
            if b[i - 1] == a[j - 1]:
                matches += 1
            else:
                subs += 1
            truth_map[i - 1], pred_map[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            dels += 1
            i -= 1
        else:
            ins += 1
            j -= 1
    return (matches, subs, dels, ins), truth_map, pred_map


def confusion_matrix(pairs, num_classes):
    """(prediction, truth) pairs of label sequences (integers in [0, num_classes), already filtered) -> the (C + 1, C + 1) int64 matrix of
    their edit scripts: row = truth class, column = predicted class, index C = nothing.  A match or substitution counts in [b][a], a deletion
    in [b][C], an insertion in [C][a]; [C][C] stays 0.  ValueError for a label outside the range."""
    C = int(num_classes)
    conf = np.zeros((C + 1, C + 1), dtype=np.int64)
    for r, (pred, truth) in enumerate(pairs):
        a, b = [int(v) for v in pred], [int(v) for v in truth]
        if any(not 0 <= v < C for v in a + b):
            raise ValueError("pair %d has a label outside [0, %d)" % (r, C))
        _, truth_map, pred_map = edit_ops(a, b)
        for k, j in enumerate(truth_map):
            conf[b[k], a[j] if j >= 0 else C] += 1
        for k, i in enumerate(pred_map):
            if i < 0:
                conf[C, a[k]] += 1
    return conf


# ---- scoring on the device (csrc/score.hip): the same numbers without a Python loop per pair ------------------------------------------
_MAX_TRUTH_COLS, _MAX_PRED_COLS = 64, 1024      # crnn_edit_distance: one 64-bit Myers word for the truth row


def check_label_metric(inverse_classes):
    """An edit distance over label rows is the edit distance over the decoded TEXTS only when every class maps to a distinct string of
    exactly one character (labels_to_text joins str(inverse_classes[c])).  Raises ValueError naming the first class that breaks that;
    accepts the {id: character} dictionary DecodeCTCPred holds, or a lexicon list."""
    seen = {}
    for k, ch in class_items(inverse_classes):
        s = str(ch)
        if len(s) != 1:
            raise ValueError("class %r maps to %r, not to one character: a distance over labels would not be the distance over texts" % (k, s))
        if s in seen:
            raise ValueError("class %r maps to %r, as class %r does: a distance over labels would not be the distance over texts" % (k, s, seen[s]))
        seen[s] = k


def device_edit_distances(pred_labels, true_labels, skip):
    """Rows of labels -> (dist, pred_len, true_len), int32 device tensors of length N, by one launch of crnn_edit_distance: each row is
    filtered of the two `skip` values (blank, -1), wherever they stand, and the rows are compared as plain integers.
    pred_labels (N, P), true_labels (N, Q): device tensors are used where they are, ndarrays (any integer dtype) are uploaded; both become int32.
    The kernel takes a truth of at most 64 columns and a prediction of at most 1024; the distance is symmetric, so when only the prediction
    fits the 64 the operands are passed swapped."""
    import torch
    from . import native
    from .engine import _ptr, _stream

    def dev(a, like=None):
        if not torch.is_tensor(a):
            a = np.asarray(a)
            if a.dtype.kind not in "iu":
                raise ValueError("label rows must be integers, got %s" % a.dtype)
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        if not a.is_cuda:
            a = a.to(like.device if like is not None and like.is_cuda else "cuda")
        return a.to(torch.int32).contiguous()
    pred = dev(pred_labels, true_labels if torch.is_tensor(true_labels) else None)
    truth = dev(true_labels, pred)
    if pred.dim() != 2 or truth.dim() != 2 or pred.shape[0] != truth.shape[0]:
        raise ValueError("expected (N, P) predictions and (N, Q) truths, got %r and %r" % (tuple(pred.shape), tuple(truth.shape)))
    skip0, skip1 = (int(s) for s in skip)
    n = pred.shape[0]
    out = torch.empty((3, n), dtype=torch.int32, device=pred.device)
    if n == 0:
        return out[0], out[1], out[2]
    a, b, la, lb = pred, truth, out[1], out[2]
    if truth.shape[1] > _MAX_TRUTH_COLS and pred.shape[1] <= _MAX_TRUTH_COLS:
        a, b, la, lb = truth, pred, out[2], out[1]
    with torch.cuda.device(pred.device):
        native.check(native.lib().crnn_edit_distance(_ptr(a), a.shape[1], _ptr(b), b.shape[1], skip0, skip1, _ptr(out[0]), _ptr(la), _ptr(lb), n,
                                                     _stream()), "edit_distance")
    return out[0], out[1], out[2]


def _device_rows(a, like=None):
    """Label rows for a launch: a device tensor where it is, an ndarray (any integer dtype) uploaded; int32, contiguous."""
    import torch
    if not torch.is_tensor(a):
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise ValueError("label rows must be integers, got %s" % a.dtype)
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
    if not a.is_cuda:
        a = a.to(like.device if like is not None and like.is_cuda else "cuda")
    return a.to(torch.int32).contiguous()


def launch_edit_ops(pred, truth, skip, num_classes, confusion=None, maps=True):
    """One launch of crnn_edit_ops over int32 device rows, nothing read back -> (ops (N, 4), dist, pred_len, true_len, truth_map, pred_map);
    the maps are None with maps=False.  What device_edit_ops and Model.score_generator share."""
    import torch
    from . import native
    from .engine import _ptr, _stream
    if pred.dim() != 2 or truth.dim() != 2 or pred.shape[0] != truth.shape[0]:
        raise ValueError("expected (N, P) predictions and (N, Q) truths, got %r and %r" % (tuple(pred.shape), tuple(truth.shape)))
    if truth.shape[1] > _MAX_TRUTH_COLS:
        raise ValueError("the truth has %d columns, crnn_edit_ops takes at most %d (the script is not symmetric: the operands cannot be swapped)"
                         % (truth.shape[1], _MAX_TRUTH_COLS))
    C = int(num_classes)
    if confusion is not None and not (torch.is_tensor(confusion) and confusion.is_cuda and confusion.dtype == torch.int32
                                      and tuple(confusion.shape) == (C + 1, C + 1) and confusion.is_contiguous()):
        raise ValueError("confusion must be a contiguous int32 device tensor of shape (%d, %d)" % (C + 1, C + 1))
    skip0, skip1 = (int(v) for v in skip)
    n = pred.shape[0]
    ops = torch.empty((n, 4), dtype=torch.int32, device=pred.device)
    out = torch.empty((3, n), dtype=torch.int32, device=pred.device)
    tmap = torch.empty((n, truth.shape[1]), dtype=torch.int32, device=pred.device) if maps else None
    pmap = torch.empty((n, pred.shape[1]), dtype=torch.int32, device=pred.device) if maps else None
    if n:
        with torch.cuda.device(pred.device):
            native.check(native.lib().crnn_edit_ops(_ptr(pred), pred.shape[1], _ptr(truth), truth.shape[1], skip0, skip1, C, _ptr(ops), _ptr(out[0]),
                                                    _ptr(out[1]), _ptr(out[2]), _ptr(tmap), _ptr(pmap), _ptr(confusion), n, _stream()), "edit_ops")
    return ops, out[0], out[1], out[2], tmap, pmap


def device_edit_ops(pred_labels, true_labels, skip, num_classes, confusion=None, maps=True):
    """Rows of labels -> (ops, dist, pred_len, true_len, truth_map, pred_map), int32 device tensors, by one launch of crnn_edit_ops
    (csrc/editops.hip): per pair the edit script metrics.edit_ops defines, over the rows filtered of the two `skip` values.  ops (N, 4) =
    matches, substitutions, deletions, insertions; truth_map (N, Q) and pred_map (N, P) hold filtered positions, -1 for a symbol without a
    counterpart, -2 past the filtered length (None with maps=False).  `confusion`: an int32 device tensor (C + 1, C + 1), C = num_classes,
    that the launch ADDS this batch's counts to (row = truth class, column = predicted class, index C = nothing); zero it once, pass it to every
    batch of a pass.  Upload and dtype handling as in device_edit_distances, but the script is not symmetric: a truth wider than 64 columns is
    a ValueError, never a swap.  Here a label indexes the matrix: a row with a kept label outside [0, C) raises ValueError naming the first such
    row (its ops come back -1 and it adds nothing to `confusion`; the check reads the ops back, which synchronises)."""
    import torch
    pred = _device_rows(pred_labels, true_labels if torch.is_tensor(true_labels) else None)
    truth = _device_rows(true_labels, pred)
    res = launch_edit_ops(pred, truth, skip, num_classes, confusion, maps)
    bad = torch.nonzero(res[0][:, 0] < 0)
    if len(bad):
        raise ValueError("row %d has a kept label outside [0, %d)" % (int(bad[0]), int(num_classes)))
    return res


class Confusions:
    """The (C + 1, C + 1) confusion counts of a validation pass as an int64 ndarray (row = truth class, column = predicted class, index C =
    nothing) with the characters of the classes: {id: character} or a list, as DecodeCTCPred holds them.  A cell of the device matrix is an
    int32: it overflows at 2^31 symbols."""

    def __init__(self, matrix, inverse_classes):
        self.matrix = np.array(matrix, dtype=np.int64)
        if self.matrix.ndim != 2 or self.matrix.shape[0] != self.matrix.shape[1] or self.matrix.shape[0] < 2:
            raise ValueError("expected a (C + 1, C + 1) matrix, got %r" % (self.matrix.shape,))
        self.inverse_classes = inverse_classes
        self.num_classes = self.matrix.shape[0] - 1
        chars = {int(k): str(ch) for k, ch in class_items(inverse_classes)}
        self.chars = [chars.get(c, "<%d>" % c) for c in range(self.num_classes)] + [""]      # '' = nothing

    @property
    def matches(self):
        return int(np.trace(self.matrix))

    @property
    def substitutions(self):
        C = self.num_classes
        return int(self.matrix[:C, :C].sum()) - int(np.trace(self.matrix[:C, :C]))

    @property
    def deletions(self):
        return int(self.matrix[:self.num_classes, self.num_classes].sum())

    @property
    def insertions(self):
        return int(self.matrix[self.num_classes, :self.num_classes].sum())

    def top(self, k):
        """The k largest off-diagonal cells as (truth character or '', predicted character or '', count): by count descending, then truth
        index, then prediction index."""
        t, p = np.nonzero(self.matrix)
        cells = sorted((-int(self.matrix[i, j]), int(i), int(j)) for i, j in zip(t, p) if i != j)
        return [(self.chars[i], self.chars[j], -c) for c, i, j in cells[:max(0, int(k))]]

    def per_class(self):
        """[(character, support, recall, precision)] per class: support = the truth symbols of the class (its row sum), recall =
        conf[c][c] / row sum, precision = conf[c][c] / column sum; None where the denominator is 0."""
        out = []
        for c in range(self.num_classes):
            hit, row, col = int(self.matrix[c, c]), int(self.matrix[c].sum()), int(self.matrix[:, c].sum())
            out.append((self.chars[c], row, hit / row if row else None, hit / col if col else None))
        return out

    def __add__(self, other):
        if not isinstance(other, Confusions) or other.matrix.shape != self.matrix.shape:
            return NotImplemented
        return Confusions(self.matrix + other.matrix, self.inverse_classes)

    def cells(self):
        """Every non-zero cell as (truth character or '', predicted character or '', count), in row-major order."""
        t, p = np.nonzero(self.matrix)
        return [(self.chars[i], self.chars[j], int(self.matrix[i, j])) for i, j in zip(t, p)]

    def to_csv(self, path):
        """truth, predicted, count of every non-zero cell ('' = nothing)."""
        import csv
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["truth", "predicted", "count"])
            w.writerows(self.cells())

    @classmethod
    def from_csv(cls, path, inverse_classes):
        import csv
        ids = {str(ch): int(k) for k, ch in class_items(inverse_classes)}
        C = max(ids.values()) + 1
        ids[""] = C
        m = np.zeros((C + 1, C + 1), dtype=np.int64)
        with open(path, newline="") as f:
            rows = list(csv.reader(f))
        for t, p, count in rows[1:]:
            m[ids[t], ids[p]] = int(count)
        return cls(m, inverse_classes)

    def report(self, k=20):
        """The totals and the top k confusions as text, one line each."""
        lines = [" [INFO] aligned symbols: %d matches, %d substitutions, %d deletions, %d insertions "
                 % (self.matches, self.substitutions, self.deletions, self.insertions)]
        name = lambda ch: repr(ch) if ch else "nothing"
        for t, p, count in self.top(k):
            lines.append(" [INFO]   %s read as %s: %d " % (name(t), name(p), count))
        return "\n".join(lines)


class Score:
    """What a validation pass brings back from the device: the decoded label rows (N, T) int32 padded with -1, and per pair the edit distance
    against the truth and the two filtered lengths, as ndarrays; with `ops` / `confusions` also the edit scripts' counts (csrc/editops.hip)."""

    def __init__(self, labels, distances, pred_lengths, true_lengths, ops=None, confusions=None):
        self.labels = np.asarray(labels, dtype=np.int32)
        self.distances = np.asarray(distances, dtype=np.int32).reshape(-1)
        self.pred_lengths = np.asarray(pred_lengths, dtype=np.int32).reshape(-1)
        self.true_lengths = np.asarray(true_lengths, dtype=np.int32).reshape(-1)
        # only from a pass that asked for them (score_generator(confusions=True)): per pair matches, substitutions, deletions, insertions
        # (N, 4), and the pass's Confusions
        self.ops = None if ops is None else np.asarray(ops, dtype=np.int32).reshape(-1, 4)
        self.confusions = confusions
        self.truth_maps = self.pred_maps = None     # score_generator(maps=True): (N, Q) / (N, T) positions, -1 no counterpart, -2 past the length

    def __len__(self):
        return len(self.distances)

    @property
    def edit_distance(self):
        """== metrics.edit_distance on the same pairs: the same float terms summed in the same order."""
        total = len(self.distances)
        return sum(float(d) / total for d in self.distances.tolist()) if total else 0

    @property
    def normalized_edit_distance(self):
        """== metrics.normalized_edit_distance on the same pairs; ZeroDivisionError for an empty truth, as there."""
        total = len(self.distances)
        return sum(float(d) / (t * total) for d, t in zip(self.distances.tolist(), self.true_lengths.tolist())) if total else 0

    @property
    def exact(self):
        return int((self.distances == 0).sum())

    @property
    def cer(self):
        """Character error rate: all edits over all truth characters."""
        return int(self.distances.sum(dtype=np.int64)) / int(self.true_lengths.sum(dtype=np.int64))

    def texts(self, decoder):
        return [decoder.labels_to_text(row) for row in self.labels]
