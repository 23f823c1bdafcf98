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


class Score:
    """What a validation pass brings back from the device: the decoded label rows (N, T) int32 padded with -1, and per pair the edit distance
    against the truth and the two filtered lengths, as ndarrays."""

    def __init__(self, labels, distances, pred_lengths, true_lengths):
        self.labels = np.asarray(labels, dtype=np.int32)
        self.distances = np.asarray(distances, dtype=np.int32).reshape(-1)
        self.pred_lengths = np.asarray(pred_lengths, dtype=np.int32).reshape(-1)
        self.true_lengths = np.asarray(true_lengths, dtype=np.int32).reshape(-1)

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
