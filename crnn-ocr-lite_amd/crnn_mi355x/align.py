"""Character alignment (beyond the reference): where on the time axis each character of a transcription sits, and how sure the network is of
each one -- the best CTC path (Viterbi) of a given label through a softmax map, with its backtrace (csrc/align.hip, crnn_ctc_align).  It turns a
word recogniser's output into character spans, lets a reviewer find the one doubtful letter of a long word, and lets a training set be cleaned
of mislabelled crops (a label whose best path sits far below its total probability, LexiconDecoder.log_prob).

The labels are what a decoder's decode_labels(device=True) returns, so forward -> decode -> align involves no host copy until the final
read-back.  Values are sums of lsm = log_softmax(log(y + 1e-7)), the quantity the CTC loss and the lexicon scores are made of.

Frames are positions on the network's time axis, that is on the STN-rectified image; mapping them back to page pixels through the STN's affine
transform is out of scope here.

Tie rule (the library's contract): of equal values the higher state index wins -- among a state's predecessors staying beats a step, so where
values tie the path moves on as early as the word allows."""
import collections

import numpy as np

from .labels import CHUNK, Alphabet, device_map, label_table  # noqa: F401  (CHUNK: importable from here as before)

MAX_FRAMES = 512             # the library's limit on T - skip: backpointers and the path live in LDS

CharSpan = collections.namedtuple("CharSpan", "char start end log_prob")
CharSpan.__doc__ = """One aligned character: frames [start, end) of the softmax map it occupies (skip included), and the sum of its log-probabilities there."""
Alignment = collections.namedtuple("Alignment", "text log_prob chars states")
Alignment.__doc__ = """text; log_prob: the value of its best path (-inf: no alignment); chars: [CharSpan]; states: (T - skip,) int32, the best path's state
per frame of the window (even = blank, odd s = character (s - 1) / 2; -1 past the path or without an alignment)."""


def ctc_align(y, labels, lengths, skip=0, input_length=None):
    """y (B, T, C) float32 device tensor, labels (B, Lmax) / lengths (B,) int32 device tensors (one row per sample, any padding),
    input_length (B,) int32 device tensor or None -> dict of device tensors: score (B,), states (B, T - skip) int32, start / end (B, Lmax) int32
    in frames of the window (frame 0 = y[:, skip]), char_logp (B, Lmax).  One pre-pass and one launch (crnn_ctc_align) per CHUNK images; the
    outputs of the whole batch are allocated at once (4 (T - skip) + 12 Lmax + 4 bytes per image, next to a map of 4 T C).  A map with a NaN, an
    infinity or a negative entry gives no alignment.  Raises ValueError for more than 512 frames."""
    import torch
    from . import native
    from .engine import _ptr, _stream
    B, T, C = y.shape
    Lmax = labels.shape[1]
    if labels.shape[0] != B or lengths.shape[0] != B:
        raise ValueError("ctc_align: %d label rows and %d lengths for %d maps" % (labels.shape[0], lengths.shape[0], B))
    if not 0 < T - skip <= MAX_FRAMES:
        raise ValueError("ctc_align: %d frames (T = %d, skip = %d); the kernel aligns 1..%d" % (T - skip, T, skip, MAX_FRAMES))
    if Lmax < 1:                                              # (a decoder that was handed nothing returns (0, 0) tensors)
        labels = torch.full((B, 1), -1, dtype=torch.int32, device=y.device)
        Lmax = 1
    lib = native.lib()
    y = y.contiguous().float()
    labels, lengths = labels.contiguous(), lengths.contiguous()
    out = {"score": torch.full((B,), float("-inf"), dtype=torch.float32, device=y.device),
           "states": torch.full((B, max(T - skip, 0)), -1, dtype=torch.int32, device=y.device),
           "start": torch.full((B, Lmax), -1, dtype=torch.int32, device=y.device),
           "end": torch.full((B, Lmax), -1, dtype=torch.int32, device=y.device),
           "char_logp": torch.full((B, Lmax), float("-inf"), dtype=torch.float32, device=y.device)}
    if B == 0:
        return out
    rows = min(B, CHUNK)
    ws = torch.empty(max(1, lib.crnn_ctc_align_workspace_bytes(rows, T, C, skip) // 4), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        for lo in range(0, B, CHUNK):
            n = min(CHUNK, B - lo)
            il = input_length[lo:lo + n].contiguous() if input_length is not None else None
            native.check(lib.crnn_ctc_align(_ptr(y[lo:lo + n]), _ptr(il), _ptr(labels[lo:lo + n]), _ptr(lengths[lo:lo + n]), _ptr(out["score"][lo:lo + n]),
                                            _ptr(out["states"][lo:lo + n]), _ptr(out["start"][lo:lo + n]), _ptr(out["end"][lo:lo + n]),
                                            _ptr(out["char_logp"][lo:lo + n]), _ptr(ws), ws.numel() * 4, n, T, C, skip, Lmax, _stream()), "ctc_align")
    return out


class CTCAligner:
    """`inverse_classes`: {id: character} (what DecodeCTCPred holds) or a list of characters.  skip: 0 aligns over the frames the decoders read,
    2 over the training loss's window; spans are reported in frames of the map either way."""

    def __init__(self, inverse_classes, skip=0):
        self.alphabet = Alphabet(inverse_classes)
        self.inverse_classes, self.classes = inverse_classes, self.alphabet.classes
        self.skip = skip

    def encode(self, text):
        """Lexicon.encode's rule: -> list of label ids, or None for a text the alphabet cannot spell or one longer than 31."""
        return self.alphabet.encode(text)

    def _table(self, texts):
        return label_table([self.encode(str(t)) for t in texts])

    def align_labels(self, result, labels, lengths):
        """result (n, T, C) softmax (ndarray or device tensor), labels (n, Lmax) / lengths (n,) int32 device tensors -> ctc_align's dict of device
        tensors; nothing is copied back.  Frames are those of the window: add `skip` for frames of `result`."""
        y = device_map(result)
        return ctc_align(y, labels.to(y.device), lengths.to(y.device), self.skip)

    def _alignments(self, out, texts):
        """ctc_align's dict (tensors or ndarrays) + the texts -> [Alignment], spans moved by `skip` into frames of the map."""
        host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in out.items()}
        res = []
        for i, text in enumerate(texts):
            score = float(host["score"][i])
            chars = []
            if score != float("-inf"):
                for l, ch in enumerate(text):
                    chars.append(CharSpan(ch, int(host["start"][i, l]) + self.skip, int(host["end"][i, l]) + self.skip, float(host["char_logp"][i, l])))
            res.append(Alignment(text, score, chars, host["states"][i]))
        return res

    def align(self, result, texts):
        """One given transcription per image -> [Alignment].  A text the alphabet cannot spell, or one longer than 31, or one the frames cannot
        hold, gives log_prob = -inf and no chars.  A host array goes up in chunks of CHUNK images, as decode_labels uploads it, and each chunk's
        results come back before the next goes up."""
        import torch
        texts = [str(t) for t in texts]
        n = result.shape[0]
        if len(texts) != n:
            raise ValueError("align: %d texts for %d images" % (len(texts), n))
        table, lens = self._table(texts)                          # (-1 = a text that cannot be aligned: the kernel does not trust it)
        res = []
        for lo in range(0, n, CHUNK):
            y = device_map(result[lo:lo + CHUNK])
            out = ctc_align(y, torch.from_numpy(table[lo:lo + CHUNK]).to(y.device), torch.from_numpy(lens[lo:lo + CHUNK]).to(y.device), self.skip)
            res += self._alignments(out, texts[lo:lo + CHUNK])
        return res

    def align_decoded(self, result, decoder):
        """Decode and align in one go: decoder.decode_labels(result, device=True) -- a DecodeCTCPred (beam or greedy) or a LexiconDecoder -- and the
        alignment of every image to its own decoding; the label rows never leave the device.  -> [Alignment], texts as decoder.decode gives them."""
        y = device_map(result)
        labels, lengths = decoder.decode_labels(y, device=True)
        out = self.align_labels(y, labels, lengths)
        rows, lens = labels.cpu().numpy(), lengths.cpu().numpy()
        texts = [decoder.labels_to_text(rows[i, :lens[i]]) for i in range(rows.shape[0])]
        return self._alignments(out, texts)


def write_alignment_csv(path, fnames, alignments):
    """alignment.csv: fname, prediction, path_log_prob, chars -- chars = `char:start:end:log_prob` items joined by spaces."""
    import csv
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["fname", "prediction", "path_log_prob", "chars"])
        for name, a in zip(fnames, alignments):
            w.writerow([name, a.text, repr(a.log_prob), " ".join("%s:%d:%d:%r" % (c.char, c.start, c.end, c.log_prob) for c in a.chars)])
