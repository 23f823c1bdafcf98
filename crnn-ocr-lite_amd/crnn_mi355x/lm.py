"""Open-vocabulary decoding with a character language model (beyond the reference): the TF beam search of DecodeCTCPred with TF's BeamScorer hooks
filled in by a dense character n-gram table (shallow fusion), and N-best output -- csrc/beam.hip, one launch per batch, nothing but labels,
lengths and scores comes back.  LexiconDecoder answers "which word of this list"; LMDecoder reads any string and lets the statistics of a word
list (or of any text) steer the beam.

The table: row = a context = the last order - 1 characters as a base-C number (C = alphabet + 1; symbol C - 1 = "before the word starts"),
column c < C - 1 = log P(c | context), column C - 1 = log P(end of word | context).  Dense: order 3 at 38 classes is 219 KB, order 4 is 8.3 MB,
order 3 at 128 classes 8.4 MB; the library's cap is 16 MiB."""
import numpy as np

from .labels import Alphabet, class_items, decode_chunks

TABLE_MAX_BYTES = 16 << 20   # CRNN_LM_TABLE_MAX_BYTES


class CharLM:
    """A character n-gram model over the model's alphabet.  `inverse_classes`: {id: character} (what DecodeCTCPred holds) or a list of characters.
    .logp: float64 [rows][V + 1], rows = (V + 1) ** (order - 1); without `logp` the model is uniform."""

    def __init__(self, order, inverse_classes, logp=None):
        self.alphabet = Alphabet(inverse_classes)
        self.inverse_classes, self.classes = inverse_classes, self.alphabet.classes
        self.order = int(order)
        self.C = len(self.classes) + 1
        if self.order < 1:
            raise ValueError("CharLM: order must be >= 1")
        self.rows = self.C ** (self.order - 1)
        if self.rows * self.C * 4 > TABLE_MAX_BYTES:
            raise ValueError("CharLM: a dense order-%d table over %d symbols is %d bytes, above the %d the decoder takes"
                             % (self.order, self.C, self.rows * self.C * 4, TABLE_MAX_BYTES))
        if sorted(self.classes.values()) != list(range(self.C - 1)):
            raise ValueError("CharLM: the alphabet's ids must be 0..V-1")
        self.logp = np.full((self.rows, self.C), -np.log(self.C)) if logp is None else np.asarray(logp, dtype=np.float64)
        if self.logp.shape != (self.rows, self.C) or not np.isfinite(self.logp).all():
            raise ValueError("CharLM: logp must be a finite (%d, %d) array" % (self.rows, self.C))
        self.rejected = []
        self._dev = {}

    @classmethod
    def from_words(cls, words, inverse_classes, order=3, counts=None, mu=1.0):
        """Counts the n-grams of every word padded with order - 1 start symbols and one end symbol (`counts`: a weight per word, default 1) and
        smooths by interpolation with the lower order, P_k(c | h) = (n(h, c) + mu * P_{k-1}(c | h')) / (n(h) + mu), h' = h without its oldest
        character, P_0 uniform over the V + 1 symbols: every entry is positive, so every log is finite.  Words with a character outside the
        alphabet go to `.rejected` as (caller position, word) and are not counted."""
        self = cls(order, inverse_classes)
        C, V = self.C, self.C - 1
        hist, sym, wt = [], [], []
        for p, w in enumerate(words):
            w = str(w)
            ids = [self.classes.get(ch) for ch in w]
            if any(i is None for i in ids):
                self.rejected.append((p, w))
                continue
            seq = np.array([V] * (order - 1) + ids + [V], dtype=np.int64)
            m = len(ids) + 1
            hist.append(np.stack([seq[j:j + m] for j in range(order - 1)], 1) if order > 1 else np.zeros((m, 0), np.int64))
            sym.append(seq[order - 1:])
            wt.append(np.full(m, 1.0 if counts is None else float(counts[p])))
        hist = np.concatenate(hist) if hist else np.zeros((0, order - 1), np.int64)
        sym = np.concatenate(sym) if sym else np.zeros(0, np.int64)
        wt = np.concatenate(wt) if wt else np.zeros(0)
        p = np.full((1, C), 1.0 / C)                          # P_0
        for k in range(1, order + 1):
            rows = C ** (k - 1)
            ctx = np.zeros(len(sym), dtype=np.int64)
            for j in range(order - k, order - 1):             # the last k - 1 characters, oldest first
                ctx = ctx * C + hist[:, j]
            n = np.zeros((rows, C))
            np.add.at(n, (ctx, sym), wt)
            lower = p[np.arange(rows) % p.shape[0]]           # h' = h mod C ** (k - 2)
            p = (n + mu * lower) / (n.sum(1, keepdims=True) + mu)
        self.logp = np.log(p)
        return self

    def log_prob(self, text):
        """log P(text, end of word) under the model, float64, by walking the table as the decoder does; -inf for a text the alphabet cannot spell"""
        ids = [self.classes.get(ch) for ch in str(text)]
        if any(i is None for i in ids):
            return float("-inf")
        ctx, lp = self.rows - 1, 0.0
        for i in ids:
            lp += self.logp[ctx, i]
            ctx = (ctx * self.C + i) % self.rows
        return float(lp + self.logp[ctx, self.C - 1])

    def save(self, path):
        chars = [""] * (self.C - 1)
        for k, ch in class_items(self.inverse_classes):
            chars[int(k)] = str(ch)
        with open(path, "wb") as f:
            np.savez(f, order=np.int64(self.order), alphabet=np.array(chars), logp=self.logp)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(int(z["order"]), {i: str(ch) for i, ch in enumerate(z["alphabet"])}, z["logp"])

    def table(self, alpha=1.0, beta=0.0, device=None):
        """-> the decoder's table, a float32 [rows][C] device tensor: label columns alpha * logp + beta (beta: the per-character bonus that offsets
        the LM's preference for short strings), end column alpha * logp.  Uploaded once per (alpha, beta, device)."""
        import torch
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        key = (float(alpha), float(beta), str(device))
        if key not in self._dev:
            t = alpha * self.logp
            t[:, :-1] += beta
            self._dev[key] = torch.from_numpy(t.astype(np.float32)).to(device)
        return self._dev[key]


def read_word_list(path):
    """one word per line, with an optional tab-separated count -> (words, counts)"""
    words, counts = [], []
    for line in open(path):
        word, _, cnt = line.rstrip("\r\n").partition("\t")
        words.append(word); counts.append(float(cnt) if cnt.strip() else 1.0)
    return words, counts


class LMDecoder:
    """The decoder protocol of DecodeCTCPred and LexiconDecoder (`inverse_classes`, `labels_to_text`, `decode`, `decode_labels(result, device=)`):
    drops into predict.py, Model.score_generator and CTCAligner.align_decoded.  lm: a CharLM, or None for the plain beam search with N-best
    output.  Each label costs alpha * log P(label | context) + beta, the end of the word alpha * log P(end | context); the scores returned are the
    beam's log-scores plus those weights.
    alpha = 0.5 and beta = 0.0 are PLACEHOLDERS: no trained recogniser was at hand to tune them on; tune both on held-out data.
    merge_repeated defaults to False here, unlike DecodeCTCPred: TF's merge_repeated=True deletes doubled letters from the path it returns
    ('cellist' -> 'celist'), the very letters the language model was trained on and asked for."""

    def __init__(self, lm=None, alpha=0.5, beta=0.0, beam_width=10, top_paths=1, merge_repeated=False, inverse_classes=None):
        if lm is None and inverse_classes is None:
            raise ValueError("LMDecoder: without a language model, pass inverse_classes")
        if not 1 <= top_paths <= beam_width:
            raise ValueError("LMDecoder: top_paths must be 1..beam_width")
        self.lm, self.alpha, self.beta = lm, alpha, beta
        self.beam_width, self.top_paths, self.merge_repeated = beam_width, top_paths, merge_repeated
        self.inverse_classes = inverse_classes if inverse_classes is not None else lm.inverse_classes

    def labels_to_text(self, labels):
        from .decode import labels_to_text
        return labels_to_text(labels, self.inverse_classes)

    def _run(self, result, top_paths):
        """-> (labels (n, k, T), lengths (n, k), scores (n, k)) device tensors"""
        import torch
        from . import engine

        def launch(chunk):
            if self.lm is not None and chunk.shape[2] != self.lm.C:
                raise ValueError("LMDecoder: the map has %d classes, the language model %d" % (chunk.shape[2], self.lm.C))
            table = self.lm.table(self.alpha, self.beta, chunk.device) if self.lm is not None else None
            return engine.beam_decode_lm(chunk, table, self.lm.order if self.lm is not None else 1, self.beam_width, top_paths, self.merge_repeated)
        done = decode_chunks(result, launch)
        if done is None:
            z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")
            return z(0, top_paths, 0), z(0, top_paths), z(0, top_paths, dt=torch.float32)
        return done

    def decode_labels(self, result, device=False):
        """DecodeCTCPred.decode_labels' contract, the best path: (n, T, C) softmax -> (n, T) int32 labels padded with -1.  device=True: ->
        (labels, lengths) int32 DEVICE tensors, nothing copied back."""
        lab, ln, _ = self._run(result, 1)
        lab, ln = lab[:, 0].contiguous(), ln[:, 0].contiguous()
        return (lab, ln) if device else lab.cpu().numpy()

    def decode(self, result):
        return [self.labels_to_text(row) for row in self.decode_labels(result)]

    def decode_topk(self, result):
        """-> per image [(text, score), ...], the top_paths best, best first; ('', -inf) where the beam held fewer paths"""
        lab, _, sc = self._run(result, self.top_paths)
        lab, sc = lab.cpu().numpy(), sc.cpu().numpy()
        return [[(self.labels_to_text(lab[i, k]), float(sc[i, k])) for k in range(lab.shape[1])] for i in range(lab.shape[0])]
