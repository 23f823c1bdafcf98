"""Lexicon-constrained decoding (beyond the reference): from a word list, the word the network gives the highest CTC probability -- the standard
way to use and to evaluate a word recogniser -- and the exact CTC log-probability of any given transcription, the model's confidence in it.
Scores are log p(word | softmax map) in Keras' semantics (the negative of K.ctc_batch_cost for that label), computed by csrc/lexicon.hip for
every (image, word) pair on the device; nothing but the chosen indices and their scores comes back.

Tie rule: of words with equal scores the one earlier in the table wins, and the table is the caller's list sorted by length with a stable sort:
the shorter word, then the earlier one in the caller's list.

Shortlists: scoring every word is exact and, at 88 000 words, slow.  LexiconDecoder(shortlist=K) decodes open-vocabulary first (the beam search's
`paths` best paths), keeps per image the K words nearest in edit distance to those paths (csrc/lexicon_nearest.hip) and scores only them, exactly;
every step stays on the device.  K = 50 is a placeholder, as LMDecoder's alpha and beta are: tune it on held-out data.  The same kernel answers
"which words are nearest to this string": Lexicon.nearest."""
import warnings

import numpy as np

from .labels import CHUNK, MAX_WORD_LEN, Alphabet, device_map, label_table  # noqa: F401  (MAX_WORD_LEN: importable from here as before)

MAX_TOP_PATHS = 8            # crnn_ctc_lexicon_topk
MAX_SHORTLIST = 1024         # crnn_lexicon_nearest: K
MAX_SHORTLIST_PATHS = 8      # crnn_lexicon_nearest: P
MAX_QUERY_COLS = 1024        # crnn_lexicon_nearest: qcols
SCORE_BYTES = 256 << 20      # default budget of the scores buffer [chunk][M] fp32: the batch is scored in chunks that stay under it


class Lexicon:
    """A word list encoded with the model's alphabet.  `inverse_classes`: {id: character} (what DecodeCTCPred holds) or a list of characters.
    Words with a character outside the alphabet, or longer than 31, go to `.rejected` as (caller position, word) and are never scored; the
    constructor warns once with their count.  The empty string is a legal word.  The accepted words are sorted by length (stable) -- words that
    share a wavefront are then alike -- and uploaded once per device:
      .words[i]   text at table index i          .order[i]   the caller's position of table index i
      .labels     (N, Lmax) int32 padded with -1  .lengths    (N,) int32        .index_of[p]  table index of caller position p, -1 if rejected"""

    def __init__(self, words, inverse_classes):
        self.alphabet = Alphabet(inverse_classes)
        self.inverse_classes, self.classes = inverse_classes, self.alphabet.classes
        words = [str(w) for w in words]
        enc, pos, self.rejected = [], [], []
        for p, w in enumerate(words):
            ids = self.encode(w)
            if ids is None:
                self.rejected.append((p, w))
            else:
                enc.append(ids); pos.append(p)
        if self.rejected:
            warnings.warn("Lexicon: %d of %d words rejected (a character outside the alphabet, or longer than %d)"
                          % (len(self.rejected), len(words), MAX_WORD_LEN))
        lens = np.array([len(e) for e in enc], dtype=np.int32)
        by_len = np.argsort(lens, kind="stable")
        self.order = np.array(pos, dtype=np.int64)[by_len]
        self.words = [words[p] for p in self.order]
        self.lengths = lens[by_len]
        self.labels = np.full((len(enc), max(1, int(lens.max()) if len(enc) else 1)), -1, dtype=np.int32)
        for i, k in enumerate(by_len):
            self.labels[i, :lens[k]] = enc[k]
        self.index_of = np.full(len(words), -1, dtype=np.int64)
        self.index_of[self.order] = np.arange(len(self.order))
        self._dev = {}

    def __len__(self):
        return len(self.words)

    def encode(self, word):
        """-> list of label ids, or None when the word cannot be scored."""
        return self.alphabet.encode(word)

    def device(self, device):
        """-> (labels, lengths) int32 tensors on `device`; uploaded on first use."""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.labels).to(device), torch.from_numpy(self.lengths).to(device))
        return self._dev[key]

    @property
    def num_classes(self):
        """C of the kernels: the alphabet's ids and the blank after them"""
        return max(list(self.classes.values()) + [0]) + 2

    def nearest(self, queries, k=5, device=None):
        """The k words nearest in edit distance to every query: a list of strings (encoded with the lexicon's alphabet; one it cannot spell raises
        ValueError naming it) or label rows -- an int array or tensor (n, cols), elements outside the alphabet (-1, the blank) dropped wherever they
        stand, as the decoders' rows are read.  -> (words, distances): per query the words (at most k, fewer for a short lexicon) ordered by
        distance, then table order, and their distances."""
        import torch
        if not 1 <= k <= MAX_SHORTLIST:
            raise ValueError("k must be 1..%d" % MAX_SHORTLIST)
        device = device or torch.device("cuda", torch.cuda.current_device())
        if torch.is_tensor(queries):
            rows = queries.to(device=device, dtype=torch.int32)
        elif isinstance(queries, np.ndarray):
            rows = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.int32)).to(device)
        else:
            enc = []
            for t in queries:
                if isinstance(t, str):
                    ids = [self.classes.get(ch) for ch in t]
                    if any(i is None for i in ids):
                        raise ValueError("Lexicon.nearest: %r has a character outside the alphabet" % t)
                else:
                    ids = [int(v) for v in t]
                enc.append(ids)
            table = np.full((len(enc), max([len(e) for e in enc] + [1])), -1, dtype=np.int32)
            for i, e in enumerate(enc):
                table[i, :len(e)] = e
            rows = torch.from_numpy(table).to(device)
        if rows.dim() != 2 or not 1 <= rows.shape[1] <= MAX_QUERY_COLS:
            raise ValueError("Lexicon.nearest: expected (n, 1..%d) label rows, got shape %r" % (MAX_QUERY_COLS, tuple(rows.shape)))
        labels, lengths = self.device(device)
        idx, dist = lexicon_nearest(rows.contiguous(), labels, lengths, k, self.num_classes)
        key = torch.where(dist < 0, torch.full_like(dist, 1 << 20), dist)
        order = torch.sort(key, dim=1, stable=True)[1]            # the rows ascend by table index: a stable sort keeps that order inside a distance
        idx, dist = torch.gather(idx, 1, order).cpu().numpy(), torch.gather(dist, 1, order).cpu().numpy()
        return ([[self.words[i] for i in row if i >= 0] for row in idx], [[int(d) for d in row if d >= 0] for row in dist])


def lexicon_nearest(queries, labels, lengths, k, C):
    """queries (B, qcols) or (B, P, qcols) int32 device tensor of decoded label rows (what beam_decode_lm returns), labels (N, Lmax) / lengths (N,)
    int32 device tensors, C classes (blank = C - 1) -> (idx (B, k) int32 table indices ascending, -1 in the unused slots at the end; dist (B, k)
    int32 edit distances, -1 there): per sample the k words nearest to any of its P rows, one call of crnn_lexicon_nearest."""
    import torch
    from . import native
    from .engine import _ptr, _stream
    if queries.dim() == 2:
        queries = queries[:, None, :]
    B, P, qcols = queries.shape
    N, Lmax = labels.shape
    queries = queries.contiguous()
    idx = torch.full((B, k), -1, dtype=torch.int32, device=queries.device)
    dist = torch.full((B, k), -1, dtype=torch.int32, device=queries.device)
    if B == 0 or N == 0:
        return idx, dist
    lib = native.lib()
    ws = torch.empty(max(1, lib.crnn_lexicon_nearest_workspace_bytes(B, N) // 4), dtype=torch.int32, device=queries.device)
    with torch.cuda.device(queries.device):
        native.check(lib.crnn_lexicon_nearest(_ptr(queries), P, qcols, _ptr(labels), _ptr(lengths), _ptr(idx), _ptr(dist), _ptr(ws), ws.numel() * 4,
                                              B, C, N, Lmax, k, _stream()), "lexicon_nearest")
    return idx, dist


def lexicon_scores(y, labels, lengths, skip=0, cand=None, input_length=None):
    """y (B, T, C) float32 device tensor, labels (N, Lmax) / lengths (N,) int32 device tensors, cand (B, K) int32 device tensor or None
    -> scores (B, N) or (B, K) float32 device tensor: one pre-pass and one scoring launch (crnn_ctc_lexicon_score)."""
    import torch
    from . import native
    from .engine import _ptr, _stream
    B, T, C = y.shape
    N, Lmax = labels.shape
    M = cand.shape[1] if cand is not None else N
    lib = native.lib()
    scores = torch.full((B, M), float("-inf"), dtype=torch.float32, device=y.device)
    if B == 0 or N == 0 or M == 0:
        return scores
    ws = torch.empty(max(1, lib.crnn_ctc_lexicon_workspace_bytes(B, T, C, skip) // 4), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        native.check(lib.crnn_ctc_lexicon_score(_ptr(y), _ptr(input_length), _ptr(labels), _ptr(lengths), _ptr(cand), _ptr(scores), _ptr(ws),
                                                ws.numel() * 4, B, T, C, skip, N, Lmax, M if cand is not None else 0, _stream()), "lexicon_score")
    return scores


def lexicon_topk(scores, k, cand=None):
    """scores (B, M) -> (idx (B, k) int32, val (B, k) float32) device tensors (crnn_ctc_lexicon_topk)."""
    import torch
    from . import native
    from .engine import _ptr, _stream
    B, M = scores.shape
    idx = torch.full((B, k), -1, dtype=torch.int32, device=scores.device)
    val = torch.full((B, k), float("-inf"), dtype=torch.float32, device=scores.device)
    if B == 0 or M == 0:
        return idx, val
    with torch.cuda.device(scores.device):
        native.check(native.lib().crnn_ctc_lexicon_topk(_ptr(scores), _ptr(cand), _ptr(idx), _ptr(val), B, M, k, _stream()), "lexicon_topk")
    return idx, val


class LexiconDecoder:
    """Drop-in where a DecodeCTCPred is passed (predict.py, Model.score_generator, metrics.Score): `inverse_classes`, `labels_to_text`,
    `decode`, `decode_labels(result, device=)`.  skip: 0 scores the frames the beam decoder reads, 2 the training loss's window.
    score_bytes: budget of the scores buffer; the batch is scored in chunks of max(1, score_bytes // (4 * words)) images.
    shortlist: None scores every word of the list against every image.  K (1..1024): per image only the K words nearest in edit distance to the
    `paths` (1..8) best paths of a beam search of width `beam_width` over the same frames are scored -- beam_decode_lm, lexicon_nearest,
    lexicon_scores and lexicon_topk back to back on the device.  The result equals the exhaustive one wherever the exhaustive best word is in
    the image's shortlist (always when K >= len(lexicon)).  An explicit `candidates=` argument wins over the shortlist."""

    def __init__(self, lexicon, top_paths=1, skip=0, score_bytes=SCORE_BYTES, shortlist=None, paths=1, beam_width=10):
        if not 1 <= top_paths <= MAX_TOP_PATHS:
            raise ValueError("top_paths must be 1..%d" % MAX_TOP_PATHS)
        if shortlist is not None:
            if not 1 <= shortlist <= MAX_SHORTLIST:
                raise ValueError("shortlist must be 1..%d" % MAX_SHORTLIST)
            if not 1 <= paths <= MAX_SHORTLIST_PATHS or paths > beam_width:
                raise ValueError("paths must be 1..%d and at most beam_width" % MAX_SHORTLIST_PATHS)
        self.shortlist, self.paths, self.beam_width = shortlist, paths, beam_width
        self.lexicon = lexicon
        self.top_paths = top_paths
        self.skip = skip
        self.score_bytes = score_bytes
        self.inverse_classes = lexicon.inverse_classes

    def labels_to_text(self, labels):
        from .decode import labels_to_text
        return labels_to_text(labels, self.inverse_classes)

    # ---- device side ----
    def _candidates(self, candidates, n):
        """list of lists of caller positions, or an int array padded with -1 -> (n, K) int32 ndarray of table indices (-1 = empty / rejected),
        every row in ascending table order with the empty slots last: neighbours in a row are then alike in length, as the table's are, and
        the tie rule of the dense mode holds -- the lower position is the shorter word, then the earlier one in the caller's list."""
        if isinstance(candidates, np.ndarray):
            c = candidates.astype(np.int64)
        else:
            K = max([len(r) for r in candidates] + [1])
            c = np.full((len(candidates), K), -1, dtype=np.int64)
            for i, r in enumerate(candidates):
                c[i, :len(r)] = r
        if c.ndim != 2 or c.shape[0] != n:
            raise ValueError("candidates: expected %d rows, got shape %r" % (n, c.shape))
        inside = (c >= 0) & (c < len(self.lexicon.index_of))
        out = np.full(c.shape, -1, dtype=np.int32)
        out[inside] = self.lexicon.index_of[c[inside]]
        key = np.where(out < 0, np.iinfo(np.int32).max, out)
        return np.take_along_axis(out, np.argsort(key, axis=1, kind="stable"), 1)

    def _shortlist(self, y, labels, lengths, K):
        """y (B, T, C) device map -> (B, K) int32 device tensor: per image the table indices of the K words nearest to its beam paths, ascending"""
        from .engine import beam_decode_lm
        paths, _, _ = beam_decode_lm(y[:, self.skip:], None, beam_width=self.beam_width, top_paths=self.paths, merge_repeated=False)
        return lexicon_nearest(paths, labels, lengths, K, y.shape[2])[0]

    def _topk(self, result, candidates, k):
        """-> (idx (n, k) int32 table indices or -1, val (n, k) float32), device tensors."""
        import torch
        n = len(result)
        cand = self._candidates(candidates, n) if candidates is not None else None
        device = result.device if torch.is_tensor(result) and result.is_cuda else torch.device("cuda", torch.cuda.current_device())
        labels, lengths = self.lexicon.device(device)
        short = min(self.shortlist, max(len(self.lexicon), 1)) if cand is None and self.shortlist is not None else None
        M = cand.shape[1] if cand is not None else short or len(self.lexicon)
        rows = max(1, min(CHUNK, self.score_bytes // (4 * max(M, 1))))
        idx, val = [], []
        for lo in range(0, n, rows):
            chunk = device_map(result[lo:lo + rows], device)
            cd = torch.from_numpy(np.ascontiguousarray(cand[lo:lo + rows])).to(device) if cand is not None else None
            if short:
                cd = self._shortlist(chunk, labels, lengths, short)
            i, v = lexicon_topk(lexicon_scores(chunk, labels, lengths, self.skip, cd), k, cd)
            idx.append(i); val.append(v)
        if not idx:
            return torch.zeros((0, k), dtype=torch.int32, device=device), torch.zeros((0, k), dtype=torch.float32, device=device)
        return (idx[0], val[0]) if len(idx) == 1 else (torch.cat(idx, 0), torch.cat(val, 0))

    # ---- the decoder surface ----
    def decode_topk(self, result, candidates=None):
        """-> (words, log_probs): per image the top_paths best words (best first, '' where no word has a finite score) and their CTC
        log-probabilities, an (n, top_paths) float32 ndarray (-inf in the empty slots)."""
        idx, val = self._topk(result, candidates, self.top_paths)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        return [[self.lexicon.words[i] if i >= 0 else "" for i in row] for row in idx], val

    def decode(self, result, candidates=None):
        """-> the best word per image; an image with no finite score decodes to ''."""
        idx, _ = self._topk(result, candidates, 1)
        return [self.lexicon.words[i] if i >= 0 else "" for i in idx[:, 0].cpu().numpy()]

    def decode_labels(self, result, device=False):
        """DecodeCTCPred.decode_labels' contract: (n, T, C) softmax -> (n, Lmax) int32 label rows of the best word padded with -1 (all -1 where
        no word has a finite score).  device=True: -> (labels, lengths) int32 DEVICE tensors, nothing copied back."""
        import torch
        idx, _ = self._topk(result, None, 1)
        labels, lengths = self.lexicon.device(idx.device)
        n, width = idx.shape[0], self.lexicon.labels.shape[1]
        if len(self.lexicon) == 0:
            rows = torch.full((n, width), -1, dtype=torch.int32, device=idx.device)
            lens = torch.zeros(n, dtype=torch.int32, device=idx.device)
        else:
            best = idx[:, 0].long()
            none = best < 0
            best = best.clamp(min=0)
            rows = torch.where(none[:, None], torch.full_like(labels[:1], -1), labels[best])
            lens = torch.where(none, torch.zeros_like(lengths[:1]), lengths[best])
        return (rows, lens) if device else rows.cpu().numpy()

    def log_prob(self, result, texts):
        """The exact CTC log-probability of one given transcription per image (one candidate per image, the same kernel): the confidence of
        a beam result.  -> (n,) float32 ndarray; -inf for a text the alphabet cannot spell, one longer than 31, or one the frames cannot hold."""
        import torch
        y = device_map(result)
        n = y.shape[0]
        if len(texts) != n:
            raise ValueError("log_prob: %d texts for %d images" % (len(texts), n))
        table, lens = label_table([self.lexicon.encode(str(t)) for t in texts])
        cand = torch.arange(n, dtype=torch.int32, device=y.device).reshape(n, 1)
        scores = lexicon_scores(y, torch.from_numpy(table).to(y.device), torch.from_numpy(lens).to(y.device), self.skip, cand)
        return scores[:, 0].cpu().numpy()
