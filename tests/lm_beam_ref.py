"""Reference (TEST INFRASTRUCTURE) of the beam search with a character language model and N-best output (csrc/beam.hip, LM = true): oracle.ctc._beam_one
-- TF r1.8's algorithm -- with a scorer.  V = C - 1 labels, blank = C - 1; table [rows][C], rows = C ** (order - 1), column V = end-of-word weight.
  * every prefix node carries ctx (root: rows - 1; child: (parent.ctx * C + label) % rows) and w = table[parent.ctx][label];
  * a re-scored entry takes nl = lse(nl, previous + w), a new child nl = inp[label] + (previous + w); -inf stays -inf; every + rounds to `dtype`;
  * after the last frame total + table[ctx][V]; the top_paths best by that sum, ties to the better rank before the addition.
Pinned by tests/test_lm_cpu.py: without a table (and with an all-zero one) it equals oracle.ctc.ctc_beam_decode exactly, and on a search small
enough to be exhaustive it equals the enumeration of all alignments.  Also the input builders of the CPU and GPU tests and their shared cases."""
import functools

import numpy as np

from oracle.ctc import _logsumexp2, EPS, NEG_INF


class _Node:
    __slots__ = ("label", "parent", "children", "ob", "ol", "ot", "nb", "nl", "nt", "ctx", "w")

    def __init__(self, label, parent, ctx, w):
        self.label = label; self.parent = parent; self.children = {}; self.ctx = ctx; self.w = w
        self.ob = self.ol = self.ot = NEG_INF
        self.nb = self.nl = self.nt = NEG_INF

    def active(self):
        return self.nt != NEG_INF


def lm_rows(C, order):
    return C ** (order - 1)


def beam_lm_one(logits, beam_width, table=None, order=1, top_paths=1, dtype=np.float32):
    """logits (T, C) = log(p + 1e-7); table (rows, C) or None (the default scorer).  -> [(path labels root->leaf, UNMERGED; score)] * top_paths,
    ([], -inf) where the leaves run out.  Arithmetic in `dtype`.
    _beam_one visits all C - 1 children of an expanding entry; a child that never entered the beam holds -inf everywhere, and being offered and
    rejected leaves it so.  Only children that exist (entered once) or whose value beats the bottom at the start of the entry's turn -- the bottom
    never falls during a step -- can change anything, so only those are visited, in label order: the same decisions, a fraction of the loop."""
    T, C = logits.shape
    blank = V = C - 1
    f = dtype
    rows = lm_rows(C, order)
    tab = None if table is None else np.asarray(table).astype(f)
    assert tab is None or tab.shape == (rows, C)
    lse = lambda a, b: f(_logsumexp2(float(a), float(b)))
    root = _Node(-1, None, rows - 1, None)
    root.nt = f(0.0); root.nb = f(0.0); root.nl = NEG_INF
    leaves = [root]
    for t in range(T):
        inp = (logits[t] - logits[t].max()).astype(f)
        branches = sorted(leaves, key=lambda n: -n.nt)  # python sort is stable
        leaves = []
        for b in branches:
            b.ob, b.ol, b.ot = b.nb, b.nl, b.nt
        for b in branches:
            if b.parent is not None:
                if b.parent.active():
                    prev = b.parent.ob if b.label == b.parent.label else b.parent.ot
                    if tab is not None and prev != NEG_INF:
                        prev = f(prev + b.w)
                    b.nl = lse(b.nl, prev)
                b.nl = f(b.nl + inp[b.label]) if b.nl != NEG_INF else NEG_INF
            b.nb = f(b.ot + inp[blank])
            b.nt = lse(b.nb, b.nl)
            leaves.append(b)

        def bottom():
            return min(leaves, key=lambda n: n.nt)

        def cand(total):
            return total > NEG_INF and (len(leaves) < beam_width or total > bottom().nt)

        for b in branches:
            if not cand(b.ot):
                continue
            prev = np.full(V, b.ot, dtype=f)
            if b.label >= 0:
                prev[b.label] = b.ob
            with np.errstate(invalid="ignore"):
                if tab is not None:
                    prev = (prev + tab[b.ctx, :V]).astype(f)          # -inf + finite = -inf
                vals = (inp[:V] + prev).astype(f)
            if len(leaves) < beam_width:
                visit = set(np.nonzero(vals > NEG_INF)[0].tolist())
            else:
                visit = set(np.nonzero(vals > bottom().nt)[0].tolist())
            visit |= set(b.children)
            for k in sorted(visit):
                c = b.children.get(k)
                if c is None:
                    c = _Node(k, b, (b.ctx * C + k) % rows, None if tab is None else tab[b.ctx, k])
                if c.active():
                    continue
                c.nb = NEG_INF
                c.nl = vals[k] if prev[k] != NEG_INF else NEG_INF
                c.nt = c.nl
                if cand(c.nt):
                    if len(leaves) == beam_width:
                        bt = bottom()
                        bt.nb = bt.nl = bt.nt = NEG_INF
                        leaves.remove(bt)
                    leaves.append(c)
                    b.children[k] = c
                else:
                    c.ob = c.ol = c.ot = NEG_INF
                    c.nb = c.nl = c.nt = NEG_INF
    ranked = sorted(leaves, key=lambda n: -n.nt)
    fin = [(n.nt if tab is None else f(n.nt + tab[n.ctx, V])) for n in ranked]
    final = sorted(range(len(ranked)), key=lambda i: -fin[i])
    out = []
    for i in final[:top_paths]:
        seq, c = [], ranked[i]
        while c.parent is not None:
            seq.append(c.label)
            c = c.parent
        out.append((seq[::-1], float(fin[i])))
    return out + [([], NEG_INF)] * (top_paths - len(out))


def merge(seq, merge_repeated):
    """merge_repeated as TF applies it: on the path's own label sequence"""
    return [k for i, k in enumerate(seq) if not merge_repeated or i == 0 or k != seq[i - 1]]


def beam_lm_decode(y_pred, beam_width=10, table=None, order=1, top_paths=1, merge_repeated=False, input_length=None, dtype=np.float32):
    """y_pred (B, T, C) softmax -> (labels (B, top_paths, T) int64 padded -1, lengths (B, top_paths), scores (B, top_paths) float64), and the
    unmerged paths [[labels] * top_paths] * B."""
    B, T, C = y_pred.shape
    out = np.full((B, top_paths, T), -1, dtype=np.int64)
    lens = np.zeros((B, top_paths), dtype=np.int64)
    scores = np.full((B, top_paths), NEG_INF, dtype=np.float64)
    raw = []
    for b in range(B):
        Tb = T if input_length is None else int(np.asarray(input_length).reshape(-1)[b])
        lg = np.log(y_pred[b, :Tb].astype(np.float32) + np.float32(EPS)).astype(dtype)
        paths = beam_lm_one(lg, beam_width, table, order, top_paths, dtype)
        raw.append([p for p, _ in paths])
        for k, (seq, sc) in enumerate(paths):
            seq = merge(seq, merge_repeated)
            out[b, k, :len(seq)] = seq; lens[b, k] = len(seq); scores[b, k] = sc
    return out, lens, scores, raw


def remerge(raw, T, merge_repeated):
    """the label / length arrays of beam_lm_decode for another merge setting, from its unmerged paths"""
    B, K = len(raw), len(raw[0])
    out = np.full((B, K, T), -1, dtype=np.int64)
    lens = np.zeros((B, K), dtype=np.int64)
    for b in range(B):
        for k in range(K):
            seq = merge(raw[b][k], merge_repeated)
            out[b, k, :len(seq)] = seq; lens[b, k] = len(seq)
    return out, lens


# ---- input builders ---------------------------------------------------------------------------------------------------------------------------
def posteriors(rs, B, T, C):
    """as tests/test_gpu_ops.py::test_beam_decode_matches_oracle: a mixture of peaked (realistic) and flat (near-ties, prefix re-entry) rows"""
    logits = rs.normal(size=(B, T, C)) * rs.choice([0.7, 2.0, 6.0], size=(B, 1, 1))
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def plant_double(y, b, label):
    """frames 0..2 of sample b read `label`, blank, `label` with 0.9 each: a doubled letter, what merge_repeated deletes (random maps hold none)"""
    C = y.shape[2]
    for t, k in enumerate((label, C - 1, label)):
        y[b, t] = 0.1 / (C - 1); y[b, t, k] = 0.9
    return y


def lm_table(rs, C, order, alpha=0.8, beta=0.5):
    p = rs.dirichlet([0.3] * C, size=lm_rows(C, order))
    return (alpha * np.log(p + 1e-6) + beta).astype(np.float32)


# ---- the plain decoder's cases: recorded by tests/golden/make_beam_bits.py, replayed by tests/test_gpu_lm.py -------------------------------------
PLAIN_B, PLAIN_T = 24, 52
PLAIN_CASES = [(C, bw, merge) for C in (38, 97) for bw in (1, 10, 64) for merge in (0, 1)]      # one and two classes per lane; the widths' three DPP paths
# the capacity edge: 4 * (1 + 251 * 64) + 64 * 16 + 64 = 65348 of the 65536 bytes of LDS, a node table far past its register copy (the LDS walk)
EDGE_C, EDGE_B, EDGE_T, EDGE_BW, EDGE_MERGE, EDGE_SEED = 38, 2, 251, 64, 1, 0


def plain_case_inputs(C, bw):
    """-> (y (PLAIN_B, PLAIN_T, C) float32 softmax, input lengths (PLAIN_B,))"""
    y = plant_double(posteriors(np.random.RandomState(C + bw), PLAIN_B, PLAIN_T, C), 5, 3)
    il = np.full(PLAIN_B, PLAIN_T); il[:4] = [1, 2, 17, 51]
    return y, il


def edge_inputs():
    """-> y (EDGE_B, EDGE_T, EDGE_C); every frame is decoded.  Seed 0: the fp32 and the fp64 run of the reference agree on both rows (no near-tie;
    tests/test_lm_cpu.py)"""
    return posteriors(np.random.RandomState(EDGE_SEED), EDGE_B, EDGE_T, EDGE_C)


# ---- the cases shared by tests/test_lm_cpu.py (numerical stability) and tests/test_gpu_lm.py (the kernel against the fp32 reference) ------------
CASE_B = 24
CASES = [(1, 66, 27), (2, 38, 52), (3, 38, 52), (2, 97, 27), (3, 12, 20)]      # (order, C, T): two classes per lane at 66 and 97; 12 ** 2 rows wrap
CASE_WIDTHS = (10, 16)
CASE_TOP = 3
NEAR_TIE_CAP = CASE_B // 8


def case_inputs(order, C, T):
    rs = np.random.RandomState(100 * order + C)
    y = plant_double(posteriors(rs, CASE_B, T, C), 5, 3)
    table = lm_table(rs, C, order)
    il = np.full(CASE_B, T); il[:4] = [1, 2, T // 3, T - 1]
    return y, table, il


@functools.lru_cache(maxsize=None)
def case_reference(order, C, T, width):
    """-> (fp32 reference: labels, lengths, scores, raw paths -- top CASE_TOP, merge_repeated False; near_tie (B,) bool: rows on which the fp32 and
    the fp64 run of the reference disagree on the top-CASE_TOP label sequences).  Computed once per process; callers must not write to it."""
    y, table, il = case_inputs(order, C, T)
    r32 = beam_lm_decode(y, width, table, order, CASE_TOP, False, il, np.float32)
    r64 = beam_lm_decode(y, width, table, order, CASE_TOP, False, il, np.float64)
    near = np.array([r32[3][b] != r64[3][b] for b in range(CASE_B)])
    return r32, near
