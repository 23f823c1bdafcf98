"""Helpers of the word-detection tests (tests/test_detect_cpu.py, tests/test_gpu_detect.py): an independent labelling of a smeared mask with
scipy, and the constructed pages -- random ones, chains that cross tile borders, corners, smears across a border, isolated pixels."""
import os

import numpy as np

from crnn_mi355x import detect as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_page.npz")
INK, PAPER = 30, 220                                        # dark ink on light paper: threshold 127, polarity 1
GAPS = [(0, 0), (1, 0), (3, 2), (64, 16)]
DENSITIES = [0.02, 0.3, 0.5, 0.7]
PLAIN = dict(threshold=127, polarity=1, gap_x=0, gap_y=0, min_w=0, min_h=0, min_ink=0, max_w=0, max_h=0)   # every component is a box


def fixture():
    """-> (page uint8, boxes (11, 4) int32 = r0 r1 c0 c1 in reading order) of scripts/make_detect_fixture.py."""
    z = np.load(GOLDEN)
    return z["page"], z["boxes"]


def scipy_boxes(mask, ink):
    """8-connected components of `mask` by scipy.ndimage -> (n, 5) int32 r0 r1 c0 c1 ink, ordered by each component's first pixel (scipy
    numbers components in that order: it scans row-major)."""
    from scipy import ndimage
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    out = np.zeros((n, 5), np.int32)
    firsts = []
    for k, sl in enumerate(ndimage.find_objects(lab)):
        out[k] = (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop, int((ink & (lab == k + 1)).sum()))
        firsts.append(int(np.flatnonzero((lab == k + 1).ravel())[0]))
    return out[np.argsort(firsts, kind="stable")]


def from_mask(mask):
    """bool mask -> page with dark ink where the mask is set."""
    return np.where(mask, INK, PAPER).astype(np.uint8)


def random_page(rows, cols, density, seed):
    """Ink with probability `density`; two narrow bands of grey values either side of 127, so that Otsu splits between them and sees the
    ink the fixed threshold sees."""
    rs = np.random.RandomState(seed)
    ink = rs.rand(rows, cols) < density
    return np.where(ink, rs.randint(20, 41, (rows, cols)), rs.randint(210, 231, (rows, cols))).astype(np.uint8)


def snake(rows, cols, step=3):
    """A one-pixel line that runs along every `step`-th row, alternately left to right and right to left, joined at the ends: one component
    that crosses every vertical tile border once per pass and every horizontal one once."""
    m = np.zeros((rows, cols), bool)
    right = True
    for r in range(0, rows, step):
        m[r, :] = True
        if r + step < rows:
            m[r:r + step, cols - 1 if right else 0] = True
        right = not right
    return m


def comb(rows, cols, spacing=2, spine=True):
    """Vertical teeth every `spacing` columns over the whole height; with `spine` they join in the last row only."""
    m = np.zeros((rows, cols), bool)
    m[:rows - 1, ::spacing] = True
    if spine:
        m[rows - 1, :] = True
    return m


def dots(rows, cols, at):
    m = np.zeros((rows, cols), bool)
    for r, c in at:
        m[r, c] = True
    return m


def check_against_scipy(page, **params):
    """detect_words_host with no filter and no cap against scipy's labelling of the same smeared mask."""
    p = dict(PLAIN, **params)
    rects, info = D.detect_words_host(page, **p)
    ink, t, dark = D.ink_mask(page, p["threshold"], p["polarity"])
    want = scipy_boxes(D.smear(ink, p["gap_x"], p["gap_y"]), ink)
    assert np.array_equal(rects, want), "boxes differ from scipy's at %r" % (p,)
    assert info.tolist() == [len(want), len(want), t, dark]
    return rects
