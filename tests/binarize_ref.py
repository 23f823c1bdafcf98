"""Helpers of the binarisation tests (tests/test_binarize_cpu.py, tests/test_gpu_binarize.py): a brute-force restatement of the rule of
include/crnn_mi355x.h (crnn_binarize_pages) written independently of crnn_mi355x.binarize.sauvola_host -- a loop per pixel over the clipped
window with Python ints and math.isqrt -- and the constructed pages: random ones, the two extremes of the arithmetic, and the shaded page that
one global threshold cannot split."""
import math

import numpy as np

EXTREME = dict(radius=31, k256=255)                          # the largest D and the largest products of the comparison
SHADED_SHAPE = (240, 640)
SHADED_BLOCK = (18, 8)                                       # rows x columns of one "letter"
SHADED_RADII = (7, 15, 31)


def sauvola_brute(page, radius, k256, polarity):
    """The rule read off the header, one pixel at a time, in Python integers of unbounded size."""
    rows, cols = page.shape
    v = [[int(x) if polarity == 1 else 255 - int(x) for x in row] for row in page]
    out = np.full((rows, cols), 255, np.uint8)
    for i in range(rows):
        ra, rb = max(0, i - radius), min(rows - 1, i + radius)
        for j in range(cols):
            ca, cb = max(0, j - radius), min(cols - 1, j + radius)
            n = S = Q = 0
            for y in range(ra, rb + 1):
                w = v[y][ca:cb + 1]
                n += len(w)
                S += sum(w)
                Q += sum(x * x for x in w)
            D = n * Q - S * S
            assert 0 <= D < 1 << 40
            lhs, rhs = v[i][j] * n * n * 32768, S * n * 128 * (256 - k256) + S * k256 * math.isqrt(D)
            assert max(lhs, rhs) < 1 << 49
            if lhs < rhs:
                out[i, j] = 0
    return out


def random_grey(rows, cols, seed):
    """Every grey value, with a few flat patches so that windows of zero variance occur."""
    rs = np.random.RandomState(seed)
    page = rs.randint(0, 256, (rows, cols)).astype(np.uint8)
    if rows > 8 and cols > 8:
        page[2:7, 3:8] = 200
        page[rows - 6:, cols - 7:] = 0
    return page


def checkerboard(rows, cols):
    i, j = np.indices((rows, cols))
    return np.where((i + j) & 1, 255, 0).astype(np.uint8)


def half_page(rows, cols):
    page = np.full((rows, cols), 255, np.uint8)
    page[:, :cols // 2] = 0
    return page


def one_dark_pixel(rows, cols, at):
    page = np.full((rows, cols), 255, np.uint8)
    page[at] = 0
    return page


def shaded_page(seed=0):
    """-> (page (240, 640) uint8, rects (32, 4) int32 = r0 r1 c0 c1 in row-major order of their first pixel).  The background falls linearly
    from 250 at the left edge to 70 at the right one; 4 lines of 8 words, a word five 18 x 8 blocks four columns apart, every block 0.45 times
    the background of its column; integer noise (a normal of sigma 3, rounded) from a seeded generator on top of everything."""
    rows, cols = SHADED_SHAPE
    bh, bw = SHADED_BLOCK
    bg = np.rint(np.linspace(250.0, 70.0, cols))[None, :].repeat(rows, 0)
    ink = np.zeros((rows, cols), bool)
    rects = []
    for line in range(4):
        r0 = 21 + 60 * line
        for w in range(8):
            c0 = 12 + 80 * w
            for b in range(5):
                ink[r0:r0 + bh, c0 + 12 * b:c0 + 12 * b + bw] = True
            rects.append((r0, r0 + bh, c0, c0 + 4 * 12 + bw))
    page = np.where(ink, np.rint(0.45 * bg), bg)
    page = page + np.rint(np.random.RandomState(seed).normal(0.0, 3.0, (rows, cols)))
    return np.clip(page, 0, 255).astype(np.uint8), np.array(rects, np.int32)
