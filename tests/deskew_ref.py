"""Helpers of the deskew tests (tests/test_deskew_cpu.py, tests/test_gpu_deskew.py): a brute-force restatement of the two rules of
include/crnn_mi355x.h (crnn_deskew_estimate, crnn_rotate_pages) written independently of crnn_mi355x.deskew -- one pixel at a time in Python
integers -- and the constructed page: 4 lines of 7 words drawn at a slope, flat or under binarize_ref.shaded_page's brightness gradient."""
import math

import numpy as np

SKEW_SHAPE = (300, 640)
SKEW_BLOCK = (18, 8)                                         # rows x columns of one "letter"
SLOPES = (0.0, 0.011, 0.02, 0.07, -0.07, 0.15, -0.12, 0.1875, -0.1875)
INDICES = (0, 3, 5, 18, -18, 38, -31, 48, -48)               # the nearest k / 256 of each slope
UNREADABLE = (-0.07, 0.15, -0.12, 0.1875, -0.1875)           # slopes at which the raw page's reading order is not the drawn one


def ink_brute(page, threshold, polarity):
    """The detector's ink for a GIVEN threshold 0..254 and polarity (Otsu is the detector's own rule and is not restated here)."""
    rows, cols = page.shape
    below = [[int(page[r, c]) <= threshold for c in range(cols)] for r in range(rows)]
    w0 = sum(sum(row) for row in below)
    dark = polarity == 1 or (polarity == 0 and w0 <= rows * cols - w0)
    return [[b == dark for b in row] for row in below]


def scores_brute(ink, steps, slope_step):
    """ink: rows of booleans -> the 2 steps + 1 scores as Python integers."""
    rows, cols = len(ink), len(ink[0])
    out = []
    for a in range(-steps, steps + 1):
        s, prof = a * slope_step, {}
        for r in range(rows):
            for c in range(cols):
                if ink[r][c]:
                    b = r - (((c - (cols >> 1)) * s + 32768) >> 16)        # Python's >> on a negative integer is the floor
                    prof[b] = prof.get(b, 0) + 1
        score = sum(v * v for v in prof.values())
        assert score < 1 << 37
        out.append(score)
    return out


def pick_brute(scores):
    """The greatest score; among equal ones the smallest |a|, then the negative a."""
    steps = (len(scores) - 1) // 2
    best = None
    for a in sorted(range(-steps, steps + 1), key=lambda a: (abs(a), a)):  # 0, -1, 1, -2, 2, ...: the first of the greatest wins
        if best is None or scores[a + steps] > scores[best + steps]:
            best = a
    return best


def rotate_brute(page, index, slope_step, fill):
    rows, cols = page.shape
    s = index * slope_step
    t = s / 65536.0
    C, S = round(65536.0 / math.sqrt(1.0 + t * t)), round(65536.0 * t / math.sqrt(1.0 + t * t))
    out = np.zeros((rows, cols), np.uint8)

    def tap(r, c):
        if 0 <= r < rows and 0 <= c < cols:
            return int(page[r, c])
        return int(page[min(max(r, 0), rows - 1), min(max(c, 0), cols - 1)]) if fill < 0 else fill
    for r in range(rows):
        for c in range(cols):
            dr, dc = 2 * r - (rows - 1), 2 * c - (cols - 1)
            X, Y = C * dc - S * dr + ((cols - 1) << 16), S * dc + C * dr + ((rows - 1) << 16)
            assert abs(X) < 1 << 31 and abs(Y) < 1 << 31
            c0, r0, fx, fy = X >> 17, Y >> 17, (X >> 9) & 255, (Y >> 9) & 255
            v = ((256 - fx) * (256 - fy) * tap(r0, c0) + fx * (256 - fy) * tap(r0, c0 + 1) + (256 - fx) * fy * tap(r0 + 1, c0)
                 + fx * fy * tap(r0 + 1, c0 + 1) + 32768) >> 16
            out[r, c] = v
    return out


def random_grey(rows, cols, seed):
    return np.random.RandomState(seed).randint(0, 256, (rows, cols)).astype(np.uint8)


def sparse_ink(rows, cols, seed, density=0.2, dark=True):
    """Light paper (200..255) with dark pixels (0..60) at `density`, or the complement: Otsu and a threshold of 127 both split it."""
    rs = np.random.RandomState(seed)
    page = np.where(rs.random_sample((rows, cols)) < density, rs.randint(0, 61, (rows, cols)), rs.randint(200, 256, (rows, cols))).astype(np.uint8)
    return page if dark else (255 - page).astype(np.uint8)


_CACHE = {}


def skewed_page(slope, shaded, seed=0):
    """-> (page (300, 640) uint8, rects (28, 4) int32 = r0 r1 c0 c1 of the words as drawn BEFORE the skew, line by line).  Line l starts at
    row 51 + 60 l, word w at column 52 + 80 w; a word is five 18 x 8 blocks 12 columns apart.  A pixel is ink when its centre, rotated back
    by atan(slope) about ((rows - 1) / 2, (cols - 1) / 2), lies in a block (half-open intervals from -0.5).  Flat paper of 220 with ink of
    0.45 of it, or binarize_ref.shaded_page's gradient 250 -> 70; rounded normal noise of sigma 3 on top.  Results are cached: do not write
    into them."""
    key = (float(slope), bool(shaded), seed)
    if key in _CACHE:
        return _CACHE[key]
    rows, cols = SKEW_SHAPE
    bh, bw = SKEW_BLOCK
    th = math.atan(slope)
    cs, sn = math.cos(th), math.sin(th)
    r, c = np.indices((rows, cols)).astype(np.float64)
    dr, dc = r - (rows - 1) / 2.0, c - (cols - 1) / 2.0
    # a line of text drawn along row y0 appears at r = y0 + slope (c - centre): the page's rows rise with the columns at `slope`
    y = (rows - 1) / 2.0 + cs * dr - sn * dc
    x = (cols - 1) / 2.0 + sn * dr + cs * dc
    ink = np.zeros((rows, cols), bool)
    rects = []
    for line in range(4):
        r0 = 51 + 60 * line
        for w in range(7):
            c0 = 52 + 80 * w
            for b in range(5):
                ink |= (y >= r0 - 0.5) & (y < r0 + bh - 0.5) & (x >= c0 + 12 * b - 0.5) & (x < c0 + 12 * b + bw - 0.5)
            rects.append((r0, r0 + bh, c0, c0 + 4 * 12 + bw))
    bg = np.rint(np.linspace(250.0, 70.0, cols))[None, :].repeat(rows, 0) if shaded else np.full((rows, cols), 220.0)
    page = np.where(ink, np.rint(0.45 * bg), bg)
    page = page + np.rint(np.random.RandomState(seed).normal(0.0, 3.0, (rows, cols)))
    _CACHE[key] = np.clip(page, 0, 255).astype(np.uint8), np.array(rects, np.int32)
    return _CACHE[key]
