"""Word detection: page images -> word boxes, the table `DeviceIngest.pages`, `Readf.run_generator(bboxs=...)` and `predict.py --boxes` take.
Classical, deterministic and integer-only (Otsu's score is four float64 operations in a fixed order): a global threshold, run-length
smearing so that the letters of a word touch, 8-connected components, boxes with a size filter.  The rule is stated once in
include/crnn_mi355x.h (crnn_detect_words); `detect_words_host` is that rule in NumPy -- the package's host path -- and `WordDetector` runs
csrc/detect.hip on pages that are already on the device (the arena `DeviceIngest.upload` makes), bit for bit the same boxes.

    det = WordDetector(gap_x=8)
    boxes = det.boxes([page])                                # [[(None, r0, c0, r1, c1), ...]] in reading order
    x, _ = DeviceIngest((100, 32, 1)).pages([page], boxes)

The defaults of gap_x, gap_y and the filter are PLACEHOLDERS: no labelled page set was at hand to tune them.  gap_x must exceed the gaps
between the letters of a word and stay below the gaps between words; both scale with the resolution of the scan.

On unevenly lit pages (photographs) one threshold per page fails: `adaptive=` puts the Sauvola binarisation of crnn_mi355x/binarize.py in front
of the rule, on the host and on the device alike.

The rule assumes that the text lines run along the pixel rows; a skewed page (a photograph) goes through crnn_mi355x/deskew.py first, and
the boxes then refer to the deskewed page.

Out of scope: learned detectors, anything that would make the result depend on arrival order."""
import ctypes
import warnings

import numpy as np

from . import native
from .binarize import Binarizer, adaptive_params, sauvola_host
from .pages import MAX_DIM, PAGE_DTYPE, check_page, device_lib, header_int, upload_pages  # noqa: F401  (PAGE_DTYPE: the GPU tests' earlier versions take it from here)

MAX_GAP_X, MAX_GAP_Y = 64, 16
PARAMS = ("threshold", "polarity", "gap_x", "gap_y", "min_w", "min_h", "min_ink", "max_w", "max_h", "cap")
DEFAULTS = dict(threshold=-1, polarity=0, gap_x=8, gap_y=0, min_w=3, min_h=3, min_ink=6, max_w=0, max_h=0, cap=1024)


TILE_R, TILE_C = header_int("CRNN_DETECT_TILE_R"), header_int("CRNN_DETECT_TILE_C")   # csrc/detect.hip labels tiles of this size in LDS


class crnn_detect_params(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_detect_params."""
    _fields_ = [(n, ctypes.c_int) for n in PARAMS]


def check_params(p):
    """The ranges crnn_detect_words accepts; -> the ten integers as a dict."""
    p = {k: int(p[k]) for k in PARAMS}
    ok = (-1 <= p["threshold"] <= 254 and 0 <= p["polarity"] <= 2 and 0 <= p["gap_x"] <= MAX_GAP_X and 0 <= p["gap_y"] <= MAX_GAP_Y
          and min(p["min_w"], p["min_h"], p["min_ink"], p["max_w"], p["max_h"]) >= 0 and p["cap"] >= 1)
    if not ok:
        raise ValueError("detection parameters out of range: %r" % (p,))
    return p


def otsu_threshold(hist):
    """The first t in 0..254 with the strictly greatest between-class score, or -1 when no t splits the histogram (a constant page)."""
    h = np.asarray(hist, dtype=np.int64)
    v = np.arange(256, dtype=np.int64)
    w0, s0 = np.cumsum(h)[:255], np.cumsum(v * h)[:255]
    N, S = int(h.sum()), int((v * h).sum())
    w1 = N - w0
    ok = (w0 > 0) & (w1 > 0)
    if not ok.any():
        return -1
    d = s0 * w1 - (S - s0) * w0                                            # int64: |d| < 2^57
    a, b = np.where(ok, w0, 1).astype(np.float64), np.where(ok, w1, 1).astype(np.float64)
    score = np.where(ok, (d.astype(np.float64) / a) * (d.astype(np.float64) / b), -1.0)
    return int(np.argmax(score))                                           # argmax: the first of equal maxima


def ink_mask(page, threshold=-1, polarity=0):
    """-> (ink (rows, cols) bool, t, ink_is_dark)."""
    page = check_page(page)
    h = np.bincount(page.ravel(), minlength=256)
    t = int(threshold) if threshold >= 0 else otsu_threshold(h)
    if t < 0:
        return np.zeros(page.shape, bool), -1, int(polarity != 2)
    w0 = int(h[:t + 1].sum())
    dark = polarity == 1 or (polarity == 0 and w0 <= page.size - w0)
    return (page <= t) == dark, t, int(dark)


def smear_rows(mask, gap):
    """Run-length smearing along axis 1: a run of 1 <= L <= gap clear pixels with a set pixel immediately on both sides becomes set."""
    if gap <= 0 or not mask.any():
        return mask.copy()
    cols = mask.shape[1]
    idx = np.arange(cols, dtype=np.int64)[None, :]
    left = np.maximum.accumulate(np.where(mask, idx, -1), axis=1)          # the nearest set pixel at or left of each pixel
    right = np.minimum.accumulate(np.where(mask, idx, cols)[:, ::-1], axis=1)[:, ::-1]
    return mask | ((left >= 0) & (right < cols) & (right - left - 1 <= gap))


def smear(ink, gap_x, gap_y):
    """Horizontal smear, then the vertical one on its result."""
    return smear_rows(smear_rows(ink, gap_x).T, gap_y).T


def components(mask, ink):
    """8-connected components of `mask` -> (n, 5) int32 r0 r1 c0 c1 ink (upper bounds exclusive, `ink` counted in the second array), ordered
    by the row-major index of each component's first pixel.  Row runs united with the runs of the row above; the root is the first run."""
    rows, cols = mask.shape
    edge = np.diff(np.pad(mask, ((0, 0), (1, 1))).astype(np.int8), axis=1)
    rr, cs = np.nonzero(edge == 1)
    ce = np.nonzero(edge == -1)[1]
    n = len(rr)
    if n == 0:
        return np.zeros((0, 5), np.int32)
    acc = np.pad(np.cumsum(ink, axis=1, dtype=np.int64), ((0, 0), (1, 0)))
    run_ink = acc[rr, ce] - acc[rr, cs]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:                                              # a parent is an earlier run
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    first = np.searchsorted(rr, np.arange(rows + 1))                       # runs of row r: first[r] .. first[r + 1]
    csl, cel = cs.tolist(), ce.tolist()
    for r in range(1, rows):
        i, iend, j, jend = first[r - 1], first[r], first[r], first[r + 1]
        while i < iend and j < jend:                                       # two pointers over the runs of both rows
            if csl[i] <= cel[j] and csl[j] <= cel[i]:                      # [cs, ce) intervals that touch, diagonally included
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            if cel[i] < cel[j]:
                i += 1
            else:
                j += 1
    root = np.array([find(x) for x in range(n)], dtype=np.int64)
    ids, inv = np.unique(root, return_inverse=True)                        # ascending root = ascending first pixel
    out = np.zeros((len(ids), 5), np.int64)
    out[:, 0], out[:, 2] = rows, cols
    np.minimum.at(out[:, 0], inv, rr)
    np.maximum.at(out[:, 1], inv, rr + 1)
    np.minimum.at(out[:, 2], inv, cs)
    np.maximum.at(out[:, 3], inv, ce)
    np.add.at(out[:, 4], inv, run_ink)
    return out.astype(np.int32)


def filter_boxes(rects, min_w=0, min_h=0, min_ink=0, max_w=0, max_h=0):
    """-> the boolean mask of the rows that pass the size filter."""
    h, w = rects[:, 1] - rects[:, 0], rects[:, 3] - rects[:, 2]
    keep = (w >= min_w) & (h >= min_h) & (rects[:, 4] >= min_ink)
    if max_w > 0:
        keep &= w <= max_w
    if max_h > 0:
        keep &= h <= max_h
    return keep


def adaptive_setup(adaptive, threshold, polarity):
    """adaptive (None, True or a dict: binarize.adaptive_params) -> (the binarisation parameters or None, threshold, polarity of the detection
    that follows).  The binarised page holds 0 for ink and 255 elsewhere, so the detection on it runs with threshold 127 and dark ink;
    ValueError when `adaptive` comes with a threshold or a polarity of the caller's own (the polarity of the ink goes into `adaptive`)."""
    if adaptive is None or adaptive is False:
        return None, threshold, polarity
    if threshold != DEFAULTS["threshold"] or polarity != DEFAULTS["polarity"]:
        raise ValueError("adaptive binarisation decides what is ink: it goes with neither threshold (%r) nor polarity (%r); the ink's polarity "
                         "is adaptive['polarity']" % (threshold, polarity))
    return adaptive_params(adaptive), 127, 1


def detect_words_host(page, threshold=-1, polarity=0, gap_x=DEFAULTS["gap_x"], gap_y=DEFAULTS["gap_y"], min_w=DEFAULTS["min_w"],
                      min_h=DEFAULTS["min_h"], min_ink=DEFAULTS["min_ink"], max_w=0, max_h=0, cap=None, adaptive=None):
    """The detection rule in NumPy (the host path, and the oracle of the device kernels): -> (rects (kept, 5) int32 = r0 r1 c0 c1 ink,
    info (4,) int32 = found kept threshold ink_is_dark).  cap=None keeps every box.  gap_x, gap_y and the filter's defaults are placeholders.
    adaptive (True, or a dict of radius, k256, polarity): the page goes through binarize.sauvola_host first and the rule runs on the result
    with threshold 127 and dark ink, so `ink` counts the binarised ink pixels of a box."""
    adaptive, threshold, polarity = adaptive_setup(adaptive, threshold, polarity)
    if adaptive is not None:
        page = sauvola_host(page, **adaptive)
    p = check_params(dict(threshold=threshold, polarity=polarity, gap_x=gap_x, gap_y=gap_y, min_w=min_w, min_h=min_h, min_ink=min_ink,
                          max_w=max_w, max_h=max_h, cap=1 if cap is None else cap))
    ink, t, dark = ink_mask(page, p["threshold"], p["polarity"])
    rects = components(smear(ink, p["gap_x"], p["gap_y"]), ink)
    rects = rects[filter_boxes(rects, p["min_w"], p["min_h"], p["min_ink"], p["max_w"], p["max_h"])]
    found = len(rects)
    kept = found if cap is None else min(found, p["cap"])
    return np.ascontiguousarray(rects[:kept]), np.array([found, kept, t, dark], dtype=np.int32)


def reading_order(rects):
    """rects (n, >= 4) = r0 r1 c0 c1 -> the permutation that lists them line by line, left to right.  Boxes are visited sorted by (r0, c0);
    a box joins the first existing line whose row interval (that of the line's first box) overlaps its own by at least half of the smaller
    of the two heights, else it starts a line; lines go by r0, the boxes of a line by c0."""
    rects = np.asarray(rects)
    rects = rects.reshape(len(rects), rects.shape[-1] if rects.ndim > 1 and len(rects) else 4)
    lines = []                                                             # [r0, r1, [box, ...]]
    for k in sorted(range(len(rects)), key=lambda k: (int(rects[k, 0]), int(rects[k, 2]), k)):
        r0, r1 = int(rects[k, 0]), int(rects[k, 1])
        for line in lines:
            overlap = min(r1, line[1]) - max(r0, line[0])
            if 2 * overlap >= min(r1 - r0, line[1] - line[0]) and overlap > 0:
                line[2].append(k)
                break
        else:
            lines.append([r0, r1, [k]])
    lines.sort(key=lambda line: (line[0], line[2][0]))
    order = [k for line in lines for k in sorted(line[2], key=lambda k: (int(rects[k, 2]), k))]
    return np.array(order, dtype=np.int64)


def to_boxes(rects):
    """rects (n, >= 4) = r0 r1 c0 c1 -> [(None, r0, c0, r1, c1), ...] in reading order: page[b[1]:b[3], b[2]:b[4]] is the word."""
    return [(None, int(rects[k, 0]), int(rects[k, 2]), int(rects[k, 1]), int(rects[k, 3])) for k in reading_order(rects)]


class WordDetector:
    """detect_words_host on the device: pages go up once (pages.upload_pages, or an arena `DeviceIngest.upload` already made), one launch
    sequence finds the boxes of every page, one copy brings rects and info back.  Parameters as detect_words_host; `cap` bounds the boxes
    per page (a page with more warns once, by its index).  The defaults of gap_x, gap_y and the filter are placeholders.
    adaptive (True, or a dict of radius, k256, polarity): binarize.Binarizer makes a binarised arena on the device first and the launch
    sequence reads that one, with threshold 127 and dark ink; the arena passed in stays as it is (the crops are cut from it)."""

    def __init__(self, device=None, adaptive=None, **params):
        unknown = set(params) - set(PARAMS)
        if unknown:
            raise TypeError("unknown detection parameters: %s" % sorted(unknown))
        self.adaptive, threshold, polarity = adaptive_setup(adaptive, params.get("threshold", DEFAULTS["threshold"]),
                                                            params.get("polarity", DEFAULTS["polarity"]))
        self.params = check_params(dict(DEFAULTS, **dict(params, threshold=threshold, polarity=polarity)))
        self.lib, self.device = device_lib("WordDetector", "detect_words_host", device)
        self._prm = crnn_detect_params(**self.params)
        self._warned = False
        self._binarizer = None if self.adaptive is None else Binarizer(self.device, **self.adaptive)

    def detect(self, pages, arena=None):
        """pages: list of (H, W) uint8 arrays, or None with an `arena` that holds them -> [(rects (kept, 5) int32, info (4,) int32) per page]."""
        import torch
        from .engine import _ptr, _stream
        if arena is None:
            arena = upload_pages(pages, self.device)
        P, cap = len(arena.pages), self.params["cap"]
        if P == 0:
            return []
        if self._binarizer is not None:
            arena = self._binarizer.run(None, arena=arena)                 # a new arena on the device; the caller's is not written
        with torch.cuda.device(self.device):
            host = arena.table.ctypes.data_as(ctypes.c_void_p)
            need = self.lib.crnn_detect_workspace_bytes(host, P, ctypes.byref(self._prm))
            if need == 0:
                raise native.CrnnError("libcrnn_mi355x detect_words: a page above %d x %d, or more than 2^31 pixels in one call" % (MAX_DIM, MAX_DIM))
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            out = torch.empty(P * cap * 5 + P * 4, dtype=torch.int32, device=self.device)
            info_ptr = ctypes.c_void_p(out.data_ptr() + 4 * P * cap * 5)
            native.check(self.lib.crnn_detect_words(ctypes.c_void_p(arena.dev.data_ptr()), arena.nbytes, host, _ptr(arena.table_dev), P, ctypes.byref(self._prm),
                                                    _ptr(out), info_ptr, _ptr(ws), need, _stream()), "detect_words")
            back = out.cpu().numpy()                                       # the one read-back
        rects, info = back[:P * cap * 5].reshape(P, cap, 5), back[P * cap * 5:].reshape(P, 4)
        over = [k for k in range(P) if info[k, 0] > cap]
        if over and not self._warned:
            self._warned = True
            warnings.warn("page %d holds %d boxes, more than cap = %d: the first %d in index order were kept" % (over[0], info[over[0], 0], cap, cap))
        return [(rects[k, :info[k, 1]].copy(), info[k].copy()) for k in range(P)]

    def boxes(self, pages, arena=None):
        """-> per page [(None, r0, c0, r1, c1), ...] in reading order."""
        return [to_boxes(r) for r, _ in self.detect(pages, arena=arena)]
