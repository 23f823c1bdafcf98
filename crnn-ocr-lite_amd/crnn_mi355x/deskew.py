"""Page deskew, the step in front of word detection on pages whose text lines do not run along the pixel rows (photographs): the skew is
estimated with sheared projection profiles and the page is resampled with fixed-point bilinear weights, in integers only.  The rules are
stated once in include/crnn_mi355x.h (crnn_deskew_estimate, crnn_rotate_pages); `estimate_skew_host` and `rotate_host` are those rules in
NumPy -- the package's host path and the oracle of the kernels -- and `Deskewer` runs csrc/deskew.hip on pages that are already on the device,
bit for bit the same scores, indices and bytes.

    arena = ing.upload(pages)
    flat = Deskewer(adaptive=True).run(None, arena=arena)     # a second arena of the same layout; nothing is read back
    boxes = det.boxes(None, arena=flat)                       # the unchanged detector and ingest read the deskewed arena
    x = ing.crops(None, index, rects, ing.plan(rects), arena=flat)

The boxes refer to the DESKEWED page, not to the photograph that went in; mapping them back is out of scope.

A candidate is a slope a * slope_step / 65536 for a in -steps .. steps.  The defaults steps = 48, slope_step = 256 (slopes k / 256, 0.22
degrees apart, up to +-10.6 degrees) and fill = -1 (samples outside the page repeat its edge) are PLACEHOLDERS, as every other detection
default here: no labelled page set was at hand to tune them."""
import ctypes
import math

import numpy as np

from . import native
from .binarize import Binarizer, sauvola_host
from .detect import DEFAULTS as DETECT_DEFAULTS, adaptive_setup, ink_mask
from .pages import MAX_DIM, check_page, device_lib, header_int, upload_pages

MAX_STEPS, MAX_SLOPE_STEP, MAX_SLOPE = 64, 1024, 16384       # steps * slope_step <= 16384: a slope of at most 0.25
PARAMS = ("threshold", "polarity", "steps", "slope_step", "fill")
DEFAULTS = dict(threshold=DETECT_DEFAULTS["threshold"], polarity=DETECT_DEFAULTS["polarity"], steps=48, slope_step=256, fill=-1)   # placeholders
STRIPS, BAND_R = header_int("CRNN_DESKEW_STRIPS"), header_int("CRNN_DESKEW_BAND_R")   # csrc/deskew.hip: a workgroup's 64-column strips and rows


class crnn_deskew_params(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_deskew_params."""
    _fields_ = [(n, ctypes.c_int) for n in PARAMS]


def check_params(threshold=DEFAULTS["threshold"], polarity=DEFAULTS["polarity"], steps=DEFAULTS["steps"], slope_step=DEFAULTS["slope_step"],
                 fill=DEFAULTS["fill"]):
    """The ranges crnn_deskew_estimate and crnn_rotate_pages accept -> the five integers as a dict."""
    given = dict(threshold=threshold, polarity=polarity, steps=steps, slope_step=slope_step, fill=fill)
    try:
        p = {k: int(v) for k, v in given.items()}
        ok = all(p[k] == given[k] for k in PARAMS)
    except (TypeError, ValueError):
        ok = False
    if not ok or not (-1 <= p["threshold"] <= 254 and 0 <= p["polarity"] <= 2 and 0 <= p["steps"] <= MAX_STEPS
                      and 1 <= p["slope_step"] <= MAX_SLOPE_STEP and p["steps"] * p["slope_step"] <= MAX_SLOPE and -1 <= p["fill"] <= 255):
        raise ValueError("deskew parameters out of range (threshold -1..254, polarity 0..2, steps 0..%d, slope_step 1..%d, steps * slope_step "
                         "<= %d, fill -1..255): %r" % (MAX_STEPS, MAX_SLOPE_STEP, MAX_SLOPE, given))
    return p


def slope_of(index, slope_step=DEFAULTS["slope_step"]):
    """The slope (rows per column) of candidate `index`."""
    return int(index) * int(slope_step) / 65536.0


def angle_of(index, slope_step=DEFAULTS["slope_step"]):
    """The angle of candidate `index` in degrees."""
    return math.degrees(math.atan(slope_of(index, slope_step)))


def rotation_pair(index, slope_step=DEFAULTS["slope_step"]):
    """-> (C, S) = 65536 (cos, sin) of atan(slope), each rounded to the nearest integer, in IEEE double."""
    s = int(index) * int(slope_step)
    t = s / 65536.0
    root = math.sqrt(1.0 + t * t)
    return int(np.rint(65536.0 / root)), int(np.rint(float(s) / root))


def _estimate_input(page, threshold, polarity, adaptive):
    """-> (the page the estimate reads, threshold, polarity): the Sauvola-binarised page with threshold 127 and dark ink under `adaptive`."""
    adaptive, threshold, polarity = adaptive_setup(adaptive, threshold, polarity)
    if adaptive is not None:
        page = sauvola_host(page, **adaptive)
    return page, threshold, polarity


def skew_scores_host(page, threshold=DEFAULTS["threshold"], polarity=DEFAULTS["polarity"], steps=DEFAULTS["steps"],
                     slope_step=DEFAULTS["slope_step"], adaptive=None):
    """The estimate's scores in NumPy: (2 steps + 1,) int64, score[a + steps] = sum_b P_a[b]^2 of the sheared row profile of the page's ink
    (detect.ink_mask at the same threshold / polarity)."""
    page, threshold, polarity = _estimate_input(check_page(page), threshold, polarity, adaptive)
    p = check_params(threshold, polarity, steps, slope_step)
    ink, _, _ = ink_mask(page, p["threshold"], p["polarity"])
    rows, cols = page.shape
    rr, cc = np.nonzero(ink)
    rr, dc = rr.astype(np.int64), cc.astype(np.int64) - (cols >> 1)
    pad = ((((cols >> 1) + 1) * MAX_SLOPE) >> 16) + 2
    scores = np.zeros(2 * p["steps"] + 1, np.int64)
    for a in range(-p["steps"], p["steps"] + 1):
        off = (dc * (a * p["slope_step"]) + 32768) >> 16                   # int64 >> is arithmetic: the floor
        prof = np.bincount(rr - off + pad, minlength=rows + 2 * pad).astype(np.int64)
        scores[a + p["steps"]] = int((prof * prof).sum())
    return scores


def pick_index(scores):
    """The candidate of the greatest score; among equal scores the smallest |a|, then the negative one."""
    scores = np.asarray(scores, np.int64)
    steps = (len(scores) - 1) // 2
    return max(range(-steps, steps + 1), key=lambda a: (int(scores[a + steps]), -abs(a), -a))


def estimate_skew_host(page, threshold=DEFAULTS["threshold"], polarity=DEFAULTS["polarity"], steps=DEFAULTS["steps"],
                       slope_step=DEFAULTS["slope_step"], adaptive=None):
    """The estimate in NumPy (the host path, and the oracle of the device kernels) -> (index, scores (2 steps + 1,) int64)."""
    scores = skew_scores_host(page, threshold, polarity, steps, slope_step, adaptive)
    return pick_index(scores), scores


def rotate_host(page, index, slope_step=DEFAULTS["slope_step"], fill=DEFAULTS["fill"]):
    """The rotation in NumPy (the host path, and the oracle of the device kernel): the page resampled about its centre by atan(index *
    slope_step / 65536), fixed-point bilinear weights of 8 bits; a sample outside the page is `fill`, or the nearest page pixel for
    fill = -1.  Index 0 returns the page's bytes."""
    page = check_page(page)
    p = check_params(steps=0, slope_step=slope_step, fill=fill)
    if int(index) != index or abs(int(index)) * p["slope_step"] > MAX_SLOPE:
        raise ValueError("index * slope_step is an integer of at most %d in magnitude, not %r * %r" % (MAX_SLOPE, index, slope_step))
    C, S = rotation_pair(index, p["slope_step"])
    rows, cols = page.shape
    dr = (2 * np.arange(rows, dtype=np.int64) - (rows - 1))[:, None]
    dc = (2 * np.arange(cols, dtype=np.int64) - (cols - 1))[None, :]
    X = C * dc - S * dr + ((cols - 1) << 16)
    Y = S * dc + C * dr + ((rows - 1) << 16)
    c0, r0, fx, fy = X >> 17, Y >> 17, (X >> 9) & 255, (Y >> 9) & 255
    src = page.astype(np.int64)

    def tap(r, c):
        v = src[np.clip(r, 0, rows - 1), np.clip(c, 0, cols - 1)]
        if p["fill"] < 0:
            return v
        return np.where((r >= 0) & (r < rows) & (c >= 0) & (c < cols), v, p["fill"])
    out = ((256 - fx) * (256 - fy) * tap(r0, c0) + fx * (256 - fy) * tap(r0, c0 + 1) + (256 - fx) * fy * tap(r0 + 1, c0)
           + fx * fy * tap(r0 + 1, c0 + 1) + 32768) >> 16
    return out.astype(np.uint8)


def deskew_host(page, threshold=DEFAULTS["threshold"], polarity=DEFAULTS["polarity"], steps=DEFAULTS["steps"],
                slope_step=DEFAULTS["slope_step"], fill=DEFAULTS["fill"], adaptive=None):
    """estimate_skew_host, then rotate_host of the GREY page by its answer -> (the deskewed page, index).  Boxes found on the result refer to
    the deskewed page.  adaptive (True, or the dict detect.adaptive_setup takes): the estimate reads the Sauvola-binarised page with threshold
    127 and dark ink; it goes with neither threshold nor polarity."""
    check_params(threshold, polarity, steps, slope_step, fill)
    index, _ = estimate_skew_host(page, threshold, polarity, steps, slope_step, adaptive)
    return rotate_host(page, index, slope_step, fill), index


class Deskewer:
    """deskew_host on the device.  .estimate(pages) or .estimate(None, arena=a) -> [(index, scores (2 steps + 1,) int64) per page], one
    read-back.  .run(pages) or .run(None, arena=a) -> a NEW PageArena on the device that holds the deskewed pages at the offsets and with the
    shapes of the input arena (`host` is None), with the device tensor of the pages' indices as `.index`; nothing is read back and the input
    arena is left as it is.  Boxes found in the result refer to the deskewed pages.  adaptive (True, or the dict detect.adaptive_setup takes):
    the estimate runs on a binarize.Binarizer arena with threshold 127 and dark ink, and goes with neither threshold nor polarity; what is
    rotated is always the grey arena.  steps, slope_step and fill default to placeholders."""

    def __init__(self, device=None, adaptive=None, **params):
        unknown = set(params) - set(PARAMS)
        if unknown:
            raise TypeError("unknown deskew parameters: %s" % sorted(unknown))
        self.adaptive, threshold, polarity = adaptive_setup(adaptive, params.get("threshold", DEFAULTS["threshold"]),
                                                            params.get("polarity", DEFAULTS["polarity"]))
        self.params = check_params(**dict(DEFAULTS, **dict(params, threshold=threshold, polarity=polarity)))
        self.lib, self.device = device_lib("Deskewer", "deskew_host", device)
        self._prm = crnn_deskew_params(**self.params)
        self._binarizer = None if self.adaptive is None else Binarizer(self.device, **self.adaptive)

    def _estimate(self, arena):
        """-> the P int64 score rows, then the P int32 indices, in one device tensor."""
        import torch
        from .engine import _ptr, _stream
        P, n = len(arena.pages), 2 * self.params["steps"] + 1
        source = arena if self._binarizer is None else self._binarizer.run(None, arena=arena)   # a new arena; the caller's is not written
        host = arena.table.ctypes.data_as(ctypes.c_void_p)
        need = self.lib.crnn_deskew_workspace_bytes(host, P, ctypes.byref(self._prm))
        if need == 0:
            raise native.CrnnError("libcrnn_mi355x deskew_estimate: a page above %d x %d, or too many pages in one call" % (MAX_DIM, MAX_DIM))
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty(P * n * 8 + P * 4, dtype=torch.uint8, device=self.device)
        index_ptr = ctypes.c_void_p(out.data_ptr() + P * n * 8)
        native.check(self.lib.crnn_deskew_estimate(ctypes.c_void_p(source.dev.data_ptr()), source.nbytes, host, _ptr(arena.table_dev), P,
                                                   ctypes.byref(self._prm), index_ptr, _ptr(out), _ptr(ws), need, _stream()), "deskew_estimate")
        return out

    def estimate(self, pages, arena=None):
        import torch
        if arena is None:
            arena = upload_pages(pages, self.device)
        P, n = len(arena.pages), 2 * self.params["steps"] + 1
        if P == 0:
            return []
        with torch.cuda.device(self.device):
            back = self._estimate(arena).cpu().numpy()                     # the one read-back
        scores, index = back[:P * n * 8].view(np.int64).reshape(P, n), back[P * n * 8:].view(np.int32)
        return [(int(index[k]), scores[k].copy()) for k in range(P)]

    def run(self, pages, arena=None):
        import torch
        from .engine import _ptr, _stream
        if arena is None:
            arena = upload_pages(pages, self.device)
        P, n = len(arena.pages), 2 * self.params["steps"] + 1
        with torch.cuda.device(self.device):
            flat = arena.blank()
            flat.index = torch.zeros(P, dtype=torch.int32, device=self.device)
            if P:
                flat.index = self._estimate(arena)[P * n * 8:].view(torch.int32)
                native.check(self.lib.crnn_rotate_pages(ctypes.c_void_p(arena.dev.data_ptr()), arena.nbytes, arena.table.ctypes.data_as(ctypes.c_void_p),
                                                        _ptr(arena.table_dev), P, _ptr(flat.index), ctypes.byref(self._prm), _ptr(flat.dev),
                                                        arena.nbytes, _stream()), "rotate_pages")
        return flat
