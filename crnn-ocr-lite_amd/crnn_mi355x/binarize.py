"""Adaptive (Sauvola) binarisation of page images, the step in front of word detection on unevenly lit pages (photographs): a pixel is ink
when it lies below the local mean, lowered by the local contrast, of the (2 r + 1)^2 window around it -- v < m (1 + k (sigma / R - 1)) with
R = 128 -- evaluated in integers only.  The rule is stated once in include/crnn_mi355x.h (crnn_binarize_pages); `sauvola_host` is that rule in
NumPy -- the package's host path and the oracle of the kernel -- and `Binarizer` runs csrc/binarize.hip on pages that are already on the
device, bit for bit the same bytes.  The result holds 0 for ink and 255 otherwise, whatever the polarity: detection on it is the plain rule
with threshold 127 and dark ink (detect.WordDetector(adaptive=...), detect.detect_words_host(adaptive=...)).

    det = WordDetector(gap_x=8, adaptive=dict(radius=15))
    boxes = det.boxes(None, arena=ing.upload(pages))         # the crops are then cut from the grey arena, not from the binarised one

The defaults radius = 15, k256 = 51 (k about 0.2) are PLACEHOLDERS, as every other detection default here: no labelled page set was at hand
to tune them.  The radius should exceed the stroke width, so that no window lies inside the ink."""
import ctypes

import numpy as np

from . import native
from .pages import check_page, device_lib, header_int, upload_pages

MAX_RADIUS, RANGE = 31, 128
PARAMS = ("radius", "k256", "polarity")
DEFAULTS = dict(radius=15, k256=51, polarity=1)              # placeholders: tune them on labelled pages
STRIP_C, BAND_R = header_int("CRNN_BINARIZE_STRIP_C"), header_int("CRNN_BINARIZE_BAND_R")   # csrc/binarize.hip: a workgroup's columns and rows


class crnn_binarize_params(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_binarize_params."""
    _fields_ = [(n, ctypes.c_int) for n in PARAMS]


def check_params(radius=DEFAULTS["radius"], k256=DEFAULTS["k256"], polarity=DEFAULTS["polarity"], k=None):
    """The ranges crnn_binarize_pages accepts -> the three integers as a dict.  k: Sauvola's k as a float, mapped to k256 = round(k * 256)
    (the integer is the definition); it takes the place of k256."""
    if k is not None:
        if k256 != DEFAULTS["k256"]:
            raise ValueError("k and k256 name the same parameter: give one of them")
        k256 = round(float(k) * 256)
    try:
        p = dict(radius=int(radius), k256=int(k256), polarity=int(polarity))
        ok = p["radius"] == radius and p["k256"] == k256 and p["polarity"] == polarity
    except (TypeError, ValueError):
        ok = False
    if not ok or not (1 <= p["radius"] <= MAX_RADIUS and 0 <= p["k256"] <= 255 and p["polarity"] in (1, 2)):
        raise ValueError("binarisation parameters out of range (radius 1..%d, k256 0..255, polarity 1 or 2): radius=%r k256=%r polarity=%r"
                         % (MAX_RADIUS, radius, k256, polarity))
    return p


def adaptive_params(adaptive):
    """The `adaptive` argument of the detectors -> check_params' dict: True for the defaults, or a dict of radius / k256 (or k) / polarity."""
    if adaptive is True:
        return check_params()
    if not isinstance(adaptive, dict):
        raise ValueError("adaptive is True or a dict of radius, k256 (or k) and polarity, not %r" % (adaptive,))
    unknown = set(adaptive) - set(PARAMS) - {"k"}
    if unknown:
        raise ValueError("unknown binarisation parameters: %s" % sorted(unknown))
    return check_params(**adaptive)


def _isqrt(D):
    """floor(sqrt(D)) of a non-negative int64 array below 2^52: the float64 root, truncated and corrected, so exact whatever sqrt rounds to."""
    s = np.sqrt(D.astype(np.float64)).astype(np.int64)
    while True:
        over = s * s > D
        if not over.any():
            break
        s[over] -= 1
    while True:
        under = (s + 1) * (s + 1) <= D
        if not under.any():
            break
        s[under] += 1
    return s


def sauvola_host(page, radius=DEFAULTS["radius"], k256=DEFAULTS["k256"], polarity=DEFAULTS["polarity"], k=None):
    """The binarisation rule in NumPy (the host path, and the oracle of the device kernel): (H, W) uint8 -> (H, W) uint8, 0 where the pixel
    is ink and 255 elsewhere.  Summed-area tables in int64, windows clipped to the page, the exact integer square root, one int64
    comparison.  radius and k256 default to placeholders."""
    p = check_params(radius, k256, polarity, k)
    page = check_page(page)
    r, kk = p["radius"], p["k256"]
    rows, cols = page.shape
    v = page.astype(np.int64) if p["polarity"] == 1 else 255 - page.astype(np.int64)
    sat1 = np.pad(v.cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    sat2 = np.pad((v * v).cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    i, j = np.arange(rows)[:, None], np.arange(cols)[None, :]
    r0, r1 = np.maximum(i - r, 0), np.minimum(i + r + 1, rows)                 # the clipped window: rows r0 .. r1 - 1, columns c0 .. c1 - 1
    c0, c1 = np.maximum(j - r, 0), np.minimum(j + r + 1, cols)
    S = sat1[r1, c1] - sat1[r0, c1] - sat1[r1, c0] + sat1[r0, c0]
    Q = sat2[r1, c1] - sat2[r0, c1] - sat2[r1, c0] + sat2[r0, c0]
    n = (r1 - r0) * (c1 - c0)
    sd = _isqrt(n * Q - S * S)
    ink = v * n * n * (RANGE * 256) < S * n * RANGE * (256 - kk) + S * kk * sd     # both sides below 2^49
    return np.where(ink, 0, 255).astype(np.uint8)


class Binarizer:
    """sauvola_host on the device: .run(pages) or .run(None, arena=a) -> a NEW PageArena on the device that holds the binarised pages at the
    offsets and with the shapes of the input arena (its alignment bytes between pages are zero).  The input arena is left as it is; nothing is
    read back and no host copy of the result is made (`host` of the returned arena is None).  radius and k256 default to placeholders."""

    def __init__(self, device=None, radius=DEFAULTS["radius"], k256=DEFAULTS["k256"], polarity=DEFAULTS["polarity"], k=None):
        self.params = check_params(radius, k256, polarity, k)
        self.lib, self.device = device_lib("Binarizer", "sauvola_host", device)
        self._prm = crnn_binarize_params(**self.params)

    def run(self, pages, arena=None):
        import torch
        from .engine import _ptr, _stream
        if arena is None:
            arena = upload_pages(pages, self.device)
        with torch.cuda.device(self.device):
            out = arena.blank()
            P = len(arena.pages)
            if P:
                native.check(self.lib.crnn_binarize_pages(ctypes.c_void_p(arena.dev.data_ptr()), arena.nbytes, arena.table.ctypes.data_as(ctypes.c_void_p),
                                                          _ptr(arena.table_dev), P, ctypes.byref(self._prm), _ptr(out.dev), arena.nbytes, _stream()),
                             "binarize_pages")
        return out
