"""Training augmentation of word images: warp (rotation, slant, scale, shift), stroke width (grey dilation / erosion), blur, tone and noise
on the uint8 batch (B, T0, T1) that the ingest writes (axis 0 = time, ink bright).  The scheme is the input side's: the host draws every
random decision (`AugmentPolicy.draw` -> one crnn_augment_item per image) and the kernel applies them.  The rule is stated once in
include/crnn_mi355x.h (crnn_augment_batch) and is integer-only; `augment_host` is that rule in NumPy -- the package's host path and the
oracle of the kernel -- and `Augmenter` runs csrc/augment.hip on a batch that is already on the device, bit for bit the same bytes.

    policy = AugmentPolicy(seed=1, p=0.5)
    gen = DeviceReadf(img_size=(100, 32, 1), normed=True, batch_size=64, classes=classes, augment=policy).run_generator(names)
    x = Augmenter((100, 32, 1)).run(u8_dev, policy.draw(len(u8_dev), (100, 32, 1)))       # device fp32 (B, 100, 32, 1)

The default ranges of AugmentPolicy are PLACEHOLDERS, as every detection default here: no trained recogniser or labelled set was at hand
to tune them."""
import ctypes
import math

import numpy as np

from . import native
from .hashing import mix32                                 # the noise stage's hash (shared with synth.py)

FIELDS = ("a00", "a01", "a10", "a11", "t0", "t1", "fill", "morph", "blur", "gain", "bias", "noise")
MAX_COEF, MAX_MORPH, MAX_BLUR, MAX_GAIN, MAX_BIAS, MAX_NOISE = 262144, 2, 2, 1024, 255, 64
MAX_PIXELS = 16384                                         # imgh * imgw of crnn_augment_batch: two 16 KiB LDS buffers


class crnn_augment_item(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_augment_item."""
    _fields_ = [(n, ctypes.c_int) for n in FIELDS] + [("seed", ctypes.c_uint)]


ITEM_DTYPE = np.dtype([(n, np.intc) for n in FIELDS] + [("seed", np.uintc)], align=True)
assert ITEM_DTYPE.itemsize == ctypes.sizeof(crnn_augment_item)


def neutral_items(n):
    """n items that change nothing: the identity warp, every other stage off."""
    t = np.zeros(int(n), ITEM_DTYPE)
    t["a00"] = t["a11"] = 65536
    t["fill"], t["gain"] = -1, 256
    return t


def check_items(items, img_size):
    """The ranges crnn_augment_batch accepts -> the items as an ITEM_DTYPE array; ValueError otherwise."""
    items = np.asarray(items)
    if items.dtype != ITEM_DTYPE or items.ndim != 1:
        raise ValueError("items are a 1-d array of augment.ITEM_DTYPE, not %s %s" % (items.dtype, items.shape))
    T0, T1 = int(img_size[0]), int(img_size[1])
    a = lambda name: np.abs(items[name].astype(np.int64))
    ok = (all((a(k) <= MAX_COEF).all() for k in ("a00", "a01", "a10", "a11")) and (a("t0") <= T0 << 17).all() and (a("t1") <= T1 << 17).all()
          and ((items["fill"] >= -1) & (items["fill"] <= 255)).all() and (a("morph") <= MAX_MORPH).all()
          and ((items["blur"] >= 0) & (items["blur"] <= MAX_BLUR)).all() and ((items["gain"] >= 0) & (items["gain"] <= MAX_GAIN)).all()
          and (a("bias") <= MAX_BIAS).all() and ((items["noise"] >= 0) & (items["noise"] <= MAX_NOISE)).all())
    if not ok:
        raise ValueError("augment item out of range (|a..| <= %d, |t0| <= T0 << 17, |t1| <= T1 << 17, fill -1..255, morph -%d..%d, blur 0..%d, "
                         "gain 0..%d, bias -%d..%d, noise 0..%d)" % (MAX_COEF, MAX_MORPH, MAX_MORPH, MAX_BLUR, MAX_GAIN, MAX_BIAS, MAX_BIAS, MAX_NOISE))
    return items


def _warp(v, it):
    T0, T1 = v.shape
    di = (2 * np.arange(T0, dtype=np.int64) - (T0 - 1))[:, None]
    dj = (2 * np.arange(T1, dtype=np.int64) - (T1 - 1))[None, :]
    Y = int(it["a00"]) * di + int(it["a01"]) * dj + int(it["t0"]) + ((T0 - 1) << 16)
    X = int(it["a10"]) * di + int(it["a11"]) * dj + int(it["t1"]) + ((T1 - 1) << 16)
    i0, j0, fy, fx = Y >> 17, X >> 17, (Y >> 9) & 255, (X >> 9) & 255          # int64 >> is arithmetic: the floor
    fill = int(it["fill"])

    def tap(i, j):
        p = v[np.clip(i, 0, T0 - 1), np.clip(j, 0, T1 - 1)]
        if fill < 0:
            return p
        return np.where((i >= 0) & (i < T0) & (j >= 0) & (j < T1), p, fill)
    return ((256 - fy) * (256 - fx) * tap(i0, j0) + (256 - fy) * fx * tap(i0, j0 + 1) + fy * (256 - fx) * tap(i0 + 1, j0)
            + fy * fx * tap(i0 + 1, j0 + 1) + 32768) >> 16


def _window(v, r, pick):
    """max or min over the (2r + 1)^2 window clipped to the image: over the shifts of the edge-replicated image, which repeat window pixels only."""
    T0, T1 = v.shape
    pad = np.pad(v, r, mode="edge")
    out = v
    for a in range(2 * r + 1):
        for b in range(2 * r + 1):
            out = pick(out, pad[a:a + T0, b:b + T1])
    return out


def _blur(v):
    p = np.pad(v, ((0, 0), (1, 1)), mode="edge")
    h = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    q = np.pad(h, ((1, 1), (0, 0)), mode="edge")
    return (q[:-2] + 2 * q[1:-1] + q[2:] + 8) >> 4


def augment_host(u8, items, table=None):
    """The rule of crnn_augment_batch in NumPy (the host path, and the oracle of the device kernel): u8 (n, T0, T1) uint8 and n items -> the
    augmented (n, T0, T1) uint8, or with `table` (256 fp32, ingest.norm_table) the fp32 table[v] of it."""
    u8 = np.asarray(u8)
    if u8.ndim != 3 or u8.dtype != np.uint8 or u8.shape[1] < 1 or u8.shape[2] < 1:
        raise ValueError("a batch is a (n, T0, T1) uint8 array, not %s %s" % (u8.dtype, u8.shape))
    items = check_items(items, u8.shape[1:])
    if len(items) != len(u8):
        raise ValueError("%d items for %d images" % (len(items), len(u8)))
    T0, T1 = u8.shape[1:]
    out = np.empty(u8.shape, np.uint8)
    offs = (np.arange(T0 * T1, dtype=np.uint64).reshape(T0, T1) * np.uint64(0x9E3779B9)) & np.uint64(0xffffffff)
    for b, it in enumerate(items):
        v = u8[b].astype(np.int64)
        if (int(it["a00"]), int(it["a01"]), int(it["a10"]), int(it["a11"]), int(it["t0"]), int(it["t1"])) != (65536, 0, 0, 65536, 0, 0):
            v = _warp(v, it)
        if it["morph"]:
            v = _window(v, abs(int(it["morph"])), np.maximum if it["morph"] > 0 else np.minimum)
        for _ in range(int(it["blur"])):
            v = _blur(v)
        if it["gain"] != 256 or it["bias"]:
            v = np.clip(((v - 128) * int(it["gain"]) + (128 + int(it["bias"])) * 256 + 128) >> 8, 0, 255)
        if it["noise"]:
            h = mix32(np.uint64(int(it["seed"])) ^ offs)
            s = ((h & np.uint64(255)) + ((h >> np.uint64(8)) & np.uint64(255)) + ((h >> np.uint64(16)) & np.uint64(255))
                 + (h >> np.uint64(24))).astype(np.int64) - 510
            v = np.clip(v + ((s * int(it["noise"])) >> 8), 0, 255)
        out[b] = v
    return out if table is None else np.asarray(table, np.float32)[out]


class AugmentPolicy:
    """The random decisions of the augmentation, drawn on the host: .draw(n, img_size) -> n crnn_augment_item (ITEM_DTYPE).

    The warp, the tone and the noise are each switched on per image with probability `p`, the stroke-width stage with `morph_p` and the blur
    with `blur_p` (None: p / 2); a stage that is on draws its parameters uniformly:
      rotate   degrees, the rotation is in [-rotate, rotate]
      slant    the shift along the text per pixel across it is in [-slant, slant]
      scale    (lo, hi): the factor along each axis, drawn for each on its own
      shift    (along, across) pixels: the shift along each axis is in [-shift, shift]
      fill     what the warp reads outside the image: 0..255, or -1 for the nearest pixel
      morph    radius 1, dilation or erosion; blur: 1 or 2 passes
      gain     (lo, hi) contrast about 128; bias (lo, hi) grey levels; noise (lo, hi) in 1/256 of the +-510 noise sum
    The matrix is composed in float64 and rounded to 16.16 integers here; only the integers are consumed afterwards, so float arithmetic
    never decides a pixel.  The policy owns a np.random.RandomState(seed) and never touches the global np.random stream (ingest.plan_crop's).
    The number of draws per call depends on n alone.  Every default range is a PLACEHOLDER: nothing was at hand to tune them."""

    def __init__(self, seed=0, p=0.5, rotate=3.0, slant=0.25, scale=(0.9, 1.1), shift=(3.0, 1.5), fill=-1, morph_p=None, blur_p=None,
                 gain=(0.75, 1.3), bias=(-20, 20), noise=(8, 32)):
        self.seed, self.p = int(seed), float(p)
        self.morph_p = self.p / 2 if morph_p is None else float(morph_p)
        self.blur_p = self.p / 2 if blur_p is None else float(blur_p)
        self.rotate, self.slant, self.scale, self.shift, self.fill = float(rotate), float(slant), tuple(scale), tuple(shift), int(fill)
        self.gain, self.bias, self.noise = tuple(gain), tuple(bias), tuple(noise)
        if not (0. <= self.p <= 1. and 0. <= self.morph_p <= 1. and 0. <= self.blur_p <= 1. and 0 < self.scale[0] <= self.scale[1]
                and -1 <= self.fill <= 255):
            raise ValueError("augment policy: probabilities in 0..1, 0 < scale[0] <= scale[1], fill -1..255")
        self.rs = np.random.RandomState(self.seed)

    def draw(self, n, img_size):
        n, T0, T1 = int(n), int(img_size[0]), int(img_size[1])
        rs = self.rs
        on = rs.uniform(size=(n, 5)) < np.array([self.p, self.morph_p, self.blur_p, self.p, self.p])
        u = rs.uniform(size=(n, 11))
        seeds = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
        span = lambda col, lo, hi: lo + (hi - lo) * u[:, col]
        t = neutral_items(n)
        t["fill"] = self.fill
        theta = np.radians(span(0, -self.rotate, self.rotate))
        sl, k0, k1 = span(1, -self.slant, self.slant), span(2, *self.scale), span(3, *self.scale)
        c, s = np.cos(theta), np.sin(theta)
        # source = R(theta) . [[1, slant], [0, 1]] . diag(1 / k0, 1 / k1) . (destination - centre) + shift + centre
        m = np.stack([c / k0, (c * sl - s) / k1, s / k0, (s * sl + c) / k1], axis=1)
        coef = np.clip(np.rint(m * 65536.0), -MAX_COEF, MAX_COEF).astype(np.int64)
        sh0 = np.clip(np.rint(span(4, -self.shift[0], self.shift[0]) * 131072.0), -(T0 << 17), T0 << 17).astype(np.int64)
        sh1 = np.clip(np.rint(span(5, -self.shift[1], self.shift[1]) * 131072.0), -(T1 << 17), T1 << 17).astype(np.int64)
        warp = on[:, 0]
        for k, name in enumerate(("a00", "a01", "a10", "a11")):
            t[name] = np.where(warp, coef[:, k], t[name])
        t["t0"], t["t1"] = np.where(warp, sh0, 0), np.where(warp, sh1, 0)
        t["morph"] = np.where(on[:, 1], np.where(u[:, 6] < 0.5, -1, 1), 0)
        t["blur"] = np.where(on[:, 2], np.where(u[:, 7] < 0.5, 1, 2), 0)
        t["gain"] = np.where(on[:, 3], np.clip(np.rint(span(8, *self.gain) * 256.0), 0, MAX_GAIN), 256)
        t["bias"] = np.where(on[:, 3], np.clip(np.rint(span(9, *self.bias)), -MAX_BIAS, MAX_BIAS), 0)
        t["noise"] = np.where(on[:, 4], np.clip(np.rint(span(10, *self.noise)), 0, MAX_NOISE), 0)
        t["seed"] = np.where(on[:, 4], seeds, 0)
        return check_items(t, img_size)


class Augmenter:
    """augment_host on the device.  .run(u8_dev, items, batch=None, return_u8=False): u8_dev the device uint8 (B, T0, T1) batch as
    DeviceIngest.crops(..., return_u8=True) returns it, items the n <= B items of its first rows -> device fp32 (batch or B, T0, T1, 1) =
    table[augmented pixel], rows past n zero [, the augmented uint8 batch].  One launch on the current stream; the items travel through
    two page-locked staging slots (pages.StagingSlots, as the ingest's box table does) and nothing is read back."""

    def __init__(self, img_size, normed=True, mean=118.24236953981779, std=36.72835353999682, device=None):
        import torch
        from .ingest import norm_table
        from .pages import StagingSlots, device_lib
        self.lib, self.device = device_lib("Augmenter", "augment.augment_host", device)
        self.img_size = tuple(img_size)
        self.T0, self.T1 = int(img_size[0]), int(img_size[1])
        self.table = torch.from_numpy(norm_table(normed, mean, std)).to(self.device)
        self._staging = StagingSlots(self.device, floor=1 << 16)

    def run(self, u8_dev, items, batch=None, return_u8=False):
        import torch
        from .engine import _ptr, _stream
        items = check_items(items, self.img_size)
        n = len(items)
        B = int(u8_dev.shape[0]) if batch is None else int(batch)
        if (u8_dev.dtype != torch.uint8 or not u8_dev.is_contiguous() or u8_dev.device != self.device or u8_dev.dim() < 3
                or tuple(u8_dev.shape[1:3]) != (self.T0, self.T1) or u8_dev.numel() != u8_dev.shape[0] * self.T0 * self.T1):
            raise ValueError("the batch is a contiguous uint8 (B, %d, %d) tensor on %s" % (self.T0, self.T1, self.device))
        if B < 1 or n > B or B > u8_dev.shape[0]:
            raise ValueError("%d items and a batch of %d do not fit the %d images given" % (n, B, u8_dev.shape[0]))
        nbytes = n * ITEM_DTYPE.itemsize
        with torch.cuda.device(self.device):
            s = self._staging.take(max(nbytes, 1))
            s["np"][:nbytes].view(ITEM_DTYPE)[:] = items
            if nbytes:
                s["dev"][:nbytes].copy_(s["host"][:nbytes], non_blocking=True)
                s["copied"].record(torch.cuda.current_stream())
            out = torch.empty((B, self.T0, self.T1, 1), dtype=torch.float32, device=self.device)
            o8 = torch.empty((B, self.T0, self.T1), dtype=torch.uint8, device=self.device) if return_u8 else None
            native.check(self.lib.crnn_augment_batch(_ptr(u8_dev), ctypes.c_void_p(s["host"].data_ptr()), ctypes.c_void_p(s["dev"].data_ptr()), n, B,
                                                     self.T0, self.T1, _ptr(self.table), _ptr(out), _ptr(o8), _stream()), "augment_batch")
        return (out, o8) if return_u8 else out
