"""Synthetic training words: word images rendered from a glyph atlas and a word list, as the uint8 batch (B, T0, T1) the ingest writes (axis 0 =
time, ink bright) -- a data source that needs no image files, no decoding and no host work per pixel.  The scheme is the input side's: the host
draws every random decision (`SynthPolicy.draw` -> one crnn_synth_item per image) and one launch places the pixels.  The rule is stated once in
include/crnn_mi355x.h (crnn_synth_words) and is integer-only; `synth_host` is that rule in NumPy -- the package's host path and the oracle of
the kernel -- and `WordSynth` runs csrc/synth.hip, bit for bit the same bytes.

    atlas = GlyphAtlas.from_fonts(["DejaVuSans.ttf"], 28, get_lexicon())          # or GlyphAtlas.load("atlas.npz")
    gen = SynthReadf(words, atlas, img_size=(100, 32, 1), batch_size=64, classes=classes, max_len=23, policy=SynthPolicy(seed=1)).run_generator()
    x = WordSynth(atlas, (100, 32, 1)).run(codes, policy.draw(codes, lens, atlas, (100, 32, 1)))      # device fp32 (n, 100, 32, 1)

The default ranges of SynthPolicy are PLACEHOLDERS, as every default of the input side here: no trained recogniser or labelled set was at hand
to tune them."""
import ctypes

import numpy as np

from . import native
from .data import Readf, norm
from .hashing import mix32

MAX_DIM, MAX_ADVANCE, MAX_LEN = 64, 128, 64                # w, h, top + h, |left| of a glyph; its advance; glyphs per word
MIN_TRACK, MAX_TRACK, MAX_JITTER = -8, 32, 8
MIN_SCALE, MAX_SCALE, MAX_OFFSET = 16384, 262144, 1 << 28
MAX_PIXELS = 16384                                         # imgh * imgw: crnn_augment_batch's limit, so the two launches compose
GLYPH_FIELDS = ("w", "h", "left", "top", "advance")
ITEM_FIELDS = ("face", "len", "track", "jitter", "sx", "sy", "ox", "oy", "fg", "bg")


class crnn_glyph(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_glyph."""
    _fields_ = [("off", ctypes.c_long)] + [(n, ctypes.c_int) for n in GLYPH_FIELDS]


class crnn_synth_item(ctypes.Structure):
    """include/crnn_mi355x.h: crnn_synth_item."""
    _fields_ = [(n, ctypes.c_int) for n in ITEM_FIELDS] + [("seed", ctypes.c_uint)]


GLYPH_DTYPE = np.dtype([("off", np.dtype("l"))] + [(n, np.intc) for n in GLYPH_FIELDS], align=True)
ITEM_DTYPE = np.dtype([(n, np.intc) for n in ITEM_FIELDS] + [("seed", np.uintc)], align=True)
assert GLYPH_DTYPE.itemsize == ctypes.sizeof(crnn_glyph)
assert ITEM_DTYPE.itemsize == ctypes.sizeof(crnn_synth_item)


def check_glyphs(table, arena_bytes):
    """The glyph tables crnn_synth_words accepts -> the table as a (nfaces, nglyphs) GLYPH_DTYPE array; ValueError otherwise."""
    table = np.asarray(table)
    if table.dtype != GLYPH_DTYPE or table.ndim != 2 or table.shape[0] < 1 or table.shape[1] < 1 or int(arena_bytes) < 1:
        raise ValueError("a glyph table is a non-empty (nfaces, nglyphs) array of synth.GLYPH_DTYPE over a non-empty arena, not %s %s"
                         % (table.dtype, table.shape))
    g = {k: table[k].astype(np.int64) for k in GLYPH_DTYPE.names}
    ok = ((g["w"] >= 0) & (g["h"] >= 0) & (g["w"] <= MAX_DIM) & (g["h"] <= MAX_DIM) & ((g["w"] == 0) == (g["h"] == 0)) & (g["top"] >= 0)
          & (g["top"] + g["h"] <= MAX_DIM) & (np.abs(g["left"]) <= MAX_DIM) & (g["advance"] >= 0) & (g["advance"] <= MAX_ADVANCE)
          & ((g["w"] == 0) | ((g["off"] >= 0) & (g["off"] <= int(arena_bytes) - g["w"] * g["h"]))))
    if not ok.all():
        raise ValueError("glyph out of range (0 <= w, h <= %d, both or neither 0, 0 <= top, top + h <= %d, |left| <= %d, 0 <= advance <= %d, "
                         "the bitmap inside the arena)" % (MAX_DIM, MAX_DIM, MAX_DIM, MAX_ADVANCE))
    return table


def check_items(items, codes, nfaces, nglyphs):
    """The ranges crnn_synth_words accepts -> (items as an ITEM_DTYPE array, codes as a contiguous (n, Lmax) intc array); ValueError otherwise.
    The kernel adds no limit of its own, so there is none here."""
    items = np.asarray(items)
    if items.dtype != ITEM_DTYPE or items.ndim != 1:
        raise ValueError("items are a 1-d array of synth.ITEM_DTYPE, not %s %s" % (items.dtype, items.shape))
    codes = np.ascontiguousarray(codes, dtype=np.intc)
    if codes.ndim != 2 or len(codes) != len(items) or not 1 <= codes.shape[1] <= MAX_LEN:
        raise ValueError("codes are (%d, Lmax) integers with 1 <= Lmax <= %d, not %s" % (len(items), MAX_LEN, codes.shape))
    within = lambda name, lo, hi: ((items[name] >= lo) & (items[name] <= hi)).all()
    inside = np.arange(codes.shape[1])[None, :] < items["len"][:, None]
    ok = (within("face", 0, int(nfaces) - 1) and within("len", 0, codes.shape[1]) and within("track", MIN_TRACK, MAX_TRACK)
          and within("jitter", 0, MAX_JITTER) and within("sx", MIN_SCALE, MAX_SCALE) and within("sy", MIN_SCALE, MAX_SCALE)
          and within("ox", -MAX_OFFSET, MAX_OFFSET) and within("oy", -MAX_OFFSET, MAX_OFFSET) and within("fg", 0, 255) and within("bg", 0, 255)
          and not (inside & ((codes < 0) | (codes >= int(nglyphs)))).any())
    if not ok:
        raise ValueError("synth item out of range (0 <= face < %d, 0 <= len <= %d, track %d..%d, jitter 0..%d, sx and sy %d..%d, |ox|, |oy| <= %d, "
                         "fg and bg 0..255, the codes inside len in [0, %d))" % (nfaces, codes.shape[1], MIN_TRACK, MAX_TRACK, MAX_JITTER, MIN_SCALE,
                                                                                 MAX_SCALE, MAX_OFFSET, nglyphs))
    return items, codes


def identity_items(n, length=0):
    """n items that read the line as it is: face 0, scale 1, no offset, no tracking, no jitter, white ink on black."""
    t = np.zeros(int(n), ITEM_DTYPE)
    t["sx"] = t["sy"] = 65536
    t["len"], t["fg"] = length, 255
    return t


class GlyphAtlas:
    """The glyph atlas of include/crnn_mi355x.h: `arena` (uint8 coverage bitmaps back to back) and `table` ((nfaces, nglyphs) GLYPH_DTYPE), glyph
    g of every face drawing class g.  One upload per device, cached (`on_device`)."""

    def __init__(self, arena, table):
        self.arena = np.ascontiguousarray(arena, dtype=np.uint8)
        self.table = np.ascontiguousarray(check_glyphs(table, self.arena.size))
        self.nfaces, self.nglyphs = self.table.shape
        self._dev = {}

    @classmethod
    def from_arrays(cls, faces):
        """faces: per face a list of (bitmap (h, w) uint8 or None, left, top, advance), one per class."""
        if not faces or any(len(f) != len(faces[0]) for f in faces) or not faces[0]:
            raise ValueError("an atlas has at least one face, and every face has the same non-zero number of glyphs")
        table = np.zeros((len(faces), len(faces[0])), GLYPH_DTYPE)
        chunks, pos = [], 0
        for f, face in enumerate(faces):
            for g, (bitmap, left, top, advance) in enumerate(face):
                bitmap = np.zeros((0, 0), np.uint8) if bitmap is None else np.asarray(bitmap)
                if bitmap.size and (bitmap.ndim != 2 or bitmap.dtype != np.uint8):
                    raise ValueError("a glyph bitmap is a (h, w) uint8 array, not %s %s" % (bitmap.dtype, bitmap.shape))
                h, w = bitmap.shape if bitmap.size else (0, 0)
                table[f, g] = (pos if bitmap.size else 0, w, h, left, top, advance)
                if bitmap.size:
                    chunks.append(bitmap.ravel())
                    pos += bitmap.size
        arena = np.concatenate(chunks + [np.zeros(-pos % 16 or (0 if pos else 16), np.uint8)])      # never empty
        return cls(arena, table)

    @classmethod
    def from_fonts(cls, paths, size, alphabet):
        """Each glyph of `alphabet` rasterised once per font file with PIL (ImageFont.truetype(path, size)); ImportError without PIL, OSError for a
        font file that cannot be read, ValueError for a size whose glyphs pass the atlas's limits."""
        try:
            from PIL import Image, ImageDraw, ImageFont
        except ImportError as e:
            raise ImportError("GlyphAtlas.from_fonts needs PIL (Pillow) to rasterise the glyphs; GlyphAtlas.load reads a saved atlas without it") from e
        faces = []
        for path in paths:
            try:
                font = ImageFont.truetype(path, int(size))
            except OSError as e:
                raise OSError("cannot read the font file %r: %s" % (path, e)) from e
            pad = 2 * int(size) + 8
            glyphs = []
            for ch in alphabet:
                img = Image.new("L", (3 * pad, 3 * pad), 0)
                ImageDraw.Draw(img).text((pad, pad), ch, fill=255, font=font, anchor="la")      # pen at x = pad, the ascender at y = pad
                a = np.array(img)
                rows, cols = np.flatnonzero(a.any(axis=1)), np.flatnonzero(a.any(axis=0))
                advance = int(round(font.getlength(ch)))
                if len(rows) == 0:
                    glyphs.append((None, 0, 0, advance))
                else:
                    glyphs.append((a[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].copy(), int(cols[0]) - pad, int(rows[0]) - pad, advance))
            rise = max([0] + [-g[2] for g in glyphs if g[0] is not None])              # ink above the ascender: the line box begins there
            faces.append([(g[0], g[1], g[2] + rise if g[0] is not None else 0, g[3]) for g in glyphs])
        return cls.from_arrays(faces)

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, arena=self.arena, off=self.table["off"].astype(np.int64), **{k: self.table[k].astype(np.int32) for k in GLYPH_FIELDS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            table = np.zeros(z["off"].shape, GLYPH_DTYPE)
            for k in GLYPH_DTYPE.names:
                table[k] = z[k]
            return cls(z["arena"], table)

    def line_height(self, face):
        """Rows of the face's line box: the lowest ink row of any glyph, at least 1."""
        t = self.table[int(face)]
        return max(1, int((t["top"] + t["h"]).max()))

    def bitmap(self, face, g):
        t = self.table[int(face), int(g)]
        return self.arena[int(t["off"]):int(t["off"]) + int(t["w"]) * int(t["h"])].reshape(int(t["h"]), int(t["w"]))

    def on_device(self, device):
        """-> (arena, table) as uint8 tensors on `device`, uploaded on first use."""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.arena).to(device), torch.from_numpy(self.table.reshape(-1).view(np.uint8).copy()).to(device))
        return self._dev[key]


def _layout(atlas, codes, items):
    """Per image and glyph slot (n, Lmax) int64: ink (inside len and with a bitmap), x of the bitmap's first column, w, y of its first row, h, off."""
    n, L = codes.shape
    k = np.arange(L, dtype=np.int64)[None, :]
    inside = k < items["len"].astype(np.int64)[:, None]
    g = atlas.table[items["face"].astype(np.int64)[:, None], np.where(inside, codes, 0)]
    step = np.where(inside, g["advance"].astype(np.int64) + items["track"].astype(np.int64)[:, None], 0)
    pen = np.cumsum(step, axis=1) - step
    h32 = mix32(items["seed"].astype(np.uint64)[:, None] ^ ((k.astype(np.uint64) * np.uint64(0x9E3779B9)) & np.uint64(0xffffffff)))
    jit = items["jitter"].astype(np.int64)[:, None]
    dy = (((h32 & np.uint64(0xffff)).astype(np.int64) * (2 * jit + 1)) >> 16) - jit
    w, h = g["w"].astype(np.int64), g["h"].astype(np.int64)
    return inside & (w > 0), pen + g["left"], w, g["top"] + dy, h, g["off"].astype(np.int64)


def synth_host(atlas, codes, items, img_size, table=None):
    """The rule of crnn_synth_words in NumPy (the host path, and the oracle of the device kernel): codes (n, Lmax) and n items -> the (n, T0, T1)
    uint8 images, or with `table` (256 fp32, ingest.norm_table) the fp32 table[v] of them."""
    T0, T1 = int(img_size[0]), int(img_size[1])
    if T0 < 1 or T1 < 1 or T0 * T1 > MAX_PIXELS:
        raise ValueError("an image has 1 <= T0 * T1 <= %d pixels, not %d x %d" % (MAX_PIXELS, T0, T1))
    items, codes = check_items(items, codes, atlas.nfaces, atlas.nglyphs)
    out = np.empty((len(items), T0, T1), np.uint8)
    ink, xlo, w, ylo, h, off = _layout(atlas, codes, items)
    i, jj = np.arange(T0, dtype=np.int64), T1 - 1 - np.arange(T1, dtype=np.int64)
    for b, it in enumerate(items):
        ks = np.flatnonzero(ink[b])
        c = np.zeros((T0, T1), np.int64)
        if len(ks):
            xa, xb, ya, yb = xlo[b, ks].min(), (xlo[b, ks] + w[b, ks]).max(), ylo[b, ks].min(), (ylo[b, ks] + h[b, ks]).max()
            line = np.zeros((yb - ya + 2, xb - xa + 2), np.int64)                      # the composed line with a border of zeros
            for k in ks:
                bm = atlas.arena[off[b, k]:off[b, k] + w[b, k] * h[b, k]].reshape(h[b, k], w[b, k])
                r, q = ylo[b, k] - ya + 1, xlo[b, k] - xa + 1
                np.maximum(line[r:r + h[b, k], q:q + w[b, k]], bm, out=line[r:r + h[b, k], q:q + w[b, k]])
            X, Y = int(it["sx"]) * i + int(it["ox"]), int(it["sy"]) * jj + int(it["oy"])       # int64 >> is arithmetic: the floor
            fx, fy = ((X >> 8) & 255)[:, None], ((Y >> 8) & 255)[None, :]
            col = lambda x: np.clip(x - xa + 1, 0, line.shape[1] - 1)[:, None]         # anything outside lands on the border
            row = lambda y: np.clip(y - ya + 1, 0, line.shape[0] - 1)[None, :]
            x0, y0 = X >> 16, Y >> 16
            c = ((256 - fy) * (256 - fx) * line[row(y0), col(x0)] + (256 - fy) * fx * line[row(y0), col(x0 + 1)]
                 + fy * (256 - fx) * line[row(y0 + 1), col(x0)] + fy * fx * line[row(y0 + 1), col(x0 + 1)] + 32768) >> 16
        out[b] = (int(it["bg"]) * (255 - c) + int(it["fg"]) * c + 127) // 255
    return out if table is None else np.asarray(table, np.float32)[out]


def ink_box(atlas, codes, items):
    """-> (has ink, xa, xb, ya, yb) per image: the line-space box [xa, xb) x [ya, yb) that holds the word's ink wherever the jitter puts each glyph
    (the rows are widened by `jitter` on both sides, so the box does not depend on the seed)."""
    ink, xlo, w, ylo, h, _ = _layout(atlas, codes, np.asarray(items))
    n, L = codes.shape
    inside = np.arange(L)[None, :] < items["len"].astype(np.int64)[:, None]
    top = atlas.table[items["face"].astype(np.int64)[:, None], np.where(inside, codes, 0)]["top"].astype(np.int64)
    jit = items["jitter"].astype(np.int64)
    big = np.int64(1) << 40
    has = ink.any(axis=1)
    xa, xb = np.where(ink, xlo, big).min(axis=1), np.where(ink, xlo + w, -big).max(axis=1)
    ya, yb = np.where(ink, top, big).min(axis=1) - jit, np.where(ink, top + h, -big).max(axis=1) + jit
    z = lambda v: np.where(has, v, 0)
    return has, z(xa), z(xb), z(ya), z(yb)


class SynthPolicy:
    """The random decisions of the synthetic words, drawn on the host: .draw(codes, lens, atlas, img_size) -> one crnn_synth_item (ITEM_DTYPE) per
    row of codes (n, Lmax), whose first lens[b] entries are the word's glyph codes.  Per image, uniformly:
      face     one of the atlas's faces
      track    (lo, hi) pixels added to every advance; jitter (lo, hi): each glyph's baseline moves by up to that many rows
      fill     (lo, hi): the share of the image's length the ink may take; height (lo, hi): the share of its width across the text
      fg, bg   (lo, hi) grey of the ink and of the ground (the ingest leaves ink bright)
      margin   output pixels kept free on every side
    From the atlas metrics the policy computes one scale for both axes (the word keeps its shape) -- the smaller magnification of "the ink's
    columns fill `fill` of T0" and "its rows fill `height` of T1", whichever binds -- and places the ink box (synth.ink_box) at a drawn position
    in the slack that is left.  Scale and offsets are computed in float64 and rounded once to integers here; the offset's range is formed from
    the integer scale, so the ink box lies inside the image exactly; only the integers are consumed afterwards.  A word too long for the
    largest scale of the ABI (4 line pixels per output pixel) starts at the margin and loses its end.  The policy owns a
    np.random.RandomState(seed) and never touches the global np.random stream; the number of draws per call depends on n alone.  Every default
    range is a PLACEHOLDER: nothing was at hand to tune them."""

    def __init__(self, seed=0, track=(-1, 3), jitter=(0, 2), fill=(0.6, 0.95), height=(0.6, 0.9), fg=(170, 255), bg=(0, 80), margin=1):
        self.seed, self.track, self.jitter, self.fill, self.height = int(seed), tuple(track), tuple(jitter), tuple(fill), tuple(height)
        self.fg, self.bg, self.margin = tuple(fg), tuple(bg), int(margin)
        if not (MIN_TRACK <= self.track[0] <= self.track[1] <= MAX_TRACK and 0 <= self.jitter[0] <= self.jitter[1] <= MAX_JITTER
                and 0 < self.fill[0] <= self.fill[1] <= 1 and 0 < self.height[0] <= self.height[1] <= 1 and 0 <= self.fg[0] <= self.fg[1] <= 255
                and 0 <= self.bg[0] <= self.bg[1] <= 255 and self.margin >= 0):
            raise ValueError("synth policy: track within %d..%d, jitter within 0..%d, 0 < fill, height <= 1, greys 0..255, margin >= 0"
                             % (MIN_TRACK, MAX_TRACK, MAX_JITTER))
        self.rs = np.random.RandomState(self.seed)

    def draw(self, codes, lens, atlas, img_size):
        codes = np.ascontiguousarray(codes, dtype=np.intc)
        n, T0, T1 = len(codes), int(img_size[0]), int(img_size[1])
        u = self.rs.uniform(size=(n, 9))
        seeds = self.rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
        pick = lambda col, lo, hi: np.minimum(lo + np.floor(u[:, col] * (hi - lo + 1)).astype(np.int64), hi)      # an integer of lo..hi
        t = np.zeros(n, ITEM_DTYPE)
        t["face"], t["len"] = pick(0, 0, atlas.nfaces - 1), lens
        t["track"], t["jitter"] = pick(1, *self.track), pick(2, *self.jitter)
        t["fg"], t["bg"], t["seed"] = pick(5, *self.fg), pick(6, *self.bg), seeds
        t["sx"] = t["sy"] = 65536
        if n == 0:
            return t
        has, xa, xb, ya, yb = ink_box(atlas, codes, t)
        m0, m1 = min(self.margin, (T0 - 1) // 2), min(self.margin, (T1 - 1) // 2)
        room0 = (self.fill[0] + (self.fill[1] - self.fill[0]) * u[:, 3]) * (T0 - 1 - 2 * m0)       # output pixels between the first and last ink centre
        room1 = (self.height[0] + (self.height[1] - self.height[0]) * u[:, 4]) * (T1 - 1 - 2 * m1)
        with np.errstate(divide="ignore", invalid="ignore"):
            need = lambda span, room: np.where(span > 0, span / room, 0.0)             # line pixels per output pixel; inf when there is no room
            s = np.maximum(need((xb - xa - 1).astype(np.float64), room0), need((yb - ya - 1).astype(np.float64), room1))
        scale = np.clip(np.rint(np.minimum(s, 8.0) * 65536.0), MIN_SCALE, MAX_SCALE).astype(np.int64)

        def place(a, b, T, m, col):
            lo, hi = ((b - 1) << 16) - scale * (T - 1 - m), (a << 16) - scale * m      # the last ink centre at or before T - 1 - m, the first at or after m
            at = lo + np.rint(u[:, col] * (hi - lo).astype(np.float64)).astype(np.int64)
            return np.clip(np.where(hi >= lo, np.clip(at, lo, hi), hi), -MAX_OFFSET, MAX_OFFSET)
        t["sx"] = t["sy"] = np.where(has, scale, 65536)
        t["ox"], t["oy"] = np.where(has, place(xa, xb, T0, m0, 7), 0), np.where(has, place(ya, yb, T1, m1, 8), 0)
        return check_items(t, codes, atlas.nfaces, atlas.nglyphs)[0]


class WordSynth:
    """synth_host on the device.  .run(codes, items, batch=None, return_u8=False): codes (n, Lmax) and the n items -> device fp32
    (batch or n, T0, T1, 1) = table[pixel], rows past n zero [, the uint8 batch].  One launch on the current stream; the atlas goes up once per
    device, the items and codes travel through two page-locked staging slots (pages.StagingSlots) and nothing is read back."""

    def __init__(self, atlas, img_size, normed=True, mean=118.24236953981779, std=36.72835353999682, device=None):
        import torch
        from .ingest import norm_table
        from .pages import StagingSlots, device_lib
        self.lib, self.device = device_lib("WordSynth", "synth.synth_host", device)
        self.atlas, self.img_size = atlas, tuple(img_size)
        self.T0, self.T1 = int(img_size[0]), int(img_size[1])
        self.table = torch.from_numpy(norm_table(normed, mean, std)).to(self.device)
        self._staging = StagingSlots(self.device, floor=1 << 16)

    def run(self, codes, items, batch=None, return_u8=False):
        import torch
        from .engine import _ptr, _stream
        items, codes = check_items(items, codes, self.atlas.nfaces, self.atlas.nglyphs)
        n, Lmax = codes.shape
        B = n if batch is None else int(batch)
        if B < 1 or n > B:
            raise ValueError("%d words do not fit a batch of %d" % (n, B))
        ibytes = -(-n * ITEM_DTYPE.itemsize // 16) * 16                                # the codes begin on a 16-byte boundary behind the items
        nbytes = ibytes + codes.nbytes
        with torch.cuda.device(self.device):
            arena, glyphs = self.atlas.on_device(self.device)
            s = self._staging.take(max(nbytes, 1))
            s["np"][:n * ITEM_DTYPE.itemsize].view(ITEM_DTYPE)[:] = items
            s["np"][ibytes:nbytes].view(np.intc)[:] = codes.ravel()
            if n:
                s["dev"][:nbytes].copy_(s["host"][:nbytes], non_blocking=True)
                s["copied"].record(torch.cuda.current_stream())
            out = torch.empty((B, self.T0, self.T1, 1), dtype=torch.float32, device=self.device)
            o8 = torch.empty((B, self.T0, self.T1), dtype=torch.uint8, device=self.device) if return_u8 else None
            host, dev = s["host"].data_ptr(), s["dev"].data_ptr()
            native.check(self.lib.crnn_synth_words(_ptr(arena), self.atlas.arena.size, self.atlas.table.ctypes.data_as(ctypes.c_void_p), _ptr(glyphs),
                                                   self.atlas.nfaces, self.atlas.nglyphs, ctypes.c_void_p(host + ibytes), ctypes.c_void_p(dev + ibytes),
                                                   ctypes.c_void_p(host), ctypes.c_void_p(dev), n, B, Lmax, self.T0, self.T1, _ptr(self.table),
                                                   _ptr(out), _ptr(o8), _stream()), "synth_words")
        return (out, o8) if return_u8 else out


class SynthReadf(Readf):
    """Readf without files: .run_generator(downsample_factor=2) is endless and yields Readf's dictionaries ('the_input', 'the_labels',
    'input_length', 'label_length', 'source_str') and {'ctc': zeros}.  Every batch draws batch_size words with replacement from `words` with the
    policy's RandomState, maps them through `classes` exactly as Readf.make_target does (the glyph codes ARE the labels, so the atlas has one
    glyph per class), lets the policy draw the items and renders them: 'the_input' is a device fp32 tensor (B,) + img_size from WordSynth, or
    with host=True Readf's float64 array from synth_host.  `augment` (an augment.AugmentPolicy): the uint8 batch goes through
    Augmenter.run -- a second launch on the same stream -- or augment_host.  Host and device modes yield the same values under the same seeds."""

    def __init__(self, words, atlas, img_size=(100, 32, 1), batch_size=32, classes={}, max_len=23, normed=False, mean=118.24236953981779,
                 std=36.72835353999682, policy=None, augment=None, device=None, host=False):
        super().__init__(img_size=img_size, max_len=max_len, normed=normed, batch_size=batch_size, classes=classes, mean=mean, std=std,
                         transform_p=0., augment=augment)
        self.words, self.atlas, self.host = list(words), atlas, bool(host)
        self.policy = SynthPolicy() if policy is None else policy
        if not self.words or max(len(w) for w in self.words) > self.max_len or not 1 <= self.max_len <= MAX_LEN:
            raise ValueError("SynthReadf needs words, none longer than max_len = %d <= %d" % (self.max_len, MAX_LEN))
        if atlas.nglyphs != len(classes):
            raise ValueError("the atlas has %d glyphs per face for %d classes" % (atlas.nglyphs, len(classes)))
        self._device, self._synth, self._augmenter = device, None, None

    def _render(self, codes, items):
        if self.host:
            pixels = synth_host(self.atlas, codes, items, self.img_size)
            if self.augment is not None:
                from .augment import augment_host
                pixels = augment_host(pixels, self.augment.draw(len(pixels), self.img_size))
            X = np.empty((self.batch_size,) + tuple(self.img_size))
            X[...] = (norm(pixels, self.mean, self.std) if self.normed else pixels)[..., np.newaxis]
            return X
        if self._synth is None:
            self._synth = WordSynth(self.atlas, self.img_size, normed=self.normed, mean=self.mean, std=self.std, device=self._device)
        if self.augment is None:
            return self._synth.run(codes, items)
        if self._augmenter is None:
            from .augment import Augmenter
            self._augmenter = Augmenter(self.img_size, normed=self.normed, mean=self.mean, std=self.std, device=self._synth.device)
        _, u8 = self._synth.run(codes, items, return_u8=True)
        return self._augmenter.run(u8, self.augment.draw(len(items), self.img_size))

    def run_generator(self, downsample_factor=2):
        steps_in = (self.img_size[0] + 4) // downsample_factor - 2
        while True:
            _, Y, in_len, lab_len = self.get_blank_matrices()
            words = [self.words[k] for k in self.policy.rs.randint(0, len(self.words), size=self.batch_size)]
            for slot, word in enumerate(words):
                ids = self.make_target(word)
                Y[slot, :len(ids)] = ids
                lab_len[slot] = len(ids)
            in_len[:] = steps_in
            items = self.policy.draw(Y, lab_len[:, 0].astype(np.int64), self.atlas, self.img_size)
            yield ({'the_input': self._render(np.ascontiguousarray(Y, dtype=np.intc), items), 'the_labels': Y, 'input_length': in_len,
                    'label_length': lab_len, 'source_str': np.array(words)}, {'ctc': np.zeros([self.batch_size])})
