"""CPU tests (no GPU) of the synthetic training words: the rule of include/crnn_mi355x.h (crnn_synth_words) as crnn_mi355x.synth.synth_host
states it, against vectors pinned from an independent prototype (tests/golden/make_synth_vectors.py) and against plain-Python loops;
the struct mirrors; every refusal of crnn_synth_words (fake non-null integers stand for the device pointers, as in tests/test_augment_cpu.py:
a case runs only where the call refuses, so nothing is launched); SynthPolicy; SynthReadf(host=True); GlyphAtlas."""
import ctypes
import glob
import os

import numpy as np
import pytest

import utils as U
from crnn_mi355x import augment as A
from crnn_mi355x import hashing
from crnn_mi355x import ingest as I
from crnn_mi355x import native
from crnn_mi355x import synth as S

ARG, UNSUPPORTED = -2, -3
FAKE = ctypes.c_void_p(1 << 22)                                        # stands for a device pointer

u8 = lambda rows: np.array(rows, np.uint8)
TOY = [
    [(u8([[10, 20, 30], [40, 50, 60]]), 0, 1, 3), (u8([[70, 80, 90], [100, 110, 120]]), 1, 0, 4), (u8([[130, 140, 150], [160, 170, 255]]), -1, 2, 2)],
    [(u8([[15, 25], [35, 45], [55, 65]]), 0, 0, 2), (u8([[75, 85], [95, 105], [115, 125]]), 0, 1, 3), (None, 0, 0, 2)],
]
PINNED = [          # (codes, item, the bytes tests/golden/make_synth_vectors.py prints)
    ([0, 1], dict(face=0, track=0, jitter=0, sx=65536, sy=65536, ox=0, oy=0, fg=255, bg=0, seed=0),
     [[0, 40, 10, 0], [0, 50, 20, 0], [0, 60, 30, 0], [0, 0, 0, 0], [0, 0, 100, 70], [0, 0, 110, 80]]),      # identity
    ([0, 1], dict(face=0, track=0, jitter=0, sx=65536, sy=65536, ox=-40000, oy=25000, fg=255, bg=0, seed=0),
     [[0, 10, 8, 1], [0, 27, 25, 5], [0, 33, 35, 9], [0, 23, 25, 7], [0, 0, 24, 31], [0, 0, 65, 85]]),      # fractional offset
    ([1, 0, 2], dict(face=0, track=-3, jitter=0, sx=65536, sy=65536, ox=0, oy=0, fg=255, bg=0, seed=0),
     [[160, 130, 0, 0], [170, 140, 100, 70], [255, 150, 110, 80], [0, 60, 120, 90], [0, 0, 0, 0], [0, 0, 0, 0]]),      # negative track, overlap
    ([0, 1, 0], dict(face=1, track=0, jitter=2, sx=65536, sy=65536, ox=0, oy=-65536, fg=255, bg=0, seed=77),
     [[35, 15, 0, 0], [45, 25, 0, 0], [95, 75, 0, 0], [105, 85, 0, 0], [0, 0, 0, 0], [35, 15, 0, 0]]),      # jitter
    ([1, 2], dict(face=0, track=1, jitter=0, sx=50000, sy=80000, ox=30000, oy=-20000, fg=20, bg=230, seed=0),
     [[230, 230, 193, 212], [230, 230, 148, 189], [230, 230, 142, 185], [230, 230, 135, 181], [187, 174, 182, 204], [144, 117, 230, 230]]),      # fg < bg
    ([], dict(face=1, track=2, jitter=1, sx=65536, sy=65536, ox=0, oy=0, fg=200, bg=33, seed=5),
     [[33, 33, 33, 33]] * 6),      # empty word
    ([0, 2, 1], dict(face=1, track=1, jitter=1, sx=90000, sy=70000, ox=-70000, oy=10000, fg=250, bg=5, seed=123456789),
     [[5, 5, 5, 5], [41, 47, 26, 8], [18, 20, 15, 6], [5, 5, 5, 5], [5, 5, 5, 5], [83, 66, 17, 5]]),      # scaled, jittered, a glyph without ink
]


def _one(codes, fields, Lmax=4):
    row = np.full((1, Lmax), 99, np.intc)                              # what lies past len is never read
    row[0, :len(codes)] = codes
    it = S.identity_items(1, len(codes))
    for k, v in fields.items():
        it[k] = v
    return row, it


@pytest.mark.parametrize("case", range(len(PINNED)))
def test_pinned_vectors(case):
    codes, fields, want = PINNED[case]
    got = S.synth_host(S.GlyphAtlas.from_arrays(TOY), *_one(codes, fields), (6, 4, 1))
    assert got.dtype == np.uint8 and got.shape == (1, 6, 4) and got[0].tolist() == want


def test_the_mirrors_and_the_shared_hash():
    assert ctypes.sizeof(S.crnn_glyph) == S.GLYPH_DTYPE.itemsize == 32 and ctypes.sizeof(S.crnn_synth_item) == S.ITEM_DTYPE.itemsize == 44
    _, it = _one([1, 2], dict(face=1, track=-8, ox=-5, seed=0xfffffff0, bg=7))
    raw = S.crnn_synth_item.from_buffer_copy(it.tobytes())
    assert (raw.face, raw.len, raw.track, raw.jitter, raw.sx, raw.sy, raw.ox, raw.oy, raw.fg, raw.bg, raw.seed) == (1, 2, -8, 0, 65536, 65536, -5, 0, 255, 7,
                                                                                                                    0xfffffff0)
    atlas = S.GlyphAtlas.from_arrays(TOY)
    g = (S.crnn_glyph * 6).from_buffer_copy(atlas.table.tobytes())[2]
    assert (g.off, g.w, g.h, g.left, g.top, g.advance) == (12, 3, 2, -1, 2, 2)
    assert A.mix32 is hashing.mix32 and S.mix32 is hashing.mix32       # one hash, stated once
    assert hashing.mix32([0, 1, 2]).tolist() == [0, 1753845952, 3507691905]


# ---- synth_host against loops --------------------------------------------------------------------------------------------------------------
def _random_atlas(seed, nfaces=2, nglyphs=9, big=12):
    rs = np.random.RandomState(seed)
    faces = []
    for _ in range(nfaces):
        face = []
        for g in range(nglyphs):
            if g == 3:
                face.append((None, 0, 0, int(rs.randint(0, 6))))
                continue
            h, w = int(rs.randint(1, big + 1)), int(rs.randint(1, big + 1))
            face.append((rs.randint(0, 256, (h, w)).astype(np.uint8), int(rs.randint(-3, 4)), int(rs.randint(0, 20)), int(rs.randint(0, big + 3))))
        faces.append(face)
    return S.GlyphAtlas.from_arrays(faces)


def _loops(atlas, codes, it, T0, T1):
    """The header's rule, pixel by pixel in Python integers."""
    placed, pen = [], 0
    for k in range(int(it["len"])):
        g = atlas.table[int(it["face"]), int(codes[k])]
        h = int(hashing.mix32(int(it["seed"]) ^ ((k * 0x9E3779B9) & 0xffffffff)))
        dy = (((h & 0xffff) * (2 * int(it["jitter"]) + 1)) >> 16) - int(it["jitter"])
        placed.append((atlas.bitmap(int(it["face"]), int(codes[k])), pen + int(g["left"]), int(g["top"]) + dy))
        pen += int(g["advance"]) + int(it["track"])

    def cov(x, y):
        return max([int(bm[y - gy, x - gx]) for bm, gx, gy in placed if 0 <= y - gy < bm.shape[0] and 0 <= x - gx < bm.shape[1]] + [0])
    out = np.zeros((T0, T1), np.uint8)
    for i in range(T0):
        for j in range(T1):
            X, Y = int(it["sx"]) * i + int(it["ox"]), int(it["sy"]) * (T1 - 1 - j) + int(it["oy"])
            x0, fx, y0, fy = X >> 16, (X >> 8) & 255, Y >> 16, (Y >> 8) & 255
            c = ((256 - fy) * (256 - fx) * cov(x0, y0) + (256 - fy) * fx * cov(x0 + 1, y0) + fy * (256 - fx) * cov(x0, y0 + 1)
                 + fy * fx * cov(x0 + 1, y0 + 1) + 32768) >> 16
            out[i, j] = (int(it["bg"]) * (255 - c) + int(it["fg"]) * c + 127) // 255
    return out


def _wild_items(rs, n, atlas, Lmax):
    it = S.identity_items(n)
    it["face"], it["len"] = rs.randint(0, atlas.nfaces, n), rs.randint(0, Lmax + 1, n)
    it["track"], it["jitter"] = rs.randint(-8, 33, n), rs.randint(0, 9, n)
    it["sx"], it["sy"] = rs.randint(16384, 262145, n), rs.randint(16384, 262145, n)
    it["ox"], it["oy"] = rs.randint(-(20 << 16), 40 << 16, n), rs.randint(-(10 << 16), 20 << 16, n)
    it["fg"], it["bg"], it["seed"] = rs.randint(0, 256, n), rs.randint(0, 256, n), rs.randint(0, 1 << 32, n, dtype=np.uint64)
    it["len"][0], it["track"][1], it["sx"][2], it["sy"][2] = 0, -8, 65536, 65536
    return it


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (33, 3), (100, 32)])
def test_synth_host_equals_the_loops(shape):
    atlas = _random_atlas(sum(shape))
    rs = np.random.RandomState(shape[0])
    n, Lmax = 6, 7
    codes = rs.randint(0, atlas.nglyphs, (n, Lmax)).astype(np.intc)
    items = _wild_items(rs, n, atlas, Lmax)
    got = S.synth_host(atlas, codes, items, shape + (1,))
    assert got.shape == (n,) + shape and got.dtype == np.uint8
    for b in range(n):
        assert np.array_equal(got[b], _loops(atlas, codes[b], items[b], *shape)), (b, items[b])
    assert len(np.unique(got)) > 2 or shape == (1, 1)
    table = I.norm_table(True)
    assert np.array_equal(S.synth_host(atlas, codes, items, shape + (1,), table), table[got])


def test_one_glyph_at_identity_scale_is_its_bitmap_flipped():
    atlas = _random_atlas(5)
    bm, g = atlas.bitmap(1, 4), atlas.table[1, 4]
    T0, T1 = bm.shape[1] + 2, int(g["top"]) + bm.shape[0] + 1
    row, it = _one([4], dict(face=1, ox=int(g["left"]) << 16))         # the image's first column is the bitmap's first
    got = S.synth_host(atlas, row, it, (T0, T1, 1))[0]
    line = np.zeros((T1, T0), np.uint8)                                # line space: y down, x along the text
    line[int(g["top"]):int(g["top"]) + bm.shape[0], :bm.shape[1]] = bm
    assert np.array_equal(got, line[::-1].T) and got.any()             # rot(i, j) = line[T1 - 1 - j, i]: the ingest's orientation


# ---- the refusals of crnn_synth_words ------------------------------------------------------------------------------------------------------
def _call(atlas, codes, items, n=None, batch=4, Lmax=None, imgh=100, imgw=32, nfaces=None, nglyphs=None, atlas_bytes=None, table=None, null=()):
    n = len(items) if n is None else n
    ptr = lambda name, v: None if name in null else v
    tab = atlas.table if table is None else table
    return native.lib().crnn_synth_words(
        ptr("atlas", FAKE), atlas.arena.size if atlas_bytes is None else atlas_bytes, ptr("glyphs", tab.ctypes.data_as(ctypes.c_void_p)),
        ptr("glyphs_dev", FAKE), atlas.nfaces if nfaces is None else nfaces, atlas.nglyphs if nglyphs is None else nglyphs,
        ptr("codes", codes.ctypes.data_as(ctypes.c_void_p)), ptr("codes_dev", FAKE), ptr("items", items.ctypes.data_as(ctypes.c_void_p)),
        ptr("items_dev", FAKE), n, batch, codes.shape[1] if Lmax is None else Lmax, imgh, imgw, ptr("table", FAKE), ptr("out", FAKE),
        ptr("out_u8", FAKE), None)


_RANGES = [("track", -8, 32), ("jitter", 0, 8), ("sx", 16384, 262144), ("sy", 16384, 262144), ("ox", -(1 << 28), 1 << 28),
           ("oy", -(1 << 28), 1 << 28), ("fg", 0, 255), ("bg", 0, 255)]


def _good(atlas, n=3, Lmax=5):
    codes = np.tile(np.arange(Lmax, dtype=np.intc) % atlas.nglyphs, (n, 1))
    return codes, S.identity_items(n, Lmax)


def test_every_refusal_of_crnn_synth_words():
    assert "crnn_synth_words" in native.parse_header() and "synth.hip" in native.SOURCES
    atlas = S.GlyphAtlas.from_arrays(TOY)
    codes, good = _good(atlas)
    ranges = _RANGES + [("face", 0, atlas.nfaces - 1), ("len", 0, codes.shape[1])]
    for name, lo, hi in ranges:
        for v in (lo - 1, hi + 1):
            for row in (0, 2):
                items = good.copy()
                items[name][row] = v
                assert _call(atlas, codes, items) == ARG, (name, v, row)
                with pytest.raises(ValueError):
                    S.check_items(items, codes, atlas.nfaces, atlas.nglyphs)
        for v in (lo, hi):
            items = good.copy()
            items[name][:] = v
            S.check_items(items, codes, atlas.nfaces, atlas.nglyphs)
    for v in (-1, atlas.nglyphs):
        bad = codes.copy()
        bad[2, 4] = v
        assert _call(atlas, bad, good) == ARG
        with pytest.raises(ValueError):
            S.check_items(good, bad, atlas.nfaces, atlas.nglyphs)
        short = good.copy()
        short["len"][2] = 4                                            # the same code past len is not judged
        S.check_items(short, bad, atlas.nfaces, atlas.nglyphs)
    assert _call(atlas, codes, good, n=5, batch=4) == ARG and _call(atlas, codes, good, n=-1) == ARG and _call(atlas, codes, good, n=0, batch=0) == ARG
    for kw in (dict(imgh=0), dict(imgw=0), dict(imgh=-100), dict(Lmax=0), dict(Lmax=65), dict(nfaces=0), dict(nglyphs=0), dict(atlas_bytes=0)):
        assert _call(atlas, codes, good, **kw) == ARG, kw
    for name in ("atlas", "glyphs", "glyphs_dev", "table", "out", "codes", "codes_dev", "items", "items_dev"):
        assert _call(atlas, codes, good, null=(name,)) == ARG, name
    for name in ("atlas", "glyphs", "glyphs_dev", "table", "out"):     # n == 0 excuses the codes and the items only
        assert _call(atlas, codes, good, n=0, null=(name,)) == ARG, name
    assert _call(atlas, codes, good, imgh=129, imgw=128) == UNSUPPORTED and _call(atlas, codes, good, imgh=16385, imgw=1) == UNSUPPORTED
    glyph_faults = [dict(w=-1), dict(w=65, h=1), dict(h=65), dict(w=0), dict(h=0), dict(top=-1), dict(top=63), dict(left=-65), dict(left=65),
                    dict(advance=-1), dict(advance=129), dict(off=-1), dict(off=atlas.arena.size - 5)]
    for fault in glyph_faults:
        for where in ((0, 0), (1, 1)):
            tab = atlas.table.copy()
            for k, v in fault.items():
                tab[k][where] = v
            assert _call(atlas, codes, good, table=tab) == ARG, (fault, where)
            with pytest.raises(ValueError):
                S.check_glyphs(tab, atlas.arena.size)
    tab = atlas.table.copy()
    tab["off"][1, 2] = -77                                             # a glyph without ink reads nothing: its off is not judged
    S.check_glyphs(tab, atlas.arena.size)
    with pytest.raises(ValueError):
        S.synth_host(atlas, codes, good, (129, 128, 1))
    with pytest.raises(ValueError):
        S.check_items(np.zeros(3, np.int32), codes, 2, 3)
    with pytest.raises(ValueError):
        S.check_items(good, codes[:2], 2, 3)


# ---- SynthPolicy ---------------------------------------------------------------------------------------------------------------------------
def _small_font_atlas(seed=0, nfaces=3, nglyphs=37):
    """Faces of a small font: ink 2..6 columns wide, advance = left + w + 1 <= 7, 12 rows of line box."""
    rs = np.random.RandomState(seed)
    faces = []
    for _ in range(nfaces):
        face = []
        for g in range(nglyphs):
            if g == nglyphs - 1:
                face.append((None, 0, 0, 4))                           # a space
                continue
            w, h, left = int(rs.randint(2, 6)), int(rs.randint(3, 11)), int(rs.randint(-1, 2))
            face.append((rs.randint(1, 256, (h, w)).astype(np.uint8), left, int(rs.randint(0, 13 - h)), max(0, left) + w + 1))
        faces.append(face)
    return S.GlyphAtlas.from_arrays(faces)


def _words(rs, n, nglyphs, Lmax=23):
    lens = rs.randint(1, Lmax + 1, n)
    codes = np.full((n, Lmax), nglyphs, np.intc)                       # the blank past len, as the_labels hold it
    for b, ln in enumerate(lens):
        codes[b, :ln] = rs.randint(0, nglyphs, ln)
    return codes, lens


def test_policy_is_deterministic_and_leaves_np_random_alone():
    atlas = _small_font_atlas()
    codes, lens = _words(np.random.RandomState(1), 8, atlas.nglyphs)
    size = (100, 32, 1)
    a, b = S.SynthPolicy(seed=3), S.SynthPolicy(seed=3)
    state = np.random.get_state()
    first = [a.draw(codes[:k], lens[:k], atlas, size) for k in (8, 5, 8)]
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert all(x.tobytes() == b.draw(codes[:len(x)], lens[:len(x)], atlas, size).tobytes() for x in first)
    assert first[0].tobytes() != first[2].tobytes() and S.SynthPolicy(seed=4).draw(codes, lens, atlas, size).tobytes() != first[0].tobytes()
    assert first[0].dtype == S.ITEM_DTYPE and len(S.SynthPolicy().draw(codes[:0], lens[:0], atlas, size)) == 0
    c, d = S.SynthPolicy(seed=9), S.SynthPolicy(seed=9)               # the number of draws depends on n alone
    c.draw(codes, lens, atlas, size), d.draw(codes[::-1], np.ones(8, int), atlas, (40, 32, 1))
    assert np.array_equal(c.rs.randint(0, 1 << 30, 4), d.rs.randint(0, 1 << 30, 4))
    wild = S.SynthPolicy(seed=6, track=(-8, 32), jitter=(0, 8), fill=(0.01, 1.0), height=(0.01, 1.0), fg=(0, 255), bg=(0, 255), margin=40)
    for size in ((1, 1, 1), (7, 5, 1), (33, 3, 1), (128, 128, 1)):     # whatever the ranges, the items stay inside the ABI's
        items = wild.draw(codes, lens, _random_atlas(2, nglyphs=37, big=64 - 20), size)
        assert S.check_items(items, codes, 2, 37)[0] is items


@pytest.mark.parametrize("size", [(100, 32, 1), (200, 32, 1)])
def test_policy_puts_the_ink_box_inside_the_image(size):
    T0, T1 = size[:2]
    atlas = _small_font_atlas(T0)
    rs = np.random.RandomState(T0 + 1)
    codes, lens = _words(rs, 500, atlas.nglyphs)
    policy = S.SynthPolicy(seed=T0)
    items = policy.draw(codes, lens, atlas, size)
    assert set(lens) == set(range(1, 24)) and len(set(items["face"])) == atlas.nfaces
    assert items["track"].min() == -1 and items["track"].max() == 3 and set(items["jitter"]) == {0, 1, 2} and (items["sx"] == items["sy"]).all()
    assert len(set(items["sx"])) > 100 and len(set(items["ox"])) > 100 and len(set(items["oy"])) > 100
    filled, placed = [], 0
    for b, it in enumerate(items):                                    # the ink box from the atlas metrics, in Python integers
        pen, xs, ys = 0, [], []
        for k in range(lens[b]):
            g = atlas.table[int(it["face"]), codes[b, k]]
            if g["w"] > 0:
                xs += [pen + int(g["left"]), pen + int(g["left"]) + int(g["w"]) - 1]            # first and last ink column
                ys += [int(g["top"]) - int(it["jitter"]), int(g["top"]) + int(g["h"]) - 1 + int(it["jitter"])]
            pen += int(g["advance"]) + int(it["track"])
        if not xs:
            continue                                                   # a word of spaces has no ink to place (asserted below to be rare)
        sx, sy, ox, oy = int(it["sx"]), int(it["sy"]), int(it["ox"]), int(it["oy"])
        # X(i) = sx i + ox reads line column X / 65536: the image spans [X(m), X(T0 - 1 - m)] inside its margin m = 1, and likewise across
        assert sx * 1 + ox <= min(xs) << 16 and max(xs) << 16 <= sx * (T0 - 2) + ox, (b, it)
        assert sy * 1 + oy <= min(ys) << 16 and max(ys) << 16 <= sy * (T1 - 2) + oy, (b, it)
        placed += 1
        if S.MIN_SCALE < sx < S.MAX_SCALE:                             # (a scale at an end of the ABI's range is not the one the policy asked for)
            filled.append(max(((max(xs) - min(xs)) << 16) / (sx * (T0 - 3.0)), ((max(ys) - min(ys)) << 16) / (sy * (T1 - 3.0))))
    # ... and on the binding axis the ink takes the share `fill` (0.6 .. 0.95) or `height` (0.6 .. 0.9) asks for, up to the rounding of the scale
    assert placed > 490 and len(filled) > 400 and 0.599 < min(filled) and max(filled) < 0.951


# ---- SynthReadf(host=True) -----------------------------------------------------------------------------------------------------------------
WORDS = ["hello", "a", "w0rld", "0123456789", "mi355x", "synthetic", "z", "glyph-atlas", "qwertyuiopasdfghjklzxcv"]


def _classes():
    return {ch: i for i, ch in enumerate(U.get_lexicon())}


def _reader(seed=1, augment=None, normed=True, **kw):
    return U.SynthReadf(WORDS, _small_font_atlas(7), img_size=(100, 32, 1), batch_size=6, classes=_classes(), max_len=23, normed=normed,
                        policy=U.SynthPolicy(seed=seed), augment=augment, host=True, **kw)


def test_synth_readf_on_the_host():
    classes = _classes()
    gen = _reader().run_generator(downsample_factor=4)
    ref = U.Readf(img_size=(100, 32, 1), batch_size=6, classes=classes, max_len=23, normed=True)
    X, Y, in_len, lab_len = ref.get_blank_matrices()
    seen = set()
    for _ in range(3):
        inputs, outputs = next(gen)
        assert sorted(inputs) == ["input_length", "label_length", "source_str", "the_input", "the_labels"] and list(outputs) == ["ctc"]
        for got, like in ((inputs["the_input"], X), (inputs["the_labels"], Y), (inputs["input_length"], in_len), (inputs["label_length"], lab_len)):
            assert got.shape == like.shape and got.dtype == like.dtype
        assert outputs["ctc"].shape == (6,) and not outputs["ctc"].any() and (inputs["input_length"] == (100 + 4) // 4 - 2).all()
        for b, word in enumerate(inputs["source_str"]):
            assert word in WORDS
            ids = ref.make_target(word)
            assert inputs["label_length"][b, 0] == len(word) and np.array_equal(inputs["the_labels"][b, :len(ids)], ids)
            assert (inputs["the_labels"][b, len(ids):] == len(classes)).all()
            seen.add(str(word))
        x = inputs["the_input"][..., 0]
        assert np.array_equal(x, x.astype(np.float32)) and (x.max(axis=(1, 2)) > x.min(axis=(1, 2))).all()      # fp32 values; every image has ink
    assert len(seen) > 4
    raw = next(_reader(normed=False).run_generator())[0]["the_input"]
    assert np.array_equal(raw, raw.astype(np.uint8)) and raw.max() > 150
    with pytest.raises(ValueError):
        U.SynthReadf(WORDS, _small_font_atlas(7), classes=classes, max_len=5)
    with pytest.raises(ValueError):
        U.SynthReadf(WORDS, _random_atlas(1), classes=classes, max_len=23)


def test_synth_readf_seeds_and_augmentation():
    def drain(reader, k=3):
        gen = reader.run_generator()
        return [(b["the_input"].copy(), b["the_labels"].copy(), list(b["source_str"])) for b, _ in (next(gen) for _ in range(k))]
    one, two, other = drain(_reader(1)), drain(_reader(1)), drain(_reader(2))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] for a, b in zip(one, two))
    assert any(a[2] != b[2] for a, b in zip(one, other)) and not any(np.array_equal(a[0], b[0]) for a, b in zip(one, other))
    assert not np.array_equal(one[0][0], one[1][0])
    aug = drain(_reader(1, augment=A.AugmentPolicy(seed=5, p=1.0), normed=False))
    plain = drain(_reader(1, normed=False))
    oracle = A.AugmentPolicy(seed=5, p=1.0)
    for a, p in zip(aug, plain):                                       # the same words and items; the pixels are augment_host's of the plain ones
        assert a[2] == p[2] and np.array_equal(a[0][..., 0], A.augment_host(p[0][..., 0].astype(np.uint8), oracle.draw(6, (100, 32, 1))))
        assert not np.array_equal(a[0], p[0])


# ---- GlyphAtlas ----------------------------------------------------------------------------------------------------------------------------
def test_atlas_npz_round_trip(tmp_path):
    atlas = _random_atlas(3)
    path = str(tmp_path / "atlas.npz")
    atlas.save(path)
    back = S.GlyphAtlas.load(path)
    assert back.arena.tobytes() == atlas.arena.tobytes() and back.table.tobytes() == atlas.table.tobytes() and back.table.dtype == S.GLYPH_DTYPE
    assert (back.nfaces, back.nglyphs) == (2, 9) and atlas.line_height(0) == int((atlas.table[0]["top"] + atlas.table[0]["h"]).max())
    assert np.array_equal(back.bitmap(1, 4), atlas.bitmap(1, 4)) and back.bitmap(0, 3).size == 0
    toy = S.GlyphAtlas.from_arrays(TOY)
    assert toy.line_height(0) == 4 and toy.line_height(1) == 4 and toy.arena.size % 16 == 0
    with pytest.raises(ValueError):
        S.GlyphAtlas.from_arrays([TOY[0], TOY[1][:2]])
    with pytest.raises(ValueError):
        S.GlyphAtlas.from_arrays([[(np.zeros((65, 1), np.uint8), 0, 0, 1)]])


def _a_font():
    try:
        import PIL
        from PIL import ImageFont  # noqa: F401
    except ImportError:
        return None
    roots = [os.path.join(os.path.dirname(PIL.__file__), "**", "*.ttf"), "/usr/share/fonts/**/*.ttf", "/usr/local/share/fonts/**/*.ttf"]
    try:
        import matplotlib
        roots.append(os.path.join(os.path.dirname(matplotlib.__file__), "mpl-data", "fonts", "ttf", "DejaVuSans.ttf"))
    except ImportError:
        pass
    for pattern in roots:
        for path in sorted(glob.glob(pattern, recursive=True)):
            try:
                ImageFont.truetype(path, 28).getlength("a")
                return path
            except OSError:
                continue
    return None


def test_atlas_from_a_font_file():
    path = _a_font()
    if path is None:
        pytest.skip("no PIL or no .ttf file on this machine")
    alphabet = U.get_lexicon()
    atlas = S.GlyphAtlas.from_fonts([path], 28, alphabet)
    assert (atlas.nfaces, atlas.nglyphs) == (1, len(alphabet))
    t = atlas.table[0]
    assert (t["w"] > 0).all() and (t["h"] > 0).all() and (t["advance"] >= t["w"] // 2).all() and (t["advance"] <= 40).all()
    assert all(atlas.bitmap(0, g).max() > 128 for g in range(len(alphabet))) and 15 <= atlas.line_height(0) <= 45
    dash, ell = t[alphabet.index("-")], t[alphabet.index("l")]
    assert dash["h"] < ell["h"] and dash["top"] > ell["top"]           # the hyphen sits lower in the line box than the top of an l
    codes, it = _one([alphabet.index(c) for c in "hello"], {}, Lmax=5)
    img = S.synth_host(atlas, codes, it, (100, 32, 1))[0]
    assert img.max() == 255 and (img > 128).mean() > 0.03              # "hello" at identity scale lands in the image
    with pytest.raises(OSError):
        S.GlyphAtlas.from_fonts([os.path.join(os.path.dirname(path), "no-such-font.ttf")], 28, alphabet)
