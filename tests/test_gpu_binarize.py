"""-m gpu tests of adaptive binarisation on the device (csrc/binarize.hip, crnn_mi355x/binarize.py).  Every case calls crnn_binarize_pages
twice on outputs pre-filled with two different sentinels and asserts that the two calls agree bit for bit, that the page bytes equal
sauvola_host (pinned to a brute-force restatement in tests/test_binarize_cpu.py), and that every byte outside the pages' rows x cols -- row
padding, the bytes between pages, a guard region past the arena -- still holds its sentinel.  Everything is integer: every comparison is exact
equality.  Shapes are the smallest at which the kernel takes every path: one-pixel, one-row and one-column pages, a page smaller than the
window, pages of several strips and bands that end off the grid, features across strip and band borders (binarize.STRIP_C x binarize.BAND_R)."""
import ctypes

import numpy as np
import pytest
import torch

import utils as U
from crnn_mi355x import binarize as B, detect as D
from crnn_mi355x.pages import pack_arena
from gpu_util import L, P, S, host, sentinel_arena as _arena
import binarize_ref as R

pytestmark = pytest.mark.gpu

S_C, B_R = B.STRIP_C, B.BAND_R
SENTINELS = (0x33, 0xc4)                                     # neither 0 nor 255
GUARD = 256


def _call(arena_dev, arena_bytes, table, table_dev, n, prm, out, out_bytes, null=None):
    args = dict(arena=P(arena_dev), pages=table.ctypes.data_as(ctypes.c_void_p), pages_dev=P(table_dev), prm=ctypes.byref(prm), out=P(out))
    if null:
        args[null] = ctypes.c_void_p(0)
    code = L().crnn_binarize_pages(args["arena"], arena_bytes, args["pages"], args["pages_dev"], n, args["prm"], args["out"], out_bytes, S())
    torch.cuda.synchronize()
    return code


def _binarize(pages, strides=None, radius=15, k256=51, polarity=1):
    """Two calls -> the output arena's bytes, equal between the calls on the pages, equal to sauvola_host, sentinels intact elsewhere."""
    prm = B.crnn_binarize_params(radius=radius, k256=k256, polarity=polarity)
    arena, table, inside = _arena(pages, strides)
    arena_dev, table_dev = torch.from_numpy(arena).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()
    outs = []
    for fill in SENTINELS:
        out = torch.full((arena.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
        code = _call(arena_dev, arena.size, table, table_dev, len(pages), prm, out, arena.size)
        assert code == 0, "crnn_binarize_pages returned %d" % code
        got = host(out)
        assert (got[arena.size:] == fill).all(), "the guard region past the arena was written"
        assert (got[:arena.size][~inside] == fill).all(), "a byte outside the pages' rows x cols was written"
        outs.append(got[:arena.size])
    assert np.array_equal(outs[0][inside], outs[1][inside]), "two calls disagree"
    assert np.array_equal(host(arena_dev), arena), "the input arena was written"
    for k, pg in enumerate(pages):
        off, st = int(table["page_off"][k]), int(table["stride"][k])
        got = outs[0][off:off + (pg.shape[0] - 1) * st + pg.shape[1]]
        got = np.concatenate([got, np.zeros(pg.shape[0] * st - got.size, np.uint8)]).reshape(pg.shape[0], st)[:, :pg.shape[1]]
        want = B.sauvola_host(pg, radius, k256, polarity)
        diff = np.argwhere(got != want)
        assert diff.size == 0, "page %d %s, r %d k256 %d polarity %d: %d pixels differ from the host's, the first at %s" % (
            k, pg.shape, radius, k256, polarity, len(diff), diff[0].tolist())
    return outs[0]


def _feature_page(rows, cols, at, seed, size=5):
    """Light paper with a little noise and dark size x size features whose top left corners are `at` (clipped to the page)."""
    rs = np.random.RandomState(seed)
    page = rs.randint(190, 221, (rows, cols)).astype(np.uint8)
    for r, c in at:
        page[max(r, 0):r + size, max(c, 0):c + size] = rs.randint(20, 60, page[max(r, 0):r + size, max(c, 0):c + size].shape)
    return page


# ---- 1. sizes, parameters -----------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 4 * 64 + 1), (4 * 64 + 1, 1), (5, 7), (2 * B_R + 5, 2 * S_C + 1)]


@pytest.mark.parametrize("polarity", [1, 2])
@pytest.mark.parametrize("k256", [0, 51, 255])
def test_random_pages_equal_the_host(k256, polarity):
    """Every size in one arena, the page narrower and lower than the window among them (5 x 7 at r = 31)."""
    pages = [R.random_grey(r, c, seed=3 * k + k256) for k, (r, c) in enumerate(SIZES)]
    for radius in (1, 31):
        out = _binarize(pages, radius=radius, k256=k256, polarity=polarity)
        assert (out == 0).any() and (out == 255).any()


def test_pages_of_different_sizes_with_row_strides():
    pages = [R.random_grey(B_R + 3, S_C + 9, seed=1), R.random_grey(2 * B_R + 1, 37, seed=2), np.full((9, 70), 131, np.uint8),
             _feature_page(40, 300, [(10, 20), (30, 290)], seed=3)]
    for radius in (2, 15):
        _binarize(pages, strides=[S_C + 9 + 7, 64, 70, 301], radius=radius)
    out = _binarize(pages[2:3], strides=[75], radius=15)
    assert (out == 0).sum() == 0                             # a constant page has no ink


# ---- 2. windows across workgroup borders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 31])
def test_features_across_strip_and_band_borders(radius):
    """A dark feature across each strip border, each band border and their corners; on the small page a window at r = 31 spans the workgroup
    border and is clipped at the page edge at once, on the big one windows reach into the second strip and band from both sides."""
    big = (2 * B_R + 5, 2 * S_C + 1)
    at_big = [(10, S_C - 2), (20, 2 * S_C - 2), (B_R - 2, 30), (2 * B_R - 2, 50), (B_R - 2, S_C - 2), (2 * B_R - 2, 2 * S_C - 2),
              (B_R - 2, 2 * S_C - 2), (2 * B_R - 2, S_C - 2), (-2, S_C - 3), (B_R - 3, -2), (2 * B_R + 2, 2 * S_C - 1)]
    small = (B_R + 5, S_C + 7)
    at_small = [(B_R - 2, S_C - 2), (0, S_C - 1), (B_R - 1, 0), (B_R + 1, S_C + 3)]
    pages = [_feature_page(*big, at_big, seed=7), _feature_page(*small, at_small, seed=8), 255 - _feature_page(*small, at_small, seed=9)]
    out = _binarize(pages, radius=radius)
    assert (out == 0).any()
    _binarize(pages[2:], radius=radius, polarity=2, k256=128)


def test_extremes_of_the_arithmetic():
    """0 / 255 over full windows at r = 31, k256 = 255: the largest D and the largest products, over a strip border and two band borders."""
    pages = [R.checkerboard(130, S_C + 8), R.half_page(130, 2 * S_C), R.half_page(S_C + 8, 130).T.copy(), R.one_dark_pixel(70, 200, (B_R, S_C))]
    for polarity in (1, 2):
        _binarize(pages, polarity=polarity, **R.EXTREME)


# ---- 3. the refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    pages = [R.random_grey(B_R + 3, S_C + 9, seed=1), R.random_grey(5, 7, seed=2)]
    arena, table, inside = _arena(pages)
    both = torch.full((2 * arena.size + GUARD,), 0x33, dtype=torch.uint8, device="cuda")      # the arena and the output in one allocation
    arena_dev, out = both[:arena.size], both[arena.size:]
    arena_dev.copy_(torch.from_numpy(arena))
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    good = dict(radius=3, k256=51, polarity=1)

    def refused(code, table=table, n=2, arena_bytes=arena.size, out=out, out_bytes=arena.size, prm={}, null=None):
        got = _call(arena_dev, arena_bytes, table, table_dev, n, B.crnn_binarize_params(**dict(good, **prm)), out, out_bytes, null=null)
        assert got == code, "expected %d, got %d" % (code, got)
        assert (host(both[arena.size:]) == 0x33).all() and np.array_equal(host(arena_dev), arena)

    def edited(k, **fields):
        t = table.copy()
        for name, v in fields.items():
            t[name][k] = v
        return t
    for name in ("arena", "pages", "pages_dev", "prm", "out"):
        refused(-2, null=name)
    refused(-2, n=-1)
    refused(0, n=0)                                                                  # n_pages == 0 launches nothing
    for bad in (dict(radius=0), dict(radius=32), dict(radius=-1), dict(k256=-1), dict(k256=256), dict(polarity=0), dict(polarity=3)):
        refused(-2, prm=bad)
    refused(-2, table=edited(0, rows=4097))                                          # a page above 4096 in either dimension
    refused(-2, table=edited(1, cols=4097, stride=4097))
    refused(-2, table=edited(0, rows=0))
    refused(-2, table=edited(1, cols=0))
    refused(-2, table=edited(0, stride=S_C + 8))                                     # stride < cols
    refused(-2, table=edited(1, page_off=-16))
    refused(-2, table=edited(1, page_off=arena.size))                                # a page table entry that does not fit the arena
    refused(-2, table=edited(1, page_off=int(table["page_off"][1]) + 16))
    refused(-2, arena_bytes=int(table["page_off"][1]) + 5 * 7 - 1)                   # ... the input arena one byte short
    refused(-2, out_bytes=int(table["page_off"][1]) + 5 * 7 - 1)                     # ... the output arena one byte short
    refused(-2, arena_bytes=0)
    refused(-2, out_bytes=0)
    refused(-2, out=arena_dev)                                                       # input and output ranges that overlap: the same range,
    refused(-2, out=both[arena.size - 1:], out_bytes=arena.size)                     # the output begins on the input's last byte,
    refused(-2, out=both[1:], out_bytes=arena.size)                                  # and one byte into the input
    assert _call(arena_dev, arena.size, table, table_dev, 2, B.crnn_binarize_params(**good), out, arena.size) == 0   # adjacent ranges do not overlap
    got = host(out)
    assert (got[arena.size:] == 0x33).all() and (got[:arena.size][~inside] == 0x33).all() and np.array_equal(host(arena_dev), arena)
    for k, pg in enumerate(pages):
        off = int(table["page_off"][k])
        assert np.array_equal(got[off:off + pg.size].reshape(pg.shape), B.sauvola_host(pg, **good))


# ---- 4. the surface -----------------------------------------------------------------------------------------------------------------------------------------
def test_binarizer_returns_a_new_arena_and_leaves_the_input():
    pages = [R.shaded_page()[0], R.random_grey(33, 50, seed=4), R.random_grey(1, 1, seed=5)]
    ing = U.DeviceIngest((100, 32, 1))
    arena = ing.upload(pages)
    before = host(arena.dev).copy()
    for kw in (dict(), dict(radius=7, k256=128, polarity=2)):
        made = U.Binarizer(**kw).run(None, arena=arena)
        assert made is not arena and made.dev.data_ptr() != arena.dev.data_ptr() and made.dev.is_cuda and made.host is None
        assert made.offsets == arena.offsets and made.nbytes == arena.nbytes and [p.shape for p in made.pages] == [p.shape for p in pages]
        want, _ = pack_arena([B.sauvola_host(pg, **kw) for pg in pages])
        assert np.array_equal(host(made.dev)[:arena.nbytes], want)
        assert np.array_equal(host(arena.dev), before)
    again = U.Binarizer().run(pages)                                                  # pages in, uploaded here
    assert np.array_equal(host(again.dev), host(U.Binarizer().run(None, arena=arena).dev))
    assert U.Binarizer().run([]).pages == []


def test_word_detector_finds_the_words_of_the_shaded_page():
    page, rects = R.shaded_page()
    other = R.random_grey(50, 90, seed=6)
    for adaptive in (dict(radius=7), dict(radius=15), dict(radius=31), True):
        det = U.WordDetector(gap_x=8, adaptive=adaptive)
        found = det.detect([page, other])
        for pg, (got, info) in zip((page, other), found):
            want, winfo = D.detect_words_host(pg, gap_x=8, cap=1024, adaptive=adaptive)
            assert np.array_equal(got, want) and info.tolist() == winfo.tolist()
        assert np.array_equal(found[0][0][:, :4], rects) and found[0][1].tolist() == [32, 32, 127, 1]
    light = U.WordDetector(gap_x=8, adaptive=dict(polarity=2)).detect([255 - page])[0]
    assert np.array_equal(light[0][:, :4], rects)
    # without `adaptive` nothing has moved: today's host result, which is not the 32 words
    got, info = U.WordDetector(gap_x=8).detect([page])[0]
    want, winfo = D.detect_words_host(page, gap_x=8, cap=1024)
    assert np.array_equal(got, want) and info.tolist() == winfo.tolist() and len(got) != 32
    for bad in (dict(threshold=127), dict(polarity=1)):
        with pytest.raises(ValueError):
            U.WordDetector(adaptive=True, **bad)


def test_boxes_come_from_the_binarised_arena_and_crops_from_the_grey_one():
    page, rects = R.shaded_page()
    pages = [page, R.shaded_page(seed=1)[0][:100, :330].copy()]
    ing = U.DeviceIngest((100, 32, 1))
    det = U.WordDetector(gap_x=8, adaptive=dict(radius=15))
    arena = ing.upload(pages)
    before = host(arena.dev).copy()
    boxes = det.boxes(None, arena=arena)
    assert np.array_equal(host(arena.dev), before)                                   # the detector binarised into an arena of its own
    assert boxes[0] == D.to_boxes(rects) and len(boxes[1]) == 8
    index = [k for k, bl in enumerate(boxes) for _ in bl]
    crops = [U.box_slices(b, pages[k].shape) for k, bl in enumerate(boxes) for b in bl]
    shared = ing.crops(None, index, crops, ing.plan(crops), arena=arena)
    plain, _ = ing.pages(pages, boxes)                                               # crops cut from the original pages at those boxes
    assert shared.shape == (40, 100, 32, 1) and torch.equal(shared, plain)
    binary, _ = ing.pages([B.sauvola_host(pg) for pg in pages], boxes)
    assert not torch.equal(shared, binary)                                           # ... and not from the binarised ones
