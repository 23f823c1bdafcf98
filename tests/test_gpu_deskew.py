"""-m gpu tests of page deskew on the device (csrc/deskew.hip, crnn_mi355x/deskew.py).  Every case calls the entry point twice on outputs
pre-filled with two different sentinels (the estimate also on a workspace poisoned with two different bytes) and asserts that the two calls agree
bit for bit, that scores and indices equal estimate_skew_host and the page bytes rotate_host (both pinned to a brute-force restatement in
tests/test_deskew_cpu.py), that the input arena is unchanged and that every byte outside the outputs -- row padding, the bytes between pages,
the guard regions -- still holds its sentinel.  Everything is integer: every comparison is exact equality.  Shapes are the smallest at which the
kernels take every path: one-pixel, one-row and one-column pages, pages of several strip groups and bands that end off the grid
(deskew.STRIPS * 64 columns x deskew.BAND_R rows), ink across their borders, the longest pages at the steepest slope."""
import ctypes

import numpy as np
import pytest
import torch

import utils as U
from crnn_mi355x import deskew as K, detect as D
from crnn_mi355x.pages import pack_arena
from gpu_util import L, P, S, host, sentinel_arena as _arena
import deskew_ref as R

pytestmark = pytest.mark.gpu

GROUP_C, BAND_R = 64 * K.STRIPS, K.BAND_R
SENTINELS = (0x33, 0xc4)
GUARD = 256


def _prm(**kw):
    return K.crnn_deskew_params(**dict(K.DEFAULTS, **kw))


def _need(table, n, prm):
    return L().crnn_deskew_workspace_bytes(table.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(prm))


def _call_estimate(arena_dev, arena_bytes, table, table_dev, n, prm, index, scores, ws, ws_bytes, null=None):
    args = dict(arena=P(arena_dev), pages=table.ctypes.data_as(ctypes.c_void_p), pages_dev=P(table_dev), prm=ctypes.byref(prm), index=P(index),
                scores=P(scores), ws=P(ws))
    if null:
        args[null] = ctypes.c_void_p(0)
    code = L().crnn_deskew_estimate(args["arena"], arena_bytes, args["pages"], args["pages_dev"], n, args["prm"], args["index"], args["scores"],
                                    args["ws"], ws_bytes, S())
    torch.cuda.synchronize()
    return code


def _call_rotate(arena_dev, arena_bytes, table, table_dev, n, index_dev, prm, out, out_bytes, null=None):
    args = dict(arena=P(arena_dev), pages=table.ctypes.data_as(ctypes.c_void_p), pages_dev=P(table_dev), index=P(index_dev), prm=ctypes.byref(prm),
                out=P(out))
    if null:
        args[null] = ctypes.c_void_p(0)
    code = L().crnn_rotate_pages(args["arena"], arena_bytes, args["pages"], args["pages_dev"], n, args["index"], args["prm"], args["out"],
                                 out_bytes, S())
    torch.cuda.synchronize()
    return code


def _estimate(pages, strides=None, **kw):
    """Two calls -> [(index, scores)] per page, equal between the calls and equal to estimate_skew_host; sentinels intact around the outputs."""
    prm = _prm(**kw)
    n, nc = len(pages), 2 * prm.steps + 1
    arena, table, _ = _arena(pages, strides)
    arena_dev, table_dev = torch.from_numpy(arena).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()
    need = _need(table, n, prm)
    assert need >= n * 1088
    runs = []
    for fill in SENTINELS:
        index = torch.full((4 * n + GUARD,), fill, dtype=torch.uint8, device="cuda")
        scores = torch.full((8 * n * nc + GUARD,), fill, dtype=torch.uint8, device="cuda")
        ws = torch.full((need + GUARD,), fill ^ 0xff, dtype=torch.uint8, device="cuda")      # poisoned: the workspace owes no zeroing
        code = _call_estimate(arena_dev, arena.size, table, table_dev, n, prm, index, scores, ws, need)
        assert code == 0, "crnn_deskew_estimate returned %d" % code
        gi, gs = host(index), host(scores)
        assert (gi[4 * n:] == fill).all() and (gs[8 * n * nc:] == fill).all(), "a guard region past the outputs was written"
        assert (host(ws)[need:] == fill ^ 0xff).all(), "the guard region past the workspace was written"
        runs.append((gi[:4 * n].view(np.int32).copy(), gs[:8 * n * nc].view(np.int64).reshape(n, nc).copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "two calls disagree"
    assert np.array_equal(host(arena_dev), arena), "the input arena was written"
    for k, pg in enumerate(pages):
        windex, wscores = K.estimate_skew_host(pg, prm.threshold, prm.polarity, prm.steps, prm.slope_step)
        bad = np.flatnonzero(runs[0][1][k] != wscores)
        assert bad.size == 0, "page %d %s %r: %d scores differ from the host's, the first at candidate %d: %d, not %d" % (
            k, pg.shape, kw, bad.size, bad[0] - prm.steps, runs[0][1][k][bad[0]], wscores[bad[0]])
        assert runs[0][0][k] == windex, "page %d %s %r: index %d, the host's is %d" % (k, pg.shape, kw, runs[0][0][k], windex)
    return [(int(runs[0][0][k]), runs[0][1][k]) for k in range(n)]


def _rotate(pages, indices, strides=None, **kw):
    """Two calls -> the output arena's bytes: equal between the calls, the pages equal to rotate_host, sentinels intact elsewhere."""
    prm = _prm(**kw)
    arena, table, inside = _arena(pages, strides)
    arena_dev, table_dev = torch.from_numpy(arena).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()
    index_dev = torch.tensor(list(indices), dtype=torch.int32, device="cuda")
    outs = []
    for fill in SENTINELS:
        out = torch.full((arena.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
        code = _call_rotate(arena_dev, arena.size, table, table_dev, len(pages), index_dev, prm, out, arena.size)
        assert code == 0, "crnn_rotate_pages returned %d" % code
        got = host(out)
        assert (got[arena.size:] == fill).all(), "the guard region past the arena was written"
        assert (got[:arena.size][~inside] == fill).all(), "a byte outside the pages' rows x cols was written"
        outs.append(got[:arena.size])
    assert np.array_equal(outs[0][inside], outs[1][inside]), "two calls disagree"
    assert np.array_equal(host(arena_dev), arena), "the input arena was written"
    assert host(index_dev).tolist() == list(indices)
    for k, pg in enumerate(pages):
        off, st = int(table["page_off"][k]), int(table["stride"][k])
        got = outs[0][off:off + (pg.shape[0] - 1) * st + pg.shape[1]]
        got = np.concatenate([got, np.zeros(pg.shape[0] * st - got.size, np.uint8)]).reshape(pg.shape[0], st)[:, :pg.shape[1]]
        a = indices[k] if abs(indices[k]) <= prm.steps else 0                   # an index outside -steps .. steps rotates by 0
        diff = np.argwhere(got != K.rotate_host(pg, a, prm.slope_step, prm.fill))
        assert diff.size == 0, "page %d %s index %d %r: %d pixels differ from the host's, the first at %s" % (
            k, pg.shape, indices[k], kw, len(diff), diff[0].tolist())
    return outs[0]


def _lines_page(rows, cols, slope, seed, at=()):
    """Light paper with a little noise, dark 3-pixel lines every 11 rows drawn at `slope` through the page's centre column, and dark 5 x 12
    features whose top left corners are `at` (clipped to the page)."""
    rs = np.random.RandomState(seed)
    page = rs.randint(200, 256, (rows, cols)).astype(np.uint8)
    r, c = np.indices((rows, cols))
    page[((r - np.floor((c - cols // 2) * slope).astype(np.int64)) % 11) < 3] = 20
    for y, x in at:
        page[max(y, 0):y + 5, max(x, 0):x + 12] = 10
    return page


# ---- 1. the estimate ------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 257), (257, 1), (5, 7), (70, 130)]


@pytest.mark.parametrize("steps", [0, 1, 48, 64])
def test_estimate_of_small_pages_equals_the_host(steps):
    """Every size in one call, row strides on all of them; Otsu with the auto polarity, and a given threshold with each polarity."""
    pages = [R.sparse_ink(r, c, seed=3 * k + steps, dark=k != 3) for k, (r, c) in enumerate(SIZES)]
    strides = [16, 300, 1, 9, 133]
    _estimate(pages, strides, steps=steps)
    for polarity in (0, 1, 2):
        found = _estimate(pages, strides, steps=steps, threshold=127, polarity=polarity)
        assert any(s.any() for _, s in found)


def test_longest_pages_at_the_steepest_slope():
    """8 x 4096 and 4096 x 8 at steps * slope_step = 16384: the largest offsets (bins 512 rows outside the page) and 22 bands of rows."""
    pages = [R.sparse_ink(8, 4096, seed=1), R.sparse_ink(4096, 8, seed=2), _lines_page(8, 4096, 0.25, seed=3)]
    found = _estimate(pages, steps=16, slope_step=1024, threshold=127, polarity=1)
    assert all(s.min() > 0 for _, s in found)
    _estimate(pages[:2], steps=64, slope_step=256)


def test_ink_across_strip_group_and_band_borders():
    """Pages of two strips + 1 column, of two strip groups + 1 column and of a band + a few rows, with lines at a slope that cross every
    64-column strip, the group border and the band border, and features on the borders and their corners."""
    at = [(10, 60), (BAND_R - 2, 30), (BAND_R - 2, GROUP_C - 6), (BAND_R + 3, 2 * GROUP_C - 5), (-2, 120), (100, -3)]
    pages = [_lines_page(40, 129, 0.05, seed=4, at=at[:1]), _lines_page(BAND_R + 9, 2 * GROUP_C + 1, -0.1, seed=5, at=at),
             _lines_page(2 * BAND_R + 1, 70, 0.17, seed=6, at=at[1:2])]
    found = _estimate(pages, strides=[129, 2 * GROUP_C + 8, 71])
    assert [a > 0 for a, _ in found] == [True, False, True] and all(a != 0 for a, _ in found)   # the sign of the lines' slopes
    _estimate([255 - pages[1]], steps=64, threshold=100, polarity=2)


def test_blank_full_and_single_pixel_pages():
    one = np.full((9, 300), 255, np.uint8)
    one[4, 258] = 0
    pages = [np.full((9, 12), 255, np.uint8), np.zeros((9, 12), np.uint8), one, np.full((200, 70), 131, np.uint8)]
    found = _estimate(pages, threshold=127, polarity=1, steps=64)
    assert [a for a, _ in found] == [0, 0, 0, 0]
    assert not found[0][1].any() and found[1][1][64] == 9 * 12 * 12 and found[2][1].tolist() == [1] * 129 and not found[3][1].any()
    found = _estimate(pages)                                                           # Otsu: the constant pages have no ink
    assert [a for a, _ in found] == [0, 0, 0, 0] and not found[0][1].any() and not found[1][1].any() and not found[3][1].any()


# ---- 2. the rotation ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [-1, 0, 255])
def test_every_index_on_two_small_pages(fill):
    a, b = R.random_grey(9, 11, seed=1), R.random_grey(12, 10, seed=2)
    idx = list(range(-64, 65))
    out = _rotate([a, b] * len(idx), [i for i in idx for _ in (0, 1)], steps=64, slope_step=256, fill=fill)
    assert len(np.unique(out)) > 100


def test_longest_pages_at_the_extreme_slopes():
    """8 x 4096 and 4096 x 8 at +-0.25: the largest coordinates of the int32 arithmetic."""
    pages = [R.random_grey(8, 4096, seed=3), R.random_grey(4096, 8, seed=4)]
    for fill in (-1, 200):
        _rotate(pages + pages, [16, 16, -16, -16], steps=16, slope_step=1024, fill=fill)
    _rotate(pages, [64, -64], steps=64, slope_step=256)


def test_indices_per_page_row_strides_and_an_index_out_of_range():
    pages = [R.random_grey(70, 130, seed=5), R.random_grey(33, 65, seed=6), R.random_grey(1, 257, seed=7), R.random_grey(257, 1, seed=8),
             R.random_grey(1, 1, seed=9), R.random_grey(17, 64, seed=10), R.random_grey(20, 30, seed=11)]
    strides = [137, 80, 257, 3, 16, 64, 31]
    out = _rotate(pages, [48, -31, 7, -48, 20, 0, 49], strides, fill=9)                  # 49 > steps = 48: rotated by 0
    t = _arena(pages, strides)[1]
    assert np.array_equal(out[int(t["page_off"][5]):][:17 * 64].reshape(17, 64), pages[5])  # index 0: byte for byte
    _rotate(pages, [-2 ** 31, 2 ** 31 - 1, 65, -65, 1000, -1, 1], strides, steps=64, slope_step=256)
    _rotate(pages[:2], [1, -1], strides[:2], steps=0)                                     # steps = 0: every index but 0 is out of range


# ---- 3. the refusals --------------------------------------------------------------------------------------------------------------------------------------
BAD_PARAMS = (dict(threshold=-2), dict(threshold=255), dict(polarity=-1), dict(polarity=3), dict(steps=-1), dict(steps=65), dict(slope_step=0),
              dict(slope_step=1025), dict(steps=17, slope_step=1024), dict(steps=64, slope_step=257), dict(fill=-2), dict(fill=256))


def _edited(table, k, **fields):
    t = table.copy()
    for name, v in fields.items():
        t[name][k] = v
    return t


def test_estimate_refusals_leave_the_outputs_untouched():
    pages = [R.sparse_ink(BAND_R + 3, GROUP_C + 9, seed=1), R.sparse_ink(5, 7, seed=2)]
    arena, table, _ = _arena(pages)
    arena_dev, table_dev = torch.from_numpy(arena).cuda(), torch.from_numpy(table.view(np.uint8)).cuda()
    good = dict(steps=4)
    need = _need(table, 2, _prm(**good))
    index = torch.full((8 + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    scores = torch.full((8 * 2 * 9 + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    ws = torch.full((need + 16,), 0x33, dtype=torch.uint8, device="cuda")

    def refused(code, table=table, n=2, arena_bytes=arena.size, prm={}, ws=ws, ws_bytes=need, null=None):
        got = _call_estimate(arena_dev, arena_bytes, table, table_dev, n, _prm(**dict(good, **prm)), index, scores, ws, ws_bytes, null=null)
        assert got == code, "expected %d, got %d" % (code, got)
        assert (host(index) == 0x33).all() and (host(scores) == 0x33).all() and np.array_equal(host(arena_dev), arena)
    for name in ("arena", "pages", "pages_dev", "prm", "index", "scores", "ws"):
        refused(-2, null=name)
    refused(-2, n=-1)
    refused(0, n=0)                                                                  # P == 0 launches nothing
    for bad in BAD_PARAMS:
        refused(-2, prm=bad)
        assert _need(table, 2, _prm(**dict(good, **bad))) == 0
    refused(-3, table=_edited(table, 0, rows=4097))                                  # a page above 4096 in either direction
    refused(-3, table=_edited(table, 1, cols=4097, stride=4097))
    for bad in (dict(rows=0), dict(cols=0), dict(stride=6), dict(page_off=-16), dict(page_off=arena.size),
                dict(page_off=int(table["page_off"][1]) + 16)):                      # table entries that do not fit
        refused(-2, table=_edited(table, 1, **bad))
        assert bad.get("page_off", -1) > 0 or _need(_edited(table, 1, **bad), 2, _prm(**good)) == 0
    refused(-2, arena_bytes=int(table["page_off"][1]) + 5 * 7 - 1)                   # the arena one byte short
    refused(-2, arena_bytes=0)
    refused(-2, ws_bytes=need - 1)                                                   # a short workspace
    refused(-2, ws=ws[4:], ws_bytes=need)                                            # a misaligned one
    assert _need(table, 0, _prm(**good)) == 0 and _need(table, -1, _prm(**good)) == 0
    assert (host(ws) == 0x33).all()
    assert _call_estimate(arena_dev, arena.size, table, table_dev, 2, _prm(**good), index, scores, ws, need) == 0
    got = host(index)[:8].view(np.int32).tolist()
    assert got == [K.estimate_skew_host(pg, **good)[0] for pg in pages] and (host(index)[8:] == 0x33).all()


def test_rotate_refusals_leave_the_output_untouched():
    pages = [R.random_grey(20, 70, seed=1), R.random_grey(5, 7, seed=2)]
    arena, table, inside = _arena(pages)
    both = torch.full((2 * arena.size + GUARD,), 0x33, dtype=torch.uint8, device="cuda")      # the arena and the output in one allocation
    arena_dev, out = both[:arena.size], both[arena.size:]
    arena_dev.copy_(torch.from_numpy(arena))
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    index_dev = torch.tensor([3, -4], dtype=torch.int32, device="cuda")
    good = dict(steps=4, fill=0)

    def refused(code, table=table, n=2, arena_bytes=arena.size, out=out, out_bytes=arena.size, prm={}, null=None):
        got = _call_rotate(arena_dev, arena_bytes, table, table_dev, n, index_dev, _prm(**dict(good, **prm)), out, out_bytes, null=null)
        assert got == code, "expected %d, got %d" % (code, got)
        assert (host(both[arena.size:]) == 0x33).all() and np.array_equal(host(arena_dev), arena)
    for name in ("arena", "pages", "pages_dev", "index", "prm", "out"):
        refused(-2, null=name)
    refused(-2, n=-1)
    refused(0, n=0)
    for bad in BAD_PARAMS:
        refused(-2, prm=bad)
    refused(-3, table=_edited(table, 0, rows=4097))
    refused(-3, table=_edited(table, 1, cols=4097, stride=4097))
    for bad in (dict(rows=0), dict(cols=0), dict(stride=6), dict(page_off=-16), dict(page_off=arena.size),
                dict(page_off=int(table["page_off"][1]) + 16)):
        refused(-2, table=_edited(table, 1, **bad))
    refused(-2, arena_bytes=int(table["page_off"][1]) + 5 * 7 - 1)                   # the input arena one byte short
    refused(-2, out_bytes=int(table["page_off"][1]) + 5 * 7 - 1)                     # the output arena one byte short
    refused(-2, arena_bytes=0)
    refused(-2, out_bytes=0)
    refused(-2, out=arena_dev)                                                       # input and output ranges that overlap: the same range,
    refused(-2, out=both[arena.size - 1:], out_bytes=arena.size)                     # the output begins on the input's last byte,
    refused(-2, out=both[1:], out_bytes=arena.size)                                  # and one byte into the input
    assert _call_rotate(arena_dev, arena.size, table, table_dev, 2, index_dev, _prm(**good), out, arena.size) == 0   # adjacent ranges do not overlap
    got = host(out)
    assert (got[arena.size:] == 0x33).all() and (got[:arena.size][~inside] == 0x33).all() and np.array_equal(host(arena_dev), arena)
    for k, pg in enumerate(pages):
        off = int(table["page_off"][k])
        assert np.array_equal(got[off:off + pg.size].reshape(pg.shape), K.rotate_host(pg, [3, -4][k], fill=0))


# ---- 4. the surface -----------------------------------------------------------------------------------------------------------------------------------------
def test_deskewer_returns_a_new_arena_and_leaves_the_input():
    pages = [R.skewed_page(0.07, False)[0], _lines_page(33, 50, -0.1, seed=4), R.random_grey(1, 1, seed=5), R.skewed_page(0.15, True)[0]]
    ing = U.DeviceIngest((100, 32, 1))
    arena = ing.upload(pages)
    before = host(arena.dev).copy()
    for kw in (dict(), dict(adaptive=dict(radius=15)), dict(steps=20, slope_step=512, fill=255, threshold=128, polarity=1)):
        made = U.Deskewer(**kw).run(None, arena=arena)
        assert made is not arena and made.dev.data_ptr() != arena.dev.data_ptr() and made.dev.is_cuda and made.host is None
        assert made.offsets == arena.offsets and made.nbytes == arena.nbytes and [p.shape for p in made.pages] == [p.shape for p in pages]
        want = [K.deskew_host(pg, **kw) for pg in pages]
        assert made.index.is_cuda and made.index.dtype == torch.int32 and host(made.index).tolist() == [a for _, a in want]
        assert np.array_equal(host(made.dev)[:arena.nbytes], pack_arena([pg for pg, _ in want])[0])
        assert np.array_equal(host(arena.dev), before)
        est = U.Deskewer(**kw).estimate(None, arena=arena)
        for pg, (a, scores), (_, wa) in zip(pages, est, want):
            hk = {k: v for k, v in kw.items() if k != "fill"}
            assert a == wa and scores.dtype == np.int64 and np.array_equal(scores, K.estimate_skew_host(pg, **hk)[1])
        assert np.array_equal(host(arena.dev), before)
    assert host(U.Deskewer().run(None, arena=arena).index).tolist()[0] == 18          # 0.07 is nearest to 18 / 256
    again = U.Deskewer().run(pages)                                                   # pages in, uploaded here
    assert np.array_equal(host(again.dev), host(U.Deskewer().run(None, arena=arena).dev))
    empty = U.Deskewer().run([])
    assert empty.pages == [] and empty.index.numel() == 0 and U.Deskewer().estimate([]) == []
    for bad in (dict(threshold=127), dict(polarity=1)):
        with pytest.raises(ValueError):
            U.Deskewer(adaptive=True, **bad)
    with pytest.raises(TypeError):
        U.Deskewer(radius=3)
    with pytest.raises(ValueError):
        U.Deskewer(steps=65)


def test_detector_and_ingest_read_the_deskewed_arena():
    """The shaded page at a slope of -0.12: the unchanged detector on the deskewed arena returns exactly the host's boxes of the host's
    deskewed page -- the 28 drawn words, line by line -- and the crops are cut from the deskewed grey page."""
    adaptive = dict(radius=15)
    page, rects = R.skewed_page(-0.12, True)
    other = R.skewed_page(0.02, True)[0][:100, :330].copy()
    ing = U.DeviceIngest((100, 32, 1))
    arena = ing.upload([page, other])
    before = host(arena.dev).copy()
    flat = U.Deskewer(adaptive=adaptive).run(None, arena=arena)
    flat_host = [K.deskew_host(pg, adaptive=adaptive) for pg in (page, other)]
    assert host(flat.index).tolist() == [a for _, a in flat_host] and flat_host[0][1] == -31
    det = U.WordDetector(gap_x=8, adaptive=adaptive)
    read, run = [], det._binarizer.run
    det._binarizer.run = lambda pages, arena=None: read.append(run(pages, arena=arena)) or read[-1]   # the binarised arena the detector reads
    for (got, info), (pg, _) in zip(det.detect(None, arena=flat), flat_host):
        want, winfo = D.detect_words_host(pg, gap_x=8, cap=1024, adaptive=adaptive)
        assert np.array_equal(got, want) and info.tolist() == winfo.tolist()
    # one page table for the upload and everything derived from it: the same host array and the same device tensor, copied once
    assert len(read) == 1 and read[0] is not flat and read[0].dev.data_ptr() != flat.dev.data_ptr()
    assert arena.table_dev.is_cuda and flat.table_dev is arena.table_dev and read[0].table_dev is arena.table_dev
    assert flat.table is arena.table and read[0].table is arena.table
    boxes = det.boxes(None, arena=flat)
    assert len(boxes[0]) == 28 and np.abs(np.array([[b[1], b[3], b[2], b[4]] for b in boxes[0]]) - rects).max() <= 1
    raw = det.boxes(None, arena=arena)[0]                                             # the raw page: 28 boxes, but taller and out of order
    assert len(raw) == 28 and max(b[3] - b[1] for b in raw) > 20 >= max(b[3] - b[1] for b in boxes[0])
    assert np.array_equal(host(arena.dev), before)
    index = [k for k, bl in enumerate(boxes) for _ in bl]
    crops = [U.box_slices(b, flat.pages[k].shape) for k, bl in enumerate(boxes) for b in bl]
    shared = ing.crops(None, index, crops, ing.plan(crops), arena=flat)
    plain, _ = ing.pages([pg for pg, _ in flat_host], boxes)                          # crops cut from the host's deskewed pages at those boxes
    assert shared.shape[0] == len(index) > 28 and torch.equal(shared, plain)
    skewed, _ = ing.pages([page, other], boxes)
    assert not torch.equal(shared, skewed)                                            # ... and not from the pages as they came
