"""CPU tests (no GPU) of the device ingest's host half (crnn_mi355x/ingest.py): plan_crop against data.open_img -- same placement, same
draws from np.random --, the box -> slice rule, the arena / table packing, a NumPy restatement of what the kernel computes from one table
entry, and the entry point's declaration, export and argument checks (those return before anything is launched)."""
import ctypes

import numpy as np
import pytest

import utils as U
from crnn_mi355x import data as D
from crnn_mi355x import ingest as I
from crnn_mi355x import native
from crnn_mi355x import pages as PG

# crop shapes (hc rows, wc columns); the rotated crop is (wc, hc).  Axis 0 (time, target T0): 1, T0//2 and T0//2 + 1 (the up-scale rule),
# T0 - size in {3, 2, 1, 0}, size > T0; axis 1 (target T1) the same.  The product also holds "larger on one axis" and "on both".
HCS = {(100, 32): [1, 2, 16, 17, 20, 29, 30, 31, 32, 40], (200, 32): [1, 16, 17, 29, 30, 32, 40], (40, 32): [1, 16, 17, 29, 30, 32, 40]}
WCS = {(100, 32): [1, 2, 33, 50, 51, 66, 97, 98, 99, 100, 130], (200, 32): [1, 100, 101, 197, 198, 200, 230], (40, 32): [1, 20, 21, 37, 38, 40, 55]}


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _rebuild(crop, img_size, up, size, place):
    """open_img's result from a plan, with NumPy: rotate, fill value, optional up-scale, placement, inversion, squash."""
    (s0, s1), (b0, b1, p0, p1) = size, place
    rot = crop[::-1].T
    fill = D._modal_value(rot)
    content = D.resize_linear(rot, (s1, s0)) if up else rot
    assert content.shape == (s0, s1)
    padded = np.full((p0, p1), fill, np.uint8)
    padded[b0:b0 + s0, b1:b1 + s1] = content
    hi = int((padded > 127).sum())
    tie = 2 * hi == padded.size
    if hi > padded.size - hi:
        padded = (255 - padded).astype(np.uint8)
    return D.resize_linear(padded, (img_size[1], img_size[0])), tie


@pytest.mark.parametrize("p", [0., 0.7, 1.0])
@pytest.mark.parametrize("shape", [(100, 32), (200, 32), (40, 32)])
def test_plan_crop_places_and_draws_as_open_img(shape, p):
    img_size = shape + (1,)
    rs = np.random.RandomState(3)
    k = 0
    for hc in HCS[shape]:
        for wc in WCS[shape]:
            for bright in (False, True):
                k += 1
                crop = rs.randint(0, 256, (hc, wc)).astype(np.uint8)
                crop = np.maximum(crop, 140) if bright else crop
                np.random.seed(k)
                ref = D.open_img(crop, img_size, p=p)[0]
                after_ref = np.random.get_state()
                np.random.seed(k)
                up, size, place = I.plan_crop(hc, wc, img_size, p=p)
                after_plan = np.random.get_state()
                assert _state_equal(after_ref, after_plan), (hc, wc, p)
                got, _ = _rebuild(crop, img_size, up, size, place)
                assert got.dtype == np.uint8 and np.array_equal(got, ref), (hc, wc, p, up, size, place)


def test_plan_crops_equals_plan_crop_at_p0():
    for shape in HCS:
        hc, wc = [a.ravel() for a in np.meshgrid(HCS[shape], WCS[shape], indexing="ij")]
        np.random.seed(11)
        one = [I.plan_crop(int(h), int(w), shape + (1,), p=0.) for h, w in zip(hc, wc)]
        after_one = np.random.get_state()
        np.random.seed(11)
        up, s0, s1, b0, b1, p0, p1 = I.plan_crops(hc, wc, shape + (1,))
        assert _state_equal(after_one, np.random.get_state())
        for k, (u, s, o) in enumerate(one):
            assert (bool(up[k]), (int(s0[k]), int(s1[k])), (int(b0[k]), int(b1[k]), int(p0[k]), int(p1[k]))) == (bool(u), s, o)


def test_box_slices_follow_python_slicing():
    page = np.arange(40 * 50).reshape(40, 50)
    vals = [None, -60, -41, -40, -7, -1, 0, 1, 5, 39, 40, 41, 49, 50, 51, 90]
    rs = np.random.RandomState(0)
    seen_empty = seen_full = 0
    for _ in range(3000):
        b = ("w",) + tuple(vals[i] for i in rs.randint(0, len(vals), 4))
        ref = page[b[1]:b[3], b[2]:b[4]]
        if ref.size == 0:
            seen_empty += 1
            with pytest.raises(ValueError):
                I.box_slices(b, page.shape)
            continue
        r0, r1, c0, c1 = I.box_slices(b, page.shape)
        assert 0 <= r0 < r1 <= 40 and 0 <= c0 < c1 <= 50 and np.array_equal(page[r0:r1, c0:c1], ref), b
        seen_full += 1
    assert seen_empty > 100 and seen_full > 100
    assert I.box_slices((None, np.int64(3), np.int32(-9), 30, 45), page.shape) == (3, 30, 41, 45)      # reversed / negative bounds, NumPy integers
    with pytest.raises(ValueError):
        I.box_slices((None, 30, 5, 3, 45), page.shape)


def _table_for(pages, index, rects, img_size, p=0.):
    rects = np.asarray(rects).reshape(-1, 4)
    rows = [(up, s[0], s[1]) + o for up, s, o in (I.plan_crop(int(r[1] - r[0]), int(r[3] - r[2]), img_size, p=p) for r in rects)]
    plans = tuple(np.array(c) for c in zip(*rows))
    arena, offs = PG.pack_arena(pages)
    return arena, offs, I.build_table(pages, offs, index, rects, plans, img_size)


def test_arena_and_table_round_trip():
    rs = np.random.RandomState(1)
    pages = [rs.randint(0, 256, s).astype(np.uint8) for s in ((37, 61), (5, 3), (64, 128))]
    pages[2] = pages[2][:, ::2]                                       # a non-contiguous view is packed row-major
    index = [0, 2, 1, 2, 0]
    rects = [(0, 37, 0, 61), (3, 20, 7, 40), (0, 5, 0, 3), (10, 11, 20, 21), (30, 37, 1, 60)]
    arena, offs, tab = _table_for(pages, index, rects, (100, 32, 1))
    assert tab.dtype.itemsize == ctypes.sizeof(I.crnn_crop_item) == 88 and arena.dtype == np.uint8
    assert all(o % 16 == 0 for o in offs) and len(arena) >= sum(p.size for p in pages)
    raw = (I.crnn_crop_item * len(tab)).from_buffer_copy(tab.tobytes())      # the bytes as the C side reads them
    for k, (pi, (r0, r1, c0, c1)) in enumerate(zip(index, rects)):
        it, pg = raw[k], pages[pi]
        assert (it.rows, it.cols, it.stride) == (pg.shape[0], pg.shape[1], pg.shape[1]) and it.page_off == offs[pi]
        back = arena[it.page_off:it.page_off + it.rows * it.stride].reshape(it.rows, it.stride)
        assert np.array_equal(back, pg) and np.array_equal(back[it.r0:it.r1, it.c0:it.c1], pg[r0:r1, c0:c1])
        up, (s0, s1), (b0, b1, p0, p1) = I.plan_crop(r1 - r0, c1 - c0, (100, 32, 1))
        assert (it.upscale, it.b0, it.b1, it.p0, it.p1) == (int(up), b0, b1, p0, p1)
        assert it.out_scale0 == p0 / float(100) and it.out_scale1 == p1 / float(32)
        if up:
            assert it.up_scale0 == (c1 - c0) / float(s0) and it.up_scale1 == (r1 - r0) / float(s1)
    with pytest.raises(ValueError):
        PG.pack_arena([np.zeros((3, 3), np.float32)])
    assert np.array_equal(I.norm_table(True, 118.5, 36.25), D.norm(np.arange(256, dtype=np.uint8), 118.5, 36.25))
    assert np.array_equal(I.norm_table(False), np.arange(256, dtype=np.float32)) and I.norm_table().dtype == np.float32


def _taps(n_out, scale, n_in):
    pos = (np.arange(n_out) + 0.5) * scale - 0.5
    lo = np.floor(pos)
    f = pos - lo
    f[(lo < 0) | (lo >= n_in - 1)] = 0.0
    lo = lo.astype(np.int64)
    return np.clip(lo, 0, n_in - 1), np.clip(lo + 1, 0, n_in - 1), f


def _resample(get, n0, n1, sc0, sc1, in0, in1):
    y0, y1, fy = _taps(n0, sc0, in0)
    x0, x1, fx = _taps(n1, sc1, in1)
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    top = get(Y0, X0) * (1 - fx) + get(Y0, X1) * fx
    bot = get(Y1, X0) * (1 - fx) + get(Y1, X1) * fx
    out = top * (1 - fy)[:, None] + bot * fy[:, None]
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


def _from_table_entry(arena, it, T0, T1):
    """What csrc/ingest.hip computes from one crnn_crop_item, pixel by pixel, without ever forming the rotated or padded image."""
    page = arena[it["page_off"]:it["page_off"] + it["rows"] * it["stride"]].reshape(it["rows"], it["stride"])
    r0, c0, hc, wc = int(it["r0"]), int(it["c0"]), int(it["r1"] - it["r0"]), int(it["c1"] - it["c0"])
    rot = lambda i, j: page[r0 + hc - 1 - j, c0 + i].astype(np.float64)
    hist = np.bincount(page[r0:r0 + hc, c0:c0 + wc].ravel(), minlength=256)
    fill = int(hist.argmax())
    s0, s1, bright, up = wc, hc, int(hist[128:].sum()), None
    if it["upscale"]:
        s0, s1 = (3 * wc) >> 1, (3 * hc) >> 1
        up = _resample(rot, s0, s1, it["up_scale0"], it["up_scale1"], wc, hc)
        bright = int((up > 127).sum())
    b0, b1, p0, p1 = int(it["b0"]), int(it["b1"]), int(it["p0"]), int(it["p1"])
    hi = bright + (p0 * p1 - s0 * s1 if fill > 127 else 0)
    inv = hi > p0 * p1 - hi

    def padded(i, j):
        i, j = np.broadcast_arrays(i - b0, j - b1)
        inside = (i >= 0) & (i < s0) & (j >= 0) & (j < s1)
        ci, cj = np.clip(i, 0, s0 - 1), np.clip(j, 0, s1 - 1)
        v = np.where(inside, up[ci, cj] if up is not None else rot(ci, cj), fill).astype(np.float64)
        return 255 - v if inv else v
    return _resample(padded, T0, T1, it["out_scale0"], it["out_scale1"], p0, p1)


@pytest.mark.parametrize("shape", [(100, 32), (40, 32)])
def test_table_entry_determines_open_img(shape):
    """The table carries everything: evaluating one entry per output pixel reproduces open_img (any placement plan_crop can draw)."""
    rs = np.random.RandomState(2)
    page = rs.randint(0, 256, (180, 260)).astype(np.uint8)
    page[:, :130] = np.maximum(page[:, :130], 150)                   # bright half: inverted crops
    page[60:90] = np.where((np.arange(260) + np.arange(60, 90)[:, None]) % 2 == 0, 127, 128)     # two grey levels, a modal tie at the threshold
    rects, k = [], 0
    for hc in HCS[shape]:
        for wc in WCS[shape]:
            k += 1
            r0, c0 = (k * 37) % (180 - hc + 1), (k * 53) % (260 - wc + 1)
            rects.append((r0, r0 + hc, c0, c0 + wc))
    rects += [(0, 180, 0, 260), (60, 90, 10, 110)]
    for p in (0., 0.7):
        np.random.seed(4)
        arena, offs, tab = _table_for([page], [0] * len(rects), rects, shape + (1,), p=p)
        np.random.seed(4)
        for it, (r0, r1, c0, c1) in zip(tab, rects):
            ref = D.open_img(page[r0:r1, c0:c1], shape + (1,), p=p)[0]
            assert np.array_equal(_from_table_entry(arena, it, *shape), ref), (r0, r1, c0, c1, p)


def test_header_declares_and_library_exports_the_entry_point():
    decl = native.parse_header()
    assert "crnn_ingest_crops" in decl
    ret, args = decl["crnn_ingest_crops"]
    assert ret is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 4
    assert hasattr(ctypes.CDLL(native.LIB_PATH), "crnn_ingest_crops")
    assert "ingest.hip" in native.SOURCES
    assert U.DeviceIngest is I.DeviceIngest and U.DeviceReadf is I.DeviceReadf and U.plan_crop is I.plan_crop
    assert issubclass(U.DeviceReadf, U.Readf)


def test_entry_point_rejects_bad_arguments_before_launching():
    """Every check of crnn_ingest_crops runs on the host before the launch, so the rejections need no GPU (the pointers are never followed)."""
    L = native.lib()
    page = np.full((50, 80), 9, np.uint8)
    arena, offs, tab = _table_for([page], [0, 0], [(0, 50, 0, 80), (5, 20, 10, 70)], (100, 32, 1))
    fake = ctypes.c_void_p(1 << 20)         # stands for a device pointer

    def call(t=tab, arena_p=fake, arena_bytes=len(arena), items_dev=fake, n=2, batch=4, imgh=100, imgw=32, table=fake, out=fake):
        return L.crnn_ingest_crops(arena_p, arena_bytes, None if t is None else t.ctypes.data_as(ctypes.c_void_p), items_dev, n, batch, imgh, imgw,
                                   table, out, None, None)

    def changed(**kw):
        t = tab.copy()
        for k, v in kw.items():
            t[k][1] = v
        return t
    assert call(n=-1) == -2 and call(n=5) == -2 and call(batch=0) == -2 and call(imgh=0) == -2
    assert call(arena_p=None) == -2 and call(t=None) == -2 and call(items_dev=None) == -2 and call(table=None) == -2 and call(out=None) == -2
    assert call(changed(r1=51)) == -2 and call(changed(c0=-1)) == -2 and call(changed(c1=81)) == -2             # a box outside its page
    assert call(changed(r1=5)) == -2 and call(changed(c0=70)) == -2                                             # an empty box
    assert call(changed(page_off=-16)) == -2 and call(changed(page_off=len(arena))) == -2                       # a page offset outside the arena
    assert call(changed(rows=51)) == -2 and call(changed(stride=79)) == -2 and call(arena_bytes=50 * 80 - 1) == -2   # a page extent outside it
    assert call(changed(upscale=1)) == -2 and call(changed(p0=1)) == -2 and call(changed(out_scale0=float("nan"))) == -2 and call(changed(out_scale1=0.)) == -2
    assert call(imgh=100000, imgw=64, batch=1, n=0) == -3                                                        # staging buffer beyond the LDS budget
    with pytest.raises(native.CrnnError):
        native.check(call(n=-1), "ingest_crops")
