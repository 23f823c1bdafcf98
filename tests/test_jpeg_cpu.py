"""CPU tests (no GPU) of the JPEG path: the NumPy definition crnn_mi355x.jpeg.jpeg_decode_host against libjpeg-turbo (through Pillow) over the
288-file grid of tests/jpeg_cases.py and against the committed files of tests/golden/jpeg/, its grey against data.read_img, and crnn_jpeg_plan
against the Python parse with every refusal code pinned.  crnn_jpeg_decode checks its arguments on the host before anything is launched, so a
fake non-null integer stands for every device pointer there (as in tests/test_pages_cpu.py)."""
import ctypes
import io
import os

import numpy as np
import pytest

import jpeg_cases as JC
from crnn_mi355x import data as D
from crnn_mi355x import jpeg as J
from crnn_mi355x import native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
W = np.array([0.299, 0.587, 0.114])


def _turbo():
    from PIL import features
    return features.check("libjpeg_turbo")


needs_turbo = pytest.mark.skipif(not _turbo(), reason="bit-equality is claimed against libjpeg-turbo; this Pillow has another JPEG library")


@needs_turbo
def test_host_definition_equals_libjpeg_turbo_on_the_grid():
    grid = JC.grid()
    assert len(grid) == 288
    bad = []
    for name, data in grid:
        planes, status = J.jpeg_decode_host(data)
        ref = JC.pillow(data, "L" if "grey" in name else "RGB")
        if status != 0 or planes.shape != ref.shape or planes.dtype != np.uint8 or not np.array_equal(planes, ref):
            bad.append((name, status))
    assert not bad, bad[:10]


def test_host_definition_equals_the_golden_files():
    expected = np.load(os.path.join(GOLDEN, "expected.npz"))
    names = sorted(k for k in expected.files if not k.endswith(":grey"))
    assert len(names) >= 5
    for name in names:
        data = open(os.path.join(GOLDEN, name), "rb").read()
        planes, status = J.jpeg_decode_host(data)
        assert status == 0 and np.array_equal(planes, expected[name]), name
        assert np.array_equal(J.jpeg_gray_host(data), expected[name + ":grey"]), name


def test_tie_table_is_the_n13_matmul():
    keys, grey = J.tie_table()
    assert len(keys) == 16782
    rgb = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], axis=1).astype(np.float64)
    assert (np.round((rgb @ np.array([299., 587., 114.]) + 500) % 1000) == 0).all()
    ref = np.clip(np.floor(rgb.reshape(-1, 1, 3) @ W + 0.5), 0, 255).astype(np.uint8).ravel()
    assert np.array_equal(grey, ref)
    assert np.array_equal(J.gray_of_rgb(rgb.astype(np.uint8)), ref)


@needs_turbo
def test_grey_against_read_img():
    ties = total = 0
    for name, data in JC.grid():
        got, ref = J.jpeg_gray_host(data), D.read_img(io.BytesIO(data))
        assert got.shape == ref.shape and got.dtype == ref.dtype == np.uint8
        if "grey" in name:
            assert np.array_equal(got, ref), name
            continue
        rgb = JC.pillow(data, "RGB").astype(np.int64)
        tie = (rgb @ np.array([299, 587, 114]) + 500) % 1000 == 0
        assert np.array_equal(got[~tie], ref[~tie]), name
        assert (np.abs(got[tie].astype(int) - ref[tie].astype(int)) <= 1).all(), name
        ties += int(tie.sum())
        total += tie.size
    assert total > 0 and ties < 0.01 * total, (ties, total)


def _plan_one(data):
    _, items, segs, pool, totals = J.plan([data])
    return items[0], segs, pool, totals


def test_plan_equals_the_python_parse_on_the_grid():
    grid = JC.grid()
    blob, items, segs, pool, totals = J.plan([d for _, d in grid])
    assert blob.nbytes == sum(len(d) for _, d in grid) and totals[1] == len(segs) and totals[0] == len(pool)
    off = arena = samples = 0
    for i, (name, data) in enumerate(grid):
        info, it = J.parse_jpeg(data), items[i]
        assert it["status"] == info["status"] == 0, name
        for f in ("rows", "cols", "ncomp", "restart", "mcux", "mcuy"):
            assert it[f] == info[f], (name, f)
        nc = info["ncomp"]
        assert list(it["hs"][:nc]) == info["hs"] and list(it["vs"][:nc]) == info["vs"], name
        assert (it["data_off"], it["scan_off"], it["scan_end"]) == (off, off + info["scan_off"], off + info["scan_end"]), name
        assert (it["page_off"], it["stride"], it["samp_off"]) == (arena, info["cols"], samples), name
        assert it["nseg"] == len(info["segs"]) and (info["restart"] == 0) == ("s2" not in name), name
        for k, sg in enumerate(info["segs"]):
            s = segs[it["seg0"] + k]
            assert (s["begin"], s["end"], s["item"], s["mcu0"], s["nmcu"]) == (off + sg[0], off + sg[1], i, sg[2], sg[3]), (name, k)
        for c in range(nc):
            assert np.array_equal(pool[it["qt"][c]:it["qt"][c] + J.QUANT_INTS], info["quant"][c]), name
            assert np.array_equal(pool[it["dc"][c]:it["dc"][c] + J.HUFF_INTS], info["dc"][c]), name
            assert np.array_equal(pool[it["ac"][c]:it["ac"][c] + J.HUFF_INTS], info["ac"][c]), name
            samples += info["mcux"] * info["hs"][c] * 8 * info["mcuy"] * info["vs"][c] * 8
        off += len(data)
        arena += -(-info["rows"] * info["cols"] // 16) * 16
    assert (totals[2], totals[3]) == (arena, samples)


def _segments(data):
    """[(marker, start of the FF, end of the segment)] up to and including SOS."""
    out, p = [], 2
    while True:
        m, L = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, p + 2 + L))
        if m == 0xDA:
            return out
        p += 2 + L


def _base(sampling="4:2:0", **st):
    return JC.encode(dict(JC._images(16, 24, 5))["walk"], sampling, **(st or dict(quality=75)))


def _status(data):
    st = int(_plan_one(data)[0]["status"])
    assert st == J.parse_jpeg(data)["status"]               # the Python twin agrees on every refusal
    return st


def test_plan_refusals():
    from PIL import Image
    base = _base()
    assert _status(base) == J.OK
    arr = dict(JC._images(16, 24, 5))["walk"]
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, "JPEG", progressive=True)
    prog = buf.getvalue()
    assert any(m == 0xC2 for m, _, _ in _segments(prog))
    it = _plan_one(prog)[0]
    assert _status(prog) == J.UNSUPPORTED and (it["rows"], it["cols"]) == (16, 24)
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").convert("CMYK").save(buf, "JPEG")
    assert _status(buf.getvalue()) == J.UNSUPPORTED
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, "PNG")
    assert _status(buf.getvalue()) == J.UNSUPPORTED           # no JPEG at all: the host's to decode
    segs = _segments(base)
    assert {0xE0, 0xDB, 0xC0, 0xC4, 0xDA} <= {m for m, _, _ in segs}
    for m, a, b in segs:                                      # cut inside every header segment, and between two of them
        assert _status(base[:(a + b) // 2]) == J.CORRUPT, hex(m)
        assert _status(base[:a]) == J.CORRUPT, hex(m)
    sof = next(a for m, a, _ in segs if m == 0xC0)
    sos = next(a for m, a, _ in segs if m == 0xDA)
    dht = next(a for m, a, _ in segs if m == 0xC4)
    dqt = next((a, b) for m, a, b in segs if m == 0xDB)
    app0 = next((a, b) for m, a, b in segs if m == 0xE0)

    def patch(at, values, src=base):
        out = bytearray(src)
        out[at:at + len(values)] = bytes(values)
        return bytes(out)
    assert _status(patch(dht + 5, [3])) == J.CORRUPT                          # three codes of length 1: the counts overflow the code space
    assert _status(patch(sof + 5, [0, 0])) == J.CORRUPT                       # zero rows
    assert _status(patch(sof + 7, [0, 0])) == J.CORRUPT                       # zero columns
    assert _status(patch(sof + 4, [12])) == J.UNSUPPORTED                     # 12-bit samples
    assert _status(patch(sof + 11, [0x12])) == J.UNSUPPORTED                  # luma sampled 1 x 2
    assert _status(patch(sof + 14, [0x21])) == J.UNSUPPORTED                  # chroma not 1 x 1
    assert _status(patch(sof + 1, [0xC9])) == J.UNSUPPORTED                   # arithmetic coding
    assert _status(patch(dqt[0] + 4, [0x10 | base[dqt[0] + 4]])) in (J.CORRUPT, J.UNSUPPORTED)   # a 16-bit table in an 8-bit table's room
    assert _status(base[:dqt[0]] + base[dqt[1]:]) == J.CORRUPT                # a missing quantiser table
    assert _status(patch(sos + 6, [0x33])) == J.CORRUPT                       # a scan that names Huffman tables nobody defined
    assert _status(patch(sos + 4, [2])) in (J.CORRUPT, J.UNSUPPORTED)         # a scan of two of the three components (its length no longer fits)
    rgb = patch(sof + 10, b"R")
    rgb = patch(sof + 13, b"G", rgb)
    rgb = patch(sof + 16, b"B", rgb)
    rgb = patch(sos + 5, b"R", rgb)
    rgb = patch(sos + 7, b"G", rgb)
    rgb = patch(sos + 9, b"B", rgb)
    assert _status(rgb) == J.OK                                               # JFIF says YCbCr whatever the ids
    assert _status(rgb[:app0[0]] + rgb[app0[1]:]) == J.UNSUPPORTED            # ids R, G, B without JFIF: RGB data
    adobe = bytes([0xFF, 0xEE, 0, 14]) + b"Adobe" + bytes([0, 100, 0, 0, 0, 0])
    assert _status(base[:app0[0]] + adobe + bytes([0]) + base[app0[1]:]) == J.UNSUPPORTED       # Adobe, transform 0
    assert _status(base[:app0[0]] + adobe + bytes([1]) + base[app0[1]:]) == J.OK                # Adobe, transform 1: YCbCr
    two = base[:-2] + base[sos:]                                              # a second scan after the first
    assert _status(two) == J.UNSUPPORTED
    # a scan cut short is the device's to report: the plan accepts it, the definition decodes zeros after the end
    cut = base[:(segs[-1][2] + len(base)) // 2]
    assert _status(cut) == J.OK
    planes, st = J.jpeg_decode_host(cut)
    assert st == J.TRUNCATED and planes.shape == (16, 24, 3) and not planes.any()
    rst = _base("4:4:4", quality=30, restart_marker_blocks=1)
    info = J.parse_jpeg(rst)
    cut = rst[:info["segs"][2][0] + 1]
    it, segs2, _, _ = _plan_one(cut)
    assert it["status"] == J.OK and it["nseg"] == len(info["segs"]) == 6
    assert [(s["begin"], s["end"]) for s in segs2[3:]] == [(len(cut), len(cut))] * 3          # the segments the file never reached: empty
    assert J.jpeg_decode_host(cut)[1] == J.TRUNCATED
    # argument faults of the call
    L = native.lib()
    blob = np.frombuffer(base, np.uint8)
    items, pool, tot = np.zeros(1, J.ITEM_DTYPE), np.zeros(J.POOL_INTS_PER_FILE, np.int32), np.zeros(4, np.dtype("l"))
    segs3 = np.zeros(4, J.SEG_DTYPE)

    def call(n=1, off=0, ln=len(base), pool_cap=len(pool), seg_cap=4, blob_p=blob.ctypes.data):
        offs, lens = np.array([off], np.dtype("l")), np.array([ln], np.dtype("l"))
        return L.crnn_jpeg_plan(blob_p, len(base), offs.ctypes.data, lens.ctypes.data, n, items.ctypes.data, pool.ctypes.data, pool_cap, segs3.ctypes.data, seg_cap,
                                tot.ctypes.data)
    assert call() == 0 and items["status"][0] == 0
    assert call(n=0) == -2 and call(ln=-1) == -2 and call(off=-1) == -2 and call(off=1) == -2 and call(blob_p=None) == -2
    assert call(pool_cap=100) == -2
    assert call(seg_cap=0) == -2 and tot[1] == 1                              # the table is too short: the size needed is reported


FAKE = 1 << 22


def test_decode_refuses_bad_arguments_before_any_launch():
    L = native.lib()
    datas = [d for _, d in JC.grid()[:6]]
    blob, items, segs, pool, totals = J.plan(datas)
    n, samples, arena = len(datas), int(totals[3]), int(totals[2])
    ws = L.crnn_jpeg_workspace_bytes(samples)
    assert ws == -(-2 * samples // 16) * 16 + -(-samples // 16) * 16 and L.crnn_jpeg_workspace_bytes(-1) == 0

    def call(items=items, segs=segs, n=n, out=FAKE, out_bytes=arena, ws_p=FAKE, ws_bytes=ws, pool_ints=len(pool), blob_bytes=blob.nbytes, status=FAKE):
        return L.crnn_jpeg_decode(FAKE, blob_bytes, items.ctypes.data, FAKE, n, segs.ctypes.data, FAKE, len(segs), FAKE, pool_ints, out, out_bytes, status, ws_p,
                                  ws_bytes, None)

    def edit(table, k, **fields):
        t = table.copy()
        for f, v in fields.items():
            t[f][k] = v
        return t
    assert call(n=0) == -2 and call(out=None) == -2 and call(status=None) == -2
    last = int(items["page_off"][-1]) + int(items["rows"][-1]) * int(items["cols"][-1])
    assert call(out_bytes=last - 1) == -2                                     # the last page does not fit (pages.h)
    assert call(items=edit(items, 1, page_off=-16)) == -2
    assert call(items=edit(items, 1, stride=items["cols"][1] - 1)) == -2
    assert call(ws_bytes=ws - 1) == -2 and call(ws_p=FAKE + 8) == -2 and call(ws_p=None) == -2
    assert call(pool_ints=len(pool) - 1) == -2                                # the last table reaches past the pool
    assert call(items=edit(items, 2, samp_off=items["samp_off"][2] + 64)) == -2
    assert call(items=edit(items, 0, ncomp=2)) == -2 and call(items=edit(items, 0, mcux=0)) == -2
    assert call(items=edit(items, 3, seg0=len(segs))) == -2
    assert call(segs=edit(segs, 0, end=blob.nbytes + 1)) == -2 and call(segs=edit(segs, 0, begin=-1)) == -2
    assert call(segs=edit(segs, 1, item=n)) == -2
    assert call(segs=edit(segs, 1, nmcu=int(items["mcux"][segs["item"][1]]) * int(items["mcuy"][segs["item"][1]]) + 1)) == -2
    assert call(blob_bytes=int(segs["end"][-1]) - 1) == -2                    # the last segment ends past the blob
