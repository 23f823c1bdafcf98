"""-m gpu tests of JPEG decoding on the device (csrc/jpeg.hip through crnn_mi355x/jpeg.py): the grey pages equal jpeg_gray_host bit for bit over
the 288-file grid of tests/jpeg_cases.py -- 1 x 1, chroma planes of at most 2 columns (7 x 3, 17 x 5: the replication branches), partial MCUs
(31 x 97, 33 x 18, 9 x 33), one row of MCUs (2 x 70), a restart interval of 1, optimised and default Huffman tables, quality 100 --, a mixed call
routes what the device cannot decode to the host, and DeviceIngest.files / DeviceReadf / predict.py give with the flag what they give without."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_cases as JC
import utils as U
from crnn_mi355x import data as D
from crnn_mi355x import jpeg as J
from crnn_mi355x import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
_HOST = {}


def _host_grey():
    """jpeg_gray_host of the grid, computed once and shared."""
    if not _HOST:
        _HOST["grey"] = [J.jpeg_gray_host(d) for _, d in JC.grid()]
    return _HOST["grey"]


def _pages(arena):
    flat = arena.dev.cpu().numpy()
    return [flat[o:o + pg.size].reshape(pg.shape) for pg, o in zip(arena.pages, arena.offsets)], flat


def test_grid_equals_the_host_definition_bit_for_bit():
    grid, ref = JC.grid(), _host_grey()
    dec = U.JpegDecoder()
    arena, status, shapes = dec.decode([d for _, d in grid])
    got, flat = _pages(arena)
    assert status.dtype == torch.int32 and not status.cpu().numpy().any()
    assert shapes == [r.shape for r in ref]
    bad = [name for (name, _), g, r in zip(grid, got, ref) if not np.array_equal(g, r)]
    assert not bad, (len(bad), bad[:10])
    used = np.zeros(flat.size, bool)
    for pg, o in zip(arena.pages, arena.offsets):
        used[o:o + pg.size] = True
    assert not flat[~used].any()                                   # the alignment bytes between pages stay zero
    arena2, status2, _ = dec.decode([d for _, d in grid])
    assert np.array_equal(arena2.dev.cpu().numpy(), flat) and not status2.cpu().numpy().any()


def _truncated():
    good = JC.encode(dict(JC._images(24, 40, 9))["walk"], "4:2:0", quality=75)
    info = J.parse_jpeg(good)
    return good[:(info["scan_off"] + info["scan_end"]) // 2]


def test_mixed_call_routes_to_the_host_and_reports_truncation(tmp_path):
    from PIL import Image
    arr = dict(JC._images(24, 40, 9))["walk"]
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, "JPEG", progressive=True)
    prog = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, "PNG")
    png = buf.getvalue()
    cut = _truncated()
    big = JC.encode(dict(JC._images(64, 256, 3))["noise"], "4:4:4", quality=100)
    good = [d for _, d in JC.grid()[::37]]
    assert max(len(d) for d in good) < len(big) // 2
    datas = good[:3] + [prog] + good[3:5] + [png, cut] + good[5:] + [big]
    dec = U.JpegDecoder(max_segment_bytes=len(big) // 2)           # `big` is supported, but over the size the device takes: the host's
    arena, status, shapes = dec.decode(datas)
    got, _ = _pages(arena)
    st = status.cpu().numpy()
    ref_cut, st_cut = J.jpeg_decode_host(cut)
    assert st_cut == J.TRUNCATED
    for k, d in enumerate(datas):
        if d is prog or d is png:
            assert st[k] == J.UNSUPPORTED and np.array_equal(got[k], D.read_img(io.BytesIO(d))), k
        elif d is big:
            assert st[k] == 0 and np.array_equal(got[k], D.read_img(io.BytesIO(d))), k
        elif d is cut:
            assert st[k] == st_cut and got[k].shape == ref_cut.shape[:2] and np.array_equal(got[k], J.jpeg_gray_host(cut)), k
        else:
            assert st[k] == 0 and np.array_equal(got[k], J.jpeg_gray_host(d)), k
    names = []
    for k, d in enumerate([good[0], cut]):
        names.append(str(tmp_path / ("%d_word_%d.jpg" % (k, k))))
        open(names[-1], "wb").write(d)
    with pytest.raises(ValueError, match="1_word_1.jpg"):
        U.DeviceIngest((100, 32, 1)).files(names, decode="device")


def test_library_call_leaves_the_guard_bytes_alone():
    """crnn_jpeg_decode on buffers of the test's own: 64 guard bytes on either side of the arena and of the workspace keep their pattern."""
    L = native.lib()
    picks = JC.grid()[5::23]
    datas = [d for _, d in picks] + [_truncated()]
    blob, items, segs, pool, totals = J.plan(datas)
    n, nbytes, samples = len(datas), int(totals[2]), int(totals[3])
    ws_bytes = L.crnn_jpeg_workspace_bytes(samples)
    G = 64
    arena = torch.full((nbytes + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = torch.full((ws_bytes + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() for a in (blob, items, segs, pool)]
    rc = L.crnn_jpeg_decode(dev[0].data_ptr(), blob.nbytes, items.ctypes.data, dev[1].data_ptr(), n, segs.ctypes.data, dev[2].data_ptr(), len(segs),
                            dev[3].data_ptr(), len(pool), arena.data_ptr() + G, nbytes, status.data_ptr() + 4, ws.data_ptr() + G, ws_bytes, None)
    assert rc == 0
    torch.cuda.synchronize()
    a, w, s = arena.cpu().numpy(), ws.cpu().numpy(), status.cpu().numpy()
    assert (a[:G] == 0xA5).all() and (a[-G:] == 0xA5).all() and (w[:G] == 0x5A).all() and (w[-G:] == 0x5A).all()
    assert s[0] == -7 and s[-1] == -7 and list(s[1:-1]) == [0] * (n - 1) + [J.TRUNCATED]
    for k, d in enumerate(datas):
        o, ref = int(items["page_off"][k]), J.jpeg_gray_host(d)
        assert np.array_equal(a[G + o:G + o + ref.size].reshape(ref.shape), ref), k


def _write(folder, sampling, n=11, ext="jpg"):
    """One-word files `<i>_<word>_<i>.jpg` of mjsynth's naming, sizes around 100 x 32."""
    from PIL import Image, ImageDraw
    rs = np.random.RandomState(7)
    names = []
    for i in range(n):
        word = "".join(rs.choice(list("abcdefghij0123"), size=rs.randint(2, 6)))
        img = Image.new("RGB", (20 + 12 * len(word) + i, 26 + i % 5), color=(235, 225, 200) if i % 3 else (30, 40, 60))
        ImageDraw.Draw(img).text((4, 6), word, fill=(20, 60, 90) if i % 3 else (230, 200, 210))
        names.append(os.path.join(folder, "%d_%s_%d.%s" % (i, word, i, ext)))
        arr = np.array(img)
        open(names[-1], "wb").write(JC.encode(arr, sampling, quality=80))
    return names


@pytest.mark.parametrize("p", [0., 0.7])
def test_ingest_files_decoded_on_the_device(tmp_path, p):
    os.makedirs(tmp_path / "g")
    os.makedirs(tmp_path / "c")
    grey, colour = _write(str(tmp_path / "g"), "grey"), _write(str(tmp_path / "c"), "4:2:0")
    ing = U.DeviceIngest((100, 32, 1))
    np.random.seed(11)
    (xh, uh), wh = ing.files(grey, transform_p=p, return_u8=True)
    after = np.random.uniform()
    np.random.seed(11)
    (xd, ud), wd = ing.files(grey, transform_p=p, return_u8=True, decode="device")
    assert np.random.uniform() == after                            # the same draws from np.random
    assert wh == wd and torch.equal(uh, ud) and torch.equal(xh, xd)
    pages = [J.jpeg_gray_host(open(f, "rb").read()) for f in colour]
    rects = [(0, pg.shape[0], 0, pg.shape[1]) for pg in pages]
    np.random.seed(12)
    xr, ur = ing.crops(pages, list(range(len(pages))), rects, ing.plan(rects, p), return_u8=True)
    np.random.seed(12)
    (xc, uc), _ = ing.files(colour, transform_p=p, return_u8=True, decode="device")
    assert torch.equal(ur, uc) and torch.equal(xr, xc)
    with pytest.raises(ValueError):
        ing.files(grey, decode="gpu")


def _classes():
    return {ch: i for i, ch in enumerate(U.get_lexicon())}


def _drain(gen, steps):
    out = []
    for _ in range(steps):
        inputs, _ = next(gen)
        out.append((inputs["the_input"].cpu().numpy().copy(), inputs["the_labels"].copy(), inputs["input_length"].copy(), inputs["label_length"].copy(),
                    list(inputs["source_str"])))
    return out


def test_readf_device_decode_equals_readf(tmp_path):
    names = _write(str(tmp_path), "grey", n=21)
    kw = dict(img_size=(100, 32, 1), normed=True, batch_size=8, classes=_classes(), max_len=23, transform_p=0.7)
    np.random.seed(3)
    ref = _drain(U.DeviceReadf(**kw).run_generator(names), 7)      # two full batches, the tail of 5, and on into the second pass
    np.random.seed(3)
    dev = _drain(U.DeviceReadf(device_decode=True, **kw).run_generator(names), 7)
    par = U.DeviceReadf(device_decode=True, workers=2, chunk=5, **kw)
    np.random.seed(3)
    two = _drain(par.run_generator(names), 7)
    par.close()
    for got in (dev, two):
        assert len(got) == len(ref)
        for k, (r, g) in enumerate(zip(ref, got)):
            assert np.array_equal(r[0], g[0]), k
            assert np.array_equal(r[1], g[1]) and np.array_equal(r[2], g[2]) and np.array_equal(r[3], g[3]) and r[4] == g[4], k


def test_predict_cli_device_decode_writes_the_same_csv(tmp_path):
    mdir = tmp_path / "models" / "m1"
    os.makedirs(mdir)
    model = U.CRNN(num_classes=38, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()
    U.save_model_json(model, str(tmp_path / "models"), "m1")
    model.save_weights(str(mdir / "final_weights.h5"))
    fdir = tmp_path / "files"
    os.makedirs(fdir)
    _write(str(fdir), "grey", n=13)
    texts = []
    for flag in ([], ["--device_decode"]):
        res = tmp_path / ("res_%d" % len(flag))
        os.makedirs(res)
        cmd = [sys.executable, os.path.join(PKG, "predict.py"), "--model_path", str(mdir), "--result_path", str(res), "--batch_size", "4", "--G", "0",
               "--image_path", str(fdir), "--device_ingest"] + flag
        done = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stderr[-2000:]
        texts.append(open(res / "prediction.csv").read())
    assert texts[0] == texts[1] and len(texts[0].splitlines()) > 10
