"""-m gpu tests of the device ingest (csrc/ingest.hip through crnn_mi355x/ingest.py): the batch built on the GPU from uint8 pages and a box
table equals data.open_img + data.norm bit for bit -- no tolerance, no excluded case --, over a box list that is itself checked to reach every
branch; the generator, predict_generator and predict.py --device_ingest give what the host path gives."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import utils as U
from crnn_mi355x import data as D
from crnn_mi355x import ingest as I
from crnn_mi355x import native
from crnn_mi355x import pages as PG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
MEAN, STD = 118.24236953981779, 36.72835353999682

HCS = {(100, 32): [1, 2, 16, 17, 20, 29, 30, 31, 32, 40], (200, 32): [1, 16, 17, 29, 30, 32, 40], (40, 32): [1, 16, 17, 29, 30, 32, 40]}
WCS = {(100, 32): [1, 2, 33, 50, 51, 66, 97, 98, 99, 100, 130], (200, 32): [1, 100, 101, 197, 198, 200, 230], (40, 32): [1, 20, 21, 37, 38, 40, 55]}
H, W, SPLIT = 300, 400, 200


def _page(seed=0):
    """Bright left half (160..255), dark right half (0..100) -- so a crop's side of the 127/128 threshold is known and a box centred on the
    boundary ties --, and a band of two grey levels, 127 and 128, in a checkerboard: modal ties at the threshold itself."""
    rs = np.random.RandomState(seed)
    page = np.empty((H, W), np.uint8)
    page[:, :SPLIT] = rs.randint(160, 256, (H, SPLIT))
    page[:, SPLIT:] = rs.randint(0, 101, (H, W - SPLIT))
    page[120:160] = np.where((np.arange(W) + np.arange(120, 160)[:, None]) % 2 == 0, 127, 128)
    return page


def _box(r0, r1, c0, c1, word=None):
    return (word, r0, c0, r1, c1)          # sliced as page[b[1]:b[3], b[2]:b[4]]


def _boxes(shape):
    T0, T1 = shape
    boxes, k = [], 0
    for hc in HCS[shape]:
        for wc in WCS[shape]:
            k += 1
            r0, c0 = (k * 37) % (H - hc + 1), (k * 53) % (W - wc + 1)
            boxes.append(_box(r0, r0 + hc, c0, c0 + wc))
    boxes.append(_box(7, 8, 9, 10))                                        # 1 x 1
    boxes.append(_box(0, H, 0, W))                                         # the whole page
    boxes.append(_box(None, None, None, None))                             # the whole page, as open slice bounds
    boxes.append(_box(-20, -8, -390, 30))                                  # 12 x 20 through negative bounds: up-scaled content
    boxes.append(_box(10, 10 + T1, SPLIT - T0 // 2, SPLIT + T0 // 2))      # no padding, half bright and half dark: the invert count ties
    boxes.append(_box(200, 200 + T1 - 4, SPLIT - T0 // 2, SPLIT + T0 // 2))   # padded on axis 1 with a bright fill: bright wins
    return boxes


def _host(page, boxes, img_size, p=0.):
    return np.stack([D.open_img(page[b[1]:b[3], b[2]:b[4]], img_size, p=p)[0] for b in boxes])


def _branch_key(page, b, img_size):
    """(upscaled, padded on axis 0, padded on axis 1, squashed on axis 0, squashed on axis 1, inverted), tie -- from the host functions alone."""
    crop = page[b[1]:b[3], b[2]:b[4]]
    up, (s0, s1), (b0, b1, p0, p1) = I.plan_crop(crop.shape[0], crop.shape[1], img_size, p=0.)
    rot = crop[::-1].T
    content = D.resize_linear(rot, (s1, s0)) if up else rot
    padded = np.full((p0, p1), D._modal_value(rot), np.uint8)
    padded[b0:b0 + s0, b1:b1 + s1] = content
    hi = int((padded > 127).sum())
    inv = hi > padded.size - hi
    out = D.resize_linear((255 - padded).astype(np.uint8) if inv else padded, (img_size[1], img_size[0]))
    assert np.array_equal(out, D.open_img(crop, img_size, p=0.)[0])        # the key describes what the host really did
    return (bool(up), p0 > s0, p1 > s1, s0 > img_size[0], s1 > img_size[1], bool(inv)), 2 * hi == padded.size


def _check(shape, normed):
    img_size = shape + (1,)
    page, boxes = _page(), _boxes(shape)
    ing = U.DeviceIngest(img_size, normed=normed, mean=MEAN, std=STD)
    (x, u8), words = ing.pages([page], [boxes], return_u8=True)
    ref = _host(page, boxes, img_size)
    assert tuple(x.shape) == (len(boxes),) + img_size and x.dtype == torch.float32 and x.is_cuda and words == ["-"] * len(boxes)
    got = u8.cpu().numpy()
    bad = [k for k in range(len(boxes)) if not np.array_equal(got[k], ref[k])]
    assert not bad, "uint8 mismatch for boxes %s" % [(boxes[k][1:], int((got[k] != ref[k]).sum())) for k in bad[:8]]
    want = D.norm(ref, MEAN, STD) if normed else ref.astype(np.float32)
    assert want.dtype == np.float32 and np.array_equal(x.cpu().numpy()[..., 0], want)
    return page, boxes


def test_bit_exact_against_open_img_over_every_branch():
    img_size = (100, 32, 1)
    page, boxes = _check((100, 32), True)
    keys, ties = zip(*[_branch_key(page, b, img_size) for b in boxes])
    for flag, name in enumerate(("upscaled", "padded on axis 0", "padded on axis 1", "squashed on axis 0", "squashed on axis 1", "inverted")):
        assert {k[flag] for k in keys} == {False, True}, "the box list never has both values of '%s'" % name
    assert any(ties), "no box with an exact tie of the invert count"
    assert not any(k[5] for k, t in zip(keys, ties) if t)                  # a tie does not invert
    assert len(set(keys)) >= 14, sorted(set(keys))


@pytest.mark.parametrize("shape,normed", [((200, 32), True), ((40, 32), True), ((100, 32), False)])
def test_other_shapes_and_unnormalised(shape, normed):
    _check(shape, normed)


def _random_boxes(n, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        hc, wc = int(rs.randint(1, 45)), int(rs.randint(1, 140))
        r0, c0 = int(rs.randint(0, H - hc + 1)), int(rs.randint(0, W - wc + 1))
        out.append(_box(r0, r0 + hc, c0, c0 + wc))
    return out


def test_whole_batch_with_random_padding_equals_the_serial_loop():
    img_size = (100, 32, 1)
    page, boxes = _page(1), _random_boxes(256, 2)
    np.random.seed(5)
    ref = _host(page, boxes, img_size, p=0.7)
    after_host = np.random.get_state()
    np.random.seed(5)
    (x, u8), _ = U.DeviceIngest(img_size).pages([page], [boxes], transform_p=0.7, return_u8=True)
    after_dev = np.random.get_state()
    assert np.array_equal(after_host[1], after_dev[1]) and after_host[2] == after_dev[2]
    assert np.array_equal(u8.cpu().numpy(), ref) and np.array_equal(x.cpu().numpy()[..., 0], D.norm(ref, MEAN, STD))
    np.random.seed(6)
    assert not np.array_equal(_host(page, boxes, img_size, p=0.7), ref)    # the placement really is random


def test_several_pages_in_one_arena():
    img_size = (100, 32, 1)
    pages = [_page(3), _page(4)[:150, :333], np.ascontiguousarray(_page(5).T)]
    boxes = [[(None,) + tuple(b[1:]) for b in _random_boxes(40, 7 + k) if b[3] <= pg.shape[0] and b[4] <= pg.shape[1]] for k, pg in enumerate(pages)]
    assert all(len(b) > 5 for b in boxes)
    (x, u8), _ = U.DeviceIngest(img_size).pages(pages, boxes, return_u8=True)
    ref = np.concatenate([_host(pg, bl, img_size) for pg, bl in zip(pages, boxes)])
    assert np.array_equal(u8.cpu().numpy(), ref)


def _raw(pages, index, rects, img_size, n=None, batch=None, mutate=None, null=()):
    """crnn_ingest_crops called directly on pre-filled outputs -> (return code, fp32 output, uint8 output)."""
    T0, T1 = img_size[0], img_size[1]
    rects = np.asarray(rects).reshape(-1, 4)
    rows = [(up, s[0], s[1]) + o for up, s, o in (I.plan_crop(int(r[1] - r[0]), int(r[3] - r[2]), img_size) for r in rects)]
    arena, offs = PG.pack_arena(pages)
    tab = I.build_table(pages, offs, index, rects, tuple(np.array(c) for c in zip(*rows)), img_size)
    if mutate is not None:
        mutate(tab)
    n = len(tab) if n is None else n
    B = n if batch is None else batch
    d_arena, d_tab = torch.from_numpy(arena).cuda(), torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    table = torch.from_numpy(I.norm_table(True, MEAN, STD)).cuda()
    out = torch.full((B, T0, T1), 7.0, device="cuda")
    u8 = torch.full((B, T0, T1), 9, dtype=torch.uint8, device="cuda")
    ptr = lambda name, t: None if name in null else ctypes.c_void_p(t.data_ptr())
    rc = native.lib().crnn_ingest_crops(ptr("arena", d_arena), len(arena), None if "items" in null else tab.ctypes.data_as(ctypes.c_void_p),
                                        ptr("items_dev", d_tab), n, B, T0, T1, ptr("table", table), ptr("out", out), ptr("u8", u8),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), u8.cpu().numpy()


def test_short_batch_rows_past_n_are_zero():
    img_size = (100, 32, 1)
    page = _page(2)
    boxes = _boxes((100, 32))[:5]
    rects = [I.box_slices(b, page.shape) for b in boxes]
    rc, out, u8 = _raw([page], [0] * 5, rects, img_size, batch=16)
    ref = _host(page, boxes, img_size)
    assert rc == 0 and np.array_equal(u8[:5], ref) and np.array_equal(out[:5], D.norm(ref, MEAN, STD))
    assert not out[5:].any() and not u8[5:].any()
    x, words = U.DeviceIngest(img_size).pages([page], [boxes], batch=16)
    assert tuple(x.shape) == (16, 100, 32, 1) and len(words) == 5
    assert np.array_equal(x.cpu().numpy()[:5, ..., 0], D.norm(ref, MEAN, STD)) and not x.cpu().numpy()[5:].any()
    rc, out, u8 = _raw([page], [0] * 5, rects, img_size, n=0, batch=3)              # nothing but the zero rows
    assert rc == 0 and not out.any() and not u8.any()
    rc, out, _ = _raw([page], [0] * 5, rects, img_size, null=("u8",))               # the uint8 output is optional
    assert rc == 0 and np.array_equal(out, D.norm(ref, MEAN, STD))


def test_bad_arguments_return_minus_two_and_write_nothing():
    img_size = (100, 32, 1)
    page = _page(2)
    rects = [(0, 30, 0, 90), (40, 60, 100, 180), (5, 17, 3, 23)]

    def field(name, value, row=1):
        def mutate(tab):
            tab[name][row] = value
        return mutate
    cases = [dict(mutate=field("r1", H + 1)), dict(mutate=field("c0", -1)), dict(mutate=field("c1", W + 1)),          # a box outside its page
             dict(mutate=field("r1", 40)), dict(mutate=field("c0", 180)),                                            # an empty box
             dict(mutate=field("page_off", -16)), dict(mutate=field("page_off", H * W)), dict(mutate=field("rows", H + 1)),   # a bad page extent
             dict(mutate=field("stride", W - 1)), dict(mutate=field("upscale", 1)), dict(mutate=field("p1", 3, row=0)),
             dict(null=("arena",)), dict(null=("items",)), dict(null=("items_dev",)), dict(null=("table",)), dict(n=-1, batch=4), dict(n=5, batch=4)]
    for kw in cases:
        rc, out, u8 = _raw([page], [0] * 3, rects, img_size, **dict(dict(batch=4), **kw))
        assert rc == -2, kw
        assert (out == 7.0).all() and (u8 == 9).all(), kw
    T0, T1 = img_size[0], img_size[1]
    out = torch.full((2, T0, T1), 7.0, device="cuda")
    rc = native.lib().crnn_ingest_crops(None, 0, None, None, 0, 2, T0, T1, ctypes.c_void_p(out.data_ptr()), None, None, None)   # null output
    assert rc == -2
    with pytest.raises(ValueError):
        U.DeviceIngest(img_size).pages([page], [[_box(10, 10, 0, 5)]])
    with pytest.raises(ValueError):
        U.DeviceIngest(img_size).pages([page], [[_box(0, 5, 0, 5)] * 3], batch=2)


# ---- generator, model and CLI (the helpers follow tests/test_gpu_cli.py / test_host_cpu.py) ----------------------------------------------
def _make_dataset(folder, n=48, seed=0):
    from PIL import Image, ImageDraw
    rs = np.random.RandomState(seed)
    alphabet = "abcdefghij0123"
    names = []
    for i in range(n):
        word = "".join(rs.choice(list(alphabet), size=rs.randint(2, 6)))
        img = Image.new("L", (20 + 12 * len(word), 28), color=235 if i % 3 else 30)
        ImageDraw.Draw(img).text((4, 6), word, fill=20 if i % 3 else 230)
        names.append(os.path.join(folder, "%d_%s_%d.png" % (i, word, i)))
        img.save(names[-1])
    return names


def _make_pages(folder, npages=2, nboxes=11):
    from PIL import Image
    names, bboxs = [], {}
    for k in range(npages):
        name = "page%d.png" % k
        Image.fromarray(_page(10 + k)).save(os.path.join(folder, name))
        words = ["w%d" % i if i % 4 else None for i in range(nboxes)]
        bboxs[name] = [(w,) + tuple(b[1:]) for w, b in zip(words, _random_boxes(nboxes, 20 + k))]
        names.append(name)
    return names, bboxs


def _classes():
    return {ch: i for i, ch in enumerate(U.get_lexicon())}


def _drain(gen, steps, batch_size, total):
    """`steps` batches of a generator, copied (Readf re-yields its arrays) -> [(input fp32 (rows that are defined), labels, lengths, words)]."""
    out = []
    full, rem = divmod(total, batch_size)
    for k in range(steps):
        inputs, outputs = next(gen)
        x = inputs["the_input"]
        with np.errstate(over="ignore", invalid="ignore"):           # the host's undefined rows may not fit fp32
            x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x).astype(np.float32)
        assert x.shape[0] == batch_size and outputs["ctc"].shape == (batch_size,)
        rows = rem if (k == full and rem) else batch_size          # the first pass' short tail: the rows past it are undefined on the host
        nlab = len(inputs["source_str"])
        assert nlab == rows
        out.append((x[:rows].astype(np.float32), inputs["the_labels"][:nlab].copy(), inputs["input_length"][:nlab].copy(),
                    inputs["label_length"][:nlab].copy(), list(inputs["source_str"]), x[rows:].astype(np.float32)))
    return out


def _assert_same_batches(host, dev):
    assert len(host) == len(dev)
    for k, (h, d) in enumerate(zip(host, dev)):
        assert h[0].dtype == d[0].dtype == np.float32 and np.array_equal(h[0], d[0]), k
        assert np.array_equal(h[1], d[1]) and np.array_equal(h[2], d[2]) and np.array_equal(h[3], d[3]) and h[4] == d[4], k
        assert not d[5].any(), k                                    # rows past a short batch: zero on the device


@pytest.mark.parametrize("p", [0., 0.7])
def test_generator_equals_readf_on_files_and_on_pages(tmp_path, p):
    names = _make_dataset(str(tmp_path), n=21)
    kw = dict(img_size=(100, 32, 1), normed=True, batch_size=8, classes=_classes(), max_len=23, transform_p=p)
    np.random.seed(3)
    host = _drain(U.Readf(**kw).run_generator(names), 7, 8, 21)      # two full batches, the tail of 5, and on into the second pass
    np.random.seed(3)
    dev = _drain(U.DeviceReadf(**kw).run_generator(names), 7, 8, 21)
    _assert_same_batches(host, dev)
    par = U.DeviceReadf(workers=2, chunk=5, **kw)                    # the files decoded by two processes: same batches
    np.random.seed(3)
    _assert_same_batches(host, _drain(par.run_generator(names), 7, 8, 21))
    par.close()
    pdir = tmp_path / "pages"
    os.makedirs(pdir)
    pnames, bboxs = _make_pages(str(pdir))
    pnames = [os.path.join(str(pdir), n) for n in pnames]
    bboxs = {os.path.join(str(pdir), k): v for k, v in bboxs.items()}
    for normed in (True, False):
        kw2 = dict(kw, normed=normed, batch_size=4)
        np.random.seed(4)
        host = _drain(U.Readf(**kw2).run_generator(pnames, bboxs=bboxs), 8, 4, 22)
        np.random.seed(4)
        dev = _drain(U.DeviceReadf(**kw2).run_generator(pnames, bboxs=bboxs), 8, 4, 22)
        _assert_same_batches(host, dev)
    mixed = pnames[:1] + names[:7] + pnames[1:] + names[7:9]         # pages between runs of one-word files, decoded by two processes
    mbb = dict({n: [n] for n in names[:9]}, **bboxs)
    kw3 = dict(kw, batch_size=4)
    np.random.seed(5)
    host = _drain(U.Readf(**kw3).run_generator(mixed, bboxs=mbb), 10, 4, 31)
    par = U.DeviceReadf(workers=2, chunk=3, **kw3)
    np.random.seed(5)
    _assert_same_batches(host, _drain(par.run_generator(mixed, bboxs=mbb), 10, 4, 31))
    par.close()


def _small_model():
    return U.CRNN(num_classes=38, max_string_len=23, shape=(100, 32, 1), time_dense_size=32, n_units=64).get_model()


def test_predict_generator_over_device_batches_equals_host_batches(tmp_path):
    names = _make_dataset(str(tmp_path), n=24)
    kw = dict(img_size=(100, 32, 1), normed=True, batch_size=8, classes=_classes(), max_len=23, transform_p=0.)
    model = U.init_predictor(_small_model())
    y_host = model.predict_generator(U.Readf(**kw).run_generator(names), steps=3)
    y_dev = model.predict_generator(U.DeviceReadf(**kw).run_generator(names), steps=3)
    assert y_host.shape == (24, 52, 38) and np.array_equal(y_host, y_dev)
    dec = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes={v: k for k, v in _classes().items()})
    assert list(dec.decode(y_host)) == list(dec.decode(y_dev))
    x, _ = U.DeviceIngest((100, 32, 1)).files(names[:8])
    assert np.array_equal(model.predict_on_batch(x), y_host[:8])


def test_predict_cli_device_ingest_writes_the_same_csv(tmp_path):
    sys.path.insert(0, PKG)
    import predict as predict_cli
    mdir = tmp_path / "models" / "m1"
    os.makedirs(mdir)
    model = _small_model()
    U.save_model_json(model, str(tmp_path / "models"), "m1")
    model.save_weights(str(mdir / "final_weights.h5"))
    pdir = tmp_path / "pages"
    os.makedirs(pdir)
    _, bboxs = _make_pages(str(pdir), npages=3, nboxes=7)
    pickle.dump(bboxs, open(tmp_path / "boxes.pickle", "wb"))
    fdir = tmp_path / "files"
    os.makedirs(fdir)
    _make_dataset(str(fdir), n=13)
    for route, extra in (("boxes", ["--image_path", str(pdir), "--boxes", str(tmp_path / "boxes.pickle")]), ("files", ["--image_path", str(fdir)])):
        texts = []
        for flag in ([], ["--device_ingest"]):
            res = tmp_path / ("res_%s_%d" % (route, len(flag)))
            os.makedirs(res)
            predict_cli.main(["--model_path", str(mdir), "--result_path", str(res), "--batch_size", "4", "--G", "0"] + extra + flag)
            texts.append(open(res / "prediction.csv").read())
        assert texts[0] == texts[1] and len(texts[0].splitlines()) > 10, route
