"""CPU tests (no GPU) of the training augmentation: the rule of include/crnn_mi355x.h (crnn_augment_batch) as crnn_mi355x.augment.augment_host
states it, against vectors pinned from an independent prototype and against plain-Python loops; AugmentPolicy; every refusal of
crnn_augment_batch (fake non-null integers stand for the device pointers, as in tests/test_pages_cpu.py: a case runs only where the call
refuses, so nothing is launched); Readf(augment=policy)."""
import ctypes
import os

import numpy as np
import pytest

import utils as U
from crnn_mi355x import augment as A
from crnn_mi355x import ingest as I
from crnn_mi355x import native

ARG, UNSUPPORTED = -2, -3
IN_P, OUT8_P, FAKE = 1 << 20, 1 << 24, ctypes.c_void_p(1 << 22)       # stand for device pointers

PIN = np.array([[0, 23, 46], [69, 92, 115], [138, 161, 184], [207, 230, 253]], np.uint8)
WARP = dict(a00=60000, a01=9000, a10=-7000, a11=70000, t0=40000, t1=-90000)
PINNED = [
    (dict(WARP, fill=7), [[12, 41, 74], [30, 101, 135], [34, 162, 196], [23, 175, 164]]),
    (dict(WARP, fill=-1), [[20, 41, 74], [83, 101, 135], [147, 162, 196], [207, 211, 235]]),
    (dict(morph=1), [[92, 115, 115], [161, 184, 184], [230, 253, 253], [230, 253, 253]]),
    (dict(morph=-1), [[0, 0, 23], [0, 0, 23], [69, 69, 92], [138, 138, 161]]),
    (dict(blur=1), [[23, 40, 58], [75, 92, 109], [144, 161, 178], [196, 213, 230]]),
    (dict(gain=400, bias=-30), [[0, 0, 0], [6, 42, 78], [114, 150, 186], [221, 255, 255]]),
    (dict(noise=64, seed=12345), [[45, 21, 19], [114, 144, 49], [160, 137, 177], [162, 255, 249]]),
    (dict(WARP, fill=7, morph=1, blur=1, gain=400, bias=-30, noise=64, seed=12345),
     [[138, 118, 105], [190, 220, 115], [198, 171, 197], [134, 226, 200]]),
]


def _items(n=1, **fields):
    t = A.neutral_items(n)
    for k, v in fields.items():
        t[k] = v
    return t


@pytest.mark.parametrize("case", range(len(PINNED)))
def test_pinned_vectors(case):
    fields, want = PINNED[case]
    got = A.augment_host(PIN[None], _items(**fields))
    assert got.dtype == np.uint8 and got.shape == (1, 4, 3) and got[0].tolist() == want


def test_mix32_and_the_item_layout():
    assert A.mix32([0, 1, 2]).tolist() == [0, 1753845952, 3507691905]
    assert ctypes.sizeof(A.crnn_augment_item) == A.ITEM_DTYPE.itemsize == 52
    raw = (A.crnn_augment_item * 2).from_buffer_copy(_items(2, a01=-5, seed=0xfffffff0, noise=3).tobytes())
    assert [(it.a00, it.a01, it.a11, it.fill, it.gain, it.noise, it.seed) for it in raw] == [(65536, -5, 65536, -1, 256, 3, 0xfffffff0)] * 2


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (7, 5), (33, 3), (100, 32)])
def test_neutral_items_return_the_input_bytes(shape):
    x = np.random.RandomState(sum(shape)).randint(0, 256, (3,) + shape).astype(np.uint8)
    x[0].flat[0], x[0].flat[-1] = 0, 255
    got = A.augment_host(x, A.neutral_items(3))
    assert got.dtype == np.uint8 and np.array_equal(got, x) and got is not x
    table = I.norm_table(True)
    assert np.array_equal(A.augment_host(x, A.neutral_items(3), table), table[x])


def _warp_loops(img, it):
    T0, T1 = img.shape
    out = np.zeros((T0, T1), np.uint8)

    def tap(i, j):
        if it["fill"] >= 0 and not (0 <= i < T0 and 0 <= j < T1):
            return int(it["fill"])
        return int(img[min(max(i, 0), T0 - 1), min(max(j, 0), T1 - 1)])
    for i in range(T0):
        for j in range(T1):
            di, dj = 2 * i - (T0 - 1), 2 * j - (T1 - 1)
            Y = int(it["a00"]) * di + int(it["a01"]) * dj + int(it["t0"]) + ((T0 - 1) << 16)       # Python integers: >> floors
            X = int(it["a10"]) * di + int(it["a11"]) * dj + int(it["t1"]) + ((T1 - 1) << 16)
            i0, j0, fy, fx = Y >> 17, X >> 17, (Y >> 9) & 255, (X >> 9) & 255
            out[i, j] = ((256 - fy) * (256 - fx) * tap(i0, j0) + (256 - fy) * fx * tap(i0, j0 + 1) + fy * (256 - fx) * tap(i0 + 1, j0)
                         + fy * fx * tap(i0 + 1, j0 + 1) + 32768) >> 16
    return out


def _blur_loops(img):
    T0, T1 = img.shape
    h = [[int(img[i, max(j - 1, 0)]) + 2 * int(img[i, j]) + int(img[i, min(j + 1, T1 - 1)]) for j in range(T1)] for i in range(T0)]
    return np.array([[(h[max(i - 1, 0)][j] + 2 * h[i][j] + h[min(i + 1, T0 - 1)][j] + 8) >> 4 for j in range(T1)] for i in range(T0)], np.uint8)


def test_loop_restatement_of_warp_and_blur():
    img = np.random.RandomState(1).randint(0, 256, (6, 5)).astype(np.uint8)
    warps = [dict(WARP, fill=7), dict(WARP, fill=-1), dict(a00=65536, a01=30000, a11=65536, fill=0), dict(a00=-262144, a10=262144, a11=-1, t0=6 << 17),
             dict(a00=65536, a11=65536, t0=-(6 << 17), t1=5 << 17, fill=200), dict(a00=70000, a01=-262144, a10=1, a11=50000, t1=-12345, fill=-1)]
    for w in warps:
        it = _items(**w)
        assert np.array_equal(A.augment_host(img[None], it)[0], _warp_loops(img, it[0])), w
    once = A.augment_host(img[None], _items(blur=1))[0]
    assert np.array_equal(once, _blur_loops(img))
    assert np.array_equal(A.augment_host(img[None], _items(blur=2))[0], _blur_loops(once))


def test_policy_draws():
    size = (100, 32, 1)
    a, b = A.AugmentPolicy(seed=3, p=0.8), A.AugmentPolicy(seed=3, p=0.8)
    state = np.random.get_state()
    first = [a.draw(n, size) for n in (8, 5, 8)]
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # the global stream is left alone
    assert all(x.tobytes() == b.draw(len(x), size).tobytes() for x in first)
    assert first[0].tobytes() != first[2].tobytes() and A.AugmentPolicy(seed=4, p=0.8).draw(8, size).tobytes() != first[0].tobytes()
    many = A.AugmentPolicy(seed=5, p=1.0, morph_p=1.0, blur_p=1.0).draw(500, size)
    assert A.check_items(many, size) is many and many.dtype == A.ITEM_DTYPE
    assert set(many["morph"]) == {-1, 1} and set(many["blur"]) == {1, 2} and (many["noise"] > 0).all() and len(set(many["seed"])) > 490
    assert (many["a00"] != 65536).any() and (many["a01"] != 0).any() and (many["t0"] != 0).any() and (many["gain"] != 256).any()
    wild = A.AugmentPolicy(seed=6, p=1.0, rotate=180., slant=9., scale=(0.1, 9.), shift=(1e6, 1e6), gain=(0., 9.), bias=(-999, 999), noise=(0, 999))
    A.check_items(wild.draw(200, (7, 5, 1)), (7, 5, 1))                  # whatever the ranges, the items stay inside the ABI's
    assert A.AugmentPolicy(seed=7, p=0.).draw(9, size).tobytes() == A.neutral_items(9).tobytes()
    assert len(A.AugmentPolicy().draw(0, size)) == 0


def test_check_items_refuses_what_the_library_refuses():
    for name, lo, hi in _RANGES(100, 32):
        for v in (lo - 1, hi + 1):
            with pytest.raises(ValueError):
                A.check_items(_items(3, **{name: v}), (100, 32, 1))
        for v in (lo, hi):
            A.check_items(_items(3, **{name: v}), (100, 32, 1))
    with pytest.raises(ValueError):
        A.check_items(np.zeros(3, np.int32), (100, 32, 1))
    with pytest.raises(ValueError):
        A.augment_host(np.zeros((2, 4, 4), np.uint8), A.neutral_items(3))


def _RANGES(T0, T1):
    c = A.MAX_COEF
    return [("a00", -c, c), ("a01", -c, c), ("a10", -c, c), ("a11", -c, c), ("t0", -(T0 << 17), T0 << 17), ("t1", -(T1 << 17), T1 << 17),
            ("fill", -1, 255), ("morph", -2, 2), ("blur", 0, 2), ("gain", 0, 1024), ("bias", -255, 255), ("noise", 0, 64)]


def _call(items, n=None, batch=4, imgh=100, imgw=32, in_p=IN_P, out8_p=OUT8_P, null=()):
    n = len(items) if n is None else n
    ptr = lambda name, v: None if name in null else (ctypes.c_void_p(v) if isinstance(v, int) else v)
    host = items.ctypes.data_as(ctypes.c_void_p)
    return native.lib().crnn_augment_batch(ptr("in", in_p), ptr("items", host), ptr("items_dev", FAKE), n, batch, imgh, imgw, ptr("table", FAKE),
                                           ptr("out", FAKE), ptr("out_u8", out8_p), None)


def test_every_refusal_of_crnn_augment_batch():
    assert "crnn_augment_batch" in native.parse_header()
    for name, lo, hi in _RANGES(100, 32):
        for v in (lo - 1, hi + 1):
            for row in (0, 2):
                items = A.neutral_items(3)
                items[name][row] = v
                assert _call(items) == ARG, (name, v, row)
    good = A.neutral_items(3)
    assert _call(good, n=5, batch=4) == ARG and _call(good, n=-1) == ARG and _call(good, n=0, batch=0) == ARG
    assert _call(good, imgh=0) == ARG and _call(good, imgw=0) == ARG and _call(good, imgh=-100) == ARG
    for name in ("in", "table", "out", "items", "items_dev"):
        assert _call(good, null=(name,)) == ARG, name
    assert _call(good, n=0, null=("in",)) == ARG and _call(good, n=0, null=("table", "items", "items_dev")) == ARG
    assert _call(good, imgh=129, imgw=128) == UNSUPPORTED and _call(good, imgh=16385, imgw=1) == UNSUPPORTED
    nbytes = 4 * 100 * 32
    for out8 in (IN_P, IN_P + nbytes - 1, IN_P - nbytes + 1):           # the same range, beginning on the last byte, ending on the first
        assert _call(good, out8_p=out8) == ARG, out8 - IN_P


# ---- Readf(augment=policy) --------------------------------------------------------------------------------------------------------------------
def _make_dataset(folder, n, seed=0):
    from PIL import Image, ImageDraw
    rs = np.random.RandomState(seed)
    names = []
    for i in range(n):
        word = "".join(rs.choice(list("abcdefghij0123"), size=rs.randint(2, 6)))
        img = Image.new("L", (20 + 12 * len(word), 28), color=235 if i % 3 else 30)
        ImageDraw.Draw(img).text((4, 6), word, fill=20 if i % 3 else 230)
        names.append(os.path.join(folder, "%d_%s_%d.png" % (i, word, i)))
        img.save(names[-1])
    return names


def _drain(gen, steps, batch, total):
    out = []
    full, rem = divmod(total, batch)
    for k in range(steps):
        inputs, _ = next(gen)
        rows = rem if (k == full and rem) else batch
        assert len(inputs["source_str"]) == rows
        out.append((np.array(inputs["the_input"][:rows, ..., 0]), inputs["the_labels"][:rows].copy(), inputs["input_length"][:rows].copy(),
                    inputs["label_length"][:rows].copy(), list(inputs["source_str"])))
    return out


def test_readf_with_a_policy(tmp_path):
    names = _make_dataset(str(tmp_path), 11)
    classes = {ch: i for i, ch in enumerate(U.get_lexicon())}
    kw = dict(img_size=(40, 32, 1), batch_size=4, classes=classes, max_len=23, transform_p=0.)
    steps = 5                                                          # two full batches, the tail of 3, and on into the second pass
    plain = _drain(U.Readf(normed=False, **kw).run_generator(names), steps, 4, 11)
    for normed in (False, True):
        got = _drain(U.Readf(normed=normed, augment=A.AugmentPolicy(seed=9, p=0.7), **kw).run_generator(names), steps, 4, 11)
        oracle = A.AugmentPolicy(seed=9, p=0.7)
        changed = 0
        for g, p in zip(got, plain):
            assert all(np.array_equal(a, b) for a, b in zip(g[1:4], p[1:4])) and g[4] == p[4]
            u8 = p[0].astype(np.uint8)
            assert np.array_equal(u8, p[0])
            want = A.augment_host(u8, oracle.draw(len(u8), kw["img_size"]))
            changed += int((want != u8).any(axis=(1, 2)).sum())
            assert np.array_equal(g[0], U.norm(want, 118.24236953981779, 36.72835353999682).astype(np.float64) if normed else want)
        assert changed > 5
    par = U.Readf(normed=True, augment=A.AugmentPolicy(seed=9, p=0.7), workers=2, chunk=3, **kw)
    two = _drain(par.run_generator(names), steps, 4, 11)
    par.close()
    for g, h in zip(got, two):
        assert all(np.array_equal(a, b) for a, b in zip(g[:4], h[:4])) and g[4] == h[4]
    again = _drain(U.Readf(normed=False, augment=None, **kw).run_generator(names), steps, 4, 11)      # no policy: what it produced before
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(again, plain))
