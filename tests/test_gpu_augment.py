"""-m gpu tests of the training augmentation (csrc/augment.hip through crnn_mi355x/augment.py): the device's fp32 and uint8 batches equal
augment.augment_host bit for bit -- no tolerance, no excluded case --, over an item table that is itself checked to reach every branch of
the rule; DeviceReadf(augment=policy) yields the batches of Readf(augment=policy); a model trains on them; train.py --device_ingest --augment
runs and validates on unaugmented batches."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import utils as U
from crnn_mi355x import augment as A
from crnn_mi355x import ingest as I
from crnn_mi355x import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
MEAN, STD = 118.24236953981779, 36.72835353999682
SHAPES = [(100, 32), (40, 32), (200, 32), (1, 1), (7, 5), (33, 3), (128, 128)]       # (128, 128): the LDS limit
B, N = 64, 61
ALL = dict(a00=60000, a01=9000, a10=-7000, a11=70000, t0=40000, t1=-90000, morph=1, blur=1, gain=400, bias=-30, noise=64, seed=12345)


def _table(shape):
    """61 items: every stage alone at both ends of its range, warps that push the whole image out, all stages together, the rest from a
    seeded policy with every stage on."""
    T0, T1 = shape
    c = A.MAX_COEF
    rows = [dict(a00=c), dict(a00=-c), dict(a01=c), dict(a01=-c, fill=0), dict(a10=c, fill=255), dict(a10=-c), dict(a11=c), dict(a11=-c, fill=9),
            dict(t0=T0 << 17, fill=0), dict(t0=-(T0 << 17), fill=255), dict(t1=T1 << 17, fill=77), dict(t1=-(T1 << 17), fill=-1),
            dict(t0=T0 << 17, t1=-(T1 << 17), fill=-1), dict(t0=T0 << 16, fill=3), dict(t1=-(1 << 16), fill=200), dict(t0=1, fill=0),
            dict(a00=0, a11=0, fill=5), dict(a00=0, a01=65536, a10=65536, a11=0),
            dict(morph=-2), dict(morph=-1), dict(morph=1), dict(morph=2), dict(blur=1), dict(blur=2),
            dict(gain=0), dict(gain=1024), dict(bias=-255), dict(bias=255), dict(gain=1024, bias=255), dict(gain=1024, bias=-255), dict(gain=257),
            dict(noise=64, seed=0), dict(noise=64, seed=0xffffffff), dict(noise=1, seed=7), dict(noise=33, seed=0x80000000),
            dict(ALL, fill=7), dict(ALL, fill=-1), dict(ALL, morph=-2, blur=2, gain=1024, bias=100, fill=255)]
    t = A.neutral_items(N)
    for k, row in enumerate(rows):
        for name, v in row.items():
            t[name][k] = v
    policy = A.AugmentPolicy(seed=T0 * 1000 + T1, p=1.0, morph_p=1.0, blur_p=1.0, rotate=8., shift=(T0 / 4., T1 / 4.), fill=40)
    t[len(rows):] = policy.draw(N - len(rows), shape)
    assert len(rows) < N - 8
    return A.check_items(t, shape)


def _images(shape, seed=0):
    """64 images: noise, smooth ramps, a bright bar on a dark ground (ink as the ingest leaves it), and flat black / white."""
    T0, T1 = shape
    rs = np.random.RandomState(seed)
    x = rs.randint(0, 256, (B,) + shape).astype(np.uint8)
    ramp = ((np.arange(T0)[:, None] * 3 + np.arange(T1)[None, :] * 5) % 256).astype(np.uint8)
    x[1::4] = ramp
    bar = np.full(shape, 12, np.uint8)
    bar[T0 // 4:T0 - T0 // 4, T1 // 3:T1 - T1 // 3] = 240
    x[2::4] = bar
    x[24], x[25], x[26], x[27] = 255, 255, 0, 255        # flat images under the rows of gain 0 / 1024 and bias -255 / 255
    return x


_REF = {}


def _ref(shape):
    """(images, items, host uint8 of the first N): computed once per shape and left unchanged."""
    if shape not in _REF:
        x, items = _images(shape), _table(shape)
        want = A.augment_host(x[:N], items)
        for a in (x, items, want):
            a.setflags(write=False)
        _REF[shape] = (x, items, want)
    return _REF[shape]


def _device(shape, x, items, batch=None, return_u8=True, normed=True):
    aug = U.Augmenter(shape + (1,), normed=normed, mean=MEAN, std=STD)
    got = aug.run(torch.from_numpy(np.array(x)).cuda(), items, batch=batch, return_u8=return_u8)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("shape", SHAPES)
def test_device_equals_host_bit_for_bit(shape):
    x, items, want = _ref(shape)
    f32, u8 = _device(shape, x, items, batch=B)
    assert tuple(f32.shape) == (B,) + shape + (1,) and f32.dtype == torch.float32 and tuple(u8.shape) == (B,) + shape and u8.dtype == torch.uint8
    got = u8.cpu().numpy()
    bad = [k for k in range(N) if not np.array_equal(got[k], want[k])]
    assert not bad, "uint8 mismatch for items %s" % [(k, int((got[k] != want[k]).sum()), items[k]) for k in bad[:6]]
    table = I.norm_table(True, MEAN, STD)
    assert np.array_equal(f32.cpu().numpy()[:N, ..., 0], table[want])
    assert not got[N:].any() and not f32.cpu().numpy()[N:].any()          # rows past n: zero
    assert (want != x[:N]).any(axis=(1, 2)).sum() > (N * 3) // 4 or shape == (1, 1)


def test_the_item_table_reaches_every_branch():
    """From the host functions alone, at 100 x 32 (the table is built the same way for every shape)."""
    shape = (100, 32)
    T0, T1 = shape
    x, items, _ = _ref(shape)
    reach = dict(fill=0, clamped=0, tone_lo=0, tone_hi=0, noise_lo=0, noise_hi=0)
    di = (2 * np.arange(T0, dtype=np.int64) - (T0 - 1))[:, None]
    dj = (2 * np.arange(T1, dtype=np.int64) - (T1 - 1))[None, :]
    for k, it in enumerate(items):
        Y = int(it["a00"]) * di + int(it["a01"]) * dj + int(it["t0"]) + ((T0 - 1) << 16)
        X = int(it["a10"]) * di + int(it["a11"]) * dj + int(it["t1"]) + ((T1 - 1) << 16)
        i0, j0 = Y >> 17, X >> 17
        outside = ((i0 < 0) | (i0 + 1 > T0 - 1) | (j0 < 0) | (j0 + 1 > T1 - 1)).any()
        reach["fill" if it["fill"] >= 0 else "clamped"] += bool(outside)
        one = items[k:k + 1].copy()
        one["gain"], one["bias"], one["noise"] = 256, 0, 0
        v = A.augment_host(x[k:k + 1], one)[0].astype(np.int64)                       # the pixels in front of the tone stage
        raw = ((v - 128) * int(it["gain"]) + (128 + int(it["bias"])) * 256 + 128) >> 8
        reach["tone_lo"] += bool((raw < 0).any())
        reach["tone_hi"] += bool((raw > 255).any())
        one["gain"], one["bias"] = it["gain"], it["bias"]
        v = A.augment_host(x[k:k + 1], one)[0].astype(np.int64)                       # ... in front of the noise stage
        h = A.mix32(np.uint64(int(it["seed"])) ^ ((np.arange(T0 * T1, dtype=np.uint64) * np.uint64(0x9E3779B9)) & np.uint64(0xffffffff)))
        s = sum(((h >> np.uint64(8 * q)) & np.uint64(255)).astype(np.int64) for q in range(4)).reshape(shape) - 510
        raw = v + ((s * int(it["noise"])) >> 8)
        reach["noise_lo"] += bool((raw < 0).any())
        reach["noise_hi"] += bool((raw > 255).any())
    assert all(v >= 2 for v in reach.values()), reach
    assert set(items["morph"]) == {-2, -1, 0, 1, 2} and set(items["blur"]) == {0, 1, 2}
    for name, lo, hi in (("gain", 0, 1024), ("bias", -255, 255), ("noise", 0, 64), ("fill", -1, 255), ("a00", -A.MAX_COEF, A.MAX_COEF),
                         ("a01", -A.MAX_COEF, A.MAX_COEF), ("a10", -A.MAX_COEF, A.MAX_COEF), ("a11", -A.MAX_COEF, A.MAX_COEF),
                         ("t0", -(T0 << 17), T0 << 17), ("t1", -(T1 << 17), T1 << 17)):
        assert items[name].min() == lo and items[name].max() == hi, name


def test_short_batches_optional_uint8_and_repeatability():
    shape = (100, 32)
    x, items, want = _ref(shape)
    f32, u8 = _device(shape, x, items, batch=B)
    again32, again8 = _device(shape, x, items, batch=B)
    assert torch.equal(f32, again32) and torch.equal(u8, again8)          # no atomics, no random numbers: equal bytes between calls
    only = _device(shape, x, items, batch=B, return_u8=False)
    assert torch.is_tensor(only) and torch.equal(only, f32)               # the uint8 output is optional
    part32, part8 = _device(shape, x, items[:5], batch=9)
    assert tuple(part32.shape) == (9, 100, 32, 1) and np.array_equal(part8.cpu().numpy()[:5], want[:5]) and not part8[5:].any() and not part32[5:].any()
    none32, none8 = _device(shape, x, items[:0], batch=3)                 # nothing but the zero rows
    assert not none32.any() and not none8.any()
    raw32, raw8 = _device(shape, x, items, batch=B, normed=False)         # the identity table
    assert np.array_equal(raw32.cpu().numpy()[:N, ..., 0], want.astype(np.float32)) and torch.equal(raw8, u8)
    odd = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), x.ravel()])).cuda()[3:].view(B, 100, 32)      # a batch that begins off a 16-byte boundary
    aug = U.Augmenter(shape + (1,), mean=MEAN, std=STD)
    assert odd.data_ptr() % 16 == 3 and torch.equal(aug.run(odd, items, return_u8=True)[1], u8)
    with pytest.raises(ValueError):
        aug.run(odd, items[:5], batch=4)
    with pytest.raises(ValueError):
        aug.run(odd.float(), items)
    bad = items.copy()
    bad["blur"][3] = 3
    with pytest.raises(ValueError):
        aug.run(odd, bad)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out, dev_items = torch.full((B, 100, 32), 7.0, device="cuda"), torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    rc = native.lib().crnn_augment_batch(p(odd), bad.ctypes.data_as(ctypes.c_void_p), p(dev_items), N, B, 100, 32, p(aug.table), p(out), None, stream)
    torch.cuda.synchronize()
    assert rc == -2 and (out == 7.0).all()                                # refused: nothing written


# ---- after the ingest, in the generators, in training ------------------------------------------------------------------------------------------
H, W = 120, 260


def _page(seed=0):
    rs = np.random.RandomState(seed)
    page = rs.randint(170, 256, (H, W)).astype(np.uint8)
    for k in range(6):
        r, c = 8 + 18 * k, 10 + 37 * k
        page[r:r + 12, c:c + 60] = rs.randint(0, 90, (12, 60))
    return page


def _page_boxes():
    return [("w%d" % k if k % 3 else None, 8 + 18 * k - 2, 10 + 37 * k - 3, 8 + 18 * k + 14, 10 + 37 * k + 63) for k in range(6)]     # (word, r0, c0, r1, c1)


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


def _classes():
    return {ch: i for i, ch in enumerate(U.get_lexicon())}


def test_neutral_items_after_the_ingest_give_the_ingests_own_fp32():
    img_size = (100, 32, 1)
    page = _page()
    ing = U.DeviceIngest(img_size, mean=MEAN, std=STD)
    (x, u8), _ = ing.pages([page], [_page_boxes()], batch=8, return_u8=True)
    y, y8 = U.Augmenter(img_size, mean=MEAN, std=STD).run(u8, A.neutral_items(6), return_u8=True)
    assert torch.equal(x, y) and torch.equal(u8, y8) and u8[:6].any() and not y[6:].any()


def _drain(gen, steps, batch_size, total):
    out = []
    full, rem = divmod(total, batch_size)
    for k in range(steps):
        inputs, _ = next(gen)
        x = inputs["the_input"]
        x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        rows = rem if (k == full and rem) else batch_size              # the first pass' short tail: the rows past it are undefined on the host
        assert x.shape[0] == batch_size and len(inputs["source_str"]) == rows
        out.append((x[:rows].astype(np.float32), inputs["the_labels"][:rows].copy(), inputs["input_length"][:rows].copy(),
                    inputs["label_length"][:rows].copy(), list(inputs["source_str"]), x[rows:].astype(np.float32) if torch.is_tensor(inputs["the_input"]) else None))
    return out


@pytest.mark.parametrize("p", [0., 0.7])
def test_device_generator_equals_readf_under_the_same_policy(tmp_path, p):
    from PIL import Image
    names = _make_dataset(str(tmp_path), 19)
    pname = os.path.join(str(tmp_path), "page.png")
    Image.fromarray(_page(3)).save(pname)
    order = names[:7] + [pname] + names[7:]
    bboxs = dict({n: [n] for n in names}, **{pname: _page_boxes()})
    kw = dict(img_size=(100, 32, 1), normed=True, batch_size=8, classes=_classes(), max_len=23, transform_p=p)
    total, steps = 25, 6                                               # three full batches, the tail of 1, and on into the second pass
    np.random.seed(3)
    host = _drain(U.Readf(augment=A.AugmentPolicy(seed=11, p=0.8), **kw).run_generator(order, bboxs=bboxs), steps, 8, total)
    np.random.seed(3)
    dev = _drain(U.DeviceReadf(augment=A.AugmentPolicy(seed=11, p=0.8), **kw).run_generator(order, bboxs=bboxs), steps, 8, total)
    np.random.seed(3)
    plain = _drain(U.DeviceReadf(**kw).run_generator(order, bboxs=bboxs), steps, 8, total)
    assert len(host) == len(dev) == steps
    for k, (h, d, q) in enumerate(zip(host, dev, plain)):
        assert h[0].dtype == d[0].dtype == np.float32 and np.array_equal(h[0], d[0]), k
        assert all(np.array_equal(a, b) for a, b in zip(h[1:4], d[1:4])) and h[4] == d[4] == q[4], k
        assert not d[5].any(), k                                       # rows past the short tail: zero
        assert not np.array_equal(d[0], q[0]), k                       # the policy really changes the batch
    par = U.DeviceReadf(augment=A.AugmentPolicy(seed=11, p=0.8), workers=2, chunk=5, **kw)
    np.random.seed(3)
    two = _drain(par.run_generator(order, bboxs=bboxs), steps, 8, total)
    par.close()
    assert all(np.array_equal(a[0], b[0]) and a[4] == b[4] for a, b in zip(dev, two))


def _tiny_model(max_len=6):
    model = U.CRNN(num_classes=38, max_string_len=max_len, shape=(40, 32, 1), time_dense_size=32, n_units=64).get_model()
    model.compile(loss={"ctc": lambda y_true, y_pred: y_pred}, optimizer=U.optimizers.Adam(lr=0.001, beta_1=0.5, beta_2=0.999, clipnorm=5))
    return model


def test_three_training_steps_on_augmented_device_batches(tmp_path):
    names = _make_dataset(str(tmp_path), 12)
    reader = U.DeviceReadf(img_size=(40, 32, 1), normed=True, batch_size=4, classes=_classes(), max_len=6, transform_p=0.7,
                           augment=A.AugmentPolicy(seed=2, p=1.0))
    model = _tiny_model()
    gen = reader.run_generator(names)
    hist = model.fit_generator(gen, steps_per_epoch=3, epochs=1, verbose=0)
    assert len(hist.history["loss"]) == 1 and np.isfinite(hist.history["loss"]).all()
    inputs, _ = next(gen)
    loss = model.train_on_batch(inputs["the_input"], inputs["the_labels"], inputs["input_length"], inputs["label_length"])
    assert np.isfinite(loss)


def test_train_cli_with_device_ingest_and_augment(tmp_path, monkeypatch):
    sys.path.insert(0, PKG)
    import train as train_cli
    from crnn_mi355x import surface
    data, out = tmp_path / "data", tmp_path / "out"
    os.makedirs(data); os.makedirs(out)
    _make_dataset(str(data), 16)
    seen = []
    evaluate = surface.Model.evaluate_generator

    def recording(self, generator, steps):
        """The validation batches as fit_generator draws them, with np.random as it was before the first one."""
        state, batches = np.random.get_state(), []

        def tee():
            for inputs, outputs in generator:
                batches.append((inputs["the_input"].cpu().numpy().copy(), list(inputs["source_str"])))
                yield inputs, outputs
        seen.append((state, batches))
        return evaluate(self, tee(), steps)
    monkeypatch.setattr(surface.Model, "evaluate_generator", recording)
    np.random.seed(0)
    train_cli.main(["--path", str(data), "--save_path", str(out), "--model_name", "m1", "--nbepochs", "1", "--norm", "--opt", "adam", "--lr", "0.001",
                    "--batch_size", "4", "--n_units", "64", "--time_dense_size", "32", "--imgh", "40", "--train_portion", "0.75", "--G", "0",
                    "--device_ingest", "--augment", "--augment_p", "1.0"])
    for f in ("final_weights.h5", "final_model.h5", "checkpoint_weights.h5", "loss_history.pickle.dat"):
        assert (out / "m1" / f).exists(), f
    assert "augment=True" in open(out / "m1" / "arguments.txt").read()
    (state, batches), = seen                                          # one epoch: one validation pass of one batch
    assert len(batches) == 1 and len(batches[0][1]) == 4
    # the validation files, as train.py picks them
    files = [os.path.join(dp, f) for dp, dn, fs in os.walk(str(data)) for f in fs]
    np.random.RandomState(42).shuffle(files)
    val = files[12:]
    max_len = max(U.get_lengths(files[:12]).values())
    np.random.set_state(state)
    plain = U.DeviceReadf(img_size=(40, 32, 1), normed=True, batch_size=4, classes=_classes(), max_len=max_len, transform_p=0.7)
    inputs, _ = next(plain.run_generator(val, downsample_factor=2))
    assert list(inputs["source_str"]) == batches[0][1] and np.array_equal(inputs["the_input"].cpu().numpy(), batches[0][0])
    policy = A.AugmentPolicy(seed=1, p=1.0)                           # ... and augmenting them would have shown
    x8 = np.clip(np.rint(batches[0][0][..., 0] * STD + MEAN), 0, 255).astype(np.uint8)
    assert not np.array_equal(A.augment_host(x8, policy.draw(4, (40, 32, 1))), x8)
