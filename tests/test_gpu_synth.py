"""-m gpu tests of the synthetic training words (csrc/synth.hip through crnn_mi355x/synth.py): the device's fp32 and uint8 batches equal
synth.synth_host bit for bit -- no tolerance, no excluded case --, over an item table that is itself checked to reach every branch of the
rule; WordSynth -> Augmenter equals augment_host(synth_host(...)); SynthReadf's device batches equal its host batches; a model trains on
them; train.py --synth runs in a child process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import utils as U
from crnn_mi355x import augment as A
from crnn_mi355x import ingest as I
from crnn_mi355x import native
from crnn_mi355x import synth as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crnn-ocr-lite_amd")
MEAN, STD = 118.24236953981779, 36.72835353999682
SHAPES = [(100, 32), (40, 32), (200, 32), (1, 1), (7, 5), (33, 3), (128, 128)]       # 16-byte stores where T0 * T1 is a multiple of 16
B, N, LMAX, NGLYPHS = 64, 61, 64, 38
GUARD = 4096


def _atlas():
    """3 random faces of 38 glyphs: glyphs without ink, a 64 x 64 glyph, negative and positive `left`, advances from 0 to the limit."""
    rs = np.random.RandomState(11)
    faces = []
    for f in range(3):
        face = []
        for g in range(NGLYPHS):
            if g in (5, 20 + f):
                face.append((None, 0, 0, int(rs.randint(0, 9))))
            elif g == 7:
                face.append((rs.randint(0, 256, (64, 64)).astype(np.uint8), -64 if f == 0 else 3, 0, 128 if f == 0 else 60))
            else:
                h, w = int(rs.randint(1, 25)), int(rs.randint(1, 21))
                face.append((rs.randint(0, 256, (h, w)).astype(np.uint8), int(rs.randint(-4, 5)), int(rs.randint(0, 64 - h + 1)),
                             int(rs.randint(0, w + 5))))
        faces.append(face)
    faces[1][9] = (np.full((3, 2), 255, np.uint8), 64, 61, 0)
    return S.GlyphAtlas.from_arrays(faces)


ATLAS = _atlas()
_REF = {}


def _table(shape):
    """61 items and their codes: every field at both ends of its range, words pushed out of the image on each side, the greys' corner cases,
    the rest from a seeded policy."""
    T0, T1 = shape
    rs = np.random.RandomState(T0 * 1000 + T1)
    codes = rs.randint(0, NGLYPHS, (N, LMAX)).astype(np.intc)
    lens = rs.randint(2, 13, N)
    far = S.MAX_OFFSET
    rows = [dict(len=0), dict(len=1), dict(len=LMAX), dict(len=LMAX, track=-8, jitter=8, sx=262144), dict(track=-8), dict(track=32, sx=131072),
            dict(jitter=8, seed=0xffffffff), dict(jitter=8, seed=1, sy=100000), dict(sx=16384, sy=262144), dict(sx=262144, sy=16384),
            dict(sx=16384, sy=16384, ox=5 << 16), dict(sx=262144, sy=262144, oy=-(9 << 16)),
            dict(ox=far), dict(ox=-far), dict(oy=far), dict(oy=-far), dict(ox=-(T0 << 16) - 65536), dict(oy=-(T1 << 16) - 65536),
            dict(ox=37777, oy=-23456), dict(ox=-(3 << 16) + 1, oy=65535),
            dict(fg=90, bg=90), dict(fg=10, bg=240), dict(fg=0, bg=255), dict(fg=255, bg=0), dict(fg=0, bg=0), dict(fg=255, bg=255),
            dict(face=2, len=3, track=-8), dict(face=1, len=5, jitter=3, seed=99)]
    t = S.identity_items(N)
    t["len"], t["face"], t["seed"] = lens, np.arange(N) % 3, rs.randint(0, 1 << 32, N, dtype=np.uint64)
    t["fg"], t["bg"] = rs.randint(150, 256, N), rs.randint(0, 90, N)
    for k, row in enumerate(rows):
        for name, v in row.items():
            t[name][k] = v
    codes[3, :8] = 7                                                   # the 64 x 64 glyphs side by side ...
    codes[26, :3] = [7, 9, 7]                                          # ... and, with face 2's advance of 60 - 8, drawn over one another
    policy = S.SynthPolicy(seed=T0 * 1000 + T1, track=(-3, 6), jitter=(0, 4))
    t[len(rows):] = policy.draw(codes[len(rows):], lens[len(rows):], ATLAS, shape)
    assert len(rows) < N - 8
    return S.check_items(t, codes, ATLAS.nfaces, NGLYPHS)


def _ref(shape):
    """(items, codes, host uint8): computed once per shape and left unchanged."""
    if shape not in _REF:
        items, codes = _table(shape)
        want = S.synth_host(ATLAS, codes, items, shape)
        for a in (items, codes, want):
            a.setflags(write=False)
        _REF[shape] = (items, codes, want)
    return _REF[shape]


def _launch(shape, items, codes, batch=B, normed=True, shift8=0, with_u8=True):
    """The entry point itself, both outputs with a guard region behind them -> (fp32 tensor with guard, uint8 tensor with guard, rc)."""
    T0, T1 = shape
    npx = T0 * T1
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    arena, glyphs = ATLAS.on_device(torch.device("cuda:0"))
    table = torch.from_numpy(I.norm_table(normed, MEAN, STD)).cuda()
    out = torch.full((batch * npx + GUARD,), 7.0, device="cuda")
    o8 = torch.full((shift8 + batch * npx + GUARD,), 7, dtype=torch.uint8, device="cuda")[shift8:]
    d_items, d_codes = torch.from_numpy(np.array(items).view(np.uint8)).cuda(), torch.from_numpy(np.array(codes)).cuda()
    items, codes = np.array(items), np.array(codes)
    rc = native.lib().crnn_synth_words(p(arena), ATLAS.arena.size, ATLAS.table.ctypes.data_as(ctypes.c_void_p), p(glyphs), ATLAS.nfaces, NGLYPHS,
                                       codes.ctypes.data_as(ctypes.c_void_p), p(d_codes), items.ctypes.data_as(ctypes.c_void_p), p(d_items),
                                       len(items), batch, codes.shape[1], T0, T1, p(table), p(out), p(o8) if with_u8 else None,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out, o8, rc


@pytest.mark.parametrize("shape", SHAPES)
def test_device_equals_host_bit_for_bit(shape):
    items, codes, want = _ref(shape)
    npx = shape[0] * shape[1]
    out, o8, rc = _launch(shape, items, codes)
    assert rc == 0
    got = o8[:B * npx].cpu().numpy().reshape((B,) + shape)
    bad = [k for k in range(N) if not np.array_equal(got[k], want[k])]
    assert not bad, "uint8 mismatch for items %s" % [(k, int((got[k] != want[k]).sum()), items[k]) for k in bad[:6]]
    f32 = out[:B * npx].cpu().numpy().reshape((B,) + shape)
    assert np.array_equal(f32[:N], I.norm_table(True, MEAN, STD)[want])
    assert not got[N:].any() and not f32[N:].any()                     # rows past n: zero
    assert (out[B * npx:] == 7.0).all() and (o8[B * npx:] == 7).all()  # the guard regions behind both outputs
    again, again8, rc = _launch(shape, items, codes)
    assert rc == 0 and torch.equal(again, out) and torch.equal(again8, o8)      # no atomics, no random numbers: equal bytes between calls
    assert (want.max(axis=(1, 2)) > want.min(axis=(1, 2))).sum() > N // 3 or shape == (1, 1)      # the images do show ink


def test_the_item_table_reaches_every_branch():
    """From the host functions alone, at 100 x 32 (the table is built the same way for every shape)."""
    shape = (100, 32)
    T0, T1 = shape
    items, codes, want = _ref(shape)
    assert {0, 1, LMAX} <= set(items["len"]) and items["track"].min() == -8 and items["track"].max() == 32
    assert items["jitter"].min() == 0 and items["jitter"].max() == 8 and set(items["face"]) == {0, 1, 2}
    for name in ("sx", "sy"):
        assert items[name].min() == S.MIN_SCALE and items[name].max() == S.MAX_SCALE
    assert (items["sx"] != items["sy"]).any() and (items["fg"] == items["bg"]).any() and (items["fg"] < items["bg"]).any()
    assert ((items["fg"] == 0) & (items["bg"] == 255)).any() and ((items["fg"] == 255) & (items["bg"] == 0)).any()
    assert items["ox"].min() == -S.MAX_OFFSET and items["ox"].max() == S.MAX_OFFSET and items["oy"].min() == -S.MAX_OFFSET and items["oy"].max() == S.MAX_OFFSET
    has, xa, xb, ya, yb = S.ink_box(ATLAS, np.array(codes), np.array(items))
    sx, sy, ox, oy = (items[k].astype(np.int64) for k in ("sx", "sy", "ox", "oy"))
    # a word wholly outside: even the tap at x0 + 1 (y0 + 1) of the last pixel lies before the ink, or the first pixel's tap behind it
    out_of = dict(before_x=has & (((sx * (T0 - 1) + ox) >> 16) + 1 < xa), behind_x=has & ((ox >> 16) >= xb),
                  before_y=has & (((sy * (T1 - 1) + oy) >> 16) + 1 < ya), behind_y=has & ((oy >> 16) >= yb))
    for side, rows in out_of.items():
        assert rows.any(), side
        assert all((want[k] == items["bg"][k]).all() for k in np.flatnonzero(rows)), side       # ... and is the ground alone
    table = ATLAS.table
    used = table[items["face"][:, None], np.array(codes)][np.arange(LMAX)[None, :] < items["len"][:, None]]
    assert (used["w"] == 0).any() and (used["w"] == 64).any() and (used["left"] < 0).any() and (used["advance"] == 0).any()
    inside = (sx + ox <= xa << 16) & ((xb - 1) << 16 <= sx * (T0 - 2) + ox) & (sy + oy <= ya << 16) & ((yb - 1) << 16 <= sy * (T1 - 2) + oy)
    assert (has & inside).sum() >= 25                                  # the policy's rows lie inside the image


def test_wordsynth_short_batches_and_the_narrow_path():
    shape = (100, 32)
    items, codes, want = _ref(shape)
    syn = U.WordSynth(ATLAS, shape + (1,), mean=MEAN, std=STD)
    f32, u8 = syn.run(codes, items, batch=B, return_u8=True)
    assert tuple(f32.shape) == (B, 100, 32, 1) and f32.dtype == torch.float32 and tuple(u8.shape) == (B, 100, 32) and u8.dtype == torch.uint8
    assert np.array_equal(u8.cpu().numpy()[:N], want) and np.array_equal(f32.cpu().numpy()[:N, ..., 0], I.norm_table(True, MEAN, STD)[want])
    assert not u8[N:].any() and not f32[N:].any()
    only = syn.run(codes, items, batch=B)
    assert torch.is_tensor(only) and torch.equal(only, f32)            # the uint8 output is optional
    part32, part8 = syn.run(codes[:5], items[:5], batch=9, return_u8=True)
    assert tuple(part32.shape) == (9, 100, 32, 1) and np.array_equal(part8.cpu().numpy()[:5], want[:5]) and not part8[5:].any() and not part32[5:].any()
    none32, none8 = syn.run(codes[:0], items[:0], batch=3, return_u8=True)      # nothing but the zero rows
    assert tuple(none8.shape) == (3, 100, 32) and not none32.any() and not none8.any()
    raw = U.WordSynth(ATLAS, shape + (1,), normed=False).run(codes, items)
    assert np.array_equal(raw.cpu().numpy()[..., 0], want.astype(np.float32))  # the identity table
    out, o8, rc = _launch(shape, items, codes, shift8=3)               # a uint8 output off the 16-byte boundary: one pixel per store
    assert rc == 0 and o8.data_ptr() % 16 == 3 and np.array_equal(o8[:B * 3200].cpu().numpy().reshape(B, 100, 32)[:N], want)
    assert (o8[B * 3200:] == 7).all() and (out[B * 3200:] == 7.0).all() and not o8[N * 3200:B * 3200].any()
    out, _, rc = _launch(shape, items, codes, with_u8=False)
    assert rc == 0 and np.array_equal(out[:N * 3200].cpu().numpy().reshape(N, 100, 32), I.norm_table(True, MEAN, STD)[want])
    with pytest.raises(ValueError):
        syn.run(codes[:5], items[:5], batch=4)
    bad = np.array(items)
    bad["jitter"][3] = 9
    with pytest.raises(ValueError):
        syn.run(codes, bad)
    out, o8, rc = _launch(shape, bad, codes)
    assert rc == -2 and (out == 7.0).all() and (o8 == 7).all()         # refused: nothing written


def test_wordsynth_then_augmenter_equals_the_host_paths():
    shape = (100, 32)
    items, codes, want = _ref(shape)
    aug_items = A.AugmentPolicy(seed=4, p=1.0, morph_p=1.0, blur_p=1.0).draw(N, shape)
    _, u8 = U.WordSynth(ATLAS, shape + (1,), mean=MEAN, std=STD).run(codes, items, batch=B, return_u8=True)
    f32, a8 = U.Augmenter(shape + (1,), mean=MEAN, std=STD).run(u8, aug_items, return_u8=True)
    host = A.augment_host(want, aug_items)
    assert np.array_equal(a8.cpu().numpy()[:N], host) and np.array_equal(f32.cpu().numpy()[:N, ..., 0], I.norm_table(True, MEAN, STD)[host])
    assert (host != want).any(axis=(1, 2)).sum() > N // 2


# ---- in the generator, in training ---------------------------------------------------------------------------------------------------------
WORDS = ["hello", "a", "w0rld", "0123456789", "mi355x", "synthetic", "z", "glyph-atlas", "qwertyuiopasdfghjklzxcv"]


def _classes():
    return {ch: i for i, ch in enumerate(U.get_lexicon())}


def _font_atlas(seed=7, nfaces=3, nglyphs=37):
    """Faces of a small font from arrays (no font file needed): ink 2..5 columns wide, 12 rows of line box, the last class a space."""
    rs = np.random.RandomState(seed)
    faces = []
    for _ in range(nfaces):
        face = []
        for g in range(nglyphs - 1):
            w, h, left = int(rs.randint(2, 6)), int(rs.randint(3, 11)), int(rs.randint(-1, 2))
            face.append((rs.randint(1, 256, (h, w)).astype(np.uint8), left, int(rs.randint(0, 13 - h)), max(0, left) + w + 1))
        faces.append(face + [(None, 0, 0, 4)])
    return S.GlyphAtlas.from_arrays(faces)


@pytest.mark.parametrize("augmented", [False, True])
def test_synthreadf_device_batches_equal_host_batches(augmented):
    atlas = _font_atlas()
    kw = dict(img_size=(100, 32, 1), batch_size=8, classes=_classes(), max_len=23, normed=True)
    make = lambda host: U.SynthReadf(WORDS, atlas, policy=U.SynthPolicy(seed=5), augment=A.AugmentPolicy(seed=6, p=0.8) if augmented else None,
                                     host=host, **kw).run_generator()
    dev, host = make(False), make(True)
    first = None
    for k in range(3):
        (d, dc), (h, hc) = next(dev), next(host)
        x = d["the_input"]
        assert torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (8, 100, 32, 1)
        assert np.array_equal(x.cpu().numpy(), h["the_input"].astype(np.float32)), k
        assert all(np.array_equal(d[key], h[key]) for key in ("the_labels", "input_length", "label_length", "source_str")) and np.array_equal(dc["ctc"], hc["ctc"])
        first = x.cpu().numpy() if first is None else first
    assert not np.array_equal(first, x.cpu().numpy()) and np.unique(first).size > 20


def _tiny_model(max_len=6):
    model = U.CRNN(num_classes=38, max_string_len=max_len, shape=(40, 32, 1), time_dense_size=32, n_units=64).get_model()
    model.compile(loss={"ctc": lambda y_true, y_pred: y_pred}, optimizer=U.optimizers.Adam(lr=0.001, beta_1=0.5, beta_2=0.999, clipnorm=5))
    return model


def test_three_training_steps_on_synthetic_batches():
    reader = U.SynthReadf(["ab", "hello", "w0rld", "x", "mi355x"], _font_atlas(), img_size=(40, 32, 1), normed=True, batch_size=4, classes=_classes(),
                          max_len=6, policy=U.SynthPolicy(seed=2), augment=A.AugmentPolicy(seed=2, p=1.0))
    model = _tiny_model()
    gen = reader.run_generator()
    hist = model.fit_generator(gen, steps_per_epoch=3, epochs=1, verbose=0)
    assert len(hist.history["loss"]) == 1 and np.isfinite(hist.history["loss"]).all()
    inputs, _ = next(gen)
    loss = model.train_on_batch(inputs["the_input"], inputs["the_labels"], inputs["input_length"], inputs["label_length"])
    assert np.isfinite(loss)


def test_train_cli_with_synth_in_a_child_process(tmp_path):
    data, out = tmp_path / "data", tmp_path / "out"
    os.makedirs(data); os.makedirs(out)                                # an empty --path: no validation set
    _font_atlas().save(str(tmp_path / "atlas.npz"))
    with open(tmp_path / "words.txt", "w") as f:
        f.write("\n".join(["hello", "a", "w0rld", "mi355x", "z", "synth", "ab12", "Caps", "no way", "x" * 40, ""]) + "\n")      # two are dropped
    done = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--path", str(data), "--save_path", str(out), "--model_name", "s1", "--nbepochs", "1",
                           "--norm", "--opt", "adam", "--lr", "0.001", "--batch_size", "64", "--n_units", "64", "--time_dense_size", "32", "--imgh", "40",
                           "--G", "0", "--synth", str(tmp_path / "words.txt"), "--synth_atlas", str(tmp_path / "atlas.npz"), "--synth_epoch", "128",
                           "--augment"], cwd=PKG, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-3000:]
    assert "2 words of" in done.stdout and "dropped" in done.stdout and "0 validation images" in done.stdout
    for f in ("final_weights.h5", "final_model.h5", "checkpoint_weights.h5", "loss_history.pickle.dat", "arguments.txt"):
        assert (out / "s1" / f).exists(), f
    import pickle
    hist = pickle.load(open(out / "s1" / "loss_history.pickle.dat", "rb"))
    assert len(hist["loss"]) == 1 and np.isfinite(hist["loss"]).all()
