#!/usr/bin/env python3
"""Synthetic training words on the device (crnn_mi355x/synth.py, csrc/synth.hip) at 100 x 32, batch 256 and 1024, words of 5..12 characters
from a three-face atlas built from arrays at the metrics of a 28-pixel font (no font file is needed):
  (a) device-event time per launch of crnn_synth_words and, in the same run as the yardsticks, of crnn_ingest_crops and of crnn_augment_batch
      with every stage on -- the synth launch as a multiple of each and as a share of the 5.90 ms train step (batch 256, README) -- and the
      bytes per second it achieves over the bytes that must move: 5 per output pixel plus the glyph bitmaps the words touch;
  (b) images/s of SynthReadf with and without an AugmentPolicy, against DeviceReadf(workers=0) from decoded page files in the same run and
      against the train step's 43.4 k images/s (README);
  (c) the compiler's resource report of csrc/synth.hip.
Every GPU step is a child process under its own time limit; the first one that fails ends the run.  usage: synth_bench.py [--out FILE]"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402
from augment_bench import ALL_ON, BATCHES, IMG_SIZE, LAUNCHES, TRAIN_STEP_MS, _events, make_pages  # noqa: E402  (the same page set and timer)

STEPS = [("kernel", 240), ("readf", 300)]            # (step, time limit in seconds)
TRAIN_IMAGES_PER_SEC = 43.4e3                        # the batch-256 train step (README)


def make_atlas(seed=0, nfaces=3, nglyphs=37):
    from crnn_mi355x import synth as S
    rs = np.random.RandomState(seed)
    faces = []
    for _ in range(nfaces):
        face = []
        for g in range(nglyphs):
            w, h = int(rs.randint(8, 19)), int(rs.randint(10, 29))
            face.append((rs.randint(0, 256, (h, w)).astype(np.uint8), int(rs.randint(0, 3)), int(rs.randint(0, 33 - h)), w + 2))
        faces.append(face)
    return S.GlyphAtlas.from_arrays(faces)


def make_words(n=4096, seed=1):
    from crnn_mi355x import data as D
    rs = np.random.RandomState(seed)
    lex = D.get_lexicon()[:-1]
    return ["".join(rs.choice(lex, size=rs.randint(5, 13))) for _ in range(n)]


def step_kernel(pnames, bboxs):
    import ctypes
    import torch
    from crnn_mi355x import augment as A, data as D, ingest as I, native, pages as PG, synth as S
    L = native.lib()
    pages = [D.read_img(n) for n in pnames]
    all_rects = np.array([I.box_slices(b, pg.shape) for n, pg in zip(pnames, pages) for b in bboxs[n]])
    all_index = np.repeat(np.arange(len(pages)), len(all_rects) // len(pages))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    atlas, words = make_atlas(), make_words()
    classes = {c: i for i, c in enumerate(D.get_lexicon())}
    out = {}
    for B in BATCHES:
        table = torch.from_numpy(I.norm_table()).cuda()
        x = torch.empty((B,) + IMG_SIZE, device="cuda")
        u8 = torch.empty((B,) + IMG_SIZE[:2], dtype=torch.uint8, device="cuda")
        # the yardsticks: the ingest launch and the augmentation with every stage on (scripts/augment_bench.py's)
        rects, index = all_rects[:B], all_index[:B]
        plans = I.plan_crops(rects[:, 1] - rects[:, 0], rects[:, 3] - rects[:, 2], IMG_SIZE)
        arena, offs = PG.pack_arena(pages)
        tab = I.build_table(pages, offs, index, rects, plans, IMG_SIZE)
        d_arena, d_tab = torch.from_numpy(arena).cuda(), torch.from_numpy(tab.view(np.uint8).copy()).cuda()
        ingest = lambda: L.crnn_ingest_crops(p(d_arena), len(arena), tab.ctypes.data_as(ctypes.c_void_p), p(d_tab), B, B, IMG_SIZE[0], IMG_SIZE[1],
                                             p(table), p(x), p(u8), stream())
        native.check(ingest(), "ingest_crops")
        res = {"ingest_us": _events(ingest)}
        aitems = A.neutral_items(B)
        for k, v in ALL_ON.items():
            aitems[k] = v
        aitems["seed"] = np.arange(B)
        d_aitems = torch.from_numpy(aitems.view(np.uint8).copy()).cuda()
        aug = lambda: L.crnn_augment_batch(p(u8), aitems.ctypes.data_as(ctypes.c_void_p), p(d_aitems), B, B, IMG_SIZE[0], IMG_SIZE[1], p(table), p(x),
                                           None, stream())
        native.check(aug(), "augment_batch")
        res["augment_all_us"] = _events(aug)
        # the synth launch on the words and items a SynthReadf batch has
        codes = np.full((B, 23), len(classes), np.intc)
        lens = np.zeros(B, np.int64)
        for b, w in enumerate(words[:B]):
            codes[b, :len(w)], lens[b] = [classes[c] for c in w], len(w)
        items = S.SynthPolicy(seed=1).draw(codes, lens, atlas, IMG_SIZE)
        d_arena2, d_glyphs = atlas.on_device(torch.device("cuda:0"))
        d_items, d_codes = torch.from_numpy(items.view(np.uint8).copy()).cuda(), torch.from_numpy(codes).cuda()
        synth = lambda: L.crnn_synth_words(p(d_arena2), atlas.arena.size, atlas.table.ctypes.data_as(ctypes.c_void_p), p(d_glyphs), atlas.nfaces,
                                           atlas.nglyphs, codes.ctypes.data_as(ctypes.c_void_p), p(d_codes), items.ctypes.data_as(ctypes.c_void_p),
                                           p(d_items), B, B, codes.shape[1], IMG_SIZE[0], IMG_SIZE[1], p(table), p(x), p(u8), stream())
        native.check(synth(), "synth_words")
        res["synth_us"] = _events(synth)
        torch.cuda.synchronize()
        assert np.array_equal(u8.cpu().numpy(), S.synth_host(atlas, codes, items, IMG_SIZE)), "the timed launch is not synth_host's batch"
        g = atlas.table[items["face"][:, None], np.where(np.arange(23)[None, :] < lens[:, None], codes, 0)]
        touched = int((g["w"].astype(np.int64) * g["h"] * (np.arange(23)[None, :] < lens[:, None])).sum())
        res["must_move_bytes"] = 5 * B * IMG_SIZE[0] * IMG_SIZE[1] + touched
        out[str(B)] = res
    return out


def step_readf(pnames, bboxs):
    import torch
    from crnn_mi355x import augment as A, data as D, ingest as I, synth as S
    classes = {c: i for i, c in enumerate(D.get_lexicon())}
    atlas, words = make_atlas(), make_words()

    def rate(gen, B):
        next(gen)                                    # warm-up: staging buffers, first launches
        torch.cuda.synchronize()
        t, k = time.time(), 0
        while time.time() - t < 4.0:
            next(gen)
            k += B
        torch.cuda.synchronize()
        return round(k / (time.time() - t), 1)
    out = {}
    for B in BATCHES:
        res = {}
        for label, policy in (("plain", None), ("augmented", A.AugmentPolicy(seed=1))):
            r = S.SynthReadf(words, atlas, img_size=IMG_SIZE, max_len=23, normed=True, batch_size=B, classes=classes, policy=S.SynthPolicy(seed=1),
                             augment=policy)
            res["synth_readf_%s_images_per_sec" % label] = rate(r.run_generator(), B)
        r = I.DeviceReadf(img_size=IMG_SIZE, max_len=23, normed=True, batch_size=B, classes=classes, transform_p=0.)
        res["device_readf_images_per_sec"] = rate(r.run_generator(pnames, bboxs=bboxs), B)
        out[str(B)] = res
    return out


def resource_report():
    """The compiler's report of csrc/synth.hip (no GPU needed) -> lines, or a note when hipcc is not at hand."""
    src = os.path.join(ROOT, "crnn-ocr-lite_amd", "csrc", "synth.hip")
    with tempfile.TemporaryDirectory() as tmp:
        try:
            done = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                                   "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "synth.o")],
                                  capture_output=True, text=True, timeout=300)
        except (OSError, subprocess.TimeoutExpired) as e:
            return ["  not available: %s" % e]
    lines = []
    for m in re.finditer(r"remark: +(Function Name: .*?|\w[\w /\[\]]*: \S+) \[-Rpass-analysis", done.stderr):
        text = m.group(1)
        lines.append(("  " if text.startswith("Function Name") else "      ") + text)
    return lines or ["  not available (hipcc exit %d)" % done.returncode]


def child(step, folder):
    spec = json.load(open(os.path.join(folder, "inputs.json")))
    args = (spec["pnames"], {k: [tuple(b) for b in v] for k, v in spec["bboxs"].items()})
    print("RESULT " + json.dumps({"kernel": step_kernel, "readf": step_readf}[step](*args)), flush=True)


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        return child(sys.argv[2], sys.argv[3])
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    report = resource_report()
    folder = tempfile.mkdtemp()
    pnames, bboxs = make_pages(folder)
    json.dump({"pnames": pnames, "bboxs": bboxs}, open(os.path.join(folder, "inputs.json"), "w"))
    res = {str(B): {} for B in BATCHES}
    for step, limit in STEPS:
        done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, folder],
                              capture_output=True, text=True)
        lines = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            print("step %s failed (exit %d); stopping\n%s" % (step, done.returncode, done.stderr[-3000:]), flush=True)
            return 1
        for k, v in json.loads(lines[-1][7:]).items():
            res[k].update(v)
        print("step %s done" % step, file=sys.stderr, flush=True)
    lines = ["synthetic training words on the device: %d x %d, words of 5..12 characters, a 3-face atlas from arrays at the metrics of a 28-pixel font; "
             "device events over %d launches per figure; page set of the yardsticks: 16 PNG pages of 1600 x 1200, 64 word boxes each"
             % (IMG_SIZE[0], IMG_SIZE[1], LAUNCHES),
             "cov is gathered straight from the atlas (the one design built: no composed line in LDS, so there is no second time to record)"]
    for B in BATCHES:
        r = res[str(B)]
        us = r["synth_us"]
        lines += ["", "batch %d" % B,
                  "  crnn_ingest_crops (yardstick):              %8.2f us per launch" % r["ingest_us"],
                  "  crnn_augment_batch, every stage on (yardstick): %4.2f us per launch" % r["augment_all_us"],
                  "  crnn_synth_words:                           %8.2f us per launch = %.2f x the ingest launch, %.2f x the augment launch, %.4f of the "
                  "%.2f ms train step" % (us, us / r["ingest_us"], us / r["augment_all_us"], us / (TRAIN_STEP_MS * 1e3), TRAIN_STEP_MS),
                  "    bytes that must move (5 per output pixel + the glyph bitmaps touched): %d -> %.1f GB/s achieved"
                  % (r["must_move_bytes"], r["must_move_bytes"] / us / 1e3)]
        a, b, d = r["synth_readf_plain_images_per_sec"], r["synth_readf_augmented_images_per_sec"], r["device_readf_images_per_sec"]
        lines.append("  SynthReadf: %9.1f images/s without a policy, %9.1f images/s with AugmentPolicy() (%.2f x); DeviceReadf(workers=0) from the page "
                     "files in this run: %9.1f images/s; the train step consumes %.1f k images/s -> SynthReadf feeds %.2f / %.2f of it"
                     % (a, b, b / a, d, TRAIN_IMAGES_PER_SEC / 1e3, a / TRAIN_IMAGES_PER_SEC, b / TRAIN_IMAGES_PER_SEC))
    lines += ["", "compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; <16>: 16 pixels per thread and 16-byte stores, "
              "<1>: one pixel per store):"] + report
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
