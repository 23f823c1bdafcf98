#!/usr/bin/env python3
"""Input side at batch 1024, 100 x 32: the device ingest (crnn_mi355x/ingest.py, csrc/ingest.hip) against the host loader (data.Readf) on the
same synthetic inputs -- a page set (16 pages with 64 word boxes each, PNG) and a word-file set (1024 JPEG crops, MJSynth-like).  Prints
  (a) the kernel's time by HIP events,
  (b) images/s of the device path end to end -- host planning + one copy + kernel from decoded pages, and through DeviceReadf (workers 0 / 16) from the files,
  (c) images/s of Readf(workers=0) and Readf(workers=16),
and the two ratios that matter: (b) over (c), and (a) per image over the 5.2-5.3 us/image of forward + beam search (README).
Every step is a child process under its own time limit; the first one that fails ends the run.  usage: ingest_bench.py [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd")]
import numpy as np  # noqa: E402

BATCH, IMG_SIZE = 1024, (100, 32, 1)
STEPS = [("kernel", 120), ("device", 300), ("readf0", 300), ("readf16", 300)]      # (step, time limit in seconds)
LAUNCHES = 4000                                                                      # timed launches per set (a window of 0.1-0.2 s)
FORWARD_BEAM_US = 5.25                                                               # per image, predict + beam search at batch 1024 (README)


def make_inputs(folder):
    """-> (page names, {page: boxes}, word-file names); written once, every step reads the same files."""
    from PIL import Image
    rs = np.random.RandomState(0)
    pnames, bboxs = [], {}
    for k in range(16):                                              # a scanned page: bright paper, dark strokes
        page = rs.randint(170, 256, (1600, 1200)).astype(np.uint8)
        boxes = []
        for i in range(64):
            hc, wc = int(rs.randint(18, 41)), int(rs.randint(40, 161))
            r0, c0 = int(rs.randint(0, 1600 - hc)), int(rs.randint(0, 1200 - wc))
            page[r0 + 4:r0 + hc - 4, c0 + 4:c0 + wc - 4:3] = rs.randint(0, 80)
            boxes.append(("w%d" % i, r0, c0, r0 + hc, c0 + wc))
        name = os.path.join(folder, "page%02d.png" % k)
        Image.fromarray(page).save(name)
        pnames.append(name)
        bboxs[name] = boxes
    words = ["hello", "world", "overfilled", "cellist", "amd", "mi355x", "ocr", "keras"]
    fnames = []
    for i in range(BATCH):                                           # MJSynth-like crops: 31 px high, 60-124 px wide JPEGs
        a = (rs.rand(31, 60 + 8 * (i % 9), 3) * 255).astype(np.uint8)
        fnames.append(os.path.join(folder, "%d_%s_%d.jpg" % (i, words[i % len(words)], i)))
        Image.fromarray(a).save(fnames[-1], quality=90)
    return pnames, bboxs, fnames


def _classes():
    from crnn_mi355x import data as D
    return {c: i for i, c in enumerate(D.get_lexicon())}


def _rate(gen, seconds=4.0, sync=None):
    next(gen)                                                        # warm-up: pools, staging buffers, first launch
    t, k = time.time(), 0
    while time.time() - t < seconds:
        next(gen)
        k += BATCH
    if sync is not None:
        sync()
    return round(k / (time.time() - t), 1)


def step_kernel(pnames, bboxs, fnames):
    import ctypes
    import torch
    from crnn_mi355x import data as D, ingest as I, native, pages as PG
    out = {}
    for label, pages, rects, index in _decoded(pnames, bboxs, fnames):
        plans = I.plan_crops(rects[:, 1] - rects[:, 0], rects[:, 3] - rects[:, 2], IMG_SIZE)
        arena, offs = PG.pack_arena(pages)
        tab = I.build_table(pages, offs, index, rects, plans, IMG_SIZE)
        d_arena, d_tab = torch.from_numpy(arena).cuda(), torch.from_numpy(tab.view(np.uint8).copy()).cuda()
        table = torch.from_numpy(I.norm_table()).cuda()
        x = torch.empty((BATCH,) + IMG_SIZE, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        fn = lambda: native.lib().crnn_ingest_crops(p(d_arena), len(arena), tab.ctypes.data_as(ctypes.c_void_p), p(d_tab), BATCH, BATCH, IMG_SIZE[0],
                                                    IMG_SIZE[1], p(table), p(x), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        for _ in range(3):
            native.check(fn(), "ingest_crops")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / LAUNCHES                          # (includes the entry point's host-side check of the table between launches)
        out[label] = {"kernel_us_per_batch": round(us, 1), "kernel_us_per_image": round(us / BATCH, 4), "arena_bytes": int(len(arena))}
    return out


def _decoded(pnames, bboxs, fnames):
    from crnn_mi355x import data as D, ingest as I
    pages = [D.read_img(n) for n in pnames]
    rects = np.array([I.box_slices(b, pg.shape) for n, pg in zip(pnames, pages) for b in bboxs[n]])
    yield "pages", pages, rects, np.repeat(np.arange(16), 64)
    files = [D.read_img(n) for n in fnames]
    yield "files", files, np.array([(0, f.shape[0], 0, f.shape[1]) for f in files]), np.arange(len(files))


def step_device(pnames, bboxs, fnames):
    import torch
    from crnn_mi355x import ingest as I
    out = {}
    ing = I.DeviceIngest(IMG_SIZE)
    for label, pages, rects, index in _decoded(pnames, bboxs, fnames):
        def memory():                                                # decoded pages in memory: planning + packing + one copy + kernel
            while True:
                yield ing.crops(pages, index, rects, ing.plan(rects, 0.), batch=BATCH)
        out[label] = {"from_memory_images_per_sec": _rate(memory(), sync=torch.cuda.synchronize)}
    kw = dict(img_size=IMG_SIZE, max_len=23, normed=True, batch_size=BATCH, classes=_classes(), transform_p=0.)
    for workers in (0, 16):
        for label, names, bb in (("pages", pnames, bboxs), ("files", fnames, {})):
            r = I.DeviceReadf(workers=workers, **kw)
            out[label]["device_readf_workers_%d_images_per_sec" % workers] = _rate(r.run_generator(names, bboxs=bb), sync=torch.cuda.synchronize)
            r.close()
    return out


def step_readf(workers, pnames, bboxs, fnames):
    from crnn_mi355x import data as D
    out = {}
    for label, names, bb in (("pages", pnames, bboxs), ("files", fnames, {})):
        r = D.Readf(img_size=IMG_SIZE, max_len=23, normed=True, batch_size=BATCH, classes=_classes(), transform_p=0., workers=workers)
        out[label] = {"readf_workers_%d_images_per_sec" % workers: _rate(r.run_generator(names, bboxs=bb), seconds=6.0)}
        r.close()
    return out


def child(step, folder):
    spec = json.load(open(os.path.join(folder, "inputs.json")))
    args = (spec["pnames"], {k: [tuple(b) for b in v] for k, v in spec["bboxs"].items()}, spec["fnames"])
    res = {"kernel": step_kernel, "device": step_device, "readf0": lambda *a: step_readf(0, *a), "readf16": lambda *a: step_readf(16, *a)}[step](*args)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        return child(sys.argv[2], sys.argv[3])
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    folder = tempfile.mkdtemp()
    pnames, bboxs, fnames = make_inputs(folder)
    json.dump({"pnames": pnames, "bboxs": bboxs, "fnames": fnames}, open(os.path.join(folder, "inputs.json"), "w"))
    res = {"pages": {}, "files": {}}
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
    lines = ["device ingest against the host loader: batch %d, %d x %d, host CPUs used by workers=16: %d of %d visible"
             % (BATCH, IMG_SIZE[0], IMG_SIZE[1], 16, os.cpu_count())]
    for label, what in (("pages", "page set: 16 PNG pages of 1600 x 1200, 64 word boxes each"), ("files", "word-file set: 1024 JPEG crops, 31 x 60..124")):
        r = res[label]
        w0, w16 = r["readf_workers_0_images_per_sec"], r["readf_workers_16_images_per_sec"]
        d0, d16 = r["device_readf_workers_0_images_per_sec"], r["device_readf_workers_16_images_per_sec"]
        lines += ["", what,
                  "  (a) kernel, HIP events:                 %9.1f us per batch = %.4f us per image  (%.3f of the %.2f us/image forward + beam search; arena %d bytes)"
                  % (r["kernel_us_per_batch"], r["kernel_us_per_image"], r["kernel_us_per_image"] / FORWARD_BEAM_US, FORWARD_BEAM_US, r["arena_bytes"]),
                  "  (b) device path, decoded pages in memory: %9.1f images/s  (host planning + packing + one copy + kernel)" % r["from_memory_images_per_sec"],
                  "  (b) device path, DeviceReadf(workers=0):  %9.1f images/s  (from the files: decoding in this process included)" % d0,
                  "  (b) device path, DeviceReadf(workers=16): %9.1f images/s  (from the files: decoding in 16 processes)" % d16,
                  "  (c) Readf(workers=0):                     %9.1f images/s" % w0,
                  "  (c) Readf(workers=16):                    %9.1f images/s" % w16,
                  "  (b) over (c), from the files at equal workers: %.2f x at workers=0, %.2f x at workers=16;  (b) from memory over (c): %.1f x workers=0, %.1f x workers=16"
                  % (d0 / w0, d16 / w16, r["from_memory_images_per_sec"] / w0, r["from_memory_images_per_sec"] / w16)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
