#!/usr/bin/env python3
"""Training augmentation on the device (crnn_mi355x/augment.py, csrc/augment.hip) at 100 x 32, batch 256 and 1024:
  (a) device-event time per launch of crnn_augment_batch with neutral items, with the warp only and with every stage on, and of the
      crnn_ingest_crops launch that feeds it, in the same run, as the yardstick -- each also as a multiple of the ingest launch and as a share
      of the 5.90 ms train step (batch 256, README);
  (b) images/s of DeviceReadf from decoded pages (page PNGs read once per pass by this process) with and without an AugmentPolicy.
Every step is a child process under its own time limit; the first one that fails ends the run.  usage: augment_bench.py [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd")]
import numpy as np  # noqa: E402

IMG_SIZE = (100, 32, 1)
BATCHES = (256, 1024)
STEPS = [("kernel", 240), ("readf", 300)]            # (step, time limit in seconds)
LAUNCHES = 2000                                      # timed launches per set
TRAIN_STEP_MS = 5.90                                 # the batch-256 train step (README)
ALL_ON = dict(a00=64000, a01=9000, a10=-3000, a11=67000, t0=300000, t1=-90000, morph=1, blur=1, gain=300, bias=-10, noise=24)


def make_pages(folder, npages=16, nboxes=64):
    from PIL import Image
    rs = np.random.RandomState(0)
    pnames, bboxs = [], {}
    for k in range(npages):                          # a scanned page: bright paper, dark strokes
        page = rs.randint(170, 256, (1600, 1200)).astype(np.uint8)
        boxes = []
        for i in range(nboxes):
            hc, wc = int(rs.randint(18, 41)), int(rs.randint(40, 161))
            r0, c0 = int(rs.randint(0, 1600 - hc)), int(rs.randint(0, 1200 - wc))
            page[r0 + 4:r0 + hc - 4, c0 + 4:c0 + wc - 4:3] = rs.randint(0, 80)
            boxes.append(("w%d" % i, r0, c0, r0 + hc, c0 + wc))
        name = os.path.join(folder, "page%02d.png" % k)
        Image.fromarray(page).save(name)
        pnames.append(name)
        bboxs[name] = boxes
    return pnames, bboxs


def _events(fn):
    import torch
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / LAUNCHES, 2)      # us per launch (the entry point's host-side check of its table included)


def step_kernel(pnames, bboxs):
    import ctypes
    import torch
    from crnn_mi355x import augment as A, data as D, ingest as I, native, pages as PG
    L = native.lib()
    pages = [D.read_img(n) for n in pnames]
    all_rects = np.array([I.box_slices(b, pg.shape) for n, pg in zip(pnames, pages) for b in bboxs[n]])
    all_index = np.repeat(np.arange(len(pages)), len(all_rects) // len(pages))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for B in BATCHES:
        rects, index = all_rects[:B], all_index[:B]
        plans = I.plan_crops(rects[:, 1] - rects[:, 0], rects[:, 3] - rects[:, 2], IMG_SIZE)
        arena, offs = PG.pack_arena(pages)
        tab = I.build_table(pages, offs, index, rects, plans, IMG_SIZE)
        d_arena, d_tab = torch.from_numpy(arena).cuda(), torch.from_numpy(tab.view(np.uint8).copy()).cuda()
        table = torch.from_numpy(I.norm_table()).cuda()
        x = torch.empty((B,) + IMG_SIZE, device="cuda")
        u8 = torch.empty((B,) + IMG_SIZE[:2], dtype=torch.uint8, device="cuda")
        ingest = lambda: L.crnn_ingest_crops(p(d_arena), len(arena), tab.ctypes.data_as(ctypes.c_void_p), p(d_tab), B, B, IMG_SIZE[0], IMG_SIZE[1],
                                             p(table), p(x), p(u8), stream())
        native.check(ingest(), "ingest_crops")
        res = {"ingest_us": _events(ingest)}
        warp = {k: v for k, v in ALL_ON.items() if k[0] in "at"}
        for label, fields in (("neutral", {}), ("warp", warp), ("all", ALL_ON)):
            items = A.neutral_items(B)
            for k, v in fields.items():
                items[k] = v
            items["seed"] = np.arange(B)
            A.check_items(items, IMG_SIZE)
            d_items = torch.from_numpy(items.view(np.uint8).copy()).cuda()
            aug = lambda: L.crnn_augment_batch(p(u8), items.ctypes.data_as(ctypes.c_void_p), p(d_items), B, B, IMG_SIZE[0], IMG_SIZE[1], p(table), p(x),
                                               None, stream())
            native.check(aug(), "augment_batch")
            res["augment_%s_us" % label] = _events(aug)
        out[str(B)] = res
    return out


def step_readf(pnames, bboxs):
    import torch
    from crnn_mi355x import augment as A, data as D, ingest as I
    classes = {c: i for i, c in enumerate(D.get_lexicon())}
    out = {}
    for B in BATCHES:
        res = {}
        for label, policy in (("plain", None), ("augmented", A.AugmentPolicy(seed=1))):
            r = I.DeviceReadf(img_size=IMG_SIZE, max_len=23, normed=True, batch_size=B, classes=classes, transform_p=0., augment=policy)
            gen = r.run_generator(pnames, bboxs=bboxs)
            next(gen)                                # warm-up: staging buffers, first launches
            torch.cuda.synchronize()
            t, k = time.time(), 0
            while time.time() - t < 4.0:
                next(gen)
                k += B
            torch.cuda.synchronize()
            res["device_readf_%s_images_per_sec" % label] = round(k / (time.time() - t), 1)
        out[str(B)] = res
    return out


def child(step, folder):
    spec = json.load(open(os.path.join(folder, "inputs.json")))
    args = (spec["pnames"], {k: [tuple(b) for b in v] for k, v in spec["bboxs"].items()})
    print("RESULT " + json.dumps({"kernel": step_kernel, "readf": step_readf}[step](*args)), flush=True)


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        return child(sys.argv[2], sys.argv[3])
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
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
    lines = ["training augmentation on the device: %d x %d, device events over %d launches per figure; page set: 16 PNG pages of 1600 x 1200, 64 word "
             "boxes each" % (IMG_SIZE[0], IMG_SIZE[1], LAUNCHES)]
    for B in BATCHES:
        r = res[str(B)]
        lines += ["", "batch %d" % B,
                  "  crnn_ingest_crops (the yardstick):      %8.2f us per launch  (%.4f of the %.2f ms train step)"
                  % (r["ingest_us"], r["ingest_us"] / (TRAIN_STEP_MS * 1e3), TRAIN_STEP_MS)]
        for label, what in (("neutral", "neutral items"), ("warp", "warp only"), ("all", "every stage on")):
            us = r["augment_%s_us" % label]
            lines.append("  crnn_augment_batch, %-19s %8.2f us per launch = %.2f x the ingest launch, %.4f of the %.2f ms train step"
                         % (what + ":", us, us / r["ingest_us"], us / (TRAIN_STEP_MS * 1e3), TRAIN_STEP_MS))
        a, b = r["device_readf_plain_images_per_sec"], r["device_readf_augmented_images_per_sec"]
        lines.append("  DeviceReadf(workers=0) from the page files: %9.1f images/s without a policy, %9.1f images/s with AugmentPolicy() (%.2f x)" % (a, b, b / a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
