#!/usr/bin/env python3
"""Word detection on the device (csrc/detect.hip) on the page set of scripts/ingest_bench.py: 16 pages of 1600 x 1200.  Prints
  (a) the launch sequence of crnn_detect_words by HIP events (Otsu, gap_x 8, gap_y 0: WordDetector's defaults),
  (b) each kernel's share of it (torch.profiler's device records, when the profiler is there),
  (c) the bytes the sequence has to move over (a), against the 8 TB/s roofline,
  (d) the same pages through detect_words_host, and through scipy.ndimage.label alone where scipy is importable,
  (e) (a) as a share of ingest + forward + beam search over the boxes it found.
Nothing here is gated on a time.  usage: detect_bench.py [--out FILE]"""
import ctypes
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

CALLS, IMG_SIZE, BATCH = 200, (100, 32, 1), 1024
ROOFLINE = 8e12


def main():
    import torch
    import utils as U
    from crnn_mi355x import data, detect as D, ingest as I, native, pages as PG
    from ingest_bench import make_inputs
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    pnames, _, _ = make_inputs(tempfile.mkdtemp())
    pages = [data.read_img(n) for n in pnames]
    det = U.WordDetector()
    ing = U.DeviceIngest(IMG_SIZE)
    arena = ing.upload(pages)
    found = det.detect(None, arena=arena)
    boxes = [D.to_boxes(r) for r, _ in found]
    n_boxes = sum(len(b) for b in boxes)

    # (a) the raw entry point, buffers allocated once
    table = PG.page_table(arena.pages, arena.offsets)
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    prm, P, cap = det._prm, len(pages), det.params["cap"]
    host = table.ctypes.data_as(ctypes.c_void_p)
    need = native.lib().crnn_detect_workspace_bytes(host, P, ctypes.byref(prm))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rects = torch.empty((P, cap, 5), dtype=torch.int32, device="cuda")
    info = torch.empty((P, 4), dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: native.lib().crnn_detect_words(p(arena.dev), arena.nbytes, host, p(table_dev), P, ctypes.byref(prm), p(rects), p(info), p(ws), need, stream)

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls
    for _ in range(3):
        native.check(call(), "detect_words")
    seq = sorted(window(call, CALLS) for _ in range(5))
    seq_us = seq[2]

    # (b) kernel shares
    shares = None
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(20):
                call()
            torch.cuda.synchronize()
        rows = [(e.key, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0), e.count) for e in prof.key_averages()]
        rows = [(k, t / c) for k, t, c in rows if ("det_" in k or "otsu_" in k) and c]
        if rows:
            total = sum(t for _, t in rows)
            shares = [(k.split("(")[0], t, t / total) for k, t in sorted(rows, key=lambda r: -r[1])]
    except Exception as e:                                             # the profiler is optional
        shares = None
        print("kernel shares not measured: %s" % e, file=sys.stderr)

    # (c) what has to move: the page read twice (histogram, tile pass), a label word written and read per pixel, the records written and read three times
    pix = sum(pg.size for pg in pages)
    slots = sum(((pg.shape[0] + 1) // 2) * ((pg.shape[1] + 1) // 2) for pg in pages)
    moved = 2 * pix + 4 * pix + 4 * 24 * slots

    # (d) the host path and scipy
    t = time.time()
    host_found = [D.detect_words_host(pg, cap=cap, **{k: v for k, v in det.params.items() if k != "cap"}) for pg in pages]
    host_s = time.time() - t
    same = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(found, host_found))
    scipy_s = None
    try:
        from scipy import ndimage
        masks = [D.smear(D.ink_mask(pg)[0], det.params["gap_x"], det.params["gap_y"]) for pg in pages]
        t = time.time()
        for m in masks:
            ndimage.find_objects(ndimage.label(m, structure=np.ones((3, 3), int))[0])
        scipy_s = time.time() - t
    except ImportError:
        pass

    # (e) ingest + forward + beam search over the boxes found
    index = [k for k, bl in enumerate(boxes) for _ in bl][:BATCH]
    crops = [I.box_slices(b, pages[k].shape) for k, bl in enumerate(boxes) for b in bl][:BATCH]
    model = U.init_predictor(U.CRNN(num_classes=38, max_string_len=23, shape=IMG_SIZE, time_dense_size=128, n_units=256).get_model())
    dec = U.DecodeCTCPred(top_paths=1, beam_width=10, inverse_classes={i: ch for i, ch in enumerate(data.get_lexicon())})
    plans = ing.plan(crops)
    eng = model._engine(BATCH)

    def rest():
        x = ing.crops(None, index, crops, plans, batch=BATCH, arena=arena)
        dec.decode_labels(eng.forward(x, train=False), device=True)
    for _ in range(3):
        rest()
    rest_us = sorted(window(rest, 20) for _ in range(5))[2]

    lines = ["word detection on the device: %d pages of %d x %d, Otsu, gap_x %d, gap_y %d; %d boxes found (%s detect_words_host)"
             % (P, pages[0].shape[0], pages[0].shape[1], det.params["gap_x"], det.params["gap_y"], n_boxes, "equal to" if same else "DIFFERENT FROM"),
             "  (a) crnn_detect_words, memset + 7 launches, HIP events: %9.1f us per call [%.1f .. %.1f] = %.1f us per page  (%d calls per window, median of 5)"
             % (seq_us, seq[0], seq[-1], seq_us / P, CALLS)]
    if shares:
        lines.append("  (b) kernels (torch.profiler device time per launch; they sum to %.1f us):" % sum(t for _, t, _ in shares))
        lines += ["        %-24s %9.1f us  %5.1f %%" % (k, t, 100 * f) for k, t, f in shares]
    else:
        lines.append("  (b) kernel shares: not measured (no profiler records)")
    lines += ["  (c) bytes that must move (page twice, a label word written and read, records written and read three times): %.1f MB -> %.2f TB/s = %.1f %% of the 8 TB/s roofline"
              % (moved / 1e6, moved / (seq_us * 1e-6) / 1e12, 100 * moved / (seq_us * 1e-6) / ROOFLINE),
              "  (d) detect_words_host, same pages:            %9.1f ms per page  (%.0f x (a))" % (1e3 * host_s / P, host_s * 1e6 / seq_us)]
    if scipy_s is not None:
        lines.append("      scipy.ndimage.label + find_objects alone:  %9.1f ms per page  (%.0f x (a); threshold and smear not counted)" % (1e3 * scipy_s / P, scipy_s * 1e6 / seq_us))
    lines.append("  (e) ingest + forward + beam search of the first %d boxes (batch %d): %9.1f us; (a) is %.3f of it" % (len(index), BATCH, rest_us, seq_us / rest_us))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
