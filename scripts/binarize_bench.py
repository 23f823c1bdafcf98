#!/usr/bin/env python3
"""Adaptive binarisation on the device (csrc/binarize.hip) on the page set of scripts/ingest_bench.py: 16 pages of 1600 x 1200.  Prints
  (a) crnn_binarize_pages by HIP events at radius 7, 15 and 31 (k256 51, dark ink), with the bytes per second over the 2 bytes per pixel that
      must move (the page read once, the result written once), against the 8 TB/s roofline,
  (b) the launch sequence of crnn_detect_words in the same run (Otsu on the grey arena: scripts/detect_bench.py's (a); and threshold 127 on
      the binarised arena, the call the adaptive detector makes), and (a) as a ratio to it,
  (c) the same pages through sauvola_host, compared byte for byte with the device's result.
Nothing here is gated on a time.  usage: binarize_bench.py [--out FILE]"""
import ctypes
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

CALLS, RADII, K256 = 200, (7, 15, 31), 51
ROOFLINE = 8e12


def main():
    import torch
    import utils as U
    from crnn_mi355x import binarize as B, data, detect as D, native, pages as PG
    from ingest_bench import make_inputs
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    pnames, _, _ = make_inputs(tempfile.mkdtemp())
    pages = [data.read_img(n) for n in pnames]
    lib, P = native.lib(), len(pages)
    arena = U.DeviceIngest((100, 32, 1)).upload(pages)
    table = PG.page_table(arena.pages, arena.offsets)
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    host = table.ctypes.data_as(ctypes.c_void_p)
    out = torch.zeros(arena.nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    def timed(fn, what):
        for _ in range(3):
            native.check(fn(), what)
        return sorted(window(fn, CALLS) for _ in range(5))

    # (a) the binariser, one launch per call
    pix = sum(pg.size for pg in pages)
    moved = 2 * pix
    bin_us, device = {}, {}
    for r in RADII:
        prm = B.crnn_binarize_params(radius=r, k256=K256, polarity=1)
        call = lambda: lib.crnn_binarize_pages(p(arena.dev), arena.nbytes, host, p(table_dev), P, ctypes.byref(prm), p(out), arena.nbytes, stream)
        bin_us[r] = timed(call, "binarize_pages")
        device[r] = out.cpu().numpy()

    # (b) the detection sequence, on the grey arena as scripts/detect_bench.py times it and on the binarised one (radius 15, left in `out`)
    def detect_call(params, src):
        prm = D.crnn_detect_params(**params)
        need = lib.crnn_detect_workspace_bytes(host, P, ctypes.byref(prm))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        rects = torch.empty((P, params["cap"], 5), dtype=torch.int32, device="cuda")
        info = torch.empty((P, 4), dtype=torch.int32, device="cuda")
        keep = (prm, ws, rects, info)
        return lambda: (keep, lib.crnn_detect_words(p(src), arena.nbytes, host, p(table_dev), P, ctypes.byref(prm), p(rects), p(info), p(ws), need, stream))[1]
    out.copy_(torch.from_numpy(device[15]))
    otsu = timed(detect_call(dict(D.DEFAULTS), arena.dev), "detect_words")
    fixed = timed(detect_call(dict(D.DEFAULTS, threshold=127, polarity=1), out), "detect_words")

    # (c) the host path, and the comparison
    same, host_s = {}, None
    for r in RADII:
        t = time.time()
        want, _ = PG.pack_arena([B.sauvola_host(pg, r, K256, 1) for pg in (pages if r == 15 else pages[:2])])
        if r == 15:
            host_s = time.time() - t
        same[r] = np.array_equal(device[r][:want.size], want)
    ink = int((device[15] == 0).sum())

    lines = ["adaptive binarisation on the device: %d pages of %d x %d, k256 %d, dark ink; %.1f MB must move per call (2 B per pixel); at radius 15 %d ink pixels (%.1f %%)"
             % (P, pages[0].shape[0], pages[0].shape[1], K256, moved / 1e6, ink, 100.0 * ink / pix),
             "  (a) crnn_binarize_pages, one launch, HIP events (%d calls per window, median of 5 [min .. max]):" % CALLS]
    for r in RADII:
        us = bin_us[r][2]
        lines.append("        radius %2d: %9.1f us per call [%.1f .. %.1f] = %.1f us per page; %.2f TB/s of must-move bytes = %.1f %% of the 8 TB/s roofline; %s sauvola_host on %s"
                     % (r, us, bin_us[r][0], bin_us[r][-1], us / P, moved / (us * 1e-6) / 1e12, 100 * moved / (us * 1e-6) / ROOFLINE,
                        "equal to" if same[r] else "DIFFERENT FROM", "all pages" if r == 15 else "the first 2 pages"))
    lines += ["  (b) crnn_detect_words in the same run: Otsu on the grey arena %9.1f us per call [%.1f .. %.1f]; threshold 127 on the binarised arena %9.1f us [%.1f .. %.1f]"
              % (otsu[2], otsu[0], otsu[-1], fixed[2], fixed[0], fixed[-1]),
              "      the binariser as a ratio to the Otsu sequence: " + ", ".join("radius %d: %.2f" % (r, bin_us[r][2] / otsu[2]) for r in RADII),
              "  (c) sauvola_host, same pages, radius 15:      %9.1f ms per page  (%.0f x (a))" % (1e3 * host_s / P, host_s * 1e6 / bin_us[15][2])]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0 if all(same.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
