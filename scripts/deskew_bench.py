#!/usr/bin/env python3
"""Page deskew on the device (csrc/deskew.hip) on 16 text-like pages of 1600 x 1200 (the size of scripts/ingest_bench.py's pages; those hold
boxes at random places, which have no skew to find): 38 lines of words made of 18 x 8 blocks on noisy bright paper, each page skewed on the
host first (rotate_host by an index of its own between -45 and 45, so that the estimate has something to find and the rotation gathers
across rows).  Prints
  (a) crnn_deskew_estimate by HIP events at the default parameters (Otsu, 97 candidates), with the bytes per second over the 1 byte per pixel
      that must move (the page read once), against the 8 TB/s roofline,
  (b) crnn_rotate_pages by the estimated indices (2 bytes per pixel: the page read once, the result written once), and by index 0 and by
      index 48 on every page,
  (c) the launch sequence of crnn_detect_words (Otsu on the grey arena: scripts/detect_bench.py's (a)) and crnn_binarize_pages (radius 15) in
      the same run, and (a), (b) as ratios to the detection sequence,
  (d) the same pages through deskew_host, compared with the device's indices, scores and bytes.
Nothing here is gated on a time.  usage: deskew_bench.py [--out FILE]"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

CALLS = 100
ROOFLINE = 8e12
SKEWS = (-45, 38, -31, 24, -18, 12, -7, 3, 0, -2, 5, -10, 15, -21, 28, 45)


def make_pages():
    rs = np.random.RandomState(0)
    pages = []
    for _ in SKEWS:
        page = rs.randint(190, 256, (1600, 1200)).astype(np.uint8)
        for r0 in range(40, 1540, 40):                                   # a line of words every 40 rows
            c0 = 60
            while c0 < 1060:
                for b in range(int(rs.randint(2, 9))):                   # a word: 2..8 blocks, 12 columns apart
                    if c0 + 8 <= 1140:
                        page[r0:r0 + 18, c0:c0 + 8] = rs.randint(10, 70)
                    c0 += 12
                c0 += 24
        pages.append(page)
    return pages


def main():
    import torch
    import utils as U
    from crnn_mi355x import binarize as B, deskew as K, detect as D, native, pages as PG
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    pages = [K.rotate_host(pg, -a) for pg, a in zip(make_pages(), SKEWS)]   # rotating by -a leaves a page whose lines run at slope a / 256
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

    pix = sum(pg.size for pg in pages)
    # (a) the estimate
    prm = K.crnn_deskew_params(**K.DEFAULTS)
    ncand = 2 * prm.steps + 1
    need = lib.crnn_deskew_workspace_bytes(host, P, ctypes.byref(prm))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    index = torch.zeros(P, dtype=torch.int32, device="cuda")
    scores = torch.zeros((P, ncand), dtype=torch.int64, device="cuda")
    est = timed(lambda: lib.crnn_deskew_estimate(p(arena.dev), arena.nbytes, host, p(table_dev), P, ctypes.byref(prm), p(index), p(scores), p(ws),
                                                 need, stream), "deskew_estimate")
    found, dev_scores = index.cpu().numpy(), scores.cpu().numpy()

    # (b) the rotation
    def rotate_call(idx):
        return lambda: lib.crnn_rotate_pages(p(arena.dev), arena.nbytes, host, p(table_dev), P, p(idx), ctypes.byref(prm), p(out), arena.nbytes, stream)
    rot = timed(rotate_call(index), "rotate_pages")
    flat = out.cpu().numpy()
    rot0 = timed(rotate_call(torch.zeros_like(index)), "rotate_pages")
    rot48 = timed(rotate_call(torch.full_like(index, 48)), "rotate_pages")

    # (c) the detection sequence and the binariser in the same run
    dprm = D.crnn_detect_params(**D.DEFAULTS)
    dneed = lib.crnn_detect_workspace_bytes(host, P, ctypes.byref(dprm))
    dws = torch.empty(dneed, dtype=torch.uint8, device="cuda")
    rects = torch.empty((P, D.DEFAULTS["cap"], 5), dtype=torch.int32, device="cuda")
    info = torch.empty((P, 4), dtype=torch.int32, device="cuda")
    det = timed(lambda: lib.crnn_detect_words(p(arena.dev), arena.nbytes, host, p(table_dev), P, ctypes.byref(dprm), p(rects), p(info), p(dws), dneed,
                                              stream), "detect_words")
    bprm = B.crnn_binarize_params(radius=15, k256=51, polarity=1)
    bout = torch.zeros(arena.nbytes, dtype=torch.uint8, device="cuda")
    bina = timed(lambda: lib.crnn_binarize_pages(p(arena.dev), arena.nbytes, host, p(table_dev), P, ctypes.byref(bprm), p(bout), arena.nbytes, stream),
                 "binarize_pages")

    # (d) the host path, and the comparison
    t = time.time()
    want = [K.estimate_skew_host(pg) for pg in pages]
    host_est = time.time() - t
    t = time.time()
    want_flat, _ = PG.pack_arena([K.rotate_host(pg, a) for pg, (a, _) in zip(pages, want)])
    host_rot = time.time() - t
    same = (found.tolist() == [a for a, _ in want], all(np.array_equal(dev_scores[k], s) for k, (_, s) in enumerate(want)),
            np.array_equal(flat[:want_flat.size], want_flat))

    def line(what, us, moved):
        return "%s %9.1f us per call [%.1f .. %.1f] = %.1f us per page; %.3f TB/s of must-move bytes = %.2f %% of the 8 TB/s roofline; %.2f x the detection sequence" % (
            what, us[2], us[0], us[-1], us[2] / P, moved / (us[2] * 1e-6) / 1e12, 100 * moved / (us[2] * 1e-6) / ROOFLINE, us[2] / det[2])
    lines = ["page deskew on the device: %d text-like pages of %d x %d drawn at the slopes k / 256, k = %s; %d candidates (steps %d, slope_step %d), Otsu; %.1f MB of pixels"
             % (P, pages[0].shape[0], pages[0].shape[1], list(SKEWS), ncand, prm.steps, prm.slope_step, pix / 1e6),
             "  HIP events, %d calls per window, median of 5 [min .. max]; workspace of the estimate %.1f MB" % (CALLS, need / 1e6),
             line("  (a) crnn_deskew_estimate (memset + 5 launches, 1 B per pixel):", est, pix),
             "      indices found: %s" % found.tolist(),
             line("  (b) crnn_rotate_pages by those indices (1 launch, 2 B per pixel):", rot, 2 * pix),
             line("      ... by index 0 on every page:                                ", rot0, 2 * pix),
             line("      ... by index 48 on every page:                               ", rot48, 2 * pix),
             "  (c) in the same run: crnn_detect_words (Otsu on the grey arena) %9.1f us per call [%.1f .. %.1f]; crnn_binarize_pages (radius 15) %9.1f us [%.1f .. %.1f]"
             % (det[2], det[0], det[-1], bina[2], bina[0], bina[-1]),
             "      estimate + rotation as a ratio to the detection sequence: %.2f" % ((est[2] + rot[2]) / det[2]),
             "  (d) deskew_host, same pages: estimate_skew_host %9.1f ms per page (%.0f x (a)), rotate_host %9.1f ms per page (%.0f x (b)); the device's indices %s, "
             "scores %s, bytes %s the host's" % (1e3 * host_est / P, host_est * 1e6 / est[2], 1e3 * host_rot / P, host_rot * 1e6 / rot[2],
                                                "equal" if same[0] else "DIFFER FROM", "equal" if same[1] else "DIFFER FROM",
                                                "equal" if same[2] else "DIFFER FROM")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0 if all(same) else 1


if __name__ == "__main__":
    sys.exit(main())
