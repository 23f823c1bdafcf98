#!/usr/bin/env python3
"""Baseline JPEG decoding on the device (csrc/jpeg.hip).  Prints
  (a) crnn_jpeg_decode by HIP events -- the whole call (2 memsets + 3 launches) -- for 1024 one-word 100 x 32 files (colour 4:2:0, and grey) and for
      16 text-like pages of 1600 x 1200 (colour 4:2:0) without restart markers (one lane decodes a whole page) and with a restart interval of one
      MCU row; per launch when --stats names the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of `--kernels` (a run of its own:
      tracing slows the host), else "not measured",
  (b) the bytes moved against the 8 TB/s roofline: what must move (the files in, the grey pages out) and what the three launches move as built
      (coefficients zeroed, written and read at 2 B per sample, planes written and read at 1 B),
  (c) the status read-back: JpegDecoder.decode alone against decode + the 4-byte-per-file copy that DeviceIngest.decoded waits for,
  (d) images/s from the files through DeviceReadf(workers=0) and DeviceReadf(workers=16), each with and without device_decode, in this run,
  (e) the device route against the host route for one page: where max_segment_bytes would have to lie,
  (f) the compiler's resource report of the three kernels (--resources FILE: a report made elsewhere; default: hipcc is run here).
Nothing here is gated on a time.  usage: jpeg_bench.py [--out FILE] [--stats CSV] [--resources FILE] | --kernels"""
import io
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

ROOFLINE = 8e12
BATCH = 256
KERNELS = ("jpeg_entropy_kernel", "jpeg_idct_kernel", "jpeg_grey_kernel")


def encode(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def word_image(rs, colour):
    """A 32-row, 100-column one-word image: smooth paper, dark strokes, a little noise."""
    base = rs.randint(150, 240) + np.cumsum(rs.randint(-2, 3, (32, 100)), axis=1)
    for k in range(int(rs.randint(3, 9))):
        c0 = 6 + 11 * k
        base[8:26, c0:c0 + int(rs.randint(2, 8))] = rs.randint(10, 80)
        base[int(rs.randint(8, 24)), c0:c0 + 9] = rs.randint(10, 80)
    img = np.clip(base + rs.randint(-6, 7, base.shape), 0, 255).astype(np.uint8)
    if not colour:
        return img
    return np.clip(img[..., None].astype(int) + rs.randint(-12, 13, 3), 0, 255).astype(np.uint8)


def page_image(rs):
    page = rs.randint(190, 256, (1600, 1200)).astype(np.uint8)
    for r0 in range(40, 1540, 40):
        c0 = 60
        while c0 < 1060:
            for _ in range(int(rs.randint(2, 9))):
                page[r0:r0 + 18, c0:c0 + 8] = rs.randint(10, 70)
                c0 += 12
            c0 += 24
    return np.stack([page, np.clip(page.astype(int) - 8, 0, 255).astype(np.uint8), np.clip(page.astype(int) - 20, 0, 255).astype(np.uint8)], axis=-1)


def workloads():
    rs = np.random.RandomState(0)
    words_c = [encode(word_image(rs, True), quality=85, subsampling="4:2:0") for _ in range(1024)]
    words_g = [encode(word_image(rs, False), quality=85) for _ in range(1024)]
    pages = [page_image(rs) for _ in range(16)]
    return [("1024 one-word 100 x 32, colour 4:2:0", words_c, 200), ("1024 one-word 100 x 32, grey", words_g, 200),
            ("16 pages 1600 x 1200, 4:2:0, no restart markers", [encode(p, quality=85, subsampling="4:2:0") for p in pages], 2),
            ("16 pages 1600 x 1200, 4:2:0, restart every MCU row", [encode(p, quality=85, subsampling="4:2:0", restart_marker_rows=1) for p in pages], 50)]


class Call:
    """One workload uploaded, crnn_jpeg_decode as a closure."""

    def __init__(self, datas):
        import torch
        from crnn_mi355x import jpeg as J, native
        lib = native.lib()
        self.blob, self.items, self.segs, self.pool, totals = J.plan(datas)
        assert not self.items["status"].any()
        self.n, self.nbytes, self.samples = len(datas), int(totals[2]), int(totals[3])
        self.pixels = int((self.items["rows"].astype(np.int64) * self.items["cols"]).sum())
        dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() for a in (self.blob, self.items, self.segs, self.pool)]
        self.keep = dev
        ws_bytes = lib.crnn_jpeg_workspace_bytes(self.samples)
        self.arena = torch.zeros(self.nbytes, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(self.n, dtype=torch.int32, device="cuda")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        self.keep.append(ws)
        stream = torch.cuda.current_stream().cuda_stream
        self.fn = lambda: lib.crnn_jpeg_decode(dev[0].data_ptr(), self.blob.nbytes, self.items.ctypes.data, dev[1].data_ptr(), self.n, self.segs.ctypes.data,
                                               dev[2].data_ptr(), len(self.segs), dev[3].data_ptr(), len(self.pool), self.arena.data_ptr(), self.nbytes,
                                               self.status.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    def must_move(self):
        return self.blob.nbytes + self.pixels

    def moved(self):
        return self.blob.nbytes + 8 * self.samples + self.pixels      # memset 2, write <= 2, read 2, planes 1 + 1 per sample


def window(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def kernel_stats(path):
    """{kernel: average ns} from rocprofv3's kernel statistics CSV."""
    import csv
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name", "")
        for k in KERNELS:
            if k in name:
                out[k] = float(row.get("AverageNs") or row.get("Average") or 0.0)
    return out


def resources(path):
    if path:
        text = open(path).read()
    else:
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-c",
               os.path.join(ROOT, "crnn-ocr-lite_amd", "csrc", "jpeg.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
        text = subprocess.run(cmd, capture_output=True, text=True).stderr
    keep = ("Function Name", "TotalSGPRs", "VGPRs:", "ScratchSize", "Occupancy", "LDS Size")
    return ["      " + ln.split("remark:")[1].strip().replace(" [-Rpass-analysis=kernel-resource-usage]", "") for ln in text.splitlines()
            if "remark:" in ln and any(k in ln for k in keep)]


def _rate(gen, seconds=3.0):
    import torch
    next(gen)
    torch.cuda.synchronize()
    t, k = time.time(), 0
    while time.time() - t < seconds:
        next(gen)
        k += BATCH
    torch.cuda.synchronize()
    return k / (time.time() - t)


def main():
    import torch
    from crnn_mi355x import data as D, ingest as I, jpeg as J, native
    arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
    loads = workloads()
    if "--kernels" in sys.argv:                      # the run rocprofv3 traces: every workload's launches, nothing else
        for _, datas, calls in loads[:2] + loads[3:]:
            c = Call(datas)
            for _ in range(20):
                native.check(c.fn(), "jpeg_decode")
            torch.cuda.synchronize()
        return 0
    class Lines(list):                               # printed as they come: the pages without restart markers take a while
        def append(self, line):
            print(line, flush=True)
            list.append(self, line)
    lines = Lines()
    lines.append("baseline JPEG decoding on the device: crnn_jpeg_decode = 2 memsets + 3 launches; HIP events, median of 5 windows [min .. max]")
    ok = True
    for what, datas, calls in loads:
        c = Call(datas)
        for _ in range(3):
            native.check(c.fn(), "jpeg_decode")
        us = sorted(window(c.fn, calls) for _ in range(5))
        ok = ok and not c.status.cpu().numpy().any()
        pick = [0, len(datas) // 2, len(datas) - 1]
        flat = c.arena.cpu().numpy()
        for k in pick if len(datas) > 16 else pick[:1]:
            ref = J.jpeg_gray_host(datas[k]) if len(datas) > 16 else None
            if ref is not None:
                o = int(c.items["page_off"][k])
                ok = ok and np.array_equal(flat[o:o + ref.size].reshape(ref.shape), ref)
        lines.append("  (a) %s: %.1f KB of files, %d segments, %.1f M samples" % (what, c.blob.nbytes / 1e3, len(c.segs), c.samples / 1e6))
        lines.append("      %10.1f us per call [%.1f .. %.1f] (%d calls per window) = %.3f us per file = %.0f files/s" % (
            us[2], us[0], us[-1], calls, us[2] / c.n, c.n / (us[2] * 1e-6)))
        lines.append("  (b) must move %.2f MB: %.3f TB/s = %.2f %% of the roofline; moved as built %.2f MB: %.3f TB/s = %.2f %%" % (
            c.must_move() / 1e6, c.must_move() / (us[2] * 1e-6) / 1e12, 100 * c.must_move() / (us[2] * 1e-6) / ROOFLINE,
            c.moved() / 1e6, c.moved() / (us[2] * 1e-6) / 1e12, 100 * c.moved() / (us[2] * 1e-6) / ROOFLINE))
    stats = kernel_stats(arg("--stats")) if arg("--stats") else {}
    lines.append("      per launch, average over the traced run's workloads (rocprofv3 --kernel-trace --stats): " + (
        ", ".join("%s %.1f us" % (k, stats[k] / 1e3) for k in KERNELS if k in stats) if stats else "not measured"))
    # (c) the status read-back
    dec = J.JpegDecoder()
    words = loads[0][1]

    def host_clock(fn, calls=30):
        fn()
        torch.cuda.synchronize()
        t = time.time()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.time() - t) / calls * 1e6
    plain = host_clock(lambda: dec.decode(words))
    back = host_clock(lambda: dec.decode(words)[1].cpu())
    lines.append("  (c) JpegDecoder.decode of the 1024 colour files (plan + one upload + the launches), host clock: %.0f us per call = %.0f files/s; with the "
                 "status read-back after every call: %.0f us (%+.0f us)" % (plain, 1024 / (plain * 1e-6), back, back - plain))
    # (d) end to end from files
    folder = tempfile.mkdtemp()
    names = []
    for i, d in enumerate(words):
        names.append(os.path.join(folder, "%d_word_%d.jpg" % (i, i)))
        with open(names[-1], "wb") as f:
            f.write(d)
    classes = {ch: i for i, ch in enumerate(D.get_lexicon())}
    for workers in (0, 16):
        for dd in (False, True):
            r = I.DeviceReadf(img_size=(100, 32, 1), max_len=23, normed=True, batch_size=BATCH, classes=classes, transform_p=0., workers=workers, device_decode=dd)
            rate = _rate(r.run_generator(names))
            r.close()
            lines.append("  (d) DeviceReadf(workers=%d, device_decode=%s) from 1024 colour one-word files, batch %d: %9.0f images/s" % (workers, dd, BATCH, rate))
    # (e) one page: the device's single lane against the host decoder
    page = loads[2][1][0]
    t = time.time()
    for _ in range(3):
        D.read_img(io.BytesIO(page))
    host_ms = (time.time() - t) / 3 * 1e3
    one = Call([page])
    native.check(one.fn(), "jpeg_decode")
    dev_us = sorted(window(one.fn, 3) for _ in range(3))[1]
    lines.append("  (e) one page of %.0f KB without restart markers: the device's one lane %.1f ms, read_img on the host %.1f ms -> the crossover of "
                 "max_segment_bytes lies near %.0f KB per segment at this content (the default of 64 KiB is a placeholder)" % (
                     len(page) / 1e3, dev_us / 1e3, host_ms, len(page) / 1e3 * host_ms / (dev_us / 1e3)))
    lines.append("  (f) the compiler's resource report (gfx950):")
    for ln in resources(arg("--resources")):
        lines.append(ln)
    lines.append("  device pages of the one-word workloads compared with jpeg_gray_host on 3 files each, all statuses 0: %s" % ("equal" if ok else "DIFFER"))
    text = "\n".join(lines) + "\n"
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
