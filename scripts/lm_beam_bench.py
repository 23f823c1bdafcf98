#!/usr/bin/env python3
"""Beam search with a character language model and N-best output at batch 1024, T = 52 (the 100 x 32 configuration), 38 classes, width 10:
crnn_ctc_beam_decode_lm (csrc/beam.hip) on the posteriors of the benchmark model (random weights, as lexicon_bench.make_engine builds it), in the
same process and on the same maps as the yardstick, the plain crnn_ctc_beam_decode launch (the same kernel without a table, top_paths 1): without a table, with dense tables of orders 1, 2 and 3
(weights 0.8 * log(dirichlet(0.3)) + 0.5, what the tests use), each with top_paths 1 and 5.  HIP events over windows of back-to-back launches after
warm-up; the launches alternate, two runs each.  Prints, and with --out writes, us per launch, the ratio to the yardstick and the kernels' resource
usage as the compiler reports it.
usage: lm_beam_bench.py [--out FILE]"""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd"), os.path.join(ROOT, "scripts")]
import numpy as np  # noqa: E402

from lexicon_bench import BATCH, T, C, BEAM, make_engine, _timed  # noqa: E402


def resources():
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(ROOT, "crnn-ocr-lite_amd", "csrc", "beam.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out = []
    for blk in err.split("Function Name: ")[1:]:
        pick = lambda key: int(re.search(r"%s: (\d+)" % re.escape(key), blk).group(1))
        m = re.search(r"ILi(\d)ELb(\d)E", blk.split()[0])
        out.append("ctc_beam_kernel<CPL = %s, LM = %s> %d VGPRs / %d SGPRs / scratch %d / VGPR spills %d / SGPR spills %d / occupancy %d"
                   % (m.group(1), m.group(2), pick("VGPRs"), pick("TotalSGPRs"), pick("ScratchSize [bytes/lane]"), pick("VGPRs Spill"), pick("SGPRs Spill"),
                      pick("Occupancy [waves/SIMD]")))
    return out


def main():
    import torch
    from crnn_mi355x import native
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    eng, x = make_engine()
    y = eng.forward(x, train=False).float().contiguous()
    eng.check_rnn_status()
    L = native.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lab = torch.empty((BATCH, T), dtype=torch.int32, device="cuda"); ln = torch.empty(BATCH, dtype=torch.int32, device="cuda")
    bsc = torch.empty(BATCH, dtype=torch.float32, device="cuda")
    outs = {k: (torch.empty((BATCH, k, T), dtype=torch.int32, device="cuda"), torch.empty((BATCH, k), dtype=torch.int32, device="cuda"),
                torch.empty((BATCH, k), dtype=torch.float32, device="cuda")) for k in (1, 5)}
    labk, lnk, sck = outs[1]
    rs = np.random.RandomState(0)
    tables = {0: None}
    for order in (1, 2, 3):
        rows = L.crnn_ctc_lm_rows(C, order)
        tables[order] = torch.from_numpy((0.8 * np.log(rs.dirichlet([0.3] * C, size=rows) + 1e-6) + 0.5).astype(np.float32)).cuda()

    def beam():
        rc = L.crnn_ctc_beam_decode(p(y), None, p(lab), p(ln), p(bsc), BATCH, T, C, BEAM, 0, st)
        assert rc == 0, rc

    def lm_launch(order, top):
        def fn():
            o, n, v = outs[top]
            rc = L.crnn_ctc_beam_decode_lm(p(y), None, p(tables[order]), max(order, 1), p(o), p(n), p(v), BATCH, T, C, BEAM, top, 0, st)
            assert rc == 0, rc
        return fn
    beam(); lm_launch(0, 1)()
    torch.cuda.synchronize()
    assert torch.equal(labk[:, 0], lab) and torch.equal(lnk[:, 0], ln) and torch.equal(sck[:, 0], bsc)       # the default scorer is the plain beam search
    names = [("beam", beam)] + [("%s, top_paths %d" % ("no table" if o == 0 else "order %d" % o, k), lm_launch(o, k)) for o in (0, 1, 2, 3) for k in (1, 5)]
    changed = {}
    for o in (1, 2, 3):
        lm_launch(o, 1)()
        torch.cuda.synchronize()
        changed[o] = int((labk[:, 0] != lab).any(1).sum())
    events = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    runs = {}
    for rnd in range(2):
        for name, fn in names:
            us, calls = _timed(fn, torch.cuda.synchronize, events, 0.3)
            runs.setdefault(name, []).append((round(us, 1), calls))
    fmt = lambda name: " / ".join("%.1f" % u for u, _ in runs[name])
    best = lambda name: min(u for u, _ in runs[name])
    lines = ["beam search with a language model: batch %d, T = %d (100 x 32), %d classes, width %d; posteriors of the benchmark model (random weights);"
             % (BATCH, T, C, BEAM),
             "dense tables of weights 0.8 * log(dirichlet(0.3)) + 0.5 (orders 1, 2, 3: %s rows); the table changes the best path of %s of %d images."
             % (", ".join(str(tables[o].shape[0]) for o in (1, 2, 3)), " / ".join(str(changed[o]) for o in (1, 2, 3)), BATCH),
             "HIP events over windows of about 0.3 s of back-to-back launches after warm-up (%d .. %d launches per window); one process; the launches alternate, two runs each."
             % (min(c for r in runs.values() for _, c in r), max(c for r in runs.values() for _, c in r)), "",
             "  %-52s %16s us" % ("yardstick: crnn_ctc_beam_decode", fmt("beam"))]
    for name, _ in names[1:]:
        lines.append("  %-52s %16s us = %.3f x the yardstick" % ("crnn_ctc_beam_decode_lm, " + name, fmt(name), best(name) / best("beam")))
    lines += ["", "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):"] + ["  " + r for r in resources()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
