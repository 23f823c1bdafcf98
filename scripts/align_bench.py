#!/usr/bin/env python3
"""Character alignment at batch 1024, T = 52 (the 100 x 32 configuration), 38 classes: crnn_ctc_align (csrc/align.hip: pre-pass + Viterbi with backtrace)
on the posteriors of the benchmark model (random weights, as lexicon_bench.make_engine builds it), the labels being the beam decoder's own output on those
maps.  In the same process, on the same maps: the beam launch the alignment follows (crnn_ctc_beam_decode, width 10) and a log_prob-style lexicon launch
(crnn_ctc_lexicon_score, one candidate per image: the same labels).  HIP events over windows of back-to-back launches after warm-up; the three alternate,
two runs each.  Prints, and with --out writes, the figures and the kernels' resource usage as the compiler reports it.
usage: align_bench.py [--out FILE]"""
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
           "-c", os.path.join(ROOT, "crnn-ocr-lite_amd", "csrc", "align.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out = []
    for blk in err.split("Function Name: ")[1:]:
        pick = lambda key: int(re.search(r"%s: (\d+)" % re.escape(key), blk).group(1))
        name = "ctc_align_kernel" if "ctc_align" in blk.split()[0] else "lex_lsm_kernel<2>" if "ILi2" in blk.split()[0] else "lex_lsm_kernel<1>"
        out.append("%s %d VGPRs / %d SGPRs / scratch %d / VGPR spills %d / SGPR spills %d / occupancy %d"
                   % (name, pick("VGPRs"), pick("TotalSGPRs"), pick("ScratchSize [bytes/lane]"), pick("VGPRs Spill"), pick("SGPRs Spill"), pick("Occupancy [waves/SIMD]")))
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

    def beam():
        rc = L.crnn_ctc_beam_decode(p(y), None, p(lab), p(ln), p(bsc), BATCH, T, C, BEAM, 1, st)
        assert rc == 0, rc
    beam()
    torch.cuda.synchronize()
    lens = ln.cpu().numpy()
    ws = torch.empty(L.crnn_ctc_align_workspace_bytes(BATCH, T, C, 0) // 4, dtype=torch.float32, device="cuda")
    score = torch.empty(BATCH, dtype=torch.float32, device="cuda")
    states = torch.empty((BATCH, T), dtype=torch.int32, device="cuda")
    start = torch.empty((BATCH, T), dtype=torch.int32, device="cuda"); end = torch.empty((BATCH, T), dtype=torch.int32, device="cuda")
    clp = torch.empty((BATCH, T), dtype=torch.float32, device="cuda")

    def align():
        rc = L.crnn_ctc_align(p(y), None, p(lab), p(ln), p(score), p(states), p(start), p(end), p(clp), p(ws), ws.numel() * 4, BATCH, T, C, 0, T, st)
        assert rc == 0, rc

    def align_score_only():
        rc = L.crnn_ctc_align(p(y), None, p(lab), p(ln), p(score), None, None, None, None, p(ws), ws.numel() * 4, BATCH, T, C, 0, T, st)
        assert rc == 0, rc
    # the lexicon launch reads a table of at most 31 columns: the same rows, narrowed (longer decodings score -inf in both)
    lab31 = lab[:, :31].contiguous()
    ln31 = torch.where(ln > 31, torch.full_like(ln, -1), ln)
    cand = torch.arange(BATCH, dtype=torch.int32, device="cuda").reshape(BATCH, 1)
    lsc = torch.empty((BATCH, 1), dtype=torch.float32, device="cuda")

    def lexicon():
        rc = L.crnn_ctc_lexicon_score(p(y), None, p(lab31), p(ln31), p(cand), p(lsc), p(ws), ws.numel() * 4, BATCH, T, C, 0, BATCH, 31, 1, st)
        assert rc == 0, rc
    align(); lexicon()
    torch.cuda.synchronize()
    a, t = score.cpu().numpy(), lsc[:, 0].cpu().numpy()
    assert np.array_equal(np.isneginf(a), np.isneginf(t)) and (a[np.isfinite(a)] <= t[np.isfinite(a)] + 1e-3 + 1e-4 * np.abs(t[np.isfinite(a)])).all()
    events = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    runs = {}
    for rnd in range(2):
        for name, fn in (("beam", beam), ("align", align), ("align, score only", align_score_only), ("lexicon", lexicon)):
            us, calls = _timed(fn, torch.cuda.synchronize, events, 0.5)
            runs.setdefault(name, []).append((round(us, 1), calls))
    fmt = lambda name: " / ".join("%.1f" % u for u, _ in runs[name])
    best = lambda name: min(u for u, _ in runs[name])
    fin = np.isfinite(a)
    lines = ["character alignment: batch %d, T = %d (100 x 32), %d classes; posteriors of the benchmark model (random weights); labels = the beam decoder's output"
             % (BATCH, T, C),
             "on those maps (width %d; mean length %.1f, longest %d; %d of %d images aligned, mean path log-prob %.2f against mean total %.2f)."
             % (BEAM, lens.mean(), lens.max(), fin.sum(), BATCH, a[fin].mean(), t[fin].mean()),
             "HIP events over windows of about 0.5 s of back-to-back launches after warm-up (%d .. %d launches per window); one process; the launches alternate, two runs each."
             % (min(c for r in runs.values() for _, c in r), max(c for r in runs.values() for _, c in r)), "",
             "  beam launch (crnn_ctc_beam_decode)                                  %16s us = %6.3f us per image" % (fmt("beam"), best("beam") / BATCH),
             "  alignment launch (crnn_ctc_align: pre-pass + Viterbi, all outputs)  %16s us = %6.3f us per image" % (fmt("align"), best("align") / BATCH),
             "  alignment launch, score only (optional outputs NULL)                %16s us = %6.3f us per image"
             % (fmt("align, score only"), best("align, score only") / BATCH),
             "  lexicon launch, one candidate per image (pre-pass + scoring)        %16s us = %6.3f us per image" % (fmt("lexicon"), best("lexicon") / BATCH),
             "  alignment / beam = %.3f" % (best("align") / best("beam")), "",
             "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):"] + ["  " + r for r in resources()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
