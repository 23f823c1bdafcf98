#!/usr/bin/env python3
"""Error analysis on the device at batch 1024, T = 52 (the 100 x 32 configuration), truth rows of 23, 38 and 97 classes: the edit-script launch
(csrc/editops.hip, crnn_edit_ops) against the distance launch it replaces (csrc/score.hip, crnn_edit_distance) in the same run.  The predictions
are the beam decoder's own output on softmax maps that decode to the truth with one symbol in ten misread.  Prints
  (a) per class count the two launches by HIP events over timed windows after warm-up, alternating (back-to-back launches: for kernels this short
      that is the launch rate), the edit-script launch also without the maps, without the matrix and without both, and their ratio;
  (b) the two kernels' own durations from a rocprofv3 --kernel-trace --stats run (38 classes, maps and matrix on) and that ratio -- the number
      to report;
  (c) the host's metrics.confusion_matrix on the same pairs, in pairs/s (its matrix must equal the device's);
  (d) Model.score_generator over the same in-memory batches with and without confusions=True, in images/s,
and the kernel's resource usage as the compiler reports it.
Every step is a child process under its own time limit; the first one that fails ends the run.  usage: editops_bench.py [--out FILE]"""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd")]
import numpy as np  # noqa: E402

BATCH, IMG_SIZE, T, MAX_LEN, BEAM = 1024, (100, 32, 1), 52, 23, 10
CLASSES = (38, 97)                                                                   # softmax widths, the blank included
STEPS = [("resources", 120), ("kernel", 300), ("trace", 300), ("e2e", 400)]          # (step, time limit in seconds)
WINDOW_S, REPEATS = 0.4, 3
E2E_BATCHES = 8
VARIANTS = (("maps + matrix", True, True), ("matrix only", False, True), ("maps only", True, False), ("counts only", False, False))


def make_pairs(C, seed=0):
    """-> (softmax maps (BATCH, T, C) fp32 that decode to the truth with a few errors, truth rows (BATCH, MAX_LEN) filled with blank)."""
    rs = np.random.RandomState(seed)
    blank = C - 1
    truth = np.full((BATCH, MAX_LEN), blank, np.int64)
    logits = rs.randn(BATCH, T, C).astype(np.float32)
    for k in range(BATCH):
        n = int(rs.randint(2, MAX_LEN + 1))
        word = rs.randint(0, blank, n)
        truth[k, :n] = word
        said = np.where(rs.rand(n) < 0.1, rs.randint(0, blank, n), word)       # one symbol in ten misread
        frames = np.full(T, blank)
        frames[2:2 + 2 * n:2] = said                                           # symbol, blank, symbol, ...
        logits[k, np.arange(T), frames] += 8.0
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32), truth


def _calls_for(fn, sync):
    """Warm-up, then the number of calls that fill a window of about WINDOW_S seconds."""
    for _ in range(20):
        fn()
    sync()
    t = time.time()
    for _ in range(50):
        fn()
    sync()
    return max(50, int(WINDOW_S / max((time.time() - t) / 50, 1e-7)))


def _window(fn, calls, sync, events):
    """us per call over `calls` back-to-back calls, by HIP events."""
    e0, e1 = events()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    sync()
    return e0.elapsed_time(e1) * 1e3 / calls


def step_resources():
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(ROOT, "crnn-ocr-lite_amd", "csrc", "editops.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    pick = lambda key: int(re.search(r"%s: (\d+)" % re.escape(key), err).group(1))
    return {"sgprs": pick("TotalSGPRs"), "vgprs": pick("VGPRs"), "agprs": pick("AGPRs"), "sgpr_spills": pick("SGPRs Spill"), "vgpr_spills": pick("VGPRs Spill"),
            "scratch_bytes_per_lane": pick("ScratchSize [bytes/lane]"), "occupancy_waves_per_simd": pick("Occupancy [waves/SIMD]")}


def step_kernel(only_full=False):
    import ctypes
    import torch
    from crnn_mi355x import metrics as M, native
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    L, st = native.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    events = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    sync = torch.cuda.synchronize
    res = {}
    for C in CLASSES[:1] if only_full else CLASSES:
        y_np, truth_np = make_pairs(C)
        y = torch.from_numpy(y_np).cuda()
        truth = torch.from_numpy(truth_np.astype(np.int32)).cuda()
        lab = torch.empty((BATCH, T), dtype=torch.int32, device="cuda")
        ln, sc = torch.empty(BATCH, dtype=torch.int32, device="cuda"), torch.empty(BATCH, dtype=torch.float32, device="cuda")
        native.check(L.crnn_ctc_beam_decode(p(y), None, p(lab), p(ln), p(sc), BATCH, T, C, BEAM, 1, st), "beam")
        out = torch.empty((3, BATCH), dtype=torch.int32, device="cuda")
        ops = torch.empty((BATCH, 4), dtype=torch.int32, device="cuda")
        tmap, pmap = torch.empty((BATCH, MAX_LEN), dtype=torch.int32, device="cuda"), torch.empty((BATCH, T), dtype=torch.int32, device="cuda")
        conf = torch.zeros((C, C), dtype=torch.int32, device="cuda")           # C - 1 characters and "nothing"
        dist = lambda: L.crnn_edit_distance(p(lab), T, p(truth), MAX_LEN, C - 1, -1, p(out[0]), p(out[1]), p(out[2]), BATCH, st)

        def ops_launch(maps, matrix):
            return lambda: L.crnn_edit_ops(p(lab), T, p(truth), MAX_LEN, C - 1, -1, C - 1, p(ops), p(out[0]), p(out[1]), p(out[2]), p(tmap if maps else None),
                                           p(pmap if maps else None), p(conf if matrix else None), BATCH, st)
        fns = [("dist", dist)] + [(name, ops_launch(maps, matrix)) for name, maps, matrix in (VARIANTS[:1] if only_full else VARIANTS)]
        for _, fn in fns:
            native.check(fn(), "launch")
        calls = {name: _calls_for(fn, sync) for name, fn in fns}
        seen = {name: [] for name, _ in fns}
        for _ in range(REPEATS):                                             # the launches alternate: what disturbs one window disturbs its neighbours
            for name, fn in fns:
                seen[name].append(_window(fn, calls[name], sync, events))
        r = {name: {"us": round(float(np.median(v)), 2), "spread": [round(min(v), 2), round(max(v), 2)], "calls": calls[name]} for name, v in seen.items()}
        if not only_full:
            # the host's matrix of the same pairs, which the device's must equal
            conf.zero_()
            native.check(ops_launch(True, True)(), "edit_ops")
            filt = lambda row: [int(v) for v in row if v != C - 1 and v != -1]
            pairs = [(filt(a), filt(b)) for a, b in zip(lab.cpu().numpy(), truth_np)]
            t = time.time()
            host = M.confusion_matrix(pairs, C - 1)
            r["host_pairs_per_sec"] = round(BATCH / (time.time() - t), 1)
            assert np.array_equal(host, conf.cpu().numpy()), "device and host disagree"
            o = ops.cpu().numpy()
            r["totals"] = [int(v) for v in o.sum(0)]
            r["mean_pred_len"], r["mean_true_len"] = float(out[1].float().mean()), float(out[2].float().mean())
        res[str(C)] = r
    return res


def step_trace():
    """The full variant at 38 classes again under rocprofv3 --kernel-trace --stats (a run of its own: tracing slows the host) -> mean kernel durations."""
    import csv
    import glob
    import tempfile
    folder = tempfile.mkdtemp()
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", folder, "-o", "editops", "--", sys.executable, os.path.abspath(__file__),
                    "--step", "kernel_full", "--window", "0.02"], capture_output=True, text=True, check=True)     # short windows: every launch is a trace record
    out = {}
    for path in glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for key, name in (("trace_ops_us", "edit_ops_kernel"), ("trace_dist_us", "edit_distance_kernel")):
                if name in row["Name"] and int(row["Calls"]) > 100:
                    out[key] = round(float(row["AverageNs"]) / 1e3, 2)
    if len(out) != 2:
        raise RuntimeError("kernel statistics not found under %s" % folder)
    return out


def step_e2e():
    """One model, the same batches, the validation pass with and without the confusions; the three integers per pair must agree."""
    import torch
    import utils as U
    from crnn_mi355x import data as D
    C = CLASSES[0]
    rs = np.random.RandomState(1)
    model = U.init_predictor(U.CRNN(num_classes=C, max_string_len=MAX_LEN, shape=IMG_SIZE, time_dense_size=128, n_units=256).get_model())
    dec = U.DecodeCTCPred(top_paths=1, beam_width=BEAM, inverse_classes={i: ch for i, ch in enumerate(D.get_lexicon())})
    x = rs.randn(BATCH, *IMG_SIZE)                                       # float64, as Readf yields it
    labels = np.full((BATCH, MAX_LEN), C - 1, np.int64)
    for k in range(BATCH):
        n = int(rs.randint(2, MAX_LEN + 1))
        labels[k, :n] = rs.randint(0, C - 1, n)

    def gen():
        while True:
            yield ({"the_input": x, "the_labels": labels}, {"ctc": np.zeros(BATCH)})
    model.score_generator(gen(), 2, dec)                                  # warm-up: engine, first launches
    model.score_generator(gen(), 2, dec, confusions=True)
    plain, conf = [], []
    for _ in range(2):                                                    # alternating
        for rates, kw in ((plain, {}), (conf, {"confusions": True})):
            torch.cuda.synchronize()
            t = time.time()
            s = model.score_generator(gen(), E2E_BATCHES, dec, **kw)
            rates.append(E2E_BATCHES * BATCH / (time.time() - t))
            if kw:
                assert np.array_equal(s.distances, ref.distances) and np.array_equal(s.ops[:, 1:].sum(1), s.distances), "the two passes disagree"
            ref = s
    return {"plain_images_per_sec": [round(v, 1) for v in plain], "confusions_images_per_sec": [round(v, 1) for v in conf]}


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        if "--window" in sys.argv:
            global WINDOW_S
            WINDOW_S = float(sys.argv[sys.argv.index("--window") + 1])
        res = {"resources": step_resources, "kernel": step_kernel, "kernel_full": lambda: step_kernel(True), "trace": step_trace, "e2e": step_e2e}[sys.argv[2]]()
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    r = {}
    for step, limit in STEPS:
        done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True)
        lines = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            print("step %s failed (exit %d); stopping\n%s" % (step, done.returncode, done.stderr[-3000:]), flush=True)
            return 1
        r.update(json.loads(lines[-1][7:]))
        print("step %s done" % step, file=sys.stderr, flush=True)
    lines = ["edit scripts and confusions on the device against the distance launch: batch %d, T = %d (100 x 32), truth rows of %d, beam width %d" % (BATCH, T, MAX_LEN, BEAM),
             "pairs: the beam decoder's output on softmax maps that decode to the truth with one symbol in ten misread",
             "HIP events: median of %d windows of about %.1f s per launch, the launches alternating (min .. max in brackets); back-to-back launches of kernels"
             % (REPEATS, WINDOW_S),
             "this short time the launch rate, so the kernels' own durations come from rocprofv3 --kernel-trace --stats in a run of its own", ""]
    for C in CLASSES:
        k = r[str(C)]
        lines.append("  %d classes (matrix %d x %d): mean lengths %.1f predicted / %.1f true; matches / substitutions / deletions / insertions = %s"
                     % (C, C, C, k["mean_pred_len"], k["mean_true_len"], " / ".join(str(v) for v in k["totals"])))
        lines.append("    (a) crnn_edit_distance:                 %8.2f us per batch [%.2f .. %.2f]  (%d launches per window)"
                     % (k["dist"]["us"], k["dist"]["spread"][0], k["dist"]["spread"][1], k["dist"]["calls"]))
        for name, _, _ in VARIANTS:
            v = k[name]
            lines.append("        crnn_edit_ops, %-13s            %8.2f us per batch [%.2f .. %.2f]  = %.2f x the distance launch"
                         % (name + ":", v["us"], v["spread"][0], v["spread"][1], v["us"] / k["dist"]["us"]))
        lines.append("    (c) host metrics.confusion_matrix on the same pairs (equal to the device's): %.1f pairs/s; the launch with maps and matrix: %.3g pairs/s"
                     % (k["host_pairs_per_sec"], BATCH / (k[VARIANTS[0][0]]["us"] * 1e-6)))
    lines += ["",
              "  (b) the kernels alone, rocprofv3 --kernel-trace, %d classes, maps and matrix: edit_ops_kernel %.2f us, edit_distance_kernel %.2f us per batch: ratio %.2f"
              % (CLASSES[0], r["trace_ops_us"], r["trace_dist_us"], r["trace_ops_us"] / r["trace_dist_us"]),
              "  (d) Model.score_generator, %d batches from memory, one model with random weights, two alternating runs each:" % E2E_BATCHES,
              "        as before:          %s images/s" % " / ".join("%.1f" % v for v in r["plain_images_per_sec"]),
              "        confusions=True:    %s images/s   (best over best: %.3f)"
              % (" / ".join("%.1f" % v for v in r["confusions_images_per_sec"]), max(r["confusions_images_per_sec"]) / max(r["plain_images_per_sec"])),
              "  the private matrix per workgroup is the only form built; one global atomic per aligned symbol was not tried",
              "",
              "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): %d VGPRs, %d AGPRs, %d SGPRs, dynamic LDS (20 bytes per prediction column "
              "and wavefront + the matrix), scratch %d bytes/lane, spills %d VGPR / %d SGPR, occupancy %d waves/SIMD"
              % (r["vgprs"], r["agprs"], r["sgprs"], r["scratch_bytes_per_lane"], r["vgpr_spills"], r["sgpr_spills"], r["occupancy_waves_per_simd"])]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
