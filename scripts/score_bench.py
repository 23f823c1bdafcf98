#!/usr/bin/env python3
"""Output side of validation at batch 1024, T = 52 (the 100 x 32 configuration), 38 classes, truth rows of 23: scoring on the device
(csrc/score.hip, metrics.device_edit_distances, Model.score_generator) against the host loop (metrics.edit_distance + normalized_edit_distance).
Prints
  (a) the score launch's time by HIP events over timed windows after warm-up (back-to-back launches: for a kernel this short that is the launch
      rate), and the kernel's own duration from a rocprofv3 --kernel-trace --stats run of the same step,
  (b) the beam launch it follows (crnn_ctc_beam_decode, beam_width 10), in the same process on the same softmax maps -- the yardstick,
  (c) the host scoring of the same pairs in pairs/s (both metrics, as predict.py --validate computes them), and images/s of score_generator end
      to end against predict_generator + decode + the two metrics over the same in-memory batches,
  (d) the ratios device over host,
and the kernel's resource usage as the compiler reports it (-Rpass-analysis=kernel-resource-usage).
Every step is a child process under its own time limit; the first one that fails ends the run.  usage: score_bench.py [--out FILE]"""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crnn-ocr-lite_amd")]
import numpy as np  # noqa: E402

BATCH, IMG_SIZE, T, C, MAX_LEN, BEAM = 1024, (100, 32, 1), 52, 38, 23, 10
STEPS = [("resources", 120), ("kernel", 180), ("trace", 300), ("e2e", 400)]         # (step, time limit in seconds)
WINDOW_S, REPEATS = 0.5, 3                                                           # timed window per kernel; windows per kernel, the two kernels alternating
E2E_BATCHES = 8


def make_pairs(seed=0):
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
           "-c", os.path.join(ROOT, "crnn-ocr-lite_amd", "csrc", "score.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    pick = lambda key: int(re.search(r"%s: (\d+)" % re.escape(key), err).group(1))
    return {"sgprs": pick("TotalSGPRs"), "vgprs": pick("VGPRs"), "agprs": pick("AGPRs"), "sgpr_spills": pick("SGPRs Spill"), "vgpr_spills": pick("VGPRs Spill"),
            "scratch_bytes_per_lane": pick("ScratchSize [bytes/lane]"), "lds_bytes": pick("LDS Size [bytes/block]"), "occupancy_waves_per_simd": pick("Occupancy [waves/SIMD]")}


def step_kernel():
    import ctypes
    import torch
    from crnn_mi355x import data as D, decode, metrics as M, native
    y_np, truth_np = make_pairs()
    y = torch.from_numpy(y_np).cuda()
    truth = torch.from_numpy(truth_np.astype(np.int32)).cuda()
    lab = torch.empty((BATCH, T), dtype=torch.int32, device="cuda")
    ln, sc = torch.empty(BATCH, dtype=torch.int32, device="cuda"), torch.empty(BATCH, dtype=torch.float32, device="cuda")
    out = torch.empty((3, BATCH), dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L, st = native.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    beam = lambda: L.crnn_ctc_beam_decode(p(y), None, p(lab), p(ln), p(sc), BATCH, T, C, BEAM, 1, st)
    score = lambda: L.crnn_edit_distance(p(lab), T, p(truth), MAX_LEN, C - 1, -1, p(out[0]), p(out[1]), p(out[2]), BATCH, st)
    native.check(beam(), "beam")
    native.check(score(), "edit_distance")
    events = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    sync = torch.cuda.synchronize
    beam_calls, score_calls = _calls_for(beam, sync), _calls_for(score, sync)
    beam_all, score_all = [], []
    for _ in range(REPEATS):                                               # the two kernels alternate: what disturbs one window disturbs its neighbour
        beam_all.append(_window(beam, beam_calls, sync, events))
        score_all.append(_window(score, score_calls, sync, events))
    beam_us, score_us = float(np.median(beam_all)), float(np.median(score_all))
    # the host's scoring of the same pairs, as predict.py --validate does it: texts, then the two metrics
    inv = {i: ch for i, ch in enumerate(D.get_lexicon())}
    dec = decode.DecodeCTCPred(inverse_classes=inv)
    pred_text = [dec.labels_to_text(r) for r in lab.cpu().numpy()]
    true_text = [dec.labels_to_text(r) for r in truth_np]
    t = time.time()
    ed, ned = M.edit_distance(pred_text, true_text), M.normalized_edit_distance(pred_text, true_text)
    host_s = time.time() - t
    s = M.Score(lab.cpu().numpy(), *[o.cpu().numpy() for o in out])
    assert s.edit_distance == ed and s.normalized_edit_distance == ned, "device and host disagree"
    return {"beam_us": round(beam_us, 2), "beam_calls": beam_calls, "score_us": round(score_us, 2), "score_calls": score_calls,
            "beam_spread": [round(min(beam_all), 2), round(max(beam_all), 2)], "score_spread": [round(min(score_all), 2), round(max(score_all), 2)],
            "host_pairs_per_sec": round(BATCH / host_s, 1), "mean_edit_distance": ed, "mean_pred_len": float(s.pred_lengths.mean()),
            "mean_true_len": float(s.true_lengths.mean())}


def _model_and_batches():
    import utils as U
    from crnn_mi355x import data as D
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
            yield ({"the_input": x, "the_labels": labels, "input_length": np.full((BATCH, 1), T - 2), "label_length": np.ones((BATCH, 1))}, {"ctc": np.zeros(BATCH)})
    return model, dec, gen, labels


def step_trace():
    """The kernel step again under rocprofv3 --kernel-trace --stats (a run of its own: tracing slows the host) -> mean duration of each kernel."""
    import csv
    import glob
    import tempfile
    folder = tempfile.mkdtemp()
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", folder, "-o", "score", "--", sys.executable, os.path.abspath(__file__),
                    "--step", "kernel", "--window", "0.02"], capture_output=True, text=True, check=True)     # short windows: every launch is a trace record
    out = {}
    for path in glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for key, name in (("trace_score_us", "edit_distance_kernel"), ("trace_beam_us", "beam")):
                if name in row["Name"] and int(row["Calls"]) > 100:
                    out[key] = round(float(row["AverageNs"]) / 1e3, 2)
    if len(out) != 2:
        raise RuntimeError("kernel statistics not found under %s" % folder)
    return out


def step_e2e():
    """One model, the same batches, both routes in one process; the device route's means must equal the host route's."""
    import torch
    from crnn_mi355x import metrics as M
    model, dec, gen, labels = _model_and_batches()
    model.score_generator(gen(), 2, dec)                                  # warm-up: engine, first launches
    model.predict_generator(gen(), 1)
    dev_rates, host_rates = [], []
    for _ in range(2):                                                    # alternating
        torch.cuda.synchronize()
        t = time.time()
        s = model.score_generator(gen(), E2E_BATCHES, dec)
        ed, ned = s.edit_distance, s.normalized_edit_distance
        dev_rates.append(E2E_BATCHES * BATCH / (time.time() - t))
        t = time.time()
        pred_text = dec.decode(model.predict_generator(gen(), E2E_BATCHES))
        true_text = [dec.labels_to_text(r) for r in np.tile(labels, (E2E_BATCHES, 1))]
        h_ed, h_ned = M.edit_distance(pred_text, true_text), M.normalized_edit_distance(pred_text, true_text)
        host_rates.append(E2E_BATCHES * BATCH / (time.time() - t))
        assert (ed, ned) == (h_ed, h_ned), "device and host disagree"
    return {"device_images_per_sec": [round(v, 1) for v in dev_rates], "host_images_per_sec": [round(v, 1) for v in host_rates],
            "e2e_mean_pred_len": float(s.pred_lengths.mean())}


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        if "--window" in sys.argv:
            global WINDOW_S
            WINDOW_S = float(sys.argv[sys.argv.index("--window") + 1])
        res = {"resources": step_resources, "kernel": step_kernel, "trace": step_trace, "e2e": step_e2e}[sys.argv[2]]()
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
    dev_pairs = BATCH / (r["score_us"] * 1e-6)
    d_rate, h_rate = max(r["device_images_per_sec"]), max(r["host_images_per_sec"])
    lines = ["scoring on the device against the host loop: batch %d, T = %d (100 x 32), %d classes, truth rows of %d, beam width %d" % (BATCH, T, C, MAX_LEN, BEAM),
             "pairs: softmax maps that decode to the truth with one symbol in ten misread; mean lengths %.1f predicted / %.1f true, mean edit distance %.3f"
             % (r["mean_pred_len"], r["mean_true_len"], r["mean_edit_distance"]),
             "HIP events: median of %d windows of about %.1f s per kernel, the two kernels alternating (min .. max in brackets)" % (REPEATS, WINDOW_S),
             "",
             "  (a) score launch (crnn_edit_distance), HIP events:    %9.2f us per batch [%.2f .. %.2f] = %.5f us per pair  (%d launches per window)"
             % (r["score_us"], r["score_spread"][0], r["score_spread"][1], r["score_us"] / BATCH, r["score_calls"]),
             "      the kernel alone, rocprofv3 --kernel-trace:       %9.2f us per batch  (back-to-back launches of a kernel this short time the launch rate, not the kernel)"
             % r["trace_score_us"],
             "  (b) beam launch (crnn_ctc_beam_decode), same process: %9.2f us per batch [%.2f .. %.2f] = %.5f us per pair  (%d launches per window)"
             % (r["beam_us"], r["beam_spread"][0], r["beam_spread"][1], r["beam_us"] / BATCH, r["beam_calls"]),
             "      the kernel alone, rocprofv3 --kernel-trace:       %9.2f us per batch" % r["trace_beam_us"],
             "      (a) / (b) = %.4f by events, %.4f by kernel trace" % (r["score_us"] / r["beam_us"], r["trace_score_us"] / r["trace_beam_us"]),
             "  (c) host scoring of the same pairs, both metrics:     %9.1f pairs/s   (metrics.edit_distance + normalized_edit_distance)" % r["host_pairs_per_sec"],
             "  (c) end to end, %d batches from memory, one model with random weights (mean predicted length %.1f), two alternating runs each:"
             % (E2E_BATCHES, r["e2e_mean_pred_len"]),
             "        score_generator:                                 %s images/s" % " / ".join("%.1f" % v for v in r["device_images_per_sec"]),
             "        predict_generator + decode + the two metrics:    %s images/s" % " / ".join("%.1f" % v for v in r["host_images_per_sec"]),
             "  (d) device over host: scoring alone %.0f x (%.3g pairs/s by the events' launch time against %.1f);  end to end %.1f x (best run of each)"
             % (dev_pairs / r["host_pairs_per_sec"], dev_pairs, r["host_pairs_per_sec"], d_rate / h_rate),
             "",
             "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): %d VGPRs, %d AGPRs, %d SGPRs, %d bytes of LDS, scratch %d bytes/lane, "
             "spills %d VGPR / %d SGPR, occupancy %d waves/SIMD"
             % (r["vgprs"], r["agprs"], r["sgprs"], r["lds_bytes"], r["scratch_bytes_per_lane"], r["vgpr_spills"], r["sgpr_spills"], r["occupancy_waves_per_simd"])]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
